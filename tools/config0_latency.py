#!/usr/bin/env python3
"""The call latency of BASELINE.json configs[0] (128-Gaussian UBM, 60 dims, 1000 frames, top-10 COMPLETE, one client; host arrays in and
out) -- the one figure where the host code of a C-API call is visible.  bench.py times the pair llk_determine_top + llk_use_top once,
after one warm-up, and only with its CPU legs on (computetest_cpu_and_config0); this repeats the same pair 401 times and prints one JSON
line: as_bench_ms = the first timed pair, as bench.py takes it; median / min / p10 / p90 over the other 400.  GMMIV_LIB_PATH selects
another build of the library (profiles/r18/gmm_capi_split_ab.json: parent and head alternated, one process each)."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

if __name__ == "__main__":
    from conftest import make_frames, make_gmm
    from lia_ral_amd import capi
    ctx = capi.Context(0)
    w0, m0, iv0 = make_gmm(128, 60, seed=0)
    x0 = make_frames(w0, m0, iv0, 1000, seed=1)
    mc = m0 + np.random.default_rng(5).normal(0, 0.1, m0.shape)
    gw, gc = ctx.gmm(w0, m0, iv0), ctx.gmm(w0, mc, iv0)
    gw.llk_determine_top(x0, 10, True)                                       # warm-up
    ms = []
    for _ in range(401):
        t0 = time.perf_counter()
        d = gw.llk_determine_top(x0, 10, True)
        gc.llk_use_top(x0, d["idx"], d["nontop_llk"], True)
        ms.append((time.perf_counter() - t0) * 1e3)
    rest = np.array(ms[1:])
    print(json.dumps({"lib": capi.LIB_PATH, "as_bench_ms": round(ms[0], 4), "median_ms": round(float(np.median(rest)), 4), "min_ms": round(float(rest.min()), 4),
                      "p10_ms": round(float(np.percentile(rest, 10)), 4), "p90_ms": round(float(np.percentile(rest, 90)), 4)}))
