#!/usr/bin/env python3
"""Batched channel compensation (JFAAcc::normalizeFeaturesBatch, one gmmiv_feat_compensate_models for all sessions) against the
per-session loop it is an alternative to (JFAAcc::normalizeFeatures: per session gmmiv_gmm_set + gmmiv_feat_compensate).

Shape: --sessions (1000) sessions at 2048 x 60, --frames (300 and 3000) frames per session, resident float32 frames, every session one
contiguous run (so neither path gathers or scatters), session model m + U x_h with rank-3 U.  Per size the two paths ALTERNATE for
--rounds calls of liagpu_jfa_normalize_features_bench; each call opens its own server, uploads the frames, runs --reps repetitions
(the first --warmup are dropped) with the host clock around one whole call and the stream drained before and after, then one more
pass with the kernel timers on.  Reported per path: every kept time, the median and the min-max spread; per-kernel times of the last
library call of the extra pass (the whole batch on the batched path; on the loop only its last session, since the timers restart with
every library call).  The bytes k_feat_comp fetches per frame need a counter pass of their own (rocprofv3 --pmc, no tracing): not taken
by this tool.  Writes one JSON file (default profiles/r16/feat_comp_models.json)."""
import argparse
import ctypes as ct
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def frames_like(w, mean, iv, T, seed):
    """frames drawn like conftest.make_frames, in pieces (3 * 10^6 x 60 at once would hold the float64 draws of all of them)"""
    rng = np.random.default_rng(seed)
    sd = 1.0 / np.sqrt(iv)
    x = np.empty((T, mean.shape[1]), np.float32)
    for b in range(0, T, 1 << 18):
        n = min(1 << 18, T - b)
        comp = rng.choice(len(w), size=n, p=w / w.sum())
        x[b:b + n] = mean[comp] + rng.standard_normal((n, mean.shape[1]), dtype=np.float32) * sd[comp]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=1000)
    ap.add_argument("--frames", type=int, nargs="+", default=[300, 3000])
    ap.add_argument("--gaussians", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=60)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "feat_comp_models.json"))
    args = ap.parse_args()
    import torch
    from conftest import make_gmm
    from lia_ral_amd import host_capi as h

    assert torch.cuda.is_available(), "this tool measures on the GPU"
    assert args.reps > args.warmup >= 0
    C, D, S = args.gaussians, args.dim, args.sessions
    w, mean, iv = make_gmm(C, D, seed=0, spread=0.1)
    cov = 1.0 / iv
    rng = np.random.default_rng(7)
    U = np.ascontiguousarray(rng.normal(0.0, 0.05, (args.rank, C * D)))
    X = np.ascontiguousarray(rng.normal(size=(S, args.rank)))
    dp, fp = ct.POINTER(ct.c_double), ct.POINTER(ct.c_float)
    d = lambda a: a.ctypes.data_as(dp)
    result = dict(device=torch.cuda.get_device_name(0), C=C, D=D, sessions=S, rank=args.rank, reps=args.reps, warmup=args.warmup, rounds=args.rounds,
                  paths={"batched": "JFAAcc::normalizeFeaturesBatch", "loop": "JFAAcc::normalizeFeatures"}, fetch_bytes_per_frame_k_feat_comp=None, runs=[])
    for n in args.frames:
        x = frames_like(w, mean, iv, S * n, seed=1)
        times = {"batched": [], "loop": []}
        kern = {}
        for _ in range(args.rounds):
            for name, which in (("batched", 0), ("loop", 1)):
                ms = np.zeros(args.reps)
                km = np.zeros(4)
                h._chk(h.lib.liagpu_jfa_normalize_features_bench(0, x.ctypes.data_as(fp), ct.c_long(S), ct.c_long(n), D, C, d(w), d(np.ascontiguousarray(mean)),
                                                                 d(np.ascontiguousarray(cov)), args.rank, d(U), d(X), which, args.reps, d(ms), d(km)))
                times[name] += [float(v) for v in ms[args.warmup:]]
                kern[name] = dict(k_gmm_pack_ms=km[0], k_llk_mfma_ms=km[1], k_feat_comp_ms=km[2], k_feat_comp_launches=int(km[3]))
        med = {k: float(np.median(v)) for k, v in times.items()}
        spread = {k: float(max(v) - min(v)) for k, v in times.items()}
        run = dict(frames_per_session=n, frames=S * n, batched_ms=times["batched"], loop_ms=times["loop"], batched_median_ms=med["batched"],
                   loop_median_ms=med["loop"], batched_spread_ms=spread["batched"], loop_spread_ms=spread["loop"],
                   loop_over_batched=med["loop"] / med["batched"],
                   batched_faster_by_more_than_spread=bool(med["loop"] - med["batched"] > max(spread.values())),
                   batched_gpairs_per_s=S * n * C / med["batched"] / 1e6, loop_gpairs_per_s=S * n * C / med["loop"] / 1e6,
                   kernels_batched_whole_call=kern["batched"], kernels_loop_last_session_only=kern["loop"])
        result["runs"].append(run)
        print("%d sessions x %d frames: batched %.1f ms (spread %.1f)  loop %.1f ms (spread %.1f)  loop / batched %.2f | batched kernels: pack %.2f, k_llk_mfma %.2f, "
              "k_feat_comp %.2f ms in %d launches" % (S, n, med["batched"], spread["batched"], med["loop"], spread["loop"], run["loop_over_batched"],
                                                      kern["batched"]["k_gmm_pack_ms"], kern["batched"]["k_llk_mfma_ms"], kern["batched"]["k_feat_comp_ms"],
                                                      kern["batched"]["k_feat_comp_launches"]), flush=True)
        del x
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
