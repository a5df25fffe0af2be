#!/usr/bin/env python3
"""Side measurement for DESIGN.md section 3.17 (not the headline bench): gmmiv_score_list_stats on device-resident lists.  One JSON
line, written to profiles/r14/score_lists.json by default.

Cases:
  (i)   a cross-product list of 4100 x 4233 scores against the dense gmmiv_score_cohort_stats (axis 0) on the same data -- the dense
        call is what a cross product was served by before lists existed.  Four modes: untrimmed mean, trimmed mean, unsorted median,
        trimmed median.  ratio = list / dense.
  (ii)  a NIST-like ragged list: 20 000 distributions, lengths uniform in 50 .. 2000.
  (iii) a skewed list: one distribution of 10^6 scores among 10^4 of length 100.
Every case is measured without and with pos (a random permutation of the slots) + pre_id (ids into 1000 pre-normalisation pairs).

Method: per measurement a warm-up call, then `repeats` windows of at least `window` seconds, each timed with a HIP event pair on the
context's stream; list and dense windows alternate in case (i).  Two figures per list measurement: call_ms -- event time per call,
which contains the call's host side (planning, the upload of its two tables and the one stream wait) -- and kernel_ms, the sum of
the call's kernel launches from the context's own event timers ("k_norm_stats", option "timing"), taken in a separate pass.
Algorithmic bytes: one read of every score of the list (8 bytes each; pos adds 8 and pre_id 4 per slot), over kernel time."""
import argparse, json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from lia_ral_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "score_lists.json"))
ap.add_argument("--dense-ref", default=os.path.join(ROOT, "profiles", "r07", "score_norm.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_score_lists: no GPU; nothing is measured without one")
dev = torch.device("cuda", 0)
ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
PH, PL = 0.05, 0.20
MODES = (("mean", 0, 0.0, 0.0), ("trimmed_mean", 0, PH, PL), ("unsorted_median", 1, 0.0, 0.0), ("trimmed_median", 1, PH, PL))
NPRE = 1000


def event_ms(f, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def reps_for(f):
    f(); torch.cuda.synchronize()                      # warm-up (allocations, code objects, LDS attributes)
    est = max(event_ms(f, 1), 1e-3)
    return max(1, int(math.ceil(args.window * 1e3 / est)))


def kernel_ms(f):
    """median over `repeats` calls of the call's own kernel time"""
    ctx.set_option("timing", 1)
    v = []
    for _ in range(args.repeats + 1):
        f(); torch.cuda.synchronize()
        v.append(ctx.kernel_ms("k_norm_stats"))
    ctx.set_option("timing", 0)
    return statistics.median(v[1:])


def summary(v):
    return {"ms": statistics.median(v), "all_ms": v, "spread_ms": max(v) - min(v)}


def measure_list(off, sc, pos, pid, pre, nslots, dense=None):
    """-> modes -> {plain, pos_pre (, dense, dense_pre, ratios)}"""
    nd = len(off) - 1
    m = torch.empty(nd, dtype=torch.float64, device=dev); s = torch.empty_like(m)
    out = {}
    for name, mode, pH, pL in MODES:
        kw = dict(mean_mode=mode, percent_h=pH, percent_l=pL, out_mean=m, out_std=s)
        calls = {"plain": lambda: ctx.score_list_stats(off, sc, **kw),
                 "pos_pre": lambda: ctx.score_list_stats(off, sc, pos=pos, pre_id=pid, pre_mean=pre[0], pre_std=pre[1], **kw)}
        if dense is not None:
            A, dpm, dps = dense
            dm = torch.empty(A.shape[0], dtype=torch.float64, device=dev); ds = torch.empty_like(dm)
            dkw = dict(mean_mode=mode, percent_h=pH, percent_l=pL, out_mean=dm, out_std=ds)
            calls["dense"] = lambda: ctx.score_cohort_stats(A, 0, **dkw)
            calls["dense_pre"] = lambda: ctx.score_cohort_stats(A, 0, pre_mean=dpm, pre_std=dps, **dkw)
        reps = {k: reps_for(f) for k, f in calls.items()}
        t = {k: [] for k in calls}
        for _ in range(args.repeats):                  # alternating
            for k, f in calls.items():
                t[k].append(event_ms(f, reps[k]))
        e = {}
        for k, f in calls.items():
            e[k] = summary(t[k])
            e[k]["kernel_ms"] = kernel_ms(f)
            nbytes = nslots * (20 if k == "pos_pre" else 8)   # the pre-normalisation vectors are small and stay in cache
            e[k]["algorithmic_bytes"] = nbytes
            e[k]["kernel_TBps"] = nbytes / (e[k]["kernel_ms"] * 1e-3) / 1e12
            e[k]["call_TBps"] = nbytes / (e[k]["ms"] * 1e-3) / 1e12
        if dense is not None:
            e["ratio_list_over_dense_call"] = e["plain"]["ms"] / e["dense"]["ms"]
            e["ratio_list_over_dense_kernel"] = e["plain"]["kernel_ms"] / e["dense"]["kernel_ms"]
            e["ratio_pos_pre_over_dense_pre_kernel"] = e["pos_pre"]["kernel_ms"] / e["dense_pre"]["kernel_ms"]
            calls["plain"](); calls["dense"](); torch.cuda.synchronize()
            e["bitwise_equal_to_dense"] = bool(torch.equal(m.view(torch.int64), dm.view(torch.int64)) and torch.equal(s.view(torch.int64), ds.view(torch.int64)))
        out[name] = e
    return out


def tables(lens, seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    sc = torch.randn(n, dtype=torch.float64, device=dev, generator=g) * 1.5 - 2.0
    pos = torch.randperm(n, device=dev, generator=g)
    pid = torch.randint(0, NPRE, (n,), dtype=torch.int32, device=dev, generator=g)
    pre = (torch.randn(NPRE, dtype=torch.float64, device=dev, generator=g) * 0.3 - 2.0,
           torch.rand(NPRE, dtype=torch.float64, device=dev, generator=g) * 1.5 + 0.5)
    return off, sc, pos, pid, pre, n


res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats, "percentH": PH, "percentL": PL, "cases": {}}

# (i) cross product against the dense call
rows, cols = 4100, 4233
off, sc, pos, pid, pre, n = tables(np.full(rows, cols), 1)
A = sc.view(rows, cols)
g = torch.Generator(device=dev); g.manual_seed(2)
dpm = torch.randn(cols, dtype=torch.float64, device=dev, generator=g) * 0.3 - 2.0
dps = torch.rand(cols, dtype=torch.float64, device=dev, generator=g) * 1.5 + 0.5
res["cases"]["cross_4100x4233"] = {"ndist": rows, "scores": n, "modes": measure_list(off, sc, pos, pid, pre, n, dense=(A, dpm, dps))}
try:
    ref = json.loads(open(args.dense_ref).read())["shapes"]["4100x4233"]["modes"]
    res["cases"]["cross_4100x4233"]["dense_r07_ms"] = {k: ref["stats_axis0_" + k]["ours_ms"] for k in ("mean", "trimmed_mean", "trimmed_median")}
except (OSError, KeyError, ValueError):
    pass
del A

# (ii) NIST-like ragged list
rng = np.random.default_rng(3)
lens = rng.integers(50, 2001, 20000)
off, sc, pos, pid, pre, n = tables(lens, 3)
res["cases"]["ragged_20000x50..2000"] = {"ndist": len(lens), "scores": n, "modes": measure_list(off, sc, pos, pid, pre, n)}

# (iii) skewed list
lens = np.full(10001, 100); lens[5000] = 1000000
off, sc, pos, pid, pre, n = tables(lens, 4)
res["cases"]["skewed_1e6_among_1e4x100"] = {"ndist": len(lens), "scores": n, "modes": measure_list(off, sc, pos, pid, pre, n)}

line = json.dumps(res)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(line + "\n")
print(line)
