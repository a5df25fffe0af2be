#!/usr/bin/env python3
"""Side measurement for DESIGN.md (not the headline bench): score normalisation (gmmiv_score_cohort_stats /
gmmiv_score_normalize) on resident matrices against the same results composed from torch-ROCm ops on the same tensors, and
against a device-to-device copy of the matrix as the streaming yardstick.  One JSON line.

Shapes: 20 000 x 20 000 (3.2 GB, beyond L2 and Infinity Cache: the shape the requirement is stated on), the cohorts
100 000 x 1000 (axis 0) and 1000 x 100 000 (axis 1), and 4100 x 4233.
Per mode: five alternating repeats (ours, torch, ours, torch, ...) of a window of at least 0.5 s each, host clock around a final
synchronise, after a warm-up call.  Requirement at the 20 k shape: median(ours) <= median(torch) + (max(torch) - min(torch)).
Algorithmic bytes: one read of the matrix for statistics; one read + one write (+ one more write with first_out) for apply;
reported over time as a fraction of 8 TB/s, and per byte against the copy (which moves 2 x the matrix)."""
import argparse, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from lia_ral_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="20000x20000,100000x1000,1000x100000,4100x4233")
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
HBM = 8.0e12
PH, PL = 0.05, 0.20


def window(f, est):
    reps = max(1, int(math.ceil(args.window / max(est, 1e-6))))
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def estimate(f):
    f(); torch.cuda.synchronize()                      # warm-up (allocations, code objects)
    t = time.perf_counter(); f(); torch.cuda.synchronize()
    return time.perf_counter() - t


def peak_extra(f):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    f(); torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def compare(ours, theirs):
    eo, et = estimate(ours), estimate(theirs)
    to, tt = [], []
    for _ in range(args.repeats):                      # alternating
        to.append(window(ours, eo)); tt.append(window(theirs, et))
    return to, tt


def torch_stats(A, dim, mode, trimmed):
    n = A.shape[dim]
    if not trimmed:
        return A.mean(dim), A.var(dim, unbiased=False).sqrt()
    dH, dL = int(float(n) * PH), int(float(n) * PL)
    k = A.sort(dim, descending=True).values.narrow(dim, dH, n - dH - dL)
    if mode == 0:
        return k.mean(dim), k.var(dim, unbiased=False).sqrt()
    med = k.select(dim, (n - dH - dL) // 2)
    return med, (k - med.unsqueeze(dim)).abs().mean(dim)


def torch_apply(X, F, order, rm, rs, cm, cs):
    z = lambda: X.sub_(rm[:, None]).div_(rs[:, None])
    t = lambda: X.sub_(cm[None, :]).div_(cs[None, :])
    if order == 0: z()
    elif order == 1: t()
    elif order == 2: t(); F.copy_(X); z()
    else: z(); F.copy_(X); t()


res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats, "percentH": PH, "percentL": PL,
       "shapes": {}}
for shp in args.shapes.split(","):
    rows, cols = [int(v) for v in shp.split("x")]
    g = torch.Generator(device=dev); g.manual_seed(rows * 31 + cols)
    A = torch.randn((rows, cols), dtype=torch.float64, device=dev, generator=g) * 1.5 - 2.0
    nbytes = A.numel() * 8
    Y = torch.empty_like(A)
    e = estimate(lambda: Y.copy_(A))
    tc = [window(lambda: Y.copy_(A), e) for _ in range(args.repeats)]
    copy_s = statistics.median(tc)
    entry = {"matrix_bytes": nbytes, "copy": {"ms": copy_s * 1e3, "spread_ms": (max(tc) - min(tc)) * 1e3,
                                               "TBps_moved": 2 * nbytes / copy_s / 1e12}, "modes": {}}

    def record(name, to, tt, moved, ours_mem, torch_mem):
        mo, mt, spread = statistics.median(to), statistics.median(tt), max(tt) - min(tt)
        entry["modes"][name] = {
            "ours_ms": mo * 1e3, "ours_all_ms": [v * 1e3 for v in to], "torch_ms": mt * 1e3, "torch_all_ms": [v * 1e3 for v in tt],
            "torch_spread_ms": spread * 1e3, "no_slower_than_torch": bool(mo <= mt + spread), "speedup_vs_torch": mt / mo,
            "algorithmic_bytes": moved, "fraction_of_8TBps": moved / mo / HBM,
            "time_per_byte_vs_copy": (mo / moved) / (copy_s / (2 * nbytes)),
            "ours_scratch_bytes": ours_mem, "torch_extra_bytes": torch_mem}

    axes = (0, 1) if shp in ("20000x20000", "4100x4233") else ((0,) if rows > cols else (1,))
    for axis in axes:
        nd = A.shape[axis]
        m = torch.empty(nd, dtype=torch.float64, device=dev); s = torch.empty_like(m)
        for name, mode, trimmed in (("mean", 0, False), ("trimmed_mean", 0, True), ("trimmed_median", 1, True)):
            kw = dict(mean_mode=mode, percent_h=PH if trimmed else 0.0, percent_l=PL if trimmed else 0.0, out_mean=m, out_std=s)
            ours = lambda: ctx.score_cohort_stats(A, axis, **kw)
            theirs = lambda: torch_stats(A, 1 - axis, mode, trimmed)
            tmem = peak_extra(theirs)
            to, tt = compare(ours, theirs)
            record("stats_axis%d_%s" % (axis, name), to, tt, nbytes, sum(ctx.workspace_bytes(i) for i in range(64)), tmem)
    if len(axes) == 2:
        F = torch.empty_like(A)
        rm = torch.full((rows,), -2.0, dtype=torch.float64, device=dev); cm = torch.full((cols,), -2.0, dtype=torch.float64, device=dev)
        rs = torch.rand(rows, dtype=torch.float64, device=dev, generator=g) * 0.8 + 1.2   # > 1: repeated in-place passes stay finite
        cs = torch.rand(cols, dtype=torch.float64, device=dev, generator=g) * 0.8 + 1.2
        X = A.clone()
        for order, name in enumerate(("z", "t", "zt_first_out", "tz_first_out")):
            ours = lambda: ctx.score_normalize(X, order, rm, rs, cm, cs, first_out=F if order >= 2 else None)
            theirs = lambda: torch_apply(X, F, order, rm, rs, cm, cs)
            tmem = peak_extra(theirs)
            to, tt = compare(ours, theirs)
            record("apply_" + name, to, tt, (3 if order >= 2 else 2) * nbytes, sum(ctx.workspace_bytes(i) for i in range(64)), tmem)
        del F, X
    res["shapes"][shp] = entry
    del A, Y
    torch.cuda.empty_cache()

gate = res["shapes"].get("20000x20000")
if gate:
    res["requirement_met_at_20k"] = {k: v["no_slower_than_torch"] for k, v in gate["modes"].items()}
line = json.dumps(res)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)
