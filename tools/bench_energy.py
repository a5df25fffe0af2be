#!/usr/bin/env python3
"""EnergyDetector over a list of files: the per-file loop (host_capi.energy_detector once per file) against the batch
(host_capi.energy_detector_batch, one call for the list) on the SAME list, in one process.

Lists: --files x 3000 frames and --files x 30000 frames (default 1000 files), a normalised energy column per file, the whole file selected,
C = 3, 10 iterations, alpha 2.  Both paths start from host arrays and end with host results (upload, training, selection, download), wall clock
around the call(s).  After a warm-up of each path the paths alternate for --reps >= 5 repetitions; the median and the min-max spread are
reported, and the batch's results are checked against the loop's (segments equal, thresholds within 1e-9).  The two kernels' own times come
from the context's timers in one extra pass on the resident list.  Writes the next free profiles/rNN/energy_detector.json (or --out).
There is no CPU fallback: without a GPU the script fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def next_free(name):
    """profiles/rNN/<name> with NN one past the highest round that exists"""
    base = os.path.join(ROOT, "profiles")
    have = [int(d[1:]) for d in os.listdir(base) if d.startswith("r") and d[1:].isdigit()] if os.path.isdir(base) else []
    return os.path.join(base, "r%02d" % (max(have, default=0) + 1), name)


def energy_like(n, rng):
    """a normalised energy column with speech and silence in stretches of about 40 frames (a frame-wise coin would give the per-file
    tool more output segments than its fixed 4096-entry arrays hold)"""
    lens = rng.geometric(1.0 / 40.0, size=n // 20 + 2)
    state = np.repeat(np.arange(len(lens)) % 2 == 1, lens)[:n]
    return np.where(state, rng.normal(1.2, 0.3, n), rng.normal(-0.9, 0.2, n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--frames", type=int, nargs="+", default=[3000, 30000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--C", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "at least five repetitions"
    import torch
    from lia_ral_amd import capi, host_capi as h
    assert torch.cuda.is_available(), "bench_energy needs a GPU"
    kw = dict(C=args.C, nb_train_it=args.iterations, variance_flooring=0.5, variance_ceiling=10.0, alpha=2.0)
    res = dict(device=torch.cuda.get_device_name(0), files=args.files, C=args.C, iterations=args.iterations, reps=args.reps, lists=[])
    for frames in args.frames:
        rng = np.random.default_rng(frames)
        energies = [energy_like(frames, rng) for _ in range(args.files)]
        segs = [(np.array([0]), np.array([frames]))] * args.files

        def loop():
            return [h.energy_detector(e, s[0], s[1], **kw) for e, s in zip(energies, segs)]

        def batch():
            return h.energy_detector_batch(energies, segs, **kw)

        one, many = loop(), batch()                                                    # warm-up of both paths, and the check
        dth = max(abs(a["threshold"] - b["threshold"]) for a, b in zip(one, many))
        same = all(np.array_equal(a["begin"], b["begin"]) and np.array_equal(a["length"], b["length"]) for a, b in zip(one, many))
        assert same and dth < 1e-9, (same, dth)
        t = dict(loop=[], batch=[])
        for _ in range(args.reps):
            for name, fn in (("loop", loop), ("batch", batch)):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); fn(); t[name].append((time.perf_counter() - t0) * 1e3)
                print("  %d frames, %s: %.1f ms" % (frames, name, t[name][-1]), flush=True)
        # the kernels alone, on the resident list
        ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
        xd = torch.from_numpy(np.concatenate(energies).reshape(-1, 1)).cuda()
        runs = np.array([(f * frames, frames, f) for f in range(args.files)], np.int64)
        ctx.energy_detect(xd, runs, args.files, **kw)
        ctx.set_option("timing", 1)
        model, th, st = ctx.energy_train(xd, runs, args.files, **kw)
        k_em = ctx.kernel_ms("k_energy_em")
        ctx.energy_select(xd, runs, args.files, th)
        k_sel = ctx.kernel_ms("k_energy_select")
        ctx.set_option("timing", 0)
        ctx.close()
        med = {k: float(np.median(v)) for k, v in t.items()}
        row = dict(frames=frames, segments_equal=bool(same), max_threshold_difference=float(dth),
                   loop_ms=t["loop"], batch_ms=t["batch"], loop_median_ms=med["loop"], batch_median_ms=med["batch"],
                   loop_spread_ms=max(t["loop"]) - min(t["loop"]), batch_spread_ms=max(t["batch"]) - min(t["batch"]),
                   loop_over_batch=med["loop"] / med["batch"], loop_ms_per_file=med["loop"] / args.files, batch_ms_per_file=med["batch"] / args.files,
                   kernel_ms=dict(k_energy_em=k_em, k_energy_select=k_sel))
        res["lists"].append(row)
        print("%d files x %d frames: loop %.1f ms (spread %.1f), batch %.1f ms (spread %.1f): %.1f x; k_energy_em %.3f ms, k_energy_select %.3f ms" % (
            args.files, frames, med["loop"], row["loop_spread_ms"], med["batch"], row["batch_spread_ms"], row["loop_over_batch"], k_em, k_sel), flush=True)
        assert med["batch"] < med["loop"], "the batch has to beat the loop of the same run"
    out = args.out or next_free("energy_detector.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
