#!/usr/bin/env python3
"""NormFeat's windowMode on resident frames: gmmiv_feat_norm_window (one launch for the whole list of files) against the per-step
composition of the existing entry points through capi -- gmmiv_frame_moments_groups, gmmiv_frame_moments_stats, a host read-back for
the blend, gmmiv_feat_norm_apply, per window and per file -- timed in the same run.  The reference tool itself cannot run here.

Workload: --files files of --frames frames (default 1000 x 3000 and 1000 x 30000), D = 60 float32, label segments of about 1 s (80 to
120 frames, 0 to 20 frames apart), windowDuration 3 s and 5 s, windowComp 1.
  batch        the planner on the host (host clock), then ONE call with device tables; device events around the call, --reps
               repetitions, every one from the original frames (the restoring copy is not timed); the kernel's own time from the
               context's timer in an extra pass.
  composition  device run tables made once; per step the accumulator is cleared, the three calls are made and mean / std come back
               to the host for the blend.  Host clock around the whole loop, ending in a synchronise.  It runs on the first
               --baseline-files files (default: all at 3000 frames, 100 at 30000) and the time for the whole list is that time scaled
               by the file count -- both numbers are recorded, and which one was measured.
The two results are compared bit for bit on the files the composition ran.  No ratio is a target; the tool records both times.
Writes one JSON file (default profiles/r27/feat_norm_window.json).  There is no CPU fallback: without a GPU the script fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D = 60


def run_table(nfiles, frames, rng):
    runs, first = [], []
    for f in range(nfiles):
        first.append(f * frames)
        p = int(rng.integers(0, 20))
        while True:
            n = int(rng.integers(80, 121))
            if p + n > frames:
                break
            runs.append((f * frames + p, n, f))
            p += n + int(rng.integers(0, 21))
    return np.array(runs, np.int64), np.array(first, np.int64)


def blend(m, s, gm, gs, a):
    na = 1.0 - a
    mp = (a * m) + (na * gm)
    d = mp - gm
    return mp, np.sqrt(((a * s) * s + (na * gs) * gs) + (na * a) * (d * d))


def composition(ctx, torch, x, runs, runs0_d, nfiles, off, st, al):
    """the per-step loop on the files [0, nfiles) -> seconds on the host clock (synchronised)"""
    acc = torch.zeros((1, 2 * D + 1), dtype=torch.float64, device="cuda")
    mean = torch.empty((1, D), dtype=torch.float64, device="cuda")
    std = torch.empty((1, D), dtype=torch.float64, device="cuda")
    bounds = np.searchsorted(runs[:, 2], np.arange(nfiles + 1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f in range(nfiles):
        lo, hi = int(bounds[f]), int(bounds[f + 1])
        if hi == lo:
            continue
        acc.zero_()
        ctx.frame_moments_groups(x, runs0_d[lo:hi], 1, acc)
        ctx.frame_moments_stats(acc, D, mean, std)
        gm, gs = mean.cpu().numpy()[0], std.cpu().numpy()[0]
        for s in range(int(off[f]), int(off[f + 1])):
            wlo, whi, alo, ahi = [int(v) for v in st[s]]
            acc.zero_()
            ctx.frame_moments_groups(x, runs0_d[wlo:whi], 1, acc)
            ctx.frame_moments_stats(acc, D, mean, std)
            mp, sp = blend(mean.cpu().numpy()[0], std.cpu().numpy()[0], gm, gs, float(al[s]))
            ctx.feat_norm_apply(x, runs0_d[alo:ahi], mp[None], sp[None], out=x)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--frames", type=int, nargs="+", default=[3000, 30000])
    ap.add_argument("--windows", type=float, nargs="+", default=[3.0, 5.0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-files", type=int, nargs="+", default=None, help="one count per --frames entry (default: all, then 100)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27", "feat_norm_window.json"))
    args = ap.parse_args()
    import torch
    from lia_ral_amd import capi
    assert torch.cuda.is_available(), "bench_feat_norm_window needs a GPU"
    base_files = args.baseline_files or [args.files if n <= 3000 else min(100, args.files) for n in args.frames]
    assert len(base_files) == len(args.frames)
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = dict(device=torch.cuda.get_device_name(0), files=args.files, D=D, dtype="float32", reps=args.reps, cases=[])
    for frames, nbase in zip(args.frames, base_files):
        rng = np.random.default_rng(frames)
        runs, first = run_table(args.files, frames, rng)
        T = args.files * frames
        g = torch.Generator(device="cuda").manual_seed(frames)
        x0 = torch.empty((T, D), dtype=torch.float32, device="cuda")
        for b in range(0, T, 1 << 22):
            n = min(1 << 22, T - b)
            x0[b:b + n] = torch.randn((n, D), device="cuda", generator=g) * 1.5 + 0.5 + (b / T)
        x = x0.clone()
        runs_d = torch.from_numpy(runs).cuda()
        runs0 = runs.copy()
        runs0[:, 2] = 0
        runs0_d = torch.from_numpy(runs0).cuda()
        for wd in args.windows:
            t0 = time.perf_counter()
            off, st, al = capi.plan_norm_windows(runs, args.files, first, wd, 1.0, 0.01)
            plan_ms = (time.perf_counter() - t0) * 1e3
            off_d, st_d, al_d = torch.from_numpy(off).cuda(), torch.from_numpy(st).cuda(), torch.from_numpy(al).cuda()

            def batch():
                ctx.feat_norm_window(x, runs_d, args.files, off_d, st_d, al_d, stats=False)
            for _ in range(2):                                                       # warm: workspace, code object, clocks
                x.copy_(x0)
                batch()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                x.copy_(x0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); batch(); e1.record(); e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            ctx.set_option("timing", 1)
            x.copy_(x0)
            batch()
            torch.cuda.synchronize()
            kernel_ms = ctx.kernel_ms("k_norm_window")
            ctx.set_option("timing", 0)
            got = x[:nbase * frames].clone()
            # the composition on the first nbase files, once after a warm-up on two files
            x.copy_(x0)
            composition(ctx, torch, x, runs, runs0_d, min(2, nbase), off, st, al)
            x.copy_(x0)
            comp_s = composition(ctx, torch, x, runs, runs0_d, nbase, off, st, al)
            equal = bool(torch.equal(got.view(torch.int32), x[:nbase * frames].view(torch.int32)))
            nbytes = int(runs[:, 1].sum()) * D * 4
            med = float(np.median(ms))
            case = dict(frames_per_file=frames, window_s=wd, runs=int(len(runs)), steps=int(len(al)), selected_frames=int(runs[:, 1].sum()),
                        planner_host_ms=plan_ms, batch_ms=ms, batch_median_ms=med, batch_spread_ms=max(ms) - min(ms), kernel_ms=kernel_ms,
                        needed_bytes=3 * nbytes, batch_tb_per_s_of_needed_bytes=3 * nbytes / (med * 1e-3) / 1e12,
                        composition_files=nbase, composition_measured_ms=comp_s * 1e3, composition_whole_list_ms=comp_s * 1e3 * args.files / nbase,
                        composition_whole_list_is="measured" if nbase == args.files else "scaled from %d files" % nbase,
                        composition_steps=int(off[nbase]), bitwise_equal_on_composition_files=equal)
            res["cases"].append(case)
            print("%d x %d frames, window %g s: %d steps; planner %.1f ms (host); batch %.3f ms median (spread %.3f, kernel %.3f); composition %.1f ms on %d files "
                  "-> %.1f ms for the list (%s); bitwise equal: %s" % (args.files, frames, wd, len(al), plan_ms, med, case["batch_spread_ms"], kernel_ms,
                                                                     comp_s * 1e3, nbase, case["composition_whole_list_ms"], case["composition_whole_list_is"], equal), flush=True)
        del x, x0
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
