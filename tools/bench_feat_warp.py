#!/usr/bin/env python3
"""NormFeat `warp true` on resident frames: gmmiv_feat_warp_hist + gmmiv_feat_warp_apply (one launch each for the whole list of files)
against liagpu::featWarpHost, the compiled host-only twin of the reference's per-file loop (std::sort per column, then warping() loop
for loop: the linear bin searches of ScoreWarp.cpp:168-206 as written), on one core, timed in the same run.  The reference tool itself
cannot run here.

Workload: --files files of --frames frames (default 1000 x 3000 and 1000 x 30000), D = 60 float32, fileMode (a unit per file: its label
segments of 80 to 120 frames, 0 to 20 frames apart), 40 bins, the 700-bin target tests/golden/table_gaussN.histo.
  batch   device tables; device events around the two calls, --reps repetitions, every one from the original frames (the restoring copy
          is not timed); the two kernels' own times from the context's timers in an extra pass, with the bytes each needs (hist reads
          the selected values once; apply reads and writes them once) against the device copy rate measured in the same run.
  twin    featWarpHost on the first --twin-files files (default 8), host clock; the time for the whole list is that time scaled by the
          file count -- both numbers are recorded, and that the second is scaled.
The two results are compared bit for bit on the twin's files.  No ratio is a target; the tool records both times.
Writes one JSON file (default profiles/r30/feat_warp.json).  There is no CPU fallback: without a GPU the script fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, NBIN = 60, 40


def run_table(nfiles, frames, rng):
    runs = []
    for f in range(nfiles):
        p = int(rng.integers(0, 20))
        while True:
            n = int(rng.integers(80, 121))
            if p + n > frames:
                break
            runs.append((f * frames + p, n, f))
            p += n + int(rng.integers(0, 21))
    return np.array(runs, np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--frames", type=int, nargs="+", default=[3000, 30000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--twin-files", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30", "feat_warp.json"))
    args = ap.parse_args()
    import torch
    from lia_ral_amd import capi, feat_warp as fw, host_capi
    assert torch.cuda.is_available(), "bench_feat_warp needs a GPU"
    tb, tc = fw.read_histo(os.path.join(ROOT, "tests", "golden", "table_gaussN.histo"))
    tb_d, tc_d = torch.from_numpy(tb).cuda(), torch.from_numpy(tc).cuda()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = dict(device=torch.cuda.get_device_name(0), files=args.files, D=D, nbin=NBIN, nbin_target=len(tc), dtype="float32", reps=args.reps, cases=[])
    for frames in args.frames:
        rng = np.random.default_rng(frames)
        runs = run_table(args.files, frames, rng)
        U, T = args.files, args.files * frames
        g = torch.Generator(device="cuda").manual_seed(frames)
        x0 = torch.empty((T, D), dtype=torch.float32, device="cuda")
        for b in range(0, T, 1 << 22):
            n = min(1 << 22, T - b)
            x0[b:b + n] = torch.randn((n, D), device="cuda", generator=g) * 1.5 + 0.5 + (b / T)
        x = x0.clone()
        runs_d = torch.from_numpy(runs).cuda()
        bd = torch.empty((U, D, NBIN + 1), dtype=torch.float64, device="cuda")
        cd = torch.empty((U, D, NBIN), dtype=torch.float64, device="cuda")
        sd = torch.empty((U, D), dtype=torch.int32, device="cuda")

        def batch():
            fw.warp_hist(ctx, x, runs_d, U, NBIN, bounds=bd, count=cd, status=sd)
            fw.warp_apply(ctx, x, runs_d, U, bd, cd, sd, tb_d, tc_d)
        for _ in range(2):                                                       # warm: workspace, code object, clocks
            x.copy_(x0)
            batch()
        torch.cuda.synchronize()
        ms, copy_ms = [], []
        for _ in range(args.reps):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(); x.copy_(x0); e1.record(); batch(); e2.record(); e2.synchronize()
            copy_ms.append(e0.elapsed_time(e1))
            ms.append(e1.elapsed_time(e2))
        ctx.set_option("timing", 1)
        x.copy_(x0)
        batch()
        torch.cuda.synchronize()
        hist_ms, apply_ms = ctx.kernel_ms("k_warp_hist"), ctx.kernel_ms("k_warp_apply")
        ctx.set_option("timing", 0)
        nt = min(args.twin_files, args.files)
        got = x[:nt * frames].cpu().numpy()
        xh = x0[:nt * frames].cpu().numpy()
        truns = runs[runs[:, 2] < nt]
        t0 = time.perf_counter()
        want = host_capi.feat_warp_host(xh, truns, nt, (tb, tc), NBIN)[0]
        twin_s = time.perf_counter() - t0
        equal = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        sel = int(runs[:, 1].sum()) * D * 4
        copy_tb = 2 * T * D * 4 / (float(np.median(copy_ms)) * 1e-3) / 1e12
        med = float(np.median(ms))
        case = dict(frames_per_file=frames, runs=int(len(runs)), selected_frames=int(runs[:, 1].sum()), degenerate_columns=int(sd.sum().item()),
                    batch_ms=ms, batch_median_ms=med, batch_spread_ms=max(ms) - min(ms), k_warp_hist_ms=hist_ms, k_warp_apply_ms=apply_ms,
                    hist_needed_bytes=sel, apply_needed_bytes=2 * sel, device_copy_tb_per_s=copy_tb,
                    hist_tb_per_s_of_needed_bytes=sel / (hist_ms * 1e-3) / 1e12, apply_tb_per_s_of_needed_bytes=2 * sel / (apply_ms * 1e-3) / 1e12,
                    twin="liagpu::featWarpHost (compiled, one core)", twin_files=nt, twin_measured_ms=twin_s * 1e3,
                    twin_whole_list_ms=twin_s * 1e3 * args.files / nt, twin_whole_list_is="measured" if nt == args.files else "scaled from %d files" % nt,
                    bitwise_equal_on_twin_files=equal)
        res["cases"].append(case)
        print("%d x %d frames: batch %.3f ms median (spread %.3f; k_warp_hist %.3f, k_warp_apply %.3f; copy rate %.2f TB/s, hist %.3f, apply %.3f TB/s of needed "
              "bytes); twin %.1f ms on %d files -> %.0f ms for the list (%s); bitwise equal: %s"
              % (args.files, frames, med, case["batch_spread_ms"], hist_ms, apply_ms, copy_tb, case["hist_tb_per_s_of_needed_bytes"],
                 case["apply_tb_per_s_of_needed_bytes"], twin_s * 1e3, nt, case["twin_whole_list_ms"], case["twin_whole_list_is"], equal), flush=True)
        del x, x0
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
