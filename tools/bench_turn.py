#!/usr/bin/env python3
"""TurnDetection on resident frames: gmmiv_turn_curve / gmmiv_turn_pick / gmmiv_turn_segments on a whole list of files against
  (1) the host twin liagpu::turnDetection (the reference's loop, fp64, one core) on the first --twin-files files, scaled to the list, and
  (2) the composition through the existing entry points -- gmmiv_frame_moments_groups, gmmiv_frame_moments_stats, a model handle,
      gmmiv_llk per window -- on the first --compose-positions positions of the first file, scaled to the list's positions.
Both baselines record what was measured and what is scaled.  The reference tool itself cannot run here.

Workload: --files files of --frames frames (default 1000 x 3000 and 1000 x 30000), D = 60 float32 drawn on the device, one segment per
file, the default windows (winSize 50, winStep 5), DGLR, alpha 0.7.
  batch   the planner on the host (host clock), then the three calls with device tables and device outputs; device events around them,
          the median of --reps repetitions after a warm-up; the curve kernel's own time from the context's timer in an extra pass.
  bound   the bytes the curve kernel needs (every frame once) and the bytes its tiles read (1 + 2 W / (P S) times), over its time, next
          to the HBM rate a float4 copy reaches (6.29 TB/s measured, MI355X); and its log-likelihood evaluations (4 W per position) per
          second.
No ratio is a target; the tool records the times.  Writes one JSON file (default profiles/r28/turn_detection.json).  There is no CPU
fallback: without a GPU the script fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, W, S, ALPHA = 60, 50, 5, 0.7
HBM_COPY_TBS = 6.29


def compose(ctx, capi, torch, x, npos):
    """the criterion of the first npos positions of x through the existing entry points -> (seconds, values)"""
    acc = torch.zeros((1, 2 * D + 1), dtype=torch.float64, device="cuda")
    out = np.zeros(npos)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(npos):
        llk = []
        for b, n in ((k * S, W), (k * S + W, W), (k * S, 2 * W)):
            acc.zero_()
            ctx.frame_moments_groups(x, np.array([[b, n, 0]], np.int64), 1, acc)
            mean, std = ctx.frame_moments_stats(acc, D)
            m, s = mean.cpu().numpy(), std.cpu().numpy()
            g = ctx.gmm(np.ones(1), m, 1.0 / (s * s))
            sums = np.zeros(2)
            g.llk(x[b:b + n], sums=sums)
            g.close()
            llk.append(sums[0])
        out[k] = -(llk[2] - (llk[0] + llk[1]))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--frames", type=int, nargs="+", default=[3000, 30000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--twin-files", type=int, nargs="+", default=[16, 4])
    ap.add_argument("--compose-positions", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28", "turn_detection.json"))
    a = ap.parse_args()
    import torch
    from lia_ral_amd import capi, host_capi
    assert torch.cuda.is_available(), "bench_turn.py needs a GPU"
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    P = capi.turn_tile_positions(D, W, S)
    res = dict(what="TurnDetection on resident frames: curve + pick + segments for a list of files", D=D, winSize=W, winStep=S, alpha=ALPHA, crit="DGLR",
               tile_positions=P, hbm_copy_TBs=HBM_COPY_TBS, cases=[])
    for ci, frames in enumerate(a.frames):
        nf = a.files
        gen = torch.Generator(device="cuda").manual_seed(frames)
        x = torch.randn((nf * frames, D), generator=gen, device="cuda", dtype=torch.float32)
        who = ((torch.arange(nf * frames, device="cuda") // 300) % 2).to(torch.float32)
        x += 2.0 * who[:, None]                                             # two "speakers" that alternate every 300 frames
        runs = np.stack([np.arange(nf) * frames, np.full(nf, frames), np.arange(nf)], 1).astype(np.int64)
        t0 = time.perf_counter()
        po = capi.plan_turn_positions(runs, nf, W, S)
        plan_ms = (time.perf_counter() - t0) * 1e3
        npos = int(po[-1])
        d_runs, d_po = torch.from_numpy(runs).cuda(), torch.from_numpy(po).cuda()
        val = torch.zeros(npos, dtype=torch.float64, device="cuda"); st = torch.zeros(npos, dtype=torch.int32, device="cuda")
        sm = torch.zeros(npos, dtype=torch.float64, device="cuda"); dec = torch.zeros(npos, dtype=torch.uint8, device="cuda")
        rs = torch.zeros((nf, 2), dtype=torch.float64, device="cuda"); nt = torch.zeros(nf, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(nf, dtype=torch.int64, device="cuda")

        def batch():
            ctx.turn_curve(x, d_runs, nf, d_po, W, S, "DGLR", value=val, status=st, npos=npos)
            ctx.turn_pick(val, d_po, ALPHA, sm, dec, rs, nt, npos=npos)
            ctx.turn_segments(d_runs, nf, d_po, dec, W, S, seg_count=cnt, npos=npos)

        batch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); batch(); e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ctx.set_option("timing", 1)
        kms = {}
        ctx.turn_curve(x, d_runs, nf, d_po, W, S, "DGLR", value=val, status=st, npos=npos); kms["k_turn_curve"] = ctx.kernel_ms("k_turn_curve")
        ctx.turn_pick(val, d_po, ALPHA, sm, dec, rs, nt, npos=npos); kms["k_turn_pick"] = ctx.kernel_ms("k_turn_pick")
        ctx.turn_segments(d_runs, nf, d_po, dec, W, S, seg_count=cnt, npos=npos); kms["k_turn_segments"] = ctx.kernel_ms("k_turn_segments")
        ctx.set_option("timing", 0)
        needed = nf * frames * D * 4
        read = needed * (1 + 2 * W / (P * S))
        k = kms["k_turn_curve"] * 1e-3
        # baseline 1: the host twin on the first files
        tf = min(a.twin_files[min(ci, len(a.twin_files) - 1)], nf)
        xh = x[:tf * frames].cpu().numpy()
        segs = [(np.array([0]), np.array([frames]))] * tf
        t0 = time.perf_counter()
        twin = host_capi.turn_detection_batch([xh[f * frames:(f + 1) * frames] for f in range(tf)], segs, twin=True)
        twin_s = time.perf_counter() - t0
        vh = val.cpu().numpy()
        n0 = int(po[1])
        diff = max(float(np.abs(vh[f * n0:(f + 1) * n0] - twin[f]["curves"][0]["value"]).max()) for f in range(tf))
        # baseline 2: the composition on the first positions of the first file
        cp = min(a.compose_positions, n0)
        comp_s, cv = compose(ctx, capi, torch, x[:frames], cp)
        res["cases"].append(dict(
            files=nf, frames_per_file=frames, positions=npos, turns=int(nt.sum().item()), segments=int(cnt.sum().item()), plan_ms=plan_ms,
            batch_ms_median=float(np.median(ms)), batch_ms_all=[float(v) for v in ms], kernel_ms=kms,
            curve_needed_bytes=needed, curve_tile_bytes=read, curve_needed_TBs=needed / k / 1e12, curve_tile_TBs=read / k / 1e12,
            curve_needed_share_of_hbm_copy=needed / k / 1e12 / HBM_COPY_TBS, curve_evaluations_per_s=4.0 * W * npos / k,
            curve_fp64_column_terms_per_s=4.0 * W * npos * D / k,
            host_twin=dict(files_measured=tf, seconds_measured=twin_s, seconds_scaled_to_the_list=twin_s * nf / tf, max_abs_value_difference=diff),
            composition=dict(positions_measured=cp, seconds_measured=comp_s, seconds_scaled_to_the_list=comp_s * npos / cp,
                             max_abs_value_difference=float(np.abs(cv - vh[:cp]).max()))))
        print(json.dumps(res["cases"][-1]))
        del x, val, st, sm, dec
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
