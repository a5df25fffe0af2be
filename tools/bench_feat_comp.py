#!/usr/bin/env python3
"""Feature-domain channel compensation on resident frames: gmmiv_feat_compensate (a) against the composition a caller had before it
from unchanged entry points (b): gmmiv_occ into a device chunk of 65 536 frames, torch.matmul with the offsets, a subtraction.

One process, 2048 x 60, resident float32 frames (10^6, and 10^7 with --big).  Both paths are warmed, then (a) and (b) ALTERNATE for
--reps repetitions each inside the same run; the median and the min-max spread of each are reported, per output variant (out of place
f32 / f64, in place).  Times are device events on the context's stream around the whole call(s).  The kernel split comes from the
context's timers in one extra, untimed-by-the-clock pass.  Writes one JSON file (default profiles/r08/feat_comp.json)."""
import argparse
import ctypes as ct
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TF = 78.6            # fp64 matrix = fp64 vector peak of the MI355X
FLOP_PER_PAIR = 360       # 240 (logit pass) + 2 D (posterior x offset contraction) at D = 60
OCC_CHUNK = 65536


def device_frames(torch, w, mean, iv, T, seed):
    """frames drawn like conftest.make_frames, on the device (10^7 x 60 on the host would take minutes)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    wd, md, sd = (torch.from_numpy(a).cuda() for a in (w, mean, 1.0 / np.sqrt(iv)))
    x = torch.empty((T, mean.shape[1]), dtype=torch.float32, device="cuda")
    for b in range(0, T, 1 << 20):
        n = min(1 << 20, T - b)
        comp = torch.multinomial(wd, n, replacement=True, generator=g)
        x[b:b + n] = (md[comp] + torch.randn((n, mean.shape[1]), dtype=torch.float64, device="cuda", generator=g) * sd[comp]).float()
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--big", action="store_true", help="also 10^7 frames")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "feat_comp.json"))
    args = ap.parse_args()
    import torch
    from conftest import make_gmm
    from lia_ral_amd import capi

    C, D = 2048, 60
    w, mean, iv = make_gmm(C, D, seed=0, spread=0.1)
    off_h = np.random.default_rng(7).normal(0.0, 0.3, (C, D))
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    g = ctx.gmm(w, mean, iv)
    off = torch.from_numpy(off_h).cuda()
    gam = torch.empty((OCC_CHUNK, C), dtype=torch.float64, device="cuda")
    nct = ((C + 15) // 16 + 1) // 2 * 2
    z_bytes = nct * 16 * 8 + nct // 2 * 4 + 8 + 4 + 8          # likelihoods, exponents, 1 / S, Efin, log-sum: written once, read once
    result = dict(device=torch.cuda.get_device_name(0), C=C, D=D, reps=args.reps, occ_chunk=OCC_CHUNK, peak_tf=PEAK_TF,
                  flop_per_pair=FLOP_PER_PAIR, runs=[])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    for T in [args.frames] + ([10000000] if args.big else []):
        x0 = device_frames(torch, w, mean, iv, T, seed=1)
        x = x0.clone()
        for name, odt, in_place in (("f32_to_f32", torch.float32, False), ("f32_to_f64", torch.float64, False), ("f32_in_place", torch.float32, True)):
            out = x if in_place else torch.empty((T, D), dtype=odt, device="cuda")

            def path_a():
                g.feat_compensate(x, off, out=out)

            def path_b():
                for b in range(0, T, OCC_CHUNK):
                    n = min(OCC_CHUNK, T - b)
                    xb = x[b:b + n]
                    capi._chk(capi.lib.gmmiv_occ(ctx._h, g._h, capi._ptr(xb), capi.F32, ct.c_int64(n), ct.c_int64(D), capi._ptr(gam)))
                    p = torch.matmul(gam[:n], off)
                    out[b:b + n] = (xb.double() - p).to(odt)

            def restore():
                if in_place:
                    x.copy_(x0)
            for fn in (path_a, path_b, path_a, path_b):               # warm both: workspaces, GEMM selection, clocks
                restore(); fn()
            torch.cuda.synchronize()
            ta, tb = [], []
            for _ in range(args.reps):
                restore(); ta.append(timed(path_a))
                restore(); tb.append(timed(path_b))
            # agreement of the two paths on this data (f64 output: a few ulps of the sums; f32: one rounding)
            restore(); path_a(); ra = out.clone() if in_place else out.double().clone()
            restore(); path_b(); rb = out.double()
            max_diff = float((ra.double() - rb).abs().max())
            del ra, rb
            # kernel split from the context's timers (events around every launch: not part of the timed repetitions)
            ctx.set_option("timing", 1)
            restore(); path_a(); torch.cuda.synchronize()
            k_llk, k_comp = ctx.kernel_ms("k_llk_mfma"), ctx.kernel_ms("k_feat_comp")
            launches = ctx.kernel_launches("k_feat_comp")
            ctx.set_option("timing", 0)
            restore()
            med_a, med_b = float(np.median(ta)), float(np.median(tb))
            spread_a, spread_b = max(ta) - min(ta), max(tb) - min(tb)
            es_o = 8 if odt == torch.float64 else 4
            bytes_a = 3 * D * 4 + 2 * z_bytes + D * es_o                # x read by the count, the logit pass and k_feat_comp; out written
            bytes_b = bytes_a + 2 * C * 8 + 2 * D * 8 + D * 4           # + a posterior row written and read back, P written and read, x read again
            pairs = T * C
            run = dict(frames=T, variant=name, a_ms=ta, b_ms=tb, a_median_ms=med_a, b_median_ms=med_b, a_spread_ms=spread_a, b_spread_ms=spread_b,
                       ratio_a_over_b=med_a / med_b, a_below_b_by_more_than_spread=bool(med_b - med_a > max(spread_a, spread_b)),
                       a_gpairs_per_s=pairs / med_a / 1e6, b_gpairs_per_s=pairs / med_b / 1e6,
                       a_fraction_of_peak=pairs / (med_a * 1e-3) * FLOP_PER_PAIR / (PEAK_TF * 1e12),
                       k_llk_mfma_ms=k_llk, k_feat_comp_ms=k_comp, k_feat_comp_launches=launches,
                       k_feat_comp_gpairs_per_s=pairs / k_comp / 1e6 if k_comp > 0 else None,
                       k_feat_comp_fraction_of_peak=pairs / (k_comp * 1e-3) * 2 * D / (PEAK_TF * 1e12) if k_comp > 0 else None,
                       bytes_per_frame_a=bytes_a, bytes_per_frame_b=bytes_b, max_abs_diff_a_vs_b=max_diff)
            result["runs"].append(run)
            print("T %d %-12s a %.2f ms (spread %.2f)  b %.2f ms (spread %.2f)  a/b %.3f  | k_llk_mfma %.2f + k_feat_comp %.2f ms | %.1f G pairs/s, %.1f %% of peak | max |a - b| %.2e"
                  % (T, name, med_a, spread_a, med_b, spread_b, med_a / med_b, k_llk, k_comp, run["a_gpairs_per_s"], 100 * run["a_fraction_of_peak"], max_diff), flush=True)
            if not in_place:
                del out
        del x, x0
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
