#!/usr/bin/env python3
"""MLLR enrolment of many clients: liagpu::adaptModelBatch with MAPAlgo "MLLR" (gmmiv_mllr_adapt_models on the device) against the
per-client liagpu::adaptModel loop (computeMLLR on the host) in the same process -- the loop is the baseline -- and the batched
"MAPOccDep" time at the same shape alongside.

Workloads: --clients x --frames float32 frames of 60 dimensions under a --gaussians x 60 world model, nbTrainIt 1 and 5, for every
frame count given (default 3000 and 300).  Per workload one CHILD process (this script with --child) under its own time limit, so a
step that hangs ends alone.  Inside it the features are resident, each path is warmed once and timed on the host around the whole
adaptation (stream drained before and after), --reps times, median reported.  The loop spends a few tenths of a second of host
arithmetic per client and iteration, so it is timed on --loop-clients clients (default 8) and reported per client; the batch runs all
of them.  Kernel times are the context's timers in one extra pass: the total of the LAST iteration's launches.  k_mllr_solve is set
against the floor derived in DESIGN.md section 3.15 (lower-triangle tiles x k-steps x 2048 FLOP x D per client at the fp64 matrix peak).
Writes one JSON file (default profiles/r11/mllr.json).  There is no CPU fallback: without a GPU the script fails."""
import argparse
import ctypes as ct
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP64_MATRIX_PEAK_TFLOPS = 78.6


def floor_ms(G, C, D):
    nt = (D + 2 + 15) // 16
    return nt * (nt + 1) // 2 * ((C + 3) // 4) * 2048.0 * D * G / (FP64_MATRIX_PEAK_TFLOPS * 1e12) * 1e3


def child(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import make_frames, make_gmm
    from lia_ral_amd import host_capi as h
    C, D, G, n = args.gaussians, 60, args.clients, args.frames
    w, mean, iv = make_gmm(C, D, seed=0)
    base = make_frames(w, mean, iv, min(G * n, 200000), seed=1)
    x = np.ascontiguousarray(np.resize(base, (G * n, D)))                     # the arithmetic does not care that frames repeat
    cov = 1.0 / iv
    dp = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_double))
    out = dict(clients=G, frames=n, gaussians=C, nb_it=args.nb_it, k_mllr_solve_floor_ms=floor_ms(G, C, D))
    means = {}
    for name, method, which, ncl in (("mllr_batch", b"MLLR", 0, G), ("mllr_loop", b"MLLR", 1, min(G, args.loop_clients)), ("map_batch", b"MAPOccDep", 0, G)):
        reps = (args.reps if which == 0 else 1) + 1
        ms = np.zeros(reps); km = np.zeros(5); m0 = np.empty((C, D))
        rc = h.lib.liagpu_bench_enroll_method(0, x.ctypes.data_as(ct.POINTER(ct.c_float)), ct.c_long(G * n), D, ct.c_long(ncl), ct.c_long(n), C, dp(w),
                                              dp(mean), dp(cov), method, args.nb_it, which, reps, ct.c_long(0 if which == 0 else 2), dp(ms), dp(km), dp(m0))
        if rc != 0:
            raise RuntimeError(h.lib.liagpu_last_error().decode())
        t = float(np.median(ms[1:]))
        means[name] = m0
        out[name] = dict(clients=ncl, ms=ms[1:].tolist(), warm_ms=float(ms[0]), median_ms=t, ms_per_client=t / ncl,
                         kernel_ms=dict(k_llk_mfma=km[0], k_stats_z=km[1], k_gmm_pack=km[2], k_mllr_solve=km[3], k_mllr_pack=km[4]))
    ks = out["mllr_batch"]["kernel_ms"]["k_mllr_solve"]
    out["k_mllr_solve_floor_fraction"] = out["k_mllr_solve_floor_ms"] / ks if ks > 0 else None
    out["speedup_per_client"] = out["mllr_loop"]["ms_per_client"] / out["mllr_batch"]["ms_per_client"]
    out["client0_mean_relerr_batch_vs_loop"] = float(np.max(np.abs(means["mllr_batch"] - means["mllr_loop"])) / np.max(np.abs(means["mllr_loop"])))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=1000)
    ap.add_argument("--loop-clients", type=int, default=8)
    ap.add_argument("--frames", type=int, nargs="+", default=[3000, 300])
    ap.add_argument("--gaussians", type=int, default=2048)
    ap.add_argument("--nb-it", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "mllr.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        args.frames, args.nb_it = args.frames[0], args.nb_it[0]
        return child(args)
    import torch
    assert torch.cuda.is_available(), "bench_mllr needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), fp64_matrix_peak_tflops=FP64_MATRIX_PEAK_TFLOPS, workloads=[])
    for n in args.frames:
        for it in args.nb_it:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--clients", str(args.clients),
                   "--loop-clients", str(args.loop_clients), "--frames", str(n), "--gaussians", str(args.gaussians), "--nb-it", str(it), "--reps", str(args.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:                                  # a step that failed ends the run: nothing more is started on the GPU
                print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
                raise SystemExit("workload %d frames x %d iterations failed (exit %d)" % (n, it, r.returncode))
            w = json.loads(line[0][7:])
            res["workloads"].append(w)
            print("%4d clients x %5d frames, nbTrainIt %d: MLLR batch %9.1f ms (%.3f ms / client), loop %.1f ms / client (on %d clients): x%.1f; MAPOccDep batch "
                  "%9.1f ms; last iteration: k_mllr_solve %.2f ms (floor %.2f ms: %.2f of it), k_mllr_pack %.3f ms, llk %.2f ms, stats %.2f ms"
                  % (w["clients"], n, it, w["mllr_batch"]["median_ms"], w["mllr_batch"]["ms_per_client"], w["mllr_loop"]["ms_per_client"], w["mllr_loop"]["clients"],
                     w["speedup_per_client"], w["map_batch"]["median_ms"], w["mllr_batch"]["kernel_ms"]["k_mllr_solve"], w["k_mllr_solve_floor_ms"],
                     w["k_mllr_solve_floor_fraction"] or 0.0, w["mllr_batch"]["kernel_ms"]["k_mllr_pack"], w["mllr_batch"]["kernel_ms"]["k_llk_mfma"],
                     w["mllr_batch"]["kernel_ms"]["k_stats_z"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
