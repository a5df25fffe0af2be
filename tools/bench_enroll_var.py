#!/usr/bin/env python3
"""Enrolment of many clients WITH VARIANCES (TrainTarget with varAdapt true): liagpu::adaptModelBatch with MAPCfg::batchVariances
(gmmiv_em_stats_models + gmmiv_map_adapt_models_full + gmmiv_gmm_batch_load_cov per iteration) against the per-client liagpu::adaptModel
loop on the same inputs in the same process -- the loop is what adaptModelBatch runs for varAdapt without the flag, and is the baseline.

Workloads: --clients x --frames float32 frames of 60 dimensions under a --gaussians x 60 world model, meanAdapt + varAdapt, nbTrainIt 1 (and
whatever --nb-it lists), for every frame count given (default 300 and 3000).  Per workload one CHILD process (this script with --child) under its own time limit, so a step
that hangs ends alone; inside it the features are resident, both paths are warmed, then timed on the host around the whole adaptation
(stream drained before and after), --reps times each, the median is reported.  The kernels' own times come from the context's timers in
one extra pass: for the batch the total of the LAST iteration's launches (all chunks), for the loop the last client's last iteration.
pair rate = clients x frames x Gaussians x iterations / time, next to the EM pass's 126 G pairs/s (10 M frames, README).
Writes one JSON file (default profiles/r15/enroll_var.json); whether the batch beats the loop is recorded per workload ("speedup"), not assumed.  There is no CPU fallback: without a GPU the script fails."""
import argparse
import ctypes as ct
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EM_PASS_GPAIRS = 126.0


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
    out = dict(clients=G, frames=n, gaussians=C, nb_it=args.nb_it, var_adapt=True)
    means, covs = {}, {}
    for which, name in ((0, "batch"), (1, "loop")):
        reps = args.reps + 1
        ms = np.zeros(reps); km = np.zeros(5); m0 = np.empty((C, D)); c0 = np.empty((C, D))
        flags = 1 | 2 | (8 if which == 0 else 0)                                 # meanAdapt, varAdapt; the batch with batchVariances
        rc = h.lib.liagpu_bench_enroll_flags(0, x.ctypes.data_as(ct.POINTER(ct.c_float)), ct.c_long(G * n), D, ct.c_long(G), ct.c_long(n), C, dp(w),
                                             dp(mean), dp(cov), None, args.nb_it, flags, which, reps, ct.c_long(0 if which == 0 else min(G, 20)), dp(ms),
                                             dp(km), dp(m0), dp(c0))
        if rc != 0:
            raise RuntimeError(h.lib.liagpu_last_error().decode())
        t = float(np.median(ms[1:]))
        means[name] = m0; covs[name] = c0
        out[name] = dict(ms=ms[1:].tolist(), warm_ms=float(ms[0]), median_ms=t, clients_per_s=G / (t * 1e-3),
                         gpairs_per_s=G * n * C * args.nb_it / (t * 1e-3) / 1e9, kernel_ms=dict(k_llk_mfma=km[0], k_stats_z=km[1], k_gmm_pack=km[2]))
    out["batch"]["share_of_em_pass_rate"] = out["batch"]["gpairs_per_s"] / EM_PASS_GPAIRS
    out["speedup"] = out["loop"]["median_ms"] / out["batch"]["median_ms"]
    out["batch_beats_loop"] = bool(out["speedup"] > 1.0)
    out["client0_mean_relerr_batch_vs_loop"] = float(np.max(np.abs(means["batch"] - means["loop"])) / np.max(np.abs(means["loop"])))
    out["client0_cov_relerr_batch_vs_loop"] = float(np.max(np.abs(covs["batch"] - covs["loop"])) / np.max(np.abs(covs["loop"])))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=1000)
    ap.add_argument("--frames", type=int, nargs="+", default=[300, 3000])
    ap.add_argument("--gaussians", type=int, default=2048)
    ap.add_argument("--nb-it", type=int, nargs="+", default=[1])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "enroll_var.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        args.frames, args.nb_it = args.frames[0], args.nb_it[0]
        return child(args)
    import torch
    assert torch.cuda.is_available(), "bench_enroll_var needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), em_pass_gpairs_per_s=EM_PASS_GPAIRS, workloads=[])
    for n in args.frames:
        for it in args.nb_it:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--clients", str(args.clients),
                   "--frames", str(n), "--gaussians", str(args.gaussians), "--nb-it", str(it), "--reps", str(args.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:                                  # a step that failed ends the run: nothing more is started on the GPU
                print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
                raise SystemExit("workload %d frames x %d iterations failed (exit %d)" % (n, it, r.returncode))
            w = json.loads(line[0][7:])
            res["workloads"].append(w)
            print("%4d clients x %5d frames, nbTrainIt %d: batch %9.1f ms (%7.1f clients/s, %5.1f G pairs/s = %.2f of the EM pass), loop %9.1f ms "
                  "(%7.1f clients/s): x%.2f; kernels of the last batch iteration: llk %.2f ms, stats %.2f ms, pack %.2f ms"
                  % (w["clients"], n, it, w["batch"]["median_ms"], w["batch"]["clients_per_s"], w["batch"]["gpairs_per_s"], w["batch"]["share_of_em_pass_rate"],
                     w["loop"]["median_ms"], w["loop"]["clients_per_s"], w["speedup"], w["batch"]["kernel_ms"]["k_llk_mfma"],
                     w["batch"]["kernel_ms"]["k_stats_z"], w["batch"]["kernel_ms"]["k_gmm_pack"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
