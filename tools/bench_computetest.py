#!/usr/bin/env python3
"""ComputeTest over a whole ndx (the GMM-UBM scoring loop): liagpu::computeTestBatch against the per-line liagpu::computeTestLLR loop over
the same lines in the same process -- the loop is the path the library had before gmmiv_llr_trials and is the baseline.

Workloads: --lines test segments of --frames float32 frames of 60 dimensions (default 3000 and 300), every line against --per-line clients
drawn from --models client models of --gaussians x 60 (the world's weights and variances, means moved), topDistribsCount --top, COMPLETE.
Per workload one CHILD process (this script with --child) under its own time limit, so a step that hangs ends alone; inside it the
features and the models are resident (one DeviceMixture per model for the loop, one DeviceMixtureBatch for the batch), both paths are
warmed by one untimed repetition, then timed on the host around the whole scoring (stream drained before and after), --reps times each;
the median is reported, and the spread (max - min) of the loop's repetitions that the batch has to beat.  "batch_upload" is the batch
called with host models: the upload of all models is inside the timed region.  The kernels' own times come from the context's timers in
one extra pass (for the loop: the last line's call).  pair rate = trials x frames / time, next to the 1.05 G frames/s per client model of
k_topc_use4 on long inputs (README).  --pieces runs the batch once more per value of the "trials_piece" knob (the A/B behind
GMMIV_TRIAL_PIECE).  Writes one JSON file (default profiles/r13/computetest_ndx.json).  There is no CPU fallback."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
USE_TOP_GFRAMES = 1.05


def child(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import make_frames, make_gmm
    from lia_ral_amd import host_capi as h
    C, D, L, n, G, per = args.gaussians, 60, args.lines, args.frames, args.models, args.per_line
    w, mean, iv = make_gmm(C, D, seed=0)
    base = make_frames(w, mean, iv, min(L * n, 200000), seed=1)
    x = np.ascontiguousarray(np.resize(base, (L * n, D)))                     # the arithmetic does not care that frames repeat
    rng = np.random.default_rng(2)
    mean_cl = (mean.ravel()[None] + rng.normal(0.0, 0.3, (G, C * D))).astype(np.float64)
    lines = np.stack([rng.choice(G, size=per, replace=False) for _ in range(L)])
    world = (w, mean, 1.0 / iv)
    out = dict(lines=L, frames=n, models=G, clients_per_line=per, gaussians=C, top=args.top, trials=L * per)
    llr = {}
    runs = [("batch", 0, 0), ("loop", 1, 0), ("batch_upload", 2, 0)] + [("piece_%d" % p, 0, p) for p in args.pieces]
    for name, which, piece in runs:
        r = h.bench_computetest(x, world, mean_cl, lines, n, top_c=args.top, complete=True, which=which, reps=args.reps + 1, trial_piece=piece)
        ms = r["ms"]
        t = float(np.median(ms[1:]))
        llr[name] = r["llr"]
        out[name] = dict(ms=ms[1:].tolist(), warm_ms=float(ms[0]), median_ms=t, spread_ms=float(ms[1:].max() - ms[1:].min()), trials_per_s=L * per / (t * 1e-3),
                         gpairs_per_s=L * per * n / (t * 1e-3) / 1e9, kernel_ms=r["kernel_ms"], piece=r["piece"])
    out["batch"]["share_of_use_top_rate"] = out["batch"]["gpairs_per_s"] / USE_TOP_GFRAMES
    out["speedup"] = out["loop"]["median_ms"] / out["batch"]["median_ms"]
    out["batch_below_loop_by_more_than_its_spread"] = bool(out["loop"]["median_ms"] - out["batch"]["median_ms"] > out["loop"]["spread_ms"])
    out["max_abs_llr_batch_minus_loop"] = float(np.max(np.abs(llr["batch"] - llr["loop"])))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1000)
    ap.add_argument("--frames", type=int, nargs="+", default=[3000, 300])
    ap.add_argument("--models", type=int, default=1000)
    ap.add_argument("--per-line", type=int, default=20)
    ap.add_argument("--gaussians", type=int, default=2048)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pieces", type=int, nargs="*", default=[])
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "computetest_ndx.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        args.frames = args.frames[0]
        return child(args)
    import torch
    assert torch.cuda.is_available(), "bench_computetest needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), use_top_gframes_per_s_per_model=USE_TOP_GFRAMES, workloads=[])
    for n in args.frames:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--lines", str(args.lines), "--frames", str(n),
               "--models", str(args.models), "--per-line", str(args.per_line), "--gaussians", str(args.gaussians), "--top", str(args.top), "--reps", str(args.reps),
               "--pieces"] + [str(p) for p in args.pieces]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:                                      # a step that failed ends the run: nothing more is started on the GPU
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            raise SystemExit("workload %d frames failed (exit %d)" % (n, r.returncode))
        w = json.loads(line[0][7:])
        res["workloads"].append(w)
        print("%4d lines x %5d frames x %d clients: batch %8.1f ms (%8.0f trials/s, %5.2f G pairs/s = %.2f of the use-top rate), with upload %8.1f ms, "
              "loop %8.1f ms (spread %.1f ms, %8.0f trials/s, %5.2f G pairs/s): x%.2f; max |dLLR| %.2e; batch kernels: world %.2f + %.2f ms, trials %.2f ms, "
              "reduce %.3f ms" % (w["lines"], n, w["clients_per_line"], w["batch"]["median_ms"], w["batch"]["trials_per_s"], w["batch"]["gpairs_per_s"],
                                   w["batch"]["share_of_use_top_rate"], w["batch_upload"]["median_ms"], w["loop"]["median_ms"], w["loop"]["spread_ms"],
                                   w["loop"]["trials_per_s"], w["loop"]["gpairs_per_s"], w["speedup"], w["max_abs_llr_batch_minus_loop"],
                                   w["batch"]["kernel_ms"]["k_llk_mfma"], w["batch"]["kernel_ms"]["k_topc_rank"], w["batch"]["kernel_ms"]["k_topc_use"],
                                   w["batch"]["kernel_ms"]["k_trial_reduce"]), flush=True)
        for p in args.pieces:
            q = w["piece_%d" % p]
            print("    piece %4d: %8.1f ms, trial kernel %.2f ms" % (p, q["median_ms"], q["kernel_ms"]["k_topc_use"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
