#!/usr/bin/env python3
"""The i-vector scoring rules on trial LISTS (include/gmmiv_iv_trials.h) against the path the library had before them: the dense rule
over all M x S cells, gmmiv_score_apply_trials on a resident flag matrix, then a gather of the listed cells.

One MI355X, M = S = --size (default 100000), dim 400 for Mahalanobis and cosine, rankF 200 for PLDA (three session counts, the models
sorted by them so that the dense rule sees three runs).  Lists:
  uniform:<density>   density x M x S pairs drawn uniformly (a pair may repeat)
  ndx                 every segment against 20 models
  skewed              density 1e-3, 1 % of the models holding half the trials
Vectors, flags and scores are resident.  A path is timed on the host around the whole call with the stream drained before and after --
for the list path that includes the host planner and the upload of its tables -- once as a warm-up, then --reps times; the median is
reported, next to the kernel's own time from the context's timer ("k_score_trials").  bytes per trial are the model of the header,
(1 + 1 / g) ldr 8 with g trials per anchor, and their rate over the kernel time is given as a share of the 6.29 TB/s the device copies at.
--pieces runs the skewed list once more per value of "iv_trials_piece" (the A/B behind GMMIV_IV_TRIAL_PIECE).  The result file
(default profiles/r22/iv_trials.json) is rewritten after every list, so a run that is cut short keeps what it has.  No CPU fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBS = 6.29


def make_list(kind, M, S, rng):
    if kind.startswith("uniform:"):
        n = max(1, int(round(float(kind.split(":")[1]) * M * S)))
        return rng.integers(0, M, n, dtype=np.int32), rng.integers(0, S, n, dtype=np.int32)
    if kind == "ndx":
        return rng.integers(0, M, 20 * S, dtype=np.int32), np.repeat(np.arange(S, dtype=np.int32), 20)
    if kind == "skewed":
        n = max(2, int(round(1e-3 * M * S)))
        hot = max(1, M // 100)
        tm = np.concatenate([rng.integers(0, hot, n // 2, dtype=np.int32), rng.integers(hot, M, n - n // 2, dtype=np.int32)])
        return tm[rng.permutation(n)], rng.integers(0, S, n, dtype=np.int32)
    raise KeyError(kind)


def timed(ctx, fn, reps):
    ms = []
    for _ in range(reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(warm_ms=ms[0], ms=ms[1:], median_ms=float(np.median(ms[1:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=100000)
    ap.add_argument("--lists", nargs="+", default=["uniform:1e-4", "uniform:1e-3", "uniform:1e-2", "uniform:5e-2", "ndx", "skewed"])
    ap.add_argument("--rules", nargs="+", default=["mahalanobis", "cosine", "plda"])
    ap.add_argument("--pieces", type=int, nargs="*", default=[128, 512, 2048])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense path (it needs 9 bytes per cell of device memory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "iv_trials.json"))
    args = ap.parse_args()
    import torch
    from lia_ral_amd import capi
    assert torch.cuda.is_available(), "bench_iv_trials needs a GPU"
    M = S = args.size
    rng = np.random.default_rng(22)
    ctx = capi.Context(0)
    ctx.set_option("timing", 1)
    gen = torch.Generator(device="cuda").manual_seed(1)
    data = {}
    for rule in args.rules:
        dim = 200 if rule == "plda" else 400
        m = torch.randn((dim, M), generator=gen, device="cuda", dtype=torch.float64)
        s = torch.randn((dim, S), generator=gen, device="cuda", dtype=torch.float64)
        A = rng.normal(size=(dim, dim))
        Q = A @ A.T / dim + (np.eye(dim) if rule != "plda" else 0.0)      # Mah (SPD) / FTJF (PSD)
        nsess = np.sort(np.array([1, 3, 5])[rng.integers(0, 3, M)]).astype(np.int64)
        data[rule] = (dim, m, s, Q, nsess)
    torch.cuda.synchronize()

    def list_call(rule, tm, ts, out):
        dim, m, s, Q, nsess = data[rule]
        if rule == "cosine":
            ctx.score_cosine_trials(m, s, tm, ts, out=out)
        elif rule == "mahalanobis":
            ctx.score_mahalanobis_trials(m, s, Q, tm, ts, out=out)
        else:
            ctx.score_plda_trials(m, nsess, s, Q, tm, ts, out=out)

    def dense_call(rule, out):
        dim, m, s, Q, nsess = data[rule]
        if rule == "cosine":
            ctx.score_cosine(m, s, out=out)
        elif rule == "mahalanobis":
            ctx.score_mahalanobis(m, s, Q, out=out)
        else:
            ctx.score_plda(m, nsess, s, Q, out=out)

    result = dict(device=torch.cuda.get_device_name(0), M=M, S=S, reps=args.reps, copy_rate_tbs=COPY_TBS, piece_default=capi.IV_TRIAL_PIECE,
                  timing="host wall time around the call, stream drained before and after; median of reps after one warm-up", lists={})

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)

    dense_buf = None
    if not args.no_dense:
        dense_buf = torch.empty((M, S), dtype=torch.float64, device="cuda")
        flags = torch.zeros(M * S, dtype=torch.uint8, device="cuda")
    for kind in args.lists:
        tm, ts = make_list(kind, M, S, rng)
        n = len(tm)
        g = n / max(1, min(len(np.unique(tm)), len(np.unique(ts))))
        entry = dict(trials=n, density=n / (float(M) * S), trials_per_anchor=g, rules={})
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        idx = None
        if dense_buf is not None:
            idx = torch.from_numpy(tm.astype(np.int64) * S + ts).cuda()
            flags.zero_()
            flags[idx] = 1
            torch.cuda.synchronize()
        for rule in args.rules:
            dim = data[rule][0]
            ldr = dim + (dim & 1)
            r = timed(ctx, lambda: list_call(rule, tm, ts, out), args.reps)
            r["kernel_ms"] = ctx.kernel_ms("k_score_trials")
            if rule != "cosine":                                            # cosine projects nothing
                r["projection_ms"] = ctx.kernel_ms("k_dgemm(score)")
            r["trials_per_s"] = n / (r["median_ms"] * 1e-3)
            r["bytes_per_trial_model"] = (1.0 + 1.0 / g) * ldr * 8
            if r["kernel_ms"] > 0:
                r["kernel_trials_per_s"] = n / (r["kernel_ms"] * 1e-3)
                r["kernel_share_of_copy_rate"] = r["bytes_per_trial_model"] * n / (r["kernel_ms"] * 1e-3) / (COPY_TBS * 1e12)
            e = dict(list=r)
            if dense_buf is not None:
                with torch.cuda.stream(ctx.torch_stream()):
                    def parent():
                        dense_call(rule, dense_buf)
                        ctx.score_apply_trials(flags.view(M, S), dense_buf, 0.0)
                        out.copy_(dense_buf.view(-1)[idx])
                    d = timed(ctx, parent, args.reps)
                d["trials_per_s"] = n / (d["median_ms"] * 1e-3)
                e["dense_then_mask_then_gather"] = d
                e["speedup"] = d["median_ms"] / r["median_ms"]
            entry["rules"][rule] = e
            print(kind, rule, json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "ms"}) for k, v in e.items()}), flush=True)
        if kind == "skewed" and args.pieces:
            ab = {}
            for P in args.pieces:
                ctx.set_option("iv_trials_piece", P)
                r = timed(ctx, lambda: list_call(args.rules[0], tm, ts, out), args.reps)
                ab[str(P)] = dict(median_ms=r["median_ms"], ms=r["ms"], kernel_ms=ctx.kernel_ms("k_score_trials"))
            ctx.set_option("iv_trials_piece", 0)
            entry["piece_ab_" + args.rules[0]] = ab
            print(kind, "pieces", json.dumps(ab), flush=True)
        result["lists"][kind] = entry
        save()
        del out, idx
    # the density at which the two paths cross, per rule: linear between the uniform lists that bracket it
    uni = sorted((v["density"], k) for k, v in result["lists"].items() if k.startswith("uniform:"))
    cross = {}
    for rule in args.rules:
        pts = [(d, result["lists"][k]["rules"][rule]) for d, k in uni if "speedup" in result["lists"][k]["rules"].get(rule, {})]
        where = None
        for (d0, a), (d1, b) in zip(pts, pts[1:]):
            f0 = a["list"]["median_ms"] - a["dense_then_mask_then_gather"]["median_ms"]
            f1 = b["list"]["median_ms"] - b["dense_then_mask_then_gather"]["median_ms"]
            if f0 < 0 <= f1:
                where = d0 + (d1 - d0) * (-f0) / (f1 - f0)
        if pts:
            cross[rule] = where if where is not None else ("above %g" % pts[-1][0] if pts[-1][1]["speedup"] > 1 else "below %g" % pts[0][0])
    result["crossing_density"] = cross
    save()
    print("RESULT " + json.dumps(dict(crossing_density=cross, out=args.out)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
