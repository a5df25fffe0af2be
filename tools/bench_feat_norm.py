#!/usr/bin/env python3
"""NormFeat on resident frames: the file-mode pass (gmmiv_frame_moments_groups, gmmiv_frame_moments_stats, gmmiv_feat_norm_apply, each
call timed on its own), the online mode (gmmiv_feat_norm_online), gmmiv_frame_moments over the same buffer and a device-to-device
hipMemcpyAsync of the same bytes, all in one process.

Workload: --sources x --frames x 60 float32 (default 10 000 x 3000 = 7.2 GB) plus one source of --long frames (3 M), one buffer.
Times are device events on the context's stream around one call; every path is warmed, the paths alternate for --reps repetitions, the
median and the min-max spread are reported.  A RATE is the bytes the algorithm needs (one read of x for the moments, one read and one
write for the apply / the online mode / the copy) over the time, given also as a share of (a) the copy's rate in this run and (b), for
the moments kernel, gmmiv_frame_moments' rate.  The kernels' own times come from the context's timers in one extra pass.
A numpy baseline of the same loops on --cpu-sources sources is timed on the host.  Writes one JSON file (default
profiles/r09/feat_norm.json).  There is no CPU fallback: without a GPU the script fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUT = 4096          # the host layer's run length


def numpy_file_mode(x):
    x64 = x.astype(np.float64)
    n = len(x64)
    mean = x64.sum(0) / n
    std = np.sqrt((x64 * x64).sum(0) / n - mean * mean)
    return ((x64 - mean) / std).astype(np.float32)


def numpy_online(x, W, L):
    x64 = x.astype(np.float64)
    n = len(x64)
    L = min(L, W)
    Wp = W - L + n if n < L else W
    head = x64[:min(L, n)]
    m = head.sum(0) / Wp
    c = np.sqrt((head * head).sum(0) / Wp - m * m)
    bw = (Wp - 1.0) / Wp
    out = np.empty_like(x64)
    for k in range(1, n + 1):
        f = x64[k - 1]
        b = 1.0 if k < L else bw
        m = b * m + (1 - b) * f
        c = np.sqrt(c * c * b + (1 - b) * (f * f))
        out[k - 1] = (f - m) / c
    return out.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=10000)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--long", type=int, default=3000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--look-ahead", type=int, default=300)
    ap.add_argument("--cpu-sources", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "feat_norm.json"))
    args = ap.parse_args()
    import torch
    from lia_ral_amd import capi
    assert torch.cuda.is_available(), "bench_feat_norm needs a GPU"

    D = 60
    lens = [args.frames] * args.sources + ([args.long] if args.long > 0 else [])
    fb = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(fb[-1])
    runs = []
    for s, n in enumerate(lens):
        for b in range(0, n, CUT):
            runs.append((fb[s] + b, min(CUT, n - b), s))
    runs = np.array(runs, np.int64)
    ngroups = len(lens)
    g = torch.Generator(device="cuda").manual_seed(1)
    mu = torch.empty(D, device="cuda").uniform_(-3, 3, generator=g)
    sg = torch.empty(D, device="cuda").uniform_(0.5, 2, generator=g)
    x0 = torch.empty((T, D), dtype=torch.float32, device="cuda")
    for b in range(0, T, 1 << 22):
        n = min(1 << 22, T - b)
        x0[b:b + n] = torch.randn((n, D), device="cuda", generator=g) * sg + mu
    x = x0.clone()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    runs_d, fb_d = torch.from_numpy(runs).cuda(), torch.from_numpy(fb).cuda()
    acc = torch.zeros((ngroups, 2 * D + 1), dtype=torch.float64, device="cuda")
    mean = torch.empty((ngroups, D), dtype=torch.float64, device="cuda")
    std = torch.empty((ngroups, D), dtype=torch.float64, device="cuda")
    acc1 = torch.zeros(2 * D + 1, dtype=torch.float64, device="cuda")
    nbytes = T * D * 4

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    paths = {
        "memcpy_d2d": (lambda: x.copy_(x0), 2 * nbytes),                                     # hipMemcpyAsync, device to device
        "frame_moments": (lambda: ctx.frame_moments(x0, acc1), nbytes),
        "moments_groups": (lambda: ctx.frame_moments_groups(x, runs_d, ngroups, acc), nbytes),
        "moments_stats": (lambda: ctx.frame_moments_stats(acc, D, mean, std), ngroups * (4 * D + 1) * 8),
        "norm_apply": (lambda: ctx.feat_norm_apply(x, runs_d, mean, std, out=x), 2 * nbytes),
        "norm_online": (lambda: ctx.feat_norm_online(x, fb_d, args.window, args.look_ahead, out=x), 2 * nbytes),
    }
    order = ["memcpy_d2d", "frame_moments", "moments_groups", "moments_stats", "norm_apply", "memcpy_d2d", "norm_online"]
    for name in order + order:                                                               # warm: workspaces, code objects, clocks
        if name == "moments_groups":
            acc.zero_()
        paths[name][0]()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(args.reps):
        for name in order:                                                                   # every in-place pass starts from x0's values
            if name == "moments_groups":
                acc.zero_()
            times[name].append(timed(paths[name][0]))
    # the kernels alone, from the context's timers
    ctx.set_option("timing", 1)
    kern = {}
    for name, timer in (("moments_groups", "k_moments_groups"), ("moments_stats", "k_moments_stats"), ("norm_apply", "k_feat_norm_apply"),
                        ("norm_online", "k_feat_norm_online"), ("frame_moments", "k_frame_moments")):
        x.copy_(x0); acc.zero_()
        paths[name][0]()
        torch.cuda.synchronize()
        kern[timer] = ctx.kernel_ms(timer)
    ctx.set_option("timing", 0)
    res = dict(device=torch.cuda.get_device_name(0), sources=args.sources, frames=args.frames, long_source=args.long, D=D, total_frames=T,
               buffer_bytes=nbytes, runs=len(runs), groups=ngroups, reps=args.reps, window=args.window, look_ahead=args.look_ahead, paths={},
               kernel_ms=kern)
    med = {k: float(np.median(v)) for k, v in times.items()}
    rate = {k: paths[k][1] / (med[k] * 1e-3) / 1e12 for k in paths}                          # TB/s of needed bytes
    for k in paths:
        res["paths"][k] = dict(ms=times[k], median_ms=med[k], spread_ms=max(times[k]) - min(times[k]), needed_bytes=paths[k][1],
                               tb_per_s=rate[k], share_of_memcpy_rate=rate[k] / rate["memcpy_d2d"])
        print("%-15s %8.3f ms (spread %.3f)  %.2f TB/s of needed bytes  %.2f of the copy's rate" % (k, med[k], res["paths"][k]["spread_ms"], rate[k],
                                                                                                 rate[k] / rate["memcpy_d2d"]), flush=True)
    res["paths"]["moments_groups"]["share_of_frame_moments_rate"] = rate["moments_groups"] / rate["frame_moments"]
    res["file_mode_pass_ms"] = med["moments_groups"] + med["moments_stats"] + med["norm_apply"]
    print("file-mode pass %.3f ms; moments_groups at %.2f of gmmiv_frame_moments' rate; kernel timers %s" % (res["file_mode_pass_ms"],
          res["paths"]["moments_groups"]["share_of_frame_moments_rate"], kern), flush=True)
    # numpy baseline of the same loops, one source at a time like the CPU tool
    ncpu = min(args.cpu_sources, args.sources)
    host = x0[:ncpu * args.frames].cpu().numpy()
    t0 = time.perf_counter()
    for s in range(ncpu):
        numpy_file_mode(host[s * args.frames:(s + 1) * args.frames])
    t1 = time.perf_counter()
    for s in range(ncpu):
        numpy_online(host[s * args.frames:(s + 1) * args.frames], args.window, args.look_ahead)
    t2 = time.perf_counter()
    res["numpy_cpu"] = dict(sources=ncpu, file_mode_s=t1 - t0, online_s=t2 - t1, file_mode_ms_per_source=(t1 - t0) / ncpu * 1e3,
                            online_ms_per_source=(t2 - t1) / ncpu * 1e3)
    print("numpy on %d sources: file mode %.3f s, online %.3f s" % (ncpu, t1 - t0, t2 - t1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
