"""Model-based feature compensation on resident frames (include/gmmiv.h: gmmiv_feat_compensate, gmmiv_feat_map, gmmiv_scatter_runs).

The reference of the compensation is written here as the reference runs (JFAAcc::normalizeFeatures, AccumulateJFAStat.cpp:4653-4675):
the linear-domain posteriors of the oracle, then the sequential `ff[i] -= P[k] * ux[k * D + i]` over k in fp64.  The bound is per
element, with no flat tolerance:

    |out - ref| <= 1e-12 sum_c |offset[c, i]| + 2 (C + 1) 2^-53 (|x_ti| + sum_c gamma_tc |offset[c, i]|)   (+ one f32 ulp for an f32 output)

the first term being the project's posterior tolerance (test_posterior_vectors_match_oracle), the second two summation orders.
Models come from make_gmm(spread=0.1): with the default spread the posteriors are one-hot and the contraction shows nothing."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import make_frames, make_gmm  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(2048, 60, 300), (128, 60, 500), (37, 13, 65), (512, 1, 200), (300, 80, 64), (64, 100, 33)]
_CASES = {}


def case(C, D, T):
    """model, frames (float32 values; the float64 frames are the same numbers), offsets, oracle posteriors and the reference -- once"""
    key = (C, D, T)
    if key not in _CASES:
        from oracle import oracle as orc
        w, mean, iv = make_gmm(C, D, seed=11 + C, spread=0.1)
        x32 = make_frames(w, mean, iv, T, seed=5 + D)
        x64 = x32.astype(np.float64)
        off = np.random.default_rng(C * 1000 + D).normal(0.0, 0.3, (C, D))
        og = orc.Gmm(w, mean, iv)
        P = orc.occ(og, x64)
        ref = x64.copy()
        for k in range(C):                                        # the reference's loop order: Gaussians outside, sequential in fp64
            ref -= P[:, k:k + 1] * off[k]
        llk = orc.llk(og, x64, -1e9, 1e9)
        bound = 1e-12 * np.abs(off).sum(0)[None, :] + 2.0 * (C + 1) * 2.0 ** -53 * (np.abs(x64) + P @ np.abs(off))
        _CASES[key] = dict(w=w, mean=mean, iv=iv, x32=x32, x64=x64, off=off, P=P, ref=ref, llk=llk, bound=bound)
        for a in _CASES[key].values():
            a.setflags(write=False)
    return _CASES[key]


def check(out, cs, what):
    out = np.asarray(out)
    bound = cs["bound"] + (np.spacing(np.abs(cs["ref"]).astype(np.float32)).astype(np.float64) if out.dtype == np.float32 else 0.0)
    err = np.abs(out.astype(np.float64) - cs["ref"])
    worst = np.max(err / bound)
    print("%s: max |out - ref| / bound = %.3g (max err %.3g)" % (what, worst, err.max()))
    assert np.all(err <= bound), (what, worst)


def padded(a, extra):
    """a copy of `a` inside a wider matrix: rows keep a stride of D + extra elements; the padding holds a sentinel"""
    wide = np.full((a.shape[0], a.shape[1] + extra), -77.0, a.dtype)
    wide[:, :a.shape[1]] = a
    return wide


def run_variants(ctx, g, cs, tag):
    import torch
    D = cs["x32"].shape[1]
    off = cs["off"]
    # 1. host f32 -> f32, compact
    check(g.feat_compensate(cs["x32"].copy(), off), cs, tag + " host f32->f32")
    # 2. host f64 -> f64, ldx and ldo > D
    xw, ow = padded(cs["x64"], 3), np.full((len(cs["x64"]), D + 5), -77.0)
    g.feat_compensate(xw[:, :D], off, out=ow[:, :D])
    check(ow[:, :D], cs, tag + " host f64->f64 strided")
    assert np.all(ow[:, D:] == -77.0) and np.array_equal(xw[:, :D], cs["x64"])
    # 3. device f32 -> f64, ldx > D, device offsets
    xd = torch.from_numpy(padded(cs["x32"], 4)).cuda()
    o = g.feat_compensate(xd[:, :D], torch.from_numpy(off.copy()).cuda(), out_dtype=1)
    check(o.cpu().numpy(), cs, tag + " device f32->f64")
    # 4. device f64 -> f32, ldo > D
    od = torch.full((len(cs["x64"]), D + 2), -77.0, dtype=torch.float32, device="cuda")
    g.feat_compensate(torch.from_numpy(cs["x64"].copy()).cuda(), off, out=od[:, :D])
    check(od[:, :D].cpu().numpy(), cs, tag + " device f64->f32 strided")
    assert bool((od[:, D:] == -77.0).all())
    # 5. device f32 in place, ld > D
    g.feat_compensate(xd[:, :D], off, out=xd[:, :D])
    check(xd[:, :D].cpu().numpy(), cs, tag + " device f32 in place")
    assert bool((xd[:, D:] == -77.0).all())
    # 6. host f64 in place
    xh = cs["x64"].copy()
    g.feat_compensate(xh, off, out=xh)
    check(xh, cs, tag + " host f64 in place")


def test_inputs_exercise_the_contraction():
    """spread 0.1: many Gaussians share every frame (one-hot posteriors would make the test vacuous), and no frame of the reference
    has likelihood 0"""
    cs = case(2048, 60, 300)
    neff = 1.0 / (cs["P"] ** 2).sum(1)
    print("median effective Gaussian count %.1f, min llk %.1f" % (np.median(neff), cs["llk"].min()))
    assert np.median(neff) >= 4.0
    for C, D, T in SHAPES:
        c = case(C, D, T)
        assert c["llk"].min() > -745.0 and np.all(np.isfinite(c["P"])) and np.max(np.abs(c["P"].sum(1) - 1.0)) < 1e-9


@pytest.mark.parametrize("stats_z", [1, 0])
@pytest.mark.parametrize("C,D,T", SHAPES)
def test_compensation_matches_the_reference_loop(C, D, T, stats_z):
    import torch
    from lia_ral_amd import capi
    cs = case(C, D, T)
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_option("stats_z", stats_z); ctx.set_option("timing", 1)
    g = ctx.gmm(cs["w"], cs["mean"], cs["iv"])
    run_variants(ctx, g, cs, "C%d D%d T%d stats_z %d" % (C, D, T, stats_z))
    fast = stats_z == 1 and D <= 60
    assert (ctx.kernel_launches("k_feat_comp") > 0) == fast, "the path taken is not the one the shape calls for"
    assert ctx.set_option("zero_llk_frames", 0) == 0
    # T = 0 is valid and touches nothing
    e = np.full((0, D), 1.0)
    assert g.feat_compensate(e, cs["off"]).shape == (0, D)
    g.close(); ctx.close()


def test_a_call_that_crosses_a_scratch_chunk():
    """z_scratch_mb 4 at 37 x 13: chunks of 6464 frames, so 7000 frames are two launches of each kernel; the second chunk's frames
    come out like the first's (bitwise: rows are compared with a one-chunk call of the default budget)"""
    import torch
    from lia_ral_amd import capi
    C, D, T = 37, 13, 7000
    cs = case(C, D, T)
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_option("timing", 1)
    g = ctx.gmm(cs["w"], cs["mean"], cs["iv"])
    one = g.feat_compensate(torch.from_numpy(cs["x32"].copy()).cuda(), cs["off"], out_dtype=1).cpu().numpy()
    assert ctx.kernel_launches("k_feat_comp") == 1
    ctx.set_option("z_scratch_mb", 4)
    xd = torch.from_numpy(cs["x32"].copy()).cuda()
    two = g.feat_compensate(xd, cs["off"], out_dtype=1).cpu().numpy()
    assert ctx.kernel_launches("k_feat_comp") == 2 and ctx.kernel_launches("k_llk_mfma") == 2
    check(two, cs, "two chunks")
    assert np.array_equal(one, two)
    g.feat_compensate(xd, cs["off"], out=xd)                      # in place across the chunk boundary
    check(xd.cpu().numpy(), cs, "two chunks, in place")
    g.close(); ctx.close()


@pytest.mark.parametrize("stats_z", [1, 0])
def test_a_frame_does_not_depend_on_its_position_or_neighbours(stats_z):
    import torch
    from lia_ral_amd import capi
    cs = case(128, 60, 500)
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_option("stats_z", stats_z)
    g = ctx.gmm(cs["w"], cs["mean"], cs["iv"])
    x = cs["x64"]
    a = g.feat_compensate(x.copy(), cs["off"])
    b = g.feat_compensate(x.copy(), cs["off"])
    assert np.array_equal(a, b)                                   # two runs
    perm = np.random.default_rng(3).permutation(len(x))
    p = g.feat_compensate(np.ascontiguousarray(x[perm]), cs["off"])
    assert np.array_equal(p, a[perm])                             # a permutation of the frames
    for t in (0, 17, 255, 256, 499):
        alone = g.feat_compensate(np.ascontiguousarray(x[t:t + 1]), cs["off"])
        assert np.array_equal(alone[0], a[t]), t                  # a frame alone against the same frame inside the batch
    g.close(); ctx.close()


@pytest.mark.parametrize("stats_z", [1, 0])
def test_zero_likelihood_frames_are_copied_through_and_counted(stats_z):
    import torch
    from lia_ral_amd import capi
    cs = case(128, 60, 500)
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_option("stats_z", stats_z)
    g = ctx.gmm(cs["w"], cs["mean"], cs["iv"])
    x = cs["x64"].copy()
    x[7, 3] = np.nan                                              # kind (1)
    x[300] = 1.0e4                                                # kind (2): at distance 1e4 from every mean
    x[499, 0] = np.inf                                            # kind (1), last frame
    bad = [7, 300, 499]
    ctx.set_option("zero_llk_frames", 0); ctx.set_option("screened_frames", 0)
    for out in (g.feat_compensate(x.copy(), cs["off"]), g.feat_compensate(torch.from_numpy(x).cuda(), cs["off"], out_dtype=0).cpu().numpy()):
        want = x if out.dtype == np.float64 else x.astype(np.float32)
        assert np.array_equal(out[bad], want[bad], equal_nan=True)
        good = np.setdiff1d(np.arange(len(x)), bad)
        bound = cs["bound"][good] + (np.spacing(np.abs(cs["ref"][good]).astype(np.float32)).astype(np.float64) if out.dtype == np.float32 else 0.0)
        assert np.all(np.abs(out[good].astype(np.float64) - cs["ref"][good]) <= bound)  # the neighbours are unaffected
    assert ctx.set_option("zero_llk_frames", 0) == 2 * len(bad)
    assert ctx.set_option("screened_frames", 0) == 2 * 2
    g.close(); ctx.close()


def test_argument_errors_come_before_any_work():
    import torch
    from lia_ral_amd import capi
    cs = case(37, 13, 65)
    D = 13
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    g = ctx.gmm(cs["w"], cs["mean"], cs["iv"])
    xd = torch.from_numpy(cs["x64"].copy()).cuda()
    keep = xd.clone()
    off = torch.from_numpy(cs["off"].copy()).cuda()
    L = capi.lib

    def comp(x, xdt, ldx, out, odt, ldo, T=65):
        return L.gmmiv_feat_compensate(ctx._h, g._h, ct.c_void_p(x), xdt, ct.c_int64(T), ct.c_int64(ldx), capi._ptr(off), ct.c_void_p(out), odt, ct.c_int64(ldo))
    base = xd.data_ptr()
    assert comp(base, 1, D, base + 8, 1, D) == -1 and b"overlaps" in L.gmmiv_last_error()          # shifted by one element
    assert comp(base, 1, D, base + 8 * D * 10, 1, D) == -1                                          # shifted by ten frames
    assert comp(base, 1, D, base, 0, D) == -1                                                        # same pointer, other dtype
    assert comp(base, 1, D, base, 1, D + 1, T=30) == -1                                              # same pointer, other stride
    assert comp(base, 2, D, base, 1, D) == -1 and b"dtype" in L.gmmiv_last_error()
    assert comp(base, 1, D, base, 7, D) == -1
    assert comp(base, 1, D - 1, base, 1, D) == -1 and comp(base, 1, D, base, 1, D, T=-1) == -1
    assert L.gmmiv_feat_compensate(ctx._h, g._h, ct.c_void_p(base), 1, ct.c_int64(65), ct.c_int64(D), None, ct.c_void_p(base), 1, ct.c_int64(D)) == -1
    torch.cuda.synchronize()
    assert torch.equal(xd, keep)
    tabs = [capi._ptr(off)] * 4
    assert L.gmmiv_feat_map(ctx._h, g._h, *tabs, ct.c_void_p(base), 1, ct.c_int64(65), ct.c_int64(D), ct.c_void_p(base + 8), 1, ct.c_int64(D), None) == -1
    assert L.gmmiv_feat_map(ctx._h, g._h, *tabs, ct.c_void_p(base), 3, ct.c_int64(65), ct.c_int64(D), ct.c_void_p(base), 1, ct.c_int64(D), None) == -1
    assert torch.equal(xd, keep)
    g.close(); ctx.close()


def test_device_pointers_only_enqueue():
    """the stream is kept busy by a spin kernel (the pattern of tests/test_gpu_degenerate.py): the compensation behind it returns at once"""
    import time
    import torch
    from lia_ral_amd import capi
    cs = case(128, 60, 500)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ctx = capi.Context(0, s.cuda_stream)
        g = ctx.gmm(cs["w"], cs["mean"], cs["iv"])
        x = cs["x32"].copy(); x[5, 5] = np.nan
        xd = torch.from_numpy(x).cuda()
        off = torch.from_numpy(cs["off"].copy()).cuda()
        out = torch.empty((500, 60), dtype=torch.float64, device="cuda")
        g.feat_compensate(xd, off, out=out)
        torch.cuda.synchronize()                                  # warm-up: the workspaces exist now
        out.zero_()
        torch.cuda._sleep(int(2.0e9))
        t0 = time.perf_counter()
        g.feat_compensate(xd, off, out=out)
        dt = time.perf_counter() - t0
        still_busy = not s.query()
        torch.cuda.synchronize()
        assert still_busy and dt < 0.25, (still_busy, dt)
        o = out.cpu().numpy()
        good = np.setdiff1d(np.arange(500), [5])
        assert np.all(np.abs(o[good] - cs["ref"][good]) <= cs["bound"][good])
        assert np.array_equal(o[5], x[5].astype(np.float64), equal_nan=True)
        g.close(); ctx.close()


@pytest.mark.parametrize("C,D,T", [(128, 60, 500), (37, 13, 65), (64, 100, 33)])
def test_feature_mapping_through_the_best_gaussian(C, D, T):
    """best is the oracle's top-1; the f64 output is numpy's sqrt(ci / cd) * (x - m) + M on those indices, bit for bit (five rounded
    operations, no fused multiply-add); a frame whose every term is 0 maps through Gaussian 0; a NaN stays where it is"""
    import torch
    from lia_ral_amd import capi
    from oracle import oracle as orc
    cs = case(C, D, T)
    rng = np.random.default_rng(C + D)
    cd_mean, cd_cov = cs["mean"], 1.0 / cs["iv"]
    ci_mean = cd_mean + rng.normal(0.0, 0.2, (C, D))
    ci_cov = cd_cov * np.exp(rng.normal(0.0, 0.3, (C, D)))
    x = cs["x64"].copy()
    x[3] = 1.0e4                                                  # every term underflows to 0: index 0
    x[9, D - 1] = np.nan
    best_ref = orc.llk_determine_top(orc.Gmm(cs["w"], cs["mean"], cs["iv"]), x[np.arange(T) != 9], 1, True)["idx"][:, 0]
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    g = ctx.gmm(cs["w"], cs["mean"], cs["iv"])

    def expect(xx, b):
        return np.sqrt(ci_cov[b] / cd_cov[b]) * (xx - cd_mean[b]) + ci_mean[b]
    out, best = g.feat_map(cd_mean, cd_cov, ci_mean, ci_cov, x.copy())
    assert best.dtype == np.int32 and best[3] == 0 and best[9] == 0
    assert np.array_equal(best[np.arange(T) != 9], best_ref)
    assert np.array_equal(out, expect(x, best), equal_nan=True) and np.isnan(out[9, D - 1]) and not np.isnan(out[9, :D - 1]).any()
    # device, f32 in / f32 out in place with a row stride, no index output
    xw = torch.from_numpy(padded(x.astype(np.float32), 3)).cuda()
    o2, b2 = g.feat_map(cd_mean, cd_cov, ci_mean, ci_cov, xw[:, :D], out=xw[:, :D], best=False)
    assert b2 is None and bool((xw[:, D:] == -77.0).all())
    x32 = x.astype(np.float32).astype(np.float64)
    b32 = orc.llk_determine_top(orc.Gmm(cs["w"], cs["mean"], cs["iv"]), x32[np.arange(T) != 9], 1, True)["idx"][:, 0]
    bb = np.zeros(T, np.int64); bb[np.arange(T) != 9] = b32
    assert np.array_equal(xw[:, :D].cpu().numpy(), expect(x32, bb).astype(np.float32), equal_nan=True)
    # device tables and a device index output
    xd = torch.from_numpy(x).cuda()
    o3, b3 = g.feat_map(*[torch.from_numpy(np.array(a)).cuda() for a in (cd_mean, cd_cov, ci_mean, ci_cov)], xd)
    assert np.array_equal(b3.cpu().numpy(), best) and np.array_equal(o3.cpu().numpy(), out, equal_nan=True)
    g.close(); ctx.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_scatter_runs_inverts_gather_runs(dtype):
    import torch
    from lia_ral_amd import capi
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(8)
    T, D = 1000, 13
    x = rng.normal(size=(T, D + 3)).astype(dtype)
    runs = np.array([[5, 0, 3], [100, 3, 64], [164, 67, 10], [990, 77, 10], [400, 87, 1]], np.int64)
    nsel = int(runs[:, 2].sum())
    for ld in (D, D + 3):
        xd = torch.from_numpy(np.ascontiguousarray(x[:, :ld])).cuda()
        view = xd[:, :D]
        sel = torch.empty((nsel, D), dtype=xd.dtype, device="cuda")
        ctx.gather_runs(view, runs, sel)
        before = xd.clone()
        xd[:, :D] = 0
        keep = xd.clone()
        ctx.scatter_runs(view, torch.from_numpy(runs).cuda() if ld == D else runs, sel)
        torch.cuda.synchronize()
        inside = np.zeros(T, bool)
        for s, _, n in runs:
            inside[s:s + n] = True
        got, b, k = xd.cpu().numpy(), before.cpu().numpy(), keep.cpu().numpy()
        assert np.array_equal(got[inside], b[inside]) and np.array_equal(got[~inside], k[~inside])
        sel2 = sel * 2
        ctx.scatter_runs(view, runs, sel2)                        # rewritten rows land on their frames
        assert np.array_equal(xd.cpu().numpy()[inside][:, :D], 2 * b[inside][:, :D])
    ctx.close()


def _host_case():
    C, D, T = 64, 20, 1200
    w, mean, iv = make_gmm(C, D, seed=21, spread=0.1)
    x = make_frames(w, mean, iv, T, seed=22)
    # 3 speakers x 2 sessions; every session a cluster of several label segments (one pair adjacent, one longer than 64 frames)
    clusters = [[(0, 30), (40, 100)], [(150, 20), (170, 15), (200, 70)], [(300, 5), (320, 66)], [(400, 100), (520, 3)],
                [(600, 64), (700, 65)], [(800, 1), (900, 130), (1100, 99)]]
    return C, D, T, w, mean, iv, x, clusters


def test_host_layer_normalize_features_per_session():
    """JFAAcc::normalizeFeatures against the per-session numpy restatement: session model m + V y + D z + U x_h, its oracle posteriors,
    the reference's sequential subtraction of U x_h; frames outside the clusters keep their bits"""
    from lia_ral_amd import host_capi
    from oracle import oracle as orc
    C, D, T, w, mean, iv, x, clusters = _host_case()
    rng = np.random.default_rng(23)
    SV, RV, RC, sps = C * D, 2, 3, [2, 2, 2]
    V, U, Dm = rng.normal(0, 0.05, (RV, SV)), rng.normal(0, 0.05, (RC, SV)), np.abs(rng.normal(0, 0.1, SV))
    Y, X, Z = rng.normal(size=(3, RV)), rng.normal(size=(6, RC)), rng.normal(size=(3, SV))
    out, ux, models = host_capi.jfa_normalize_features(x, sps, clusters, (w, mean, 1.0 / iv), V, U, Dm, Y, X, Z)
    inside = np.zeros(T, bool)
    for h, clu in enumerate(clusters):
        s = h // 2
        ux_ref = X[h] @ U
        sp_ref = mean.ravel() + Y[s] @ V + Dm * Z[s] + ux_ref
        assert np.allclose(ux[h], ux_ref, rtol=0, atol=1e-13 * np.abs(U).sum(0).max()) and np.allclose(models[h], sp_ref, rtol=1e-13, atol=1e-13)
        rows = np.concatenate([np.arange(b, b + n) for b, n in clu])
        inside[rows] = True
        xs = x[rows].astype(np.float64)
        P = orc.occ(orc.Gmm(w, models[h].reshape(C, D), iv), xs)
        off = ux[h].reshape(C, D)
        ref = xs.copy()
        for k in range(C):
            ref -= P[:, k:k + 1] * off[k]
        bound = (1e-12 * np.abs(off).sum(0)[None, :] + 2.0 * (C + 1) * 2.0 ** -53 * (np.abs(xs) + P @ np.abs(off))
                 + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
        err = np.abs(out[rows].astype(np.float64) - ref)
        print("session %d: max err / bound %.3g, moved by up to %.3g" % (h, np.max(err / bound), np.abs(ref - xs).max()))
        assert np.all(err <= bound) and np.abs(ref - xs).max() > 1e-3
    assert np.array_equal(out[~inside], x[~inside]) and (~inside).sum() > 100


def test_host_layer_feature_mapping():
    from lia_ral_amd import host_capi
    from oracle import oracle as orc
    C, D, T, w, mean, iv, x, clusters = _host_case()
    rng = np.random.default_rng(24)
    cd_cov = 1.0 / iv
    ci_mean, ci_cov = mean + rng.normal(0, 0.2, (C, D)), cd_cov * np.exp(rng.normal(0, 0.3, (C, D)))
    cluster = clusters[1] + clusters[4]
    out = host_capi.feature_mapping(x, cluster, (w, mean, cd_cov), (w, ci_mean, ci_cov))
    rows = np.concatenate([np.arange(b, b + n) for b, n in cluster])
    xs = x[rows].astype(np.float64)
    best = orc.llk_determine_top(orc.Gmm(w, mean, 1.0 / cd_cov), xs, 1, True)["idx"][:, 0]
    want = (np.sqrt(ci_cov[best] / cd_cov[best]) * (xs - mean[best]) + ci_mean[best]).astype(np.float32)
    assert np.array_equal(out[rows], want)
    rest = np.setdiff1d(np.arange(T), rows)
    assert np.array_equal(out[rest], x[rest])
