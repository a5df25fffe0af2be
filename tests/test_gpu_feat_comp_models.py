"""Batched channel compensation on the GPU: gmmiv_feat_compensate_models (a session model and an offset per segment), its host layer
JFAAcc::normalizeFeaturesBatch and liagpu::computeTestJFABatch.

The reference of a segment is the reference's own loop (JFAAcc::normalizeFeatures, AccumulateJFAStat.cpp:4653-4675) under the segment's
model: the linear-domain posteriors of the oracle, then the sequential `ff[i] -= P[k] * ux[k * D + i]` over k in fp64.  The bound is the
one tests/test_gpu_feat_comp.py states, per element, restated here:

    |out - ref| <= 1e-12 sum_c |offset[c, i]| + 2 (C + 1) 2^-53 (|x_ti| + sum_c gamma_tc |offset[c, i]|)   (+ one f32 ulp for an f32 output)

(the project's posterior tolerance, then two summation orders).  The derived criterion has no tolerance: every segment has the BITS of
gmmiv_feat_compensate on a single-model handle.  Models come from make_gmm(spread=0.1), so that the posteriors are not one-hot.

Layout: 5 leading and 7 trailing frames of no segment, segment lengths [1, 3, 4, 0, 16, 17, 40, 15, 130, 33] -- block 0 holds three
segments and the start of a fourth --, G = 5 models of which model 4 is unused and the others serve two or three segments each.

Chunking by models: "models_scratch_mb" counts MiB and a packed 37 x 13 model takes 20 KiB, so no value holds exactly two such models.
The (37, 13) case therefore runs under "models_scratch_mb" 0 (one model per chunk, the least the library allows), and a budget that
holds exactly two models (4 MiB at 2048 x 60, 2 MiB each) is exercised at that shape on the standard layout."""
import ctypes as ct
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trials_ref as tr  # noqa: E402
from conftest import make_frames, make_gmm  # noqa: E402

pytestmark = pytest.mark.gpu

G = 5
LEAD, TRAIL = 5, 7
LENS = [1, 3, 4, 0, 16, 17, 40, 15, 130, 33]
SEG_BEGIN = LEAD + np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
SEG_MODEL = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1], np.int32)
T_ALL = int(SEG_BEGIN[-1]) + TRAIL
FAST = [(37, 13), (128, 60), (2048, 60)]
WALK = [(64, 100)]
_CASES = {}


def models_of(C, D):
    w, mean, iv = make_gmm(C, D, seed=11 + C, spread=0.1)
    rng = np.random.default_rng(C * 1000 + D)
    means = mean[None] + rng.normal(0.0, 0.05, (G, C, D))          # G models whose means differ
    offs = rng.normal(0.0, 0.3, (G, C, D))
    return w, mean, iv, means, offs


def reference(w, iv, mean, off, x64):
    """the reference loop on the frames of one segment under one model -> (ref, bound, posteriors)"""
    from oracle import oracle as orc
    C = len(w)
    P = orc.occ(orc.Gmm(w, mean, iv), x64)
    ref = x64.copy()
    for k in range(C):                                             # Gaussians outside, sequential in fp64
        ref -= P[:, k:k + 1] * off[k]
    bound = 1e-12 * np.abs(off).sum(0)[None, :] + 2.0 * (C + 1) * 2.0 ** -53 * (np.abs(x64) + P @ np.abs(off))
    return ref, bound, P


def case(C, D, sb=SEG_BEGIN, sm=SEG_MODEL, T=T_ALL):
    """models, offsets, frames (float32 values; the float64 frames are the same numbers) and the reference of every segment -- once"""
    key = (C, D, T)
    if key not in _CASES:
        w, mean, iv, means, offs = models_of(C, D)
        x32 = make_frames(w, mean, iv, T, seed=5 + D)
        x64 = x32.astype(np.float64)
        ref, bound, inside = x64.copy(), np.zeros_like(x64), np.zeros(T, bool)
        P = []
        for s in range(len(sm)):
            a, b = int(sb[s]), int(sb[s + 1])
            if b > a:
                ref[a:b], bound[a:b], p = reference(w, iv, means[sm[s]], offs[sm[s]], x64[a:b])
                inside[a:b] = True
                P.append(p)
        _CASES[key] = dict(w=w, iv=iv, means=means, offs=offs, x32=x32, x64=x64, ref=ref, bound=bound, inside=inside, P=np.concatenate(P))
        for a in _CASES[key].values():
            a.setflags(write=False)
    return _CASES[key]


def check(out, cs, what):
    out = np.asarray(out)
    m = cs["inside"]
    ref = cs["ref"][m]
    bound = cs["bound"][m] + (np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) if out.dtype == np.float32 else 0.0)
    err = np.abs(out[m].astype(np.float64) - ref)
    print("%s: max |out - ref| / bound = %.3g (max err %.3g, moved by up to %.3g)" % (what, np.max(err / bound), err.max(), np.abs(ref - cs["x64"][m]).max()))
    assert np.all(err <= bound), (what, np.max(err / bound))
    assert np.abs(ref - cs["x64"][m]).max() > 1e-3                 # the compensation moves the frames


def padded(a, extra):
    wide = np.full((a.shape[0], a.shape[1] + extra), -77.0, a.dtype)
    wide[:, :a.shape[1]] = a
    return wide


def new_ctx(**opts):
    import torch
    from lia_ral_amd import capi
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_option("timing", 1)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def batch_of(ctx, cs):
    C, D = cs["means"].shape[1:]
    return ctx.gmm_batch(G, C, D).load(cs["w"], cs["means"], cs["iv"])


def run_variants(b, cs, tag):
    """f32 / f64 x host / device x strided, out != x and in place: the segments against the reference, frames of no segment and
    padding columns against a sentinel -> the f64 -> f64 and the f32 -> f32 results (for the bitwise comparison)"""
    import torch
    D = cs["x32"].shape[1]
    offs, out_rows = cs["offs"], ~cs["inside"]
    sb, sm = SEG_BEGIN, SEG_MODEL
    # 1. host f32 -> f32, compact, a fresh output (it starts as a copy of x)
    o1 = b.feat_compensate(cs["x32"].copy(), sb, sm, offs)
    check(o1, cs, tag + " host f32->f32")
    assert o1.dtype == np.float32 and np.array_equal(o1[out_rows], cs["x32"][out_rows])
    # 2. host f64 -> f64, ldx and ldo > D, the output full of a sentinel
    xw, ow = padded(cs["x64"], 3), np.full((T_ALL, D + 5), -55.0)
    ow[:, D:] = -77.0
    b.feat_compensate(xw[:, :D], sb, sm, offs, out=ow[:, :D])
    check(ow[:, :D], cs, tag + " host f64->f64 strided")
    assert np.all(ow[:, D:] == -77.0) and np.all(ow[out_rows, :D] == -55.0) and np.array_equal(xw[:, :D], cs["x64"]) and np.all(xw[:, D:] == -77.0)
    # 3. device f32 -> f64, ldx > D, device offsets
    xd = torch.from_numpy(padded(cs["x32"], 4)).cuda()
    o3 = b.feat_compensate(xd[:, :D], sb, sm, torch.from_numpy(offs.copy()).cuda(), out_dtype=1)
    check(o3.cpu().numpy(), cs, tag + " device f32->f64")
    # 4. device f64 -> f32, ldo > D, the output full of a sentinel
    od = torch.full((T_ALL, D + 2), -55.0, dtype=torch.float32, device="cuda")
    od[:, D:] = -77.0
    b.feat_compensate(torch.from_numpy(cs["x64"].copy()).cuda(), sb, sm, offs, out=od[:, :D])
    o4 = od.cpu().numpy()
    check(o4[:, :D], cs, tag + " device f64->f32 strided")
    assert np.all(o4[:, D:] == -77.0) and np.all(o4[out_rows, :D] == -55.0)
    # 5. device f32 in place, ld > D: the frames of no segment keep their bits
    b.feat_compensate(xd[:, :D], sb, sm, offs, out=xd[:, :D])
    o5 = xd.cpu().numpy()
    check(o5[:, :D], cs, tag + " device f32 in place")
    assert np.all(o5[:, D:] == -77.0) and np.array_equal(o5[out_rows, :D], cs["x32"][out_rows])
    assert np.array_equal(o5[:, :D], o1)                           # host / device, in place or not: one result
    # 6. host f64 in place
    xh = cs["x64"].copy()
    b.feat_compensate(xh, sb, sm, offs, out=xh)
    check(xh, cs, tag + " host f64 in place")
    assert np.array_equal(xh[out_rows], cs["x64"][out_rows]) and np.array_equal(xh[cs["inside"]], ow[cs["inside"], :D])
    return xh, o1


def single_model_bits(ctx, cs, got64, got32):
    """every segment against gmmiv_feat_compensate on a single-model handle: no tolerance"""
    for s, m in enumerate(SEG_MODEL):
        a, e = int(SEG_BEGIN[s]), int(SEG_BEGIN[s + 1])
        if e == a:
            continue
        g = ctx.gmm(cs["w"], cs["means"][m], cs["iv"])
        one64 = g.feat_compensate(np.ascontiguousarray(cs["x64"][a:e]), cs["offs"][m])
        one32 = g.feat_compensate(np.ascontiguousarray(cs["x32"][a:e]), cs["offs"][m])
        g.close()
        assert np.array_equal(one64, got64[a:e]), ("f64", s)
        assert np.array_equal(one32, got32[a:e]), ("f32", s)


def test_inputs_exercise_the_contraction():
    cs = case(2048, 60)
    neff = 1.0 / (cs["P"] ** 2).sum(1)
    print("median effective Gaussian count %.1f" % np.median(neff))
    assert np.median(neff) >= 4.0
    assert len(set(SEG_MODEL)) == 4 and 4 not in SEG_MODEL
    assert SEG_BEGIN[3] < SEG_BEGIN[4] + 1 <= 16 < SEG_BEGIN[5]    # block 0: three segments, an empty one and the start of a fourth
    for C, D in FAST + WALK:
        c = case(C, D)
        assert np.all(np.isfinite(c["P"])) and np.max(np.abs(c["P"].sum(1) - 1.0)) < 1e-9


@pytest.mark.parametrize("C,D", FAST + WALK)
def test_segments_match_the_reference_loop_and_the_single_model_bits(C, D):
    cs = case(C, D)
    ctx = new_ctx()
    b = batch_of(ctx, cs)
    got64, got32 = run_variants(b, cs, "C%d D%d" % (C, D))
    # the path taken: ONE k_feat_comp launch for the ten segments at default budgets; none for vectSize 100 (the walk's generic path)
    # (the library reports -1, "none", for a kernel that never ran in the context: no launch either way)
    n = max(ctx.kernel_launches("k_feat_comp"), 0)
    assert n == (1 if (C, D) in FAST else 0), n
    assert ctx.set_option("zero_llk_frames", 0) == 0
    single_model_bits(ctx, cs, got64, got32)
    # T = 0 and nseg = 0 are valid and touch nothing
    assert b.feat_compensate(np.full((0, D), 1.0), [0], [], cs["offs"]).shape == (0, D)
    keep = np.full((9, D), 3.0)
    assert np.array_equal(b.feat_compensate(keep.copy(), [4], [], cs["offs"], out=keep), np.full((9, D), 3.0))
    # one offset row shared by all models (stride 0)
    sh = b.feat_compensate(cs["x64"].copy(), SEG_BEGIN, SEG_MODEL, cs["offs"][2])
    g = ctx.gmm(cs["w"], cs["means"][3], cs["iv"])
    a, e = int(SEG_BEGIN[7]), int(SEG_BEGIN[8])
    assert np.array_equal(sh[a:e], g.feat_compensate(np.ascontiguousarray(cs["x64"][a:e]), cs["offs"][2]))
    g.close(); b.close(); ctx.close()


def test_the_walk_serves_the_fast_shapes_too():
    """ "stats_z" 0: the segments go one by one through the single-model code; same bits as that code, no k_feat_comp launch"""
    cs = case(128, 60)
    ctx = new_ctx(stats_z=0)
    b = batch_of(ctx, cs)
    got64, got32 = run_variants(b, cs, "C128 D60 stats_z 0")
    assert max(ctx.kernel_launches("k_feat_comp"), 0) == 0
    single_model_bits(ctx, cs, got64, got32)
    b.close(); ctx.close()


def _long_layout():
    """about 40 segments over about 7200 frames; no inner bound is a multiple of 16, so every chunk boundary cuts a 16-frame block"""
    lens = np.array([170 + 5 * (i % 5) for i in range(40)])
    sb = (LEAD + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
    sm = np.array([(i // 3) % 4 for i in range(40)], np.int32)     # runs of three segments per model
    assert np.all(sb[1:-1] % 16 != 0) and 7000 < sb[-1] < 7400
    return sb, sm, int(sb[-1]) + TRAIL


@pytest.mark.parametrize("option,value", [("z_scratch_mb", 4), ("models_scratch_mb", 0)])
def test_chunks_of_whole_segments(option, value):
    import torch
    C, D = 37, 13
    sb, sm, T = _long_layout()
    w, mean, iv, means, offs = models_of(C, D)
    x32 = make_frames(w, mean, iv, T, seed=77)
    ctx = new_ctx()
    b = ctx.gmm_batch(G, C, D).load(w, means, iv)
    one = b.feat_compensate(torch.from_numpy(x32.copy()).cuda(), sb, sm, offs, out_dtype=1).cpu().numpy()
    assert ctx.kernel_launches("k_feat_comp") == 1
    ctx.set_option(option, value)
    xd = torch.from_numpy(x32.copy()).cuda()
    two = b.feat_compensate(xd, sb, sm, offs, out_dtype=1).cpu().numpy()
    n = ctx.kernel_launches("k_feat_comp")
    print("%s %d: %d launches of k_feat_comp, %d of k_llk_mfma for %d segments" % (option, value, n, ctx.kernel_launches("k_llk_mfma"), len(sm)))
    assert 2 <= n < len(sm) and ctx.kernel_launches("k_llk_mfma") == n
    assert np.array_equal(one, two)
    b.feat_compensate(xd, sb, sm, offs, out=xd)                    # in place: a 16-frame block straddles every chunk boundary
    inp = xd.cpu().numpy()
    assert np.array_equal(inp, one.astype(np.float32)) and ctx.kernel_launches("k_feat_comp") == n
    # a few segments against the reference as well
    for s in (0, 13, 39):
        a, e = int(sb[s]), int(sb[s + 1])
        ref, bound, _ = reference(w, iv, means[sm[s]], offs[sm[s]], x32[a:e].astype(np.float64))
        assert np.all(np.abs(two[a:e] - ref) <= bound), s
    b.close(); ctx.close()


def test_a_model_scratch_that_holds_two_models():
    """2048 x 60: 2 MiB per packed model, "models_scratch_mb" 4 -> chunks of two distinct models"""
    import torch
    cs = case(2048, 60)
    ctx = new_ctx()
    b = batch_of(ctx, cs)
    one = b.feat_compensate(torch.from_numpy(cs["x32"].copy()).cuda(), SEG_BEGIN, SEG_MODEL, cs["offs"], out_dtype=1).cpu().numpy()
    assert ctx.kernel_launches("k_feat_comp") == 1
    ctx.set_option("models_scratch_mb", 4)
    xd = torch.from_numpy(cs["x32"].copy()).cuda()
    two = b.feat_compensate(xd, SEG_BEGIN, SEG_MODEL, cs["offs"], out_dtype=1).cpu().numpy()
    n = ctx.kernel_launches("k_feat_comp")
    assert 2 <= n < len(SEG_MODEL) and np.array_equal(one, two), n
    b.feat_compensate(xd, SEG_BEGIN, SEG_MODEL, cs["offs"], out=xd)
    assert np.array_equal(xd.cpu().numpy(), one.astype(np.float32))
    b.close(); ctx.close()


@pytest.mark.parametrize("C,D", [(128, 60), (64, 100)])
def test_degenerate_frames_are_copied_through_and_counted_once(C, D):
    import torch
    cs = case(C, D)
    ctx = new_ctx()
    b = batch_of(ctx, cs)
    clean = b.feat_compensate(cs["x64"].copy(), SEG_BEGIN, SEG_MODEL, cs["offs"])
    x = cs["x64"].copy()
    nan_t, far_t = int(SEG_BEGIN[1]) + 1, int(SEG_BEGIN[6]) + 9      # in block 0 (shared by four segments) and inside a longer segment
    x[nan_t, 3] = np.nan                                           # unusable
    x[far_t] = 1.0e4                                               # likelihood 0 in fp64
    bad = [nan_t, far_t]
    ctx.set_option("zero_llk_frames", 0)
    got = b.feat_compensate(x.copy(), SEG_BEGIN, SEG_MODEL, cs["offs"])
    assert ctx.set_option("zero_llk_frames", 0) == 2
    assert np.array_equal(got[bad], x[bad], equal_nan=True)
    rest = np.setdiff1d(np.arange(T_ALL), bad)
    assert np.array_equal(got[rest], clean[rest])                  # every other frame keeps its bits, neighbours in the same block included
    gd = b.feat_compensate(torch.from_numpy(x).cuda(), SEG_BEGIN, SEG_MODEL, cs["offs"], out_dtype=0).cpu().numpy()
    assert ctx.set_option("zero_llk_frames", 0) == 2
    assert np.array_equal(gd[bad], x[bad].astype(np.float32), equal_nan=True) and np.array_equal(gd[rest], clean[rest].astype(np.float32))
    b.close(); ctx.close()


def test_argument_errors_leave_out_untouched():
    import torch
    from lia_ral_amd import capi
    C, D = 37, 13
    cs = case(C, D)
    ctx = new_ctx()
    b = batch_of(ctx, cs)
    other = new_ctx()
    xd = torch.from_numpy(cs["x64"].copy()).cuda()
    od = torch.full((T_ALL + 4, D), -55.0, dtype=torch.float64, device="cuda")
    keep_x, keep_o = xd.clone(), od.clone()
    off = torch.from_numpy(cs["offs"].copy()).cuda()
    L = capi.lib
    sb, sm = SEG_BEGIN.copy(), SEG_MODEL.copy()
    CD = C * D

    def comp(x, out, xdt=1, odt=1, ldx=D, ldo=D, T=T_ALL, sb=sb, sm=sm, offp=None, stride=CD, c=ctx, sbp=None, smp=None):
        return L.gmmiv_feat_compensate_models(c._h, b._h, ct.c_void_p(x), xdt, ct.c_int64(T), ct.c_int64(ldx),
                                              ct.c_void_p(sbp) if sbp else sb.ctypes.data_as(ct.c_void_p),
                                              ct.c_void_p(smp) if smp else sm.ctypes.data_as(ct.c_void_p), ct.c_int64(len(sm)),
                                              capi._ptr(off) if offp is None else offp, ct.c_int64(stride), ct.c_void_p(out), odt, ct.c_int64(ldo))
    base, o = xd.data_ptr(), od.data_ptr()
    assert comp(base, o) == 0                                                                        # the call as such is fine
    od.copy_(keep_o)
    assert comp(base, base + 8) == -1 and b"overlaps" in L.gmmiv_last_error()                       # shifted by one element
    assert comp(base, base + 8 * D * 10) == -1                                                       # shifted by ten frames
    assert comp(base, base, odt=0) == -1                                                             # same pointer, other dtype
    bad = sm.copy(); bad[5] = G
    assert comp(base, o, sm=bad) == -1 and b"outside" in L.gmmiv_last_error()                        # index out of range
    bad[5] = -1
    assert comp(base, o, sm=bad) == -1
    dec = sb.copy(); dec[4] = dec[3] - 1
    assert comp(base, o, sb=dec) == -1 and b"non-decreasing" in L.gmmiv_last_error()                 # decreasing table
    far = sb.copy(); far[-1] = T_ALL + 1
    assert comp(base, o, sb=far) == -1
    sbd, smd = torch.from_numpy(sb).cuda(), torch.from_numpy(sm).cuda()
    assert comp(base, o, sbp=sbd.data_ptr()) == -1 and b"host arrays" in L.gmmiv_last_error()        # device tables
    assert comp(base, o, smp=smd.data_ptr()) == -1
    assert comp(base, o, offp=ct.c_void_p(0)) == -1 and b"offset == NULL" in L.gmmiv_last_error()
    assert comp(base, o, stride=CD - 1) == -1 and b"offset_stride" in L.gmmiv_last_error()
    assert comp(base, o, xdt=2) == -1 and b"dtype" in L.gmmiv_last_error()
    assert comp(base, o, odt=7) == -1 and comp(base, o, ldx=D - 1) == -1 and comp(base, o, T=-1) == -1
    assert comp(base, o, c=other) == -1 and b"different context" in L.gmmiv_last_error()             # a batch of another context
    torch.cuda.synchronize()
    assert torch.equal(xd, keep_x) and torch.equal(od, keep_o)
    b.close(); ctx.close(); other.close()


# ---- host layer -------------------------------------------------------------------------------------------------------------------------
def _host_case():
    C, D, T = 64, 20, 1200
    w, mean, iv = make_gmm(C, D, seed=21, spread=0.1)
    x = make_frames(w, mean, iv, T, seed=22)
    # 3 speakers x 2 sessions; every session a cluster of several label segments (one pair adjacent, one longer than 64 frames)
    clusters = [[(0, 30), (40, 100)], [(150, 20), (170, 15), (200, 70)], [(300, 5), (320, 66)], [(400, 100), (520, 3)],
                [(600, 64), (700, 65)], [(800, 1), (900, 130), (1100, 99)]]
    rng = np.random.default_rng(23)
    SV, RV, RC = C * D, 2, 3
    V, U, Dm = rng.normal(0, 0.05, (RV, SV)), rng.normal(0, 0.05, (RC, SV)), np.abs(rng.normal(0, 0.1, SV))
    Y, X, Z = rng.normal(size=(3, RV)), rng.normal(size=(6, RC)), rng.normal(size=(3, SV))
    return x, [2, 2, 2], clusters, (w, mean, 1.0 / iv), V, U, Dm, Y, X, Z


def test_host_layer_batched_normalisation_has_the_bits_of_the_loop():
    from lia_ral_amd import host_capi as h
    x, sps, clusters, ubm, V, U, Dm, Y, X, Z = _host_case()
    loop = h.jfa_normalize_features(x, sps, clusters, ubm, V, U, Dm, Y, X, Z, batched=False)
    legacy = h.jfa_normalize_features(x, sps, clusters, ubm, V, U, Dm, Y, X, Z)[0]
    got = h.jfa_normalize_features(x, sps, clusters, ubm, V, U, Dm, Y, X, Z, batched=True)
    inside = np.zeros(len(x), bool)
    for clu in clusters:
        for a, n in clu:
            inside[a:a + n] = True
    assert np.array_equal(loop, legacy) and np.array_equal(got, loop)
    assert np.array_equal(got[~inside], x[~inside]) and np.abs(got[inside] - x[inside]).max() > 1e-3
    # two sessions share frames: the loop depends on the order of the sessions, so the batched call takes the loop
    shared = [list(c) for c in clusters]
    shared[3] = [(400, 100), (50, 60)]                             # frames 50 .. 109 are session 0's too
    a = h.jfa_normalize_features(x, sps, shared, ubm, V, U, Dm, Y, X, Z, batched=False)
    b = h.jfa_normalize_features(x, sps, shared, ubm, V, U, Dm, Y, X, Z, batched=True)
    assert np.array_equal(a, b) and not np.array_equal(a[50:110], loop[50:110])


def _jfa_lines():
    C, D, RC = 64, 20, 3
    world = make_gmm(C, D, seed=31, spread=0.1)
    models = tr.make_models(world, False, seed=32)
    x = make_frames(*world, 2000, seed=33)
    rng = np.random.default_rng(34)
    x = (x + np.repeat(rng.normal(0, 0.3, (8, D)), 250, axis=0)).astype(np.float32)    # a shift per line: something for the channel factor to find
    U = rng.normal(0, 0.05, (RC, C * D))
    seg_begin = [[250 * l + 3, 250 * l + 120] for l in range(8)]
    seg_len = [[100 + l, 90 - 7 * l] for l in range(8)]
    seg_len[5] = [17, 1]
    clients = [[0, 3], [4, 1, 2], [3], [0], [1, 2], [2, 4], [0, 1, 2, 3, 4], [4]]
    hm = lambda m: (m[0], m[1], 1.0 / m[2])                        # the host layer takes variances
    return x, seg_begin, seg_len, world, models, hm(world), [hm(tr.model_of(models, g)) for g in range(tr.N_MODELS)], clients, U


def test_host_layer_compute_test_jfa():
    from lia_ral_amd import host_capi as h
    x, sbeg, slen, world, models, hworld, hmodels, clients, U = _jfa_lines()
    C, D = world[1].shape
    keep = x.copy()
    llr, comp, X = h.compute_test_jfa(x, sbeg, slen, hworld, U, hmodels, clients)
    assert np.array_equal(x, keep) and X.shape == (8, 3) and np.abs(X).max() > 1e-2
    # (a) bit for bit the composition of the existing calls on one accumulator
    llr2, comp2, X2 = h.compute_test_jfa(x, sbeg, slen, hworld, U, hmodels, clients, compose=True)
    assert np.array_equal(X, X2) and np.array_equal(comp, comp2) and all(np.array_equal(p, q) for p, q in zip(llr, llr2))
    # (b) the compensated frames against the reference loop evaluated with the GPU's own X
    rows = [np.concatenate([np.arange(b, b + n) for b, n in zip(sbeg[l], slen[l])]) for l in range(8)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    for l in range(8):
        ux = (X[l] @ U).reshape(C, D)
        xs = x[rows[l]].astype(np.float64)
        ref, bound, _ = reference(world[0], world[2], world[1] + ux, ux, xs)
        bound = bound + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        err = np.abs(comp[off[l]:off[l + 1]].astype(np.float64) - ref)
        print("line %d: max err / bound %.3g, moved by up to %.3g" % (l, np.max(err / bound), np.abs(ref - xs).max()))
        assert np.all(err <= bound) and np.abs(ref - xs).max() > 1e-3
    # (c) the LLRs against the CPU oracle scoring those same compensated frames
    lw, lc = tr.frame_ref(world, models, comp, 10, True)
    for l in range(8):
        sl = slice(off[l], off[l + 1])
        want = np.array([lc[g][sl].mean() - lw[sl].mean() for g in clients[l]])
        assert llr[l].shape == want.shape and np.max(np.abs(llr[l] - want)) < 1e-9, (l, llr[l] - want)
    # (d) a line scored alone agrees with the same line inside the list
    for l in (0, 5, 6):
        alone = h.compute_test_jfa(x, [sbeg[l]], [slen[l]], hworld, U, hmodels, [clients[l]])[0][0]
        assert np.max(np.abs(alone - llr[l])) < 1e-9, (l, alone - llr[l])
