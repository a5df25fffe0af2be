"""A model per segment (gmmiv_gmm_batch, gmmiv_llk_models, gmmiv_tv_stats_models, gmmiv_map_adapt_models) against the oracle run per
segment with that segment's model.  The shapes are the smallest at which the tile logic can go wrong: segment boundaries off every
multiple of 4 / 16 / 32 / 256, an empty segment, a model used twice, frames that belong to no segment at both ends."""
import functools

import numpy as np
import pytest

from conftest import make_frames, make_gmm
from models_ref import LEAD, N_MODELS, SEG_LEN, SEG_MODEL, map_adapt_np, relerr, seg_layout
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [(128, 60), (96, 60), (37, 13), (2, 1), (33, 101)]      # (33, 101): no MFMA instantiation, the segment-by-segment walk
SENTINEL = 123.25


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(C, D, dtype, variant="means"):
    """models, frames and the oracle's per-segment results (computed once, read-only).  variant "means": w and covinv shared by the five
    models (stride 0), "all": every table per model"""
    w, mean, iv = make_gmm(C, D, seed=C + D)
    rng = np.random.default_rng(C * 7 + D)
    means = mean[None] + rng.normal(0.0, 0.3, (N_MODELS, C, D))
    if variant == "all":
        ws = rng.dirichlet(np.ones(C) * 5, N_MODELS)
        ivs = iv[None] * np.exp(rng.normal(0.0, 0.2, (N_MODELS, C, D)))
    else:
        ws, ivs = np.broadcast_to(w, (N_MODELS, C)), np.broadcast_to(iv, (N_MODELS, C, D))
    sb, sm, T = seg_layout()
    x = make_frames(w, mean, iv, T, seed=3, dtype=dtype)
    ref_llk, ref_N, ref_F = [], [], []
    for s, m in enumerate(sm):
        xs = x[sb[s]:sb[s + 1]].astype(np.float64)
        og = orc.Gmm(ws[m], means[m], ivs[m])
        ref_llk.append(orc.llk(og, xs, -1e9, 1e9) if len(xs) else np.zeros(0))
        if len(xs):
            No, Fo = orc.tv_stats(og, xs, np.zeros(len(xs), np.int64), 1)
        else:
            No, Fo = np.zeros((1, C)), np.zeros((1, C * D))
        ref_N.append(No[0]); ref_F.append(Fo[0])
    out = dict(w=w, mean=mean, iv=iv, ws=ws, means=means, ivs=ivs, sb=sb, sm=sm, T=T, x=x, llk=ref_llk, N=np.array(ref_N), F=np.array(ref_F))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def load(ctx, k, variant="means"):
    C, D = k["mean"].shape
    b = ctx.gmm_batch(N_MODELS, C, D)
    if variant == "all":
        return b.load(np.ascontiguousarray(k["ws"]), k["means"], np.ascontiguousarray(k["ivs"]))
    return b.load(k["w"], k["means"], k["iv"])


LLK_CASES = [(C, D, "means") for C, D in SHAPES] + [(128, 60, "all"), (37, 13, "all")]


@pytest.mark.parametrize("C,D,variant", LLK_CASES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_llk_models_match_oracle_and_single_model_calls(ctx, C, D, variant, dtype):
    k = case(C, D, dtype, variant)
    b = load(ctx, k, variant)
    sb, sm, T, x = k["sb"], k["sm"], k["T"], k["x"]
    got, ssum = b.llk(x, sb, sm, -1e9, 1e9, out=np.full(T, SENTINEL))
    assert np.all(got[:LEAD] == SENTINEL) and np.all(got[sb[-1]:] == SENTINEL)          # frames of no segment are not touched
    for s, m in enumerate(sm):
        seg = got[sb[s]:sb[s + 1]]
        assert len(seg) == SEG_LEN[s]
        if not len(seg):
            assert ssum[s] == 0.0
            continue
        assert np.max(np.abs(seg - k["llk"][s])) < 1e-9, s
        assert abs(ssum[s] - k["llk"][s].sum()) < 1e-8 * len(seg), s
        # a frame's arithmetic does not depend on its row in a tile: the bits of gmmiv_llk on a single-model handle
        one = ctx.gmm(k["ws"][m], k["means"][m], k["ivs"][m]).llk(np.ascontiguousarray(x[sb[s]:sb[s + 1]]), -1e9, 1e9)
        assert np.array_equal(seg, one), s
    ctx.set_option("glds", 0)
    try:
        got2, ssum2 = b.llk(x, sb, sm, -1e9, 1e9, out=np.full(T, SENTINEL))
    finally:
        ctx.set_option("glds", 1)
    assert np.array_equal(got, got2) and np.array_equal(ssum, ssum2)
    # the clamp
    got3, ssum3 = b.llk(x, sb, sm, -20.0, -10.0, out=np.full(T, SENTINEL))
    inside = slice(sb[0], sb[-1])
    assert np.array_equal(got3[inside], np.clip(got[inside], -20.0, -10.0)) and np.all(got3[:LEAD] == SENTINEL)


def test_models_on_device_tensors_and_packed_blocks(ctx):
    """device-resident frames, outputs and model tables give the bits of the host-array call; the packed block of a model does not
    depend on whether its shared tables were given once (stride 0) or per model"""
    import torch
    k = case(128, 60, np.float32)
    b = load(ctx, k)
    sb, sm, T = k["sb"], k["sm"], k["T"]
    ref, rsum = b.llk(k["x"], sb, sm, -1e9, 1e9, out=np.full(T, SENTINEL))
    N0, F0, L0 = b.tv_stats(k["x"], sb, sm)
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    b2 = ctx.gmm_batch(N_MODELS, 128, 60).load(dev(k["ws"]), dev(k["means"]), dev(k["ivs"]))
    out = torch.full((T,), SENTINEL, dtype=torch.float64, device="cuda")
    ssum = torch.empty(len(sm), dtype=torch.float64, device="cuda")
    b2.llk(dev(k["x"]), sb, sm, -1e9, 1e9, out=out, seg_sum=ssum)
    N = torch.empty((len(sm), 128), dtype=torch.float64, device="cuda"); F = torch.empty((len(sm), 128 * 60), dtype=torch.float64, device="cuda")
    L = torch.empty((len(sm), 2), dtype=torch.float64, device="cuda")
    b2.tv_stats(dev(k["x"]), sb, sm, N=N, F=F, seg_llk=L)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(ssum.cpu().numpy(), rsum)
    assert np.array_equal(N.cpu().numpy(), N0) and np.array_equal(F.cpu().numpy(), F0) and np.array_equal(L.cpu().numpy(), L0)
    for g in range(N_MODELS):
        assert np.array_equal(b.packed(g), b2.packed(g))
    assert len(b.packed(0)) == 8 * 32 * 64 and not np.array_equal(b.packed(0), b.packed(1))


@pytest.mark.parametrize("C,D", SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tv_stats_models_match_oracle(ctx, C, D, dtype):
    k = case(C, D, dtype)
    b = load(ctx, k)
    sb, sm = k["sb"], k["sm"]
    N, F, L = b.tv_stats(k["x"], sb, sm)
    assert relerr(N, k["N"]) < 1e-9 and relerr(F, k["F"]) < 1e-9
    for s in range(len(sm)):
        if SEG_LEN[s]:
            assert relerr(N[s], k["N"][s]) < 1e-9 and relerr(F[s], k["F"][s]) < 1e-9, s
            assert abs(L[s, 0] - k["llk"][s].sum()) < 1e-8 * SEG_LEN[s]
    assert not N[1].any() and not F[1].any() and not L[1].any()                        # the empty segment
    assert np.array_equal(L[:, 1], np.asarray(SEG_LEN, np.float64))


def test_chunks_by_frames_and_by_models_give_the_unchunked_result(ctx):
    """512 x 60: a packed model is 512 KiB and a frame 4 KiB of likelihood scratch, so 1 MiB of model scratch holds two of the five
    models and 4 MiB of likelihood scratch 768 of the 854 frames -- at least two chunks either way (counted through the kernel timer)."""
    k = case(512, 60, np.float32)
    b = load(ctx, k)
    sb, sm, T = k["sb"], k["sm"], k["T"]
    ctx.set_option("timing", 1)
    prev_z = ctx.set_option("z_scratch_mb", 16384)
    prev_m = ctx.set_option("models_scratch_mb", 2048)
    try:
        N0, F0, L0 = b.tv_stats(k["x"], sb, sm)
        assert ctx.kernel_launches("k_llk_mfma") == 1
        l0, s0 = b.llk(k["x"], sb, sm, -1e9, 1e9, out=np.full(T, SENTINEL))
        assert relerr(N0, k["N"]) < 1e-9 and relerr(F0, k["F"]) < 1e-9
        ctx.set_option("z_scratch_mb", 4)
        b.tv_stats(k["x"], sb, sm)
        assert ctx.kernel_launches("k_llk_mfma") >= 2 and ctx.kernel_launches("k_stats_z") >= 2       # frame chunks
        ctx.set_option("z_scratch_mb", 16384)
        ctx.set_option("models_scratch_mb", 1)
        b.tv_stats(k["x"], sb, sm)
        assert ctx.kernel_launches("k_llk_mfma") >= 2 and ctx.kernel_launches("k_gmm_pack") >= 2      # model chunks
        ctx.set_option("z_scratch_mb", 4)
        N1, F1, L1 = b.tv_stats(k["x"], sb, sm)
        assert ctx.kernel_launches("k_llk_mfma") >= 3
        l1, s1 = b.llk(k["x"], sb, sm, -1e9, 1e9, out=np.full(T, SENTINEL))
        assert ctx.kernel_launches("k_llk_mfma") >= 2
    finally:
        ctx.set_option("z_scratch_mb", prev_z)
        ctx.set_option("models_scratch_mb", prev_m)
        ctx.set_option("timing", 0)
    assert relerr(N1, N0) < 1e-13 and relerr(F1, F0) < 1e-13 and relerr(L1, L0) < 1e-13
    assert not N1[1].any() and np.array_equal(L1[:, 1], L0[:, 1])
    assert np.array_equal(l1, l0) and relerr(s1, s0) < 1e-13


@pytest.mark.parametrize("C,D", [(128, 60), (33, 101)])
def test_degenerate_frames_in_a_segment(ctx, C, D):
    """one NaN frame and one frame 1e6 away from every mean: llk = min_llk, nothing added to N / F, counted like gmmiv_llk /
    gmmiv_tv_stats count them (both are zero-likelihood frames, the NaN frame is also a screened one)"""
    k = case(C, D, np.float32)
    b = load(ctx, k)
    sb, sm, T = k["sb"], k["sm"], k["T"]
    x = k["x"].copy()
    t_nan, t_far = int(sb[2]) + 17, int(sb[7]) + 250                                   # segments 2 (model 2) and 7 (model 1)
    x[t_nan, D // 2] = np.nan
    x[t_far, :] = 1e6
    ctx.set_option("zero_llk_frames", 0); ctx.set_option("screened_frames", 0)
    got, ssum = b.llk(x, sb, sm, -200.0, 200.0, out=np.full(T, SENTINEL))
    assert ctx.set_option("zero_llk_frames", 0) == 2 and ctx.set_option("screened_frames", 0) == 1
    assert got[t_nan] == -200.0 and got[t_far] == -200.0
    clean, _ = b.llk(k["x"], sb, sm, -200.0, 200.0, out=np.full(T, SENTINEL))
    keep = np.ones(T, bool); keep[[t_nan, t_far]] = False
    assert np.array_equal(got[keep], clean[keep])
    ctx.set_option("zero_llk_frames", 0); ctx.set_option("screened_frames", 0)
    N, F, L = b.tv_stats(x, sb, sm)
    assert ctx.set_option("zero_llk_frames", 0) == 2 and ctx.set_option("screened_frames", 0) == 1
    for s, t in ((2, t_nan), (7, t_far)):
        xs = np.delete(k["x"][sb[s]:sb[s + 1]].astype(np.float64), t - sb[s], axis=0)
        m = sm[s]
        og = orc.Gmm(k["ws"][m], k["means"][m], k["ivs"][m])
        No, Fo = orc.tv_stats(og, xs, np.zeros(len(xs), np.int64), 1)
        assert relerr(N[s], No[0]) < 1e-9 and relerr(F[s], Fo[0]) < 1e-9
        assert L[s, 1] == SEG_LEN[s] - 1 and abs(L[s, 0] - orc.llk(og, xs, -1e9, 1e9).sum()) < 1e-8 * len(xs)
    others = [s for s in range(len(sm)) if s not in (2, 7)]
    assert relerr(N[others], k["N"][others]) < 1e-9 and relerr(F[others], k["F"][others]) < 1e-9


@pytest.mark.parametrize("method", ["MAPOccDep", "MAPModelBased", "MAPConst", "MAPConst2"])
@pytest.mark.parametrize("weight", [False, True])
def test_map_adapt_kernel_matches_compute_map(ctx, method, weight):
    """gmmiv_map_adapt_models against host_capi.compute_map on the same ML estimate, error normalised by max |ref|: < 1e-14 (at most
    six roundings of 1.1e-16 per element, ten times that as margin for contraction differences)"""
    import torch
    from lia_ral_amd import host_capi as h
    rng = np.random.default_rng(5)
    G, C, D = N_MODELS, 37, 13
    w0 = rng.dirichlet(np.ones(C)); mean0 = rng.normal(size=(C, D)); cov0 = rng.uniform(0.5, 2.0, (C, D))
    count = np.array([731.0, 40.0, 3000.0, 1.0, 259.0])
    N = rng.dirichlet(np.ones(C), G) * count[:, None]
    N[1, 4] = 0.0                                                                      # keeps its current mean, weight 0
    F = ((mean0 + rng.normal(0, 0.3, (G, C, D))) * N[:, :, None]).reshape(G, C * D)
    cur = (mean0 + rng.normal(0, 0.1, (G, C, D))).reshape(G, C * D)
    reg = (14.0, 9.0, 20.0)
    b = ctx.gmm_batch(G, C, D)
    m, w = b.map_adapt(N, F, count, w0, mean0, cur, method, True, weight, reg, 0.6)
    for g in range(G):
        ml = np.where(N[g][:, None] > 0, F[g].reshape(C, D) / np.where(N[g] > 0, N[g], 1.0)[:, None], cur[g].reshape(C, D))
        rw, rm, _ = h.compute_map(method, (w0, mean0, cov0), (N[g] / count[g], ml, cov0), count[g], mean=True, weight=weight, reg=reg, alpha_mean=0.6)
        assert relerr(m[g].reshape(C, D), rm) < 1e-14 and relerr(w[g], rw) < 1e-14, g
    mn, wn = map_adapt_np(N, F, count, w0, mean0, cur, method, True, weight, reg, 0.6)
    assert relerr(m, mn.reshape(G, -1)) < 1e-14 and relerr(w, wn) < 1e-14
    # device tensors in and out, the counts read with a stride (the seg_llk layout), a shared current mean
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    cl = np.stack([np.zeros(G), count], axis=1)
    md, wd = b.map_adapt(dev(N), dev(F), dev(cl).reshape(-1)[1:], dev(w0), dev(mean0), dev(cur), method, True, weight, reg, 0.6, count_stride=2)
    ctx.sync()
    assert np.array_equal(md.cpu().numpy(), m) and np.array_equal(wd.cpu().numpy(), w)
    ms, _ = b.map_adapt(N, F, count, w0, mean0, mean0, method, True, weight, reg, 0.6)
    keep = np.ones((G, C), bool); keep[1, 4] = False
    assert np.array_equal(ms.reshape(G, C, D)[keep], m.reshape(G, C, D)[keep])
    if method != "MAPConst2":
        exp = mean0[4] if method != "MAPConst" else (0.6 * mean0[4]) + ((1 - 0.6) * mean0[4])
        assert relerr(ms.reshape(G, C, D)[1, 4], exp) < 1e-15


def test_map_adapt_mean_off_and_unknown_method(ctx):
    rng = np.random.default_rng(6)
    G, C, D = 2, 5, 3
    w0 = rng.dirichlet(np.ones(C)); mean0 = rng.normal(size=(C, D))
    count = np.array([10.0, 0.0])
    N = rng.dirichlet(np.ones(C), G) * count[:, None]
    F = rng.normal(size=(G, C * D)) * np.repeat(N, D, axis=1)
    cur = rng.normal(size=(G, C * D))
    b = ctx.gmm_batch(G, C, D)
    m, w = b.map_adapt(N, F, count, w0, mean0, cur, "MAPOccDep", False, False)
    assert np.array_equal(m, np.broadcast_to(mean0.ravel(), m.shape)) and np.array_equal(w, np.broadcast_to(w0, w.shape))
    m, w = b.map_adapt(N, F, count, w0, mean0, cur, "MLLR?", True, True)                # "No adaptation": the ML estimate
    assert np.allclose(m[0], F[0] / np.repeat(N[0], D), rtol=1e-15) and np.allclose(w[0], N[0] / 10.0, rtol=1e-15)
    assert np.array_equal(m[1], cur[1]) and not w[1].any()                             # a model without frames: current means, weight 0
    m, w = b.map_adapt(N, F, count, w0, mean0, cur, "MAPOccDep", True, False)
    assert np.array_equal(m[1], mean0.ravel())                                         # alpha = 0: the a-priori mean


# ---- enrolment end to end: liagpu::adaptModelBatch through host_capi.train_target_batch -----------------------------------------------
def oracle_enroll(x, seg_begin, seg_len, world, nb_it, reg=(16.0, 16.0, 16.0), method="MAPOccDep", **kw):
    """adaptModel restated on the oracle: nb_it x (EM statistics under the current client model, ML estimate, computeMAP)"""
    xd = x.astype(np.float64)
    fr = np.concatenate([np.arange(b, b + n) for b, n in zip(seg_begin, seg_len)])
    cw, cm, cc = [np.array(a, np.float64) for a in world]
    for _ in range(nb_it):
        acc = orc.em_accumulate(orc.Gmm(cw, cm, 1.0 / cc), xd[fr])
        mw, mm, mc = orc.em_get(acc, cm, cc)
        cw, cm, cc = orc.compute_map(method, world, (mw, mm, mc), float(int(acc["count"])), reg=reg, **kw)
    return cw, cm, cc


@functools.lru_cache(maxsize=None)
def enroll_case():
    """6 clients of 40 to 400 frames, 128 x 60, one or two segments each with gaps between them"""
    w, mean, iv = make_gmm(128, 60, seed=21)
    lens = [40, 400, 131, 256, 77, 300]
    rng = np.random.default_rng(2)
    x = make_frames(w, mean + rng.normal(0, 0.2, mean.shape), iv, sum(lens) + 60, seed=22)
    cb, sb, sl, pos = [0], [], [], 3
    for i, n in enumerate(lens):
        cut = n // 3 if i % 2 else 0
        if cut:
            sb += [pos, pos + cut + 5]; sl += [cut, n - cut]; pos += n + 5
        else:
            sb += [pos]; sl += [n]; pos += n
        pos += 4
        cb.append(len(sb))
    return (w, mean, 1.0 / iv), x, np.array(cb), np.array(sb), np.array(sl)


def test_train_target_batch_meets_the_traintarget_golden(golden_dir):
    """the reference's own TrainTarget vector as client 0, next to two synthetic clients: client 0 meets the golden within the
    fixture's tolerances, weights and variances are the world's (mean-only adaptation)"""
    import os
    from lia_ral_amd import host_capi as h
    k = np.load(os.path.join(golden_dir, "kat2_traintarget.npz"))
    world = (k["w"], k["mean_world"], 1.0 / k["covinv"])
    extra = make_frames(k["w"] / k["w"].sum(), k["mean_world"], k["covinv"], 300, seed=4)
    x = np.concatenate([k["x"], extra])
    n0 = len(k["x"])
    sb = np.concatenate([k["seg_begin"], [n0, n0 + 120, n0 + 190]]); sl = np.concatenate([k["seg_len"], [120, 60, 110]])
    cb = np.array([0, len(k["seg_begin"]), len(k["seg_begin"]) + 1, len(sb)])
    w, mean, cov = h.train_target_batch(x, cb, sb, sl, world, nb_it=1, reg=(float(k["reg_factor"]),) * 3)
    diff = np.abs(mean[0] - k["mean_expected"])
    assert np.median(diff) < float(k["median_tol"]) and diff.max() < float(k["max_tol"])
    for i in range(3):
        assert np.array_equal(w[i], k["w"]) and np.allclose(cov[i], 1.0 / k["covinv"], rtol=1e-15)
        ref = oracle_enroll(x, sb[cb[i]:cb[i + 1]], sl[cb[i]:cb[i + 1]], world, 1, reg=(float(k["reg_factor"]),) * 3)
        assert relerr(mean[i], ref[1]) < 1e-9, i


def test_train_target_batch_matches_the_oracle_loop():
    from lia_ral_amd import host_capi as h
    world, x, cb, sb, sl = enroll_case()
    w, mean, cov = h.train_target_batch(x, cb, sb, sl, world, nb_it=1)
    for i in range(len(cb) - 1):
        ref = oracle_enroll(x, sb[cb[i]:cb[i + 1]], sl[cb[i]:cb[i + 1]], world, 1)
        assert relerr(mean[i], ref[1]) < 1e-9, i
        assert np.array_equal(w[i], world[0])
    # all four methods, with the weight branch: against the oracle's computeMAP
    for method in ("MAPModelBased", "MAPConst", "MAPConst2"):
        w, mean, cov = h.train_target_batch(x, cb, sb, sl, world, method=method, nb_it=1, weight=True, reg=(14.0, 9.0, 20.0), alpha_mean=0.6)
        for i in (0, 3):
            ref = oracle_enroll(x, sb[cb[i]:cb[i + 1]], sl[cb[i]:cb[i + 1]], world, 1, reg=(14.0, 9.0, 20.0), method=method, weight=True, alpha_mean=0.6)
            assert relerr(mean[i], ref[1]) < 1e-9 and relerr(w[i], ref[0]) < 1e-9, (method, i)


def test_train_target_batch_three_iterations():
    """nb_it = 3: every iteration evaluates the frames under the model the previous one left, so a difference in the last bits of
    the statistics is amplified.  e_seq = relerr(sequential train_target_ex per client, oracle loop) and e_batch = relerr(batch, oracle
    loop) are measured on the same input; the bar for e_batch is 1e-9, or 10 e_seq if the sequential path itself is above 1e-9.
    Measured on an MI355X: e_seq = 1.04e-16, e_batch = 1.04e-16 -- three iterations amplify nothing visible at this size, the 1e-9 bar
    holds."""
    from lia_ral_amd import host_capi as h
    world, x, cb, sb, sl = enroll_case()
    w, mean, cov = h.train_target_batch(x, cb, sb, sl, world, nb_it=3)
    e_seq = e_batch = 0.0
    for i in range(len(cb) - 1):
        seg = (sb[cb[i]:cb[i + 1]], sl[cb[i]:cb[i + 1]])
        ref = oracle_enroll(x, seg[0], seg[1], world, 3)
        one = h.train_target_ex(x, seg[0], seg[1], world, nb_it=3)
        e_seq = max(e_seq, relerr(one[1], ref[1])); e_batch = max(e_batch, relerr(mean[i], ref[1]))
    print("nb_it = 3: e_seq = %.3e, e_batch = %.3e" % (e_seq, e_batch))
    assert e_batch < (1e-9 if e_seq <= 1e-9 else 10 * e_seq)


def test_train_target_batch_bagged_draws_follow_the_sequential_order():
    """baggedFrameProbability 0.6, two iterations: from the same srand state, the batch draws every client's selections in the order
    the client-after-client calls draw them (client-major, srand(trainIt) after each draw)"""
    import ctypes as ct
    from lia_ral_amd import host_capi as h
    world, x, cb, sb, sl = enroll_case()
    libc = ct.CDLL("libc.so.6")
    libc.srand(777)
    seq = [h.train_target_ex(x, sb[cb[i]:cb[i + 1]], sl[cb[i]:cb[i + 1]], world, nb_it=2, bagged_p=0.6) for i in range(len(cb) - 1)]
    libc.srand(777)
    w, mean, cov = h.train_target_batch(x, cb, sb, sl, world, nb_it=2, bagged_p=0.6)
    full = h.train_target_batch(x, cb, sb, sl, world, nb_it=2)[1]
    for i in range(len(cb) - 1):
        assert relerr(mean[i], seq[i][1]) < 1e-9, i
        assert relerr(mean[i], full[i]) > 1e-6                                      # the draws did leave frames out


def test_train_target_batch_unbatched_configurations_run_the_client_loop():
    """varAdapt and normalizeModel are not batched: the function runs adaptModel client after client -- the same bits"""
    from lia_ral_amd import host_capi as h
    world, x, cb, sb, sl = enroll_case()
    w, mean, cov = h.train_target_batch(x, cb[:3], sb[:cb[2]], sl[:cb[2]], world, nb_it=1, var=True)
    for i in range(2):
        one = h.train_target_ex(x, sb[cb[i]:cb[i + 1]], sl[cb[i]:cb[i + 1]], world, nb_it=1, var=True)
        assert np.array_equal(mean[i], one[1]) and np.array_equal(cov[i], one[2]) and np.array_equal(w[i], one[0])
