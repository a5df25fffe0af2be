"""Batched enrolment with variances on the GPU: gmmiv_em_stats_models judged per (segment, Gaussian, dimension) against the long double
reference of tests/em_models_ref.py, its documented bitwise properties, gmmiv_map_adapt_models_full / gmmiv_normalize_models per element,
gmmiv_gmm_batch_load_cov, and liagpu::adaptModelBatch with MAPCfg::batchVariances against the oracle loop."""
import contextlib
import functools

import numpy as np
import pytest

import em_models_ref as er
import gmm_ref as gr
from conftest import make_frames, make_gmm
from models_ref import relerr
from oracle import oracle as orc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gr.HAVE_LONGDOUBLE, reason=gr.SKIP_MESSAGE)]

REG = (14.0, 9.0, 20.0)
Z_CASE = (129, 60, 256, 2.0)           # the stored-likelihood path with more than one Gaussian group of tiles


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def options(ctx, opts):
    prev = {k: ctx.set_option(k, v) for k, v in opts.items()}
    try:
        yield
    finally:
        for k, v in prev.items():
            ctx.set_option(k, v)


def load(ctx, case):
    C, D = case[:2]
    return ctx.gmm_batch(3, C, D).load(*er.models(case))


def label(case, dtype, extra=""):
    return "%s %s%s" % (gr.case_name(case), gr.dtype_name(dtype), extra)


def judge_rows(j, case, dtype, N, F, S, L, what=""):
    C, D = case[:2]
    sb, sm = er.segments(case)
    for s, r in enumerate(er.segment_rows(case, gr.dtype_name(dtype))):
        lo, hi = int(sb[s]), int(sb[s + 1])
        if r is None:
            j("%sN seg %d (empty)" % (what, s), N[s], 0.0, 0.0)
            j("%sF seg %d (empty)" % (what, s), F[s], 0.0, 0.0)
            j("%sS seg %d (empty)" % (what, s), S[s], 0.0, 0.0)
        else:
            j("%sN seg %d" % (what, s), N[s], r["occ"], r["occ_b"])
            j("%sF seg %d" % (what, s), F[s].reshape(C, D), r["sx"], r["sx_b"])
            j("%sS seg %d" % (what, s), S[s].reshape(C, D), r["sxx"], r["sxx_b"])
        if L is not None:
            want, bar = er.reference(case, gr.dtype_name(dtype), int(sm[s])).llk_sum(lo, hi)
            j("%sseg_llk %d" % (what, s), L[s, 0], want, bar)
            if L[s, 1] != hi - lo:
                j.note("%sseg_llk %d: frame count %r, expected %d" % (what, s, L[s, 1], hi - lo))


def arrange(x, sb, sm, order):
    """the segments `order` (indices into sb / sm, repeats allowed) laid out one after the other in a new frame matrix, every one at its
    original position modulo 16 (the statistics kernels sum a segment block by block): filler frames owned by model 0 in between.
    -> (frames, seg_begin, seg_model, row of every listed segment)"""
    pieces, begin, model, rows, pos = [], [0], [], [], 0
    for s in order:
        lo, hi = int(sb[s]), int(sb[s + 1])
        pad = (lo - pos) % 16
        if pad:
            pieces.append(x[:pad]); pos += pad
            begin.append(pos); model.append(0)
        pieces.append(x[lo:hi]); pos += hi - lo
        begin.append(pos); model.append(int(sm[s])); rows.append(len(model) - 1)
    return np.ascontiguousarray(np.concatenate(pieces)), np.array(begin, np.int64), np.array(model, np.int32), rows


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("case", er.EM_CASES, ids=gr.case_name)
def test_em_stats_rows_per_element_and_their_bits(ctx, case, dtype):
    """every element of N, F, S against its bar; then the same bits for every segment as the only one of the call, for the segments in
    reverse order (a new frame matrix), for three copies of the list under the smallest scratch options (z_scratch_mb 1: chunks of
    512 frames at 129 x 60; models_scratch_mb 0: one model per chunk), and z_waves 4 within the bars"""
    b = load(ctx, case)
    x = gr.frames(case, dtype)
    sb, sm = er.segments(case)
    N, F, S, L = b.em_stats(x, sb, sm)
    j = er.Judge(label(case, dtype))
    judge_rows(j, case, dtype, N, F, S, L)
    for s in range(len(sm)):
        N1, F1, S1, L1 = b.em_stats(x, sb[s:s + 2], sm[s:s + 1])
        for name, a, full in (("N", N1, N), ("F", F1, F), ("S", S1, S), ("seg_llk", L1, L)):
            j.same_bits("segment %d alone, %s" % (s, name), a[0], full[s])
    order = list(range(len(sm)))
    for what, ordr, opts in (("reversed", order[::-1], {}), ("three copies, smallest scratch", order * 3, {"z_scratch_mb": 1, "models_scratch_mb": 0, "timing": 1})):
        xa, ba, ma, rows = arrange(x, sb, sm, ordr)
        with options(ctx, opts):
            Na, Fa, Sa, La = b.em_stats(xa, ba, ma)
            launches = ctx.kernel_launches("k_gmm_pack") if opts else 0
        if opts and case[1] <= 60 and launches < 2:
            j.note("%s: %d launches of k_gmm_pack, the call was not cut into chunks" % (what, launches))
        for s, row in zip(ordr, rows):
            for name, a, full in (("N", Na, N), ("F", Fa, F), ("S", Sa, S), ("seg_llk", La, L)):
                j.same_bits("%s: segment %d, %s" % (what, s, name), a[row], full[s])
    with options(ctx, {"z_waves": 4}):
        N4, F4, S4, L4 = b.em_stats(x, sb, sm)
    judge_rows(j, case, dtype, N4, F4, S4, L4, "z_waves 4: ")
    b.close()
    j.finish()


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
def test_em_stats_on_device_tensors_in_a_wider_matrix(ctx, dtype):
    """frames as rows of a wider device matrix, device outputs: the bits of the host-array call (the call only enqueues: ctx.sync() first)"""
    import torch
    case = Z_CASE
    C, D, T, _ = case
    b = load(ctx, case)
    x = gr.frames(case, dtype)
    sb, sm = er.segments(case)
    N, F, S, L = b.em_stats(x, sb, sm)
    wide = torch.full((T, D + 5), 1e30, dtype=torch.from_numpy(x).dtype, device="cuda")     # the filler must never be read as a feature
    wide[:, :D] = torch.from_numpy(x).cuda()
    mk = lambda n: torch.full((len(sm), n), 7.5, dtype=torch.float64, device="cuda")
    Nd, Fd, Sd, Ld = mk(C), mk(C * D), mk(C * D), mk(2)
    torch.cuda.synchronize()
    b.em_stats(wide[:, :D], sb, sm, N=Nd, F=Fd, S=Sd, seg_llk=Ld)
    ctx.sync()
    j = er.Judge(label(case, dtype, " ldx=D+5"))
    for name, a, h in (("N", Nd, N), ("F", Fd, F), ("S", Sd, S), ("seg_llk", Ld, L)):
        j.same_bits("device %s" % name, a.cpu().numpy(), h)
    judge_rows(j, case, dtype, Nd.cpu().numpy(), Fd.cpu().numpy(), Sd.cpu().numpy(), Ld.cpu().numpy(), "device: ")
    b.close()
    j.finish()


@pytest.mark.parametrize("case", [Z_CASE, (40, 61, 66, 2.0)], ids=gr.case_name)
def test_one_segment_under_one_model_against_em_accumulate(ctx, case):
    """both are within their bars of the same reference, so they differ by at most two bars"""
    C, D = case[:2]
    b = load(ctx, case)
    x = gr.frames(case, np.float32)
    sb, sm = er.segments(case)
    s = 3
    lo, hi, k = int(sb[s]), int(sb[s + 1]), int(sm[s])
    N, F, S, L = b.em_stats(x, sb[s:s + 2], sm[s:s + 1])
    g = ctx.gmm(*er.model(case, k))
    a = g.split_acc(g.em_accumulate(np.ascontiguousarray(x[lo:hi])))
    r = er.segment_rows(case, "float32")[s]
    j = er.Judge(label(case, np.float32, " segment %d" % s))
    for name, got, acc in (("occ", N[0], a["occ"]), ("sx", F[0].reshape(C, D), a["sx"]), ("sxx", S[0].reshape(C, D), a["sxx"])):
        j("em_accumulate %s" % name, acc, r[name], r[name + "_b"])
        j("em_stats - em_accumulate %s" % name, got, acc.astype(gr.LD), 2 * r[name + "_b"])
    if a["count"] != L[0, 1] or abs(a["llk"] - L[0, 0]) > 1e-9 * (hi - lo):
        j.note("count / log-likelihood sum differ: %r %r, %r %r" % (a["count"], L[0, 1], a["llk"], L[0, 0]))
    g.close(); b.close()
    j.finish()


@pytest.mark.parametrize("case", [Z_CASE, (40, 97, 66, 0.5)], ids=gr.case_name)
def test_degenerate_frames_are_left_out_and_counted_once(ctx, case):
    """a NaN frame and a frame 1e6 away from every mean: nothing added to N / F / S, counted as gmmiv_tv_stats_models counts them"""
    C, D = case[:2]
    b = load(ctx, case)
    x = gr.frames(case, np.float32).copy()
    sb, sm = er.segments(case)
    t_nan, t_far = int(sb[0]) + 5, int(sb[3]) + 9
    x[t_nan, D // 2] = np.nan
    x[t_far, :] = 1e6
    ctx.set_option("zero_llk_frames", 0); ctx.set_option("screened_frames", 0)
    N, F, S, L = b.em_stats(x, sb, sm)
    counted = (ctx.set_option("zero_llk_frames", 0), ctx.set_option("screened_frames", 0))
    Nt, Ft, Lt = b.tv_stats(x, sb, sm)
    counted_tv = (ctx.set_option("zero_llk_frames", 0), ctx.set_option("screened_frames", 0))
    assert counted == counted_tv == (2, 1)
    assert np.array_equal(L, Lt)
    j = er.Judge(label(case, np.float32, " degenerate"))
    clean = gr.frames(case, np.float32)
    for s, t in ((0, t_nan), (3, t_far)):
        lo, hi = int(sb[s]), int(sb[s + 1])
        assert L[s, 1] == hi - lo - 1
        w, mean, iv = er.model(case, int(sm[s]))
        r = gr.Reference(w, mean, iv, np.delete(clean[lo:hi], t - lo, axis=0)).sums()
        j("N seg %d" % s, N[s], r["occ"], r["occ_b"])
        j("F seg %d" % s, F[s].reshape(C, D), r["sx"], r["sx_b"])
        j("S seg %d" % s, S[s].reshape(C, D), r["sxx"], r["sxx_b"])
    b.close()
    j.finish()


# ---------------------------------------------------------------- computeMAP with the variance branch
@pytest.fixture(scope="module")
def device_stats(ctx):
    """the device's own statistics rows of Z_CASE (float32 frames), with one Gaussian of segment 0 emptied; read-only"""
    case = Z_CASE
    b = load(ctx, case)
    sb, sm = er.segments(case)
    N, F, S, L = b.em_stats(gr.frames(case, np.float32), sb, sm)
    b.close()
    N[0, 64] = 0.0
    ws, means, ivs = er.models(case)
    w0, mean0, iv0 = er.model(case, 0)
    out = (N, F, S, np.ascontiguousarray(L[:, 1]), w0, mean0, 1.0 / iv0, np.ascontiguousarray(means[sm].reshape(len(sm), -1)),
           np.ascontiguousarray((1.0 / ivs[sm]).reshape(len(sm), -1)))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("weight", [False, True])
@pytest.mark.parametrize("method", er.METHODS)
def test_map_adapt_full_without_var_adapt_gives_the_bits_of_map_adapt_models(ctx, device_stats, method, weight):
    N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov = device_stats
    C, D = mean0.shape
    b = ctx.gmm_batch(len(N), C, D)
    m, w = b.map_adapt(N, F, count, w0, mean0, cur_mean, method, True, weight, REG, 0.6)
    for var in (False, True):                                          # the mean and the weights do not depend on var_adapt
        mf, cf, wf, st = b.map_adapt_full(N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov, method, True, var, weight, REG, 0.6)
        assert np.array_equal(mf, m) and np.array_equal(wf, w), (method, weight, var)
    mf, cf, wf, st = b.map_adapt_full(N, F, None, count, w0, mean0, cov0, cur_mean, None, method, True, False, weight, REG, 0.6, want=("mean", "w"))
    assert cf is None and np.array_equal(mf, m) and np.array_equal(wf, w) and not st.any()
    if method != "ML":
        _, cf, _, st = b.map_adapt_full(N, F, None, count, w0, mean0, cov0, cur_mean, None, method, True, False, weight, REG, 0.6, want=("cov",))
        assert np.array_equal(cf, np.broadcast_to(cov0.ravel(), cf.shape)) and not st.any()      # var_adapt = 0: the a-priori variances
    b.close()


@pytest.mark.parametrize("method", er.METHODS)
def test_map_adapt_full_variance_branch_per_element(ctx, device_stats, method):
    """on the device's own statistics, against the long double computeMAP; the Gaussian without occupancy; device tensors"""
    import torch
    N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov = device_stats
    G, (C, D) = len(N), mean0.shape
    b = ctx.gmm_batch(G, C, D)
    ref = er.map_ld(N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov, method, True, True, True, REG, 0.6)
    m, c, w, st = b.map_adapt_full(N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov, method, True, True, True, REG, 0.6)
    j = er.Judge("map_adapt_full %s" % method)
    j("mean", m.reshape(G, C, D), ref["mean"], ref["mean_b"])
    j("cov", c.reshape(G, C, D), ref["cov"], ref["cov_b"])
    j("w", w, ref["w"], ref["w_b"])
    cm, cc = cur_mean.reshape(G, C, D), cur_cov.reshape(G, C, D)
    if method == "ML":                                                 # N = 0: the current mean and variance, weight 0
        j.same_bits("N = 0 mean", m.reshape(G, C, D)[0, 64], cm[0, 64])
        j.same_bits("N = 0 cov", c.reshape(G, C, D)[0, 64], cc[0, 64])
        j.same_bits("N = 0 weight", w[0, 64], 0.0)
    elif method in ("MAPOccDep", "MAPModelBased"):                     # alpha = 0: the a-priori mean and variance
        j.same_bits("N = 0 mean", m.reshape(G, C, D)[0, 64], mean0[64])
        j.same_bits("N = 0 cov", c.reshape(G, C, D)[0, 64], cov0[64])
    bad = ~((c > 0) & np.isfinite(c))                                  # (the ML variance of the one-frame segment is x^2 - x^2)
    if not np.array_equal(st, bad.sum(1)) or (method != "ML" and st.any()):
        j.note("status %r, the output has %r entries that are not positive and finite" % (st, bad.sum(1)))
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    md, cd, wd, sd = b.map_adapt_full(dev(N), dev(F), dev(S), dev(count), dev(w0), dev(mean0), dev(cov0), dev(cur_mean), dev(cur_cov), method, True, True,
                                      True, REG, 0.6)
    ctx.sync()
    for name, a, h in (("mean", md, m), ("cov", cd, c), ("w", wd, w), ("status", sd, st)):
        j.same_bits("device %s" % name, a.cpu().numpy(), h)
    b.close()
    j.finish()


@pytest.mark.parametrize("method", ["MAPOccDep", "ML"])
def test_map_adapt_full_status_counts_a_planted_non_positive_variance(ctx, device_stats, method):
    N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov = device_stats
    G, (C, D) = len(N), mean0.shape
    b = ctx.gmm_batch(G, C, D)
    _, c0, _, st0 = b.map_adapt_full(N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov, method, True, True, False, REG, 0.6)
    S = S.copy()
    g2, g3 = int(np.argmax(N[2])), int(np.argmax(N[3]))                # the best occupied Gaussians: their clean variances are positive
    assert (c0.reshape(G, C, D)[2, g2] > 0).all() and (c0.reshape(G, C, D)[3, g3] > 0).all()
    S.reshape(G, C, D)[2, g2, :4] = -1e6 * N[2, g2]                    # S / N = -1e6: four variances of model 2 below zero
    S.reshape(G, C, D)[3, g3, 1] = np.nan
    _, c, _, st = b.map_adapt_full(N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov, method, True, True, False, REG, 0.6)
    bad = ~((c > 0) & np.isfinite(c))
    assert st.dtype == np.int32 and np.array_equal(st, bad.sum(1))
    assert np.array_equal(st - st0, [0, 0, 4, 1, 0])
    assert bad.reshape(G, C, D)[2, g2, :4].all() and bad.reshape(G, C, D)[3, g3, 1]
    b.close()


# ---------------------------------------------------------------- normalizeMixture
@pytest.mark.parametrize("mean_only", [False, True])
@pytest.mark.parametrize("case", [Z_CASE, (37, 17, 300, 2.0)], ids=gr.case_name)
def test_normalize_models_per_element(ctx, case, mean_only):
    """nb_it = 1 per element against the long double fold; nb_it = 2 is the bits of two calls with nb_it = 1, whose second step is
    judged on its own input; weights per model and shared"""
    import torch
    C, D = case[:2]
    ws, means, ivs = er.models(case)
    covs = 1.0 / ivs
    b = ctx.gmm_batch(3, C, D)
    dev = lambda a: torch.from_numpy(np.array(a.reshape(3, -1), order="C")).cuda()
    j = er.Judge("normalize %s mean_only %d" % (gr.case_name(case), mean_only))

    def step(m_in, c_in, name):
        m, c = dev(m_in), dev(c_in)
        b.normalize(ws, m, c, 1, mean_only)
        ctx.sync()
        m, c = m.cpu().numpy().reshape(3, C, D), c.cpu().numpy().reshape(3, C, D)
        for k in range(3):
            nm, nc, mb, cb = er.normalize_ld(ws[k], m_in[k], c_in[k], mean_only)
            j("%s mean, model %d" % (name, k), m[k], nm, mb)
            j("%s cov, model %d" % (name, k), c[k], nc, cb)
        return m, c

    m1, c1 = step(means, covs, "first iteration")
    m2, c2 = step(m1, c1, "second iteration")
    m, c = dev(means), dev(covs)
    b.normalize(ws, m, c, 2, mean_only)
    ctx.sync()
    j.same_bits("nb_it 2 mean", m.cpu().numpy().reshape(3, C, D), m2)
    j.same_bits("nb_it 2 cov", c.cpu().numpy().reshape(3, C, D), c2)
    if mean_only:
        j.same_bits("mean_only leaves the variances", c2, covs)
    m, c = dev(means), dev(covs)
    b.normalize(ws[0], m, c, 1, mean_only)                             # one weight vector shared by the three models
    ctx.sync()
    nm, nc, mb, cb = er.normalize_ld(ws[0], means[2], covs[2], mean_only)
    j("shared weights mean, model 2", m.cpu().numpy().reshape(3, C, D)[2], nm, mb)
    j("shared weights cov, model 2", c.cpu().numpy().reshape(3, C, D)[2], nc, cb)
    b.close()
    j.finish()


@pytest.mark.parametrize("case", [Z_CASE, (37, 17, 300, 2.0)], ids=gr.case_name)
def test_batch_load_cov_packs_the_bits_of_load_with_the_reciprocal(ctx, case):
    import torch
    C, D = case[:2]
    ws, means, ivs = er.models(case)
    covs = 1.0 / ivs
    b1 = ctx.gmm_batch(3, C, D).load(ws, means, 1.0 / covs)
    b2 = ctx.gmm_batch(3, C, D).load_cov(ws, means, covs)
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    b3 = ctx.gmm_batch(3, C, D).load_cov(dev(ws[1]), dev(means), dev(covs[1]))           # device tables, shared weights and variances
    b4 = ctx.gmm_batch(3, C, D).load(ws[1], means, 1.0 / covs[1])
    for g in range(3):
        assert np.array_equal(b1.packed(g), b2.packed(g)), g
        assert np.array_equal(b3.packed(g), b4.packed(g)), g
    x = gr.frames(case, np.float32)
    sb, sm = er.segments(case)
    for a, c in zip(b1.em_stats(x, sb, sm), b2.em_stats(x, sb, sm)):
        assert np.array_equal(a, c)
    for b in (b1, b2, b3, b4):
        b.close()


# ---------------------------------------------------------------- the host layer: adaptModelBatch with MAPCfg::batchVariances
def oracle_enroll(x, seg_begin, seg_len, world, nb_it, reg=(16.0, 16.0, 16.0), method="MAPOccDep", normalize=False, **kw):
    """adaptModel restated on the oracle: nb_it x (EM statistics under the current client model, ML estimate, computeMAP, normalizeMixture)"""
    xd = x.astype(np.float64)
    fr = np.concatenate([np.arange(b, b + n) for b, n in zip(seg_begin, seg_len)])
    cw, cm, cc = [np.array(a, np.float64) for a in world]
    for _ in range(nb_it):
        acc = orc.em_accumulate(orc.Gmm(cw, cm, 1.0 / cc), xd[fr])
        mw, mm, mc = orc.em_get(acc, cm, cc)
        cw, cm, cc = orc.compute_map(method, world, (mw, mm, mc), float(int(acc["count"])), reg=reg, **kw)
        if normalize:
            cm, cc = orc.normalize_mixture(cw, cm, cc, 1, False)
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


def model_err(got, ref):
    """the largest of the three tables' errors, each normalised by its largest reference entry"""
    return max(relerr(np.asarray(g), np.asarray(r)) for g, r in zip(got, ref))


@pytest.mark.parametrize("nb_it,normalize", [(1, False), (3, False), (1, True), (3, True)])
def test_train_target_batch_with_variances_matches_the_oracle_loop(nb_it, normalize):
    """var=True, weight=True (and normalizeModel) with batch_variances=True, judged like test_train_target_batch_three_iterations: e_seq =
    the per-client path against the oracle loop, e_batch = the batch against the oracle loop, on the same input, over weights, means and
    variances (each table normalised by its largest entry); the bar for e_batch is 1e-9, or 10 e_seq where the sequential path itself
    is above 1e-9 (another summation order fed through the next iteration's posteriors).
    Both values are printed.  Not yet measured on an MI355X (none was available when the test was written): the pairs go here."""
    from lia_ral_amd import host_capi as h
    world, x, cb, sb, sl = enroll_case()
    kw = dict(nb_it=nb_it, var=True, weight=True, reg=REG, normalize=normalize)
    got = h.train_target_batch(x, cb, sb, sl, world, batch_variances=True, **kw)
    e_seq = e_batch = 0.0
    for i in range(len(cb) - 1):
        seg = (sb[cb[i]:cb[i + 1]], sl[cb[i]:cb[i + 1]])
        ref = oracle_enroll(x, seg[0], seg[1], world, nb_it, reg=REG, normalize=normalize, var=True, weight=True)
        one = h.train_target_ex(x, seg[0], seg[1], world, **kw)
        e_seq = max(e_seq, model_err(one, ref)); e_batch = max(e_batch, model_err([t[i] for t in got], ref))
    print("nb_it = %d, normalize = %s: e_seq = %.3e, e_batch = %.3e" % (nb_it, normalize, e_seq, e_batch))
    assert e_batch < (1e-9 if e_seq <= 1e-9 else 10 * e_seq)


def test_train_target_batch_with_variances_bagged_and_without_the_flag():
    """baggedFrameProbability 0.6, two iterations: the draws follow the sequential order, so from the same srand state the batch meets the
    client-after-client calls (which stand in for the oracle loop: it does not draw) to 1e-9.  Without the flag var=True still runs the
    per-client loop: its bits."""
    import ctypes as ct
    from lia_ral_amd import host_capi as h
    world, x, cb, sb, sl = enroll_case()
    kw = dict(nb_it=2, bagged_p=0.6, var=True, reg=REG)
    libc = ct.CDLL("libc.so.6")
    libc.srand(777)
    seq = [h.train_target_ex(x, sb[cb[i]:cb[i + 1]], sl[cb[i]:cb[i + 1]], world, **kw) for i in range(len(cb) - 1)]
    libc.srand(777)
    got = h.train_target_batch(x, cb, sb, sl, world, batch_variances=True, **kw)
    libc.srand(777)
    loop = h.train_target_batch(x, cb, sb, sl, world, **kw)
    full = h.train_target_batch(x, cb, sb, sl, world, batch_variances=True, nb_it=2, var=True, reg=REG)
    e = 0.0
    for i in range(len(cb) - 1):
        e = max(e, model_err([t[i] for t in got], seq[i]))
        assert all(np.array_equal(t[i], q) for t, q in zip(loop, seq[i])), i                 # no flag: the per-client loop
        assert relerr(got[2][i], full[2][i]) > 1e-6                                          # the draws did leave frames out
    print("bagged 0.6, nb_it = 2: batch against the sequential calls %.3e" % e)
    assert e < 1e-9
