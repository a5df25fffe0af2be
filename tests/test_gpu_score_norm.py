"""Score normalisation (include/gmmiv.h, "score normalisation") against a numpy restatement of the reference,
LIA_SpkDet/ComputeNorm/src/ComputeNorm.cpp, written as the reference runs: descending sort, slice, sequential accumulation.

Bounds (no constant tolerance).  Any summation order satisfies |fl(sum) - sum| <= (n - 1) u sum|x| with u = 2^-53, so two orders
(the device's and the checker's) differ by at most twice that.  With size = the kept scores:
    |mean - mean_ref|   <= 2 (size - 1) u mean|x| + 2 ulp(mean_ref)                                     =: dm
    |msq  - msq_ref|    <= 2 (size - 1) u mean(x^2) + 2 ulp(msq_ref)                                    =: dq     (msq = sum2 / size)
    var = msq - mean * mean (one rounded product, one rounded subtraction on each side):
    |var - var_ref|     <= dq + 2 |mean_ref| dm + dm^2 + 2 u (msq_ref + mean_ref^2)                     =: dvar
    |std - std_ref|     <= dvar / std_ref + 2 ulp(std_ref)           (sqrt a - sqrt b = (a - b) / (sqrt a + sqrt b))
meanMode 1: the median is an order statistic (exact); the mean absolute deviation obeys the bound of a mean, over |x - median|.
On integer scores in [-50, 50] every partial sum and square sum is exact in any order: results must be np.array_equal."""
import time

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

U = 2.0 ** -53
NS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 16383, 16384, 16385, 100003]
PCTS = [(0.0, 0.0), (0.1, 0.0), (0.0, 0.1), (0.05, 0.2), (0.29, 0.3), (0.5, 0.49)]


# ---- the checker ------------------------------------------------------------------------------------------------------------
def seq_sum(v):
    """sum += v[i] for i in order (ComputeNorm.cpp:140-143, :149-150): np.cumsum accumulates sequentially."""
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


def ref_mean_std(scores, mode, pH, pL):
    """DistribNorm::computeMeanStd, ComputeNorm.cpp:121-159.  Returns (mean, std, kept scores)."""
    x = np.asarray(scores, dtype=np.float64)
    n = len(x)
    assert n > 0                                                       # :122
    begin, end, size = 0, n, n                                         # :124-126
    if pH != 0 or pL != 0:                                             # :127
        x = np.sort(x, kind="stable")[::-1]                            # :128 descendingSort
        dH, dL = int(float(n) * pH), int(float(n) * pL)                # :129-130 (unsigned long)((double)size * percent)
        size -= dH + dL                                                # :131
        begin, end = dH, n - dL                                        # :132-133
    kept = x[begin:end]
    assert size > 0 and len(kept) == size
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == 0:
            s, s2 = seq_sum(kept), seq_sum(kept * kept)                # :140-143
            mean = np.float64(s) / np.float64(size)                    # :144
            std = np.sqrt(np.float64(s2) / np.float64(size) - mean * mean)   # :145
        else:
            mean = kept[size // 2]                                     # :148
            std = np.float64(seq_sum(np.abs(kept - mean))) / np.float64(size)   # :149-151
    return mean, std, kept


def ref_stats(A, axis, mode, pH, pL, select=None, pre=None):
    """Every distribution of a cohort matrix; selectImp (:436-445) as a mask along the cohort axis, the first normalisation of
    getAllScoresFirstNormed (:466-489) as numpy's (x - m) / s."""
    A = np.asarray(A, dtype=np.float64)
    D = A if axis == 0 else A.T
    with np.errstate(invalid="ignore", divide="ignore"):
        if pre is not None:
            D = (D - pre[0][None, :]) / pre[1][None, :]
    if select is not None:
        D = D[:, np.asarray(select) != 0]
    res = [ref_mean_std(r, mode, pH, pL) for r in D]
    return np.array([r[0] for r in res]), np.array([r[1] for r in res]), [r[2] for r in res]


def ulp(v):
    return np.spacing(np.abs(v))


def bounds(mean_ref, std_ref, kept, mode, E=0.0):
    """(bound on |mean - mean_ref|, bound on |std - std_ref|) from the data, see the module docstring.  E: what each INPUT score
    may differ by between the two sides (the chains feed normalised scores whose parameters carry their own error).  Order
    statistics, and with them the trimmed mean, move by at most E when every score moves by at most E; a square by at most
    E (2 |x| + E); an absolute deviation from the median by at most 2 E."""
    size = len(kept)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == 1:
            dev = np.abs(kept - mean_ref)
            return E, 2 * E + 2 * (size - 1) * U * dev.mean() + 2 * ulp(std_ref)
        dm = E + 2 * (size - 1) * U * np.abs(kept).mean() + 2 * ulp(mean_ref)
        msq = (kept * kept).mean()
        dq = E * (2 * np.abs(kept).max() + E) + 2 * (size - 1) * U * msq + 2 * ulp(msq)
        dvar = dq + 2 * abs(mean_ref) * dm + dm * dm + 2 * U * (msq + mean_ref * mean_ref)
        # |sqrt a - sqrt b| <= |a - b| / sqrt b, and <= sqrt |a - b| (the one that is left when std_ref == 0)
        return dm, min(dvar / std_ref if std_ref > 0 else np.inf, np.sqrt(dvar)) + 2 * ulp(std_ref)


def check_within(got_m, got_s, ref, mode, what):
    rm, rs, kept = ref
    for i in range(len(rm)):
        bm, bs = bounds(rm[i], rs[i], kept[i], mode)
        em, es = abs(got_m[i] - rm[i]), abs(got_s[i] - rs[i])
        assert em <= bm and es <= bs, (what, i, em, bm, es, bs)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lia_ral_amd import capi
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)       # ordered with the torch work of the tests
    yield c
    c.close()


def masked(rng, n):
    """a cohort axis of length L > n with exactly n selected positions"""
    L = n + max(1, n // 3)
    sel = np.zeros(L, np.uint8)
    sel[rng.choice(L, n, replace=False)] = 1
    return L, sel


# ---- 1. exact on exactly-summable data --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_integer_scores_are_exact(ctx, n):
    rng = np.random.default_rng(n)
    nd = 3
    for use_mask in (False, True):
        L, sel = masked(rng, n) if use_mask else (n, None)
        for axis in (0, 1):
            A = rng.integers(-50, 51, size=(nd, L) if axis == 0 else (L, nd)).astype(np.float64)
            for mode in (0, 1):
                for pH, pL in PCTS:
                    size = n - int(n * pH) - int(n * pL)
                    assert size >= 1                       # none of the listed combinations has an empty kept range
                    m, s = ctx.score_cohort_stats(A, axis, select=sel, mean_mode=mode, percent_h=pH, percent_l=pL)
                    rm, rs, _ = ref_stats(A, axis, mode, pH, pL, sel)
                    assert same(m, rm) and same(s, rs), (n, use_mask, axis, mode, pH, pL, m, rm, s, rs)


def test_constant_negative_and_input_order_median(ctx):
    rng = np.random.default_rng(5)
    for L in (1, 7, 300, 5000, 20000):
        A = np.vstack([np.full(L, 7.0), np.full(L, -3.0), -rng.integers(1, 50, L).astype(np.float64),
                       rng.integers(-50, 51, L).astype(np.float64)])
        for axis, B in ((0, A), (1, np.ascontiguousarray(A.T))):
            for mode in (0, 1):
                for pH, pL in PCTS:
                    if L - int(L * pH) - int(L * pL) < 1:
                        continue
                    m, s = ctx.score_cohort_stats(B, axis, mean_mode=mode, percent_h=pH, percent_l=pL)
                    rm, rs, _ = ref_stats(B, axis, mode, pH, pL)
                    assert same(m, rm) and same(s, rs), (L, axis, mode, pH, pL)
        # the quirk: meanMode 1 without discards takes the score at n / 2 in INPUT order (:148 without :128)
        m, _ = ctx.score_cohort_stats(A, 0, mean_mode=1)
        assert same(m, A[:, L // 2])
        sel = np.zeros(L, np.uint8)
        sel[::2] = 1
        m, _ = ctx.score_cohort_stats(A, 0, select=sel, mean_mode=1)
        assert same(m, A[:, ::2][:, ((L + 1) // 2) // 2])


def test_key_mapping_on_zeros_denormals_and_huge_values(ctx):
    rng = np.random.default_rng(11)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e300, -1e300, 1e300, -1e300, 2.2250738585072014e-308])
    for L in (64, 1000, 20000):
        rows = []
        for _ in range(4):
            r = np.concatenate([special, rng.integers(-50, 51, L - len(special)).astype(np.float64)])
            rng.shuffle(r)
            rows.append(r)
        A = np.array(rows)
        for axis, B in ((0, A), (1, np.ascontiguousarray(A.T))):
            for pH, pL in PCTS[1:]:
                m, _ = ctx.score_cohort_stats(B, axis, mean_mode=1, percent_h=pH, percent_l=pL)
                rm, _, _ = ref_stats(B, axis, 1, pH, pL)
                assert same(m, rm), (L, axis, pH, pL, m, rm)           # the selected order statistic
            for pH, pL in ((0.05, 0.2), (0.29, 0.3)):                  # both discards remove the two +-1e300
                assert int(L * pH) >= 2 and int(L * pL) >= 2
                m, s = ctx.score_cohort_stats(B, axis, percent_h=pH, percent_l=pL)
                check_within(m, s, ref_stats(B, axis, 0, pH, pL), 0, ("special", L, axis, pH, pL))


def test_empty_kept_range(ctx):
    import torch
    from lia_ral_amd import capi
    with pytest.raises(capi.GmmivError, match="2 scores"):
        ctx.score_cohort_stats(np.array([[1.0, 2.0]]), 0, percent_h=0.5, percent_l=0.5)
    with pytest.raises(capi.GmmivError, match="0 scores"):
        ctx.score_cohort_stats(np.array([[1.0]]), 0, select=np.zeros(1, np.uint8))
    # a device-resident mask is counted on the device: nothing is read back, the empty range gives NaN
    A = torch.tensor([[1.0, 2.0, 3.0]], dtype=torch.float64, device="cuda")
    m = torch.zeros(1, dtype=torch.float64, device="cuda")
    s = torch.zeros(1, dtype=torch.float64, device="cuda")
    ctx.score_cohort_stats(A, 0, select=torch.zeros(3, dtype=torch.uint8, device="cuda"), out_mean=m, out_std=s)
    ctx.score_cohort_stats(A.t().contiguous(), 1, select=torch.zeros(3, dtype=torch.uint8, device="cuda"), out_mean=m, out_std=s)
    torch.cuda.synchronize()
    assert bool(torch.isnan(m).all()) and bool(torch.isnan(s).all())
    sel = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    ctx.score_cohort_stats(A, 0, select=sel, percent_h=0.5, percent_l=0.5, out_mean=m, out_std=s)     # 2 scores, 1 + 1 discarded
    torch.cuda.synchronize()
    assert bool(torch.isnan(m).all()) and bool(torch.isnan(s).all())
    ctx.score_cohort_stats(A, 0, select=sel, mean_mode=1, out_mean=m, out_std=s)                      # input-order median: 3.0
    torch.cuda.synchronize()
    assert m.item() == 3.0 and s.item() == 1.0


def test_argument_errors(ctx):
    from lia_ral_amd import capi
    A = np.zeros((3, 4))
    for kw in (dict(percent_h=1.0), dict(percent_l=-0.1), dict(mean_mode=2)):
        with pytest.raises(capi.GmmivError):
            ctx.score_cohort_stats(A, 0, **kw)
    with pytest.raises(capi.GmmivError):
        ctx.score_cohort_stats(A, 2)
    with pytest.raises(capi.GmmivError):
        ctx.score_normalize(A, 7, row_mean=np.zeros(3), row_std=np.ones(3))
    with pytest.raises(capi.GmmivError):
        ctx.score_normalize(A, capi.NORM_ZT, row_mean=np.zeros(3), row_std=np.ones(3))       # column vectors missing
    m, s = ctx.score_cohort_stats(np.zeros((0, 4)), 0)                                       # no distribution: a no-op
    assert len(m) == 0 and len(s) == 0


# ---- 2. real-valued data within the derived bound ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 16384, 100003])
def test_real_scores_within_the_derived_bound(ctx, n):
    rng = np.random.default_rng(100 + n)
    nd = 4
    for use_mask in (False, True):
        L, sel = masked(rng, n) if use_mask else (n, None)
        for use_pre in (False, True):
            pre = (rng.normal(-2.0, 0.3, L), rng.uniform(0.5, 2.0, L)) if use_pre else None
            for axis in (0, 1):
                A = rng.normal(-2.0, 1.5, size=(nd, L) if axis == 0 else (L, nd))
                for mode in (0, 1):
                    for pH, pL in ((0.0, 0.0), (0.05, 0.2), (0.29, 0.3)):
                        m, s = ctx.score_cohort_stats(A, axis, select=sel, pre_mean=pre[0] if pre else None,
                                                      pre_std=pre[1] if pre else None, mean_mode=mode, percent_h=pH, percent_l=pL)
                        ref = ref_stats(A, axis, mode, pH, pL, sel, pre)
                        if mode == 1:
                            assert same(m, ref[0]), (n, use_mask, use_pre, axis, pH, pL)      # selection is exact
                        check_within(m, s, ref, mode, (n, use_mask, use_pre, axis, mode, pH, pL))


# ---- 3. axis agreement, ld > cols -----------------------------------------------------------------------------------------
def test_axes_agree_and_strided_views_match_packed_copies(ctx):
    import torch
    rng = np.random.default_rng(3)
    for shape in ((37, 501), (700, 96), (1, 1), (5000, 17)):
        Ai = rng.integers(-50, 51, size=shape).astype(np.float64)
        Ar = rng.normal(-2.0, 1.5, size=shape)
        for mode in (0, 1):
            for pH, pL in ((0.0, 0.0), (0.05, 0.2)):
                if min(shape) - int(min(shape) * pH) - int(min(shape) * pL) < 1:
                    continue
                kw = dict(mean_mode=mode, percent_h=pH, percent_l=pL)
                mc, sc = ctx.score_cohort_stats(Ai, 1, **kw)
                mr, sr = ctx.score_cohort_stats(np.ascontiguousarray(Ai.T), 0, **kw)
                assert same(mc, mr) and same(sc, sr), (shape, mode, pH, pL)
                mc, sc = ctx.score_cohort_stats(Ar, 1, **kw)
                check_within(mc, sc, ref_stats(np.ascontiguousarray(Ar.T), 0, mode, pH, pL), mode, ("axes", shape, mode, pH, pL))
                # a view with ld = cols + 5 gives the bits of its packed copy, on both axes
                big = torch.zeros((shape[0], shape[1] + 5), dtype=torch.float64, device="cuda")
                big[:, :shape[1]] = torch.from_numpy(Ar).cuda()
                view = big[:, :shape[1]]
                for axis in (0, 1):
                    nd = shape[axis]
                    om = torch.empty(nd, dtype=torch.float64, device="cuda"); os_ = torch.empty_like(om)
                    ctx.score_cohort_stats(view, axis, out_mean=om, out_std=os_, **kw)
                    torch.cuda.synchronize()
                    pm_, ps_ = ctx.score_cohort_stats(Ar, axis, **kw)
                    assert same(om.cpu().numpy(), pm_) and same(os_.cpu().numpy(), ps_), (shape, axis, mode, pH, pL)


# ---- 4. apply is exact ------------------------------------------------------------------------------------------------------
def ref_apply(X, order, rm, rs, cm, cs):
    """the chains of ComputeNorm.cpp:530-751 in matrix form: every step is (x - mean) / std"""
    with np.errstate(invalid="ignore", divide="ignore"):
        z = lambda Y: (Y - rm[:, None]) / rs[:, None]
        t = lambda Y: (Y - cm[None, :]) / cs[None, :]
        if order == 0:
            return z(X), None
        if order == 1:
            return t(X), None
        first = t(X) if order == 2 else z(X)
        return (z(first) if order == 2 else t(first)), first


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (129, 257), (4100, 4233)])
def test_apply_is_exact(ctx, shape):
    import torch
    M, S = shape
    rng = np.random.default_rng(M * 7 + S)
    X = rng.normal(-2.0, 1.5, size=shape)
    rm, cm = rng.normal(-2.0, 0.5, M), rng.normal(-2.0, 0.5, S)
    rs, cs = rng.uniform(0.3, 3.0, M), rng.uniform(0.3, 3.0, S)
    rs[M // 2] = 0.0                                            # a constant cohort: Inf / NaN in the same cells
    cs[S // 3] = 0.0
    X[M // 2, S // 2] = rm[M // 2]                              # 0 / 0
    for order in range(4):
        ref, ref_first = ref_apply(X, order, rm, rs, cm, cs)
        got, first = X.copy(), np.full(shape, 99.0)
        ctx.score_normalize(got, order, rm, rs, cm, cs, first_out=first)
        assert same(got, ref), (shape, order)
        assert same(first, ref_first) if order >= 2 else np.all(first == 99.0)
        got2 = ctx.score_normalize(X.copy(), order, rm, rs, cm, cs)          # without the second output
        assert same(got2, ref)
    # device-resident, the matrix used in place
    Xd = torch.from_numpy(X).cuda()
    Fd = torch.empty_like(Xd)
    d = lambda v: torch.from_numpy(v).cuda()
    ctx.score_normalize(Xd, 3, d(rm), d(rs), d(cm), d(cs), first_out=Fd)
    torch.cuda.synchronize()
    ref, ref_first = ref_apply(X, 3, rm, rs, cm, cs)
    assert same(Xd.cpu().numpy(), ref) and same(Fd.cpu().numpy(), ref_first)


# ---- 5. the four chains end to end through the host layer ---------------------------------------------------------------------
def norm_bound(y_ref, dm, ds, sd_ref, e_in=0.0):
    """y = (x - mu) / sd against y_ref = (x_ref - mu_ref) / sd_ref with |x - x_ref| <= e_in, |mu - mu_ref| <= dm, |sd - sd_ref| <= ds:
    y - y_ref = ((x - x_ref) + (mu_ref - mu)) / sd + y_ref (sd_ref - sd) / sd, |sd| >= sd_ref - ds; plus two roundings (<= u each,
    relative) on each side."""
    b = (e_in + dm + np.abs(y_ref) * ds) / (sd_ref - ds)
    return b + 4 * U * (np.abs(y_ref) + b)


def stats_with_bounds(A, axis, mode, pH, pL, mask, pre=None, E=None):
    rm, rs, kept = ref_stats(A, axis, mode, pH, pL, mask, pre)
    b = [bounds(rm[i], rs[i], kept[i], mode, 0.0 if E is None else E[i]) for i in range(len(rm))]
    return rm, rs, np.array([v[0] for v in b]), np.array([v[1] for v in b])


def chain_ref(X, Z, T, ZT, norm_type, mode, pH, pL, mT, mZ):
    """ComputeNorm.cpp:530-751 on matrices; -> (scores, bound, first scores or None, their bound)"""
    col = lambda v: v[:, None]
    row = lambda v: v[None, :]
    if norm_type == "znorm":                                                           # :573, :587
        mu, sd, dm, ds = stats_with_bounds(Z, 0, mode, pH, pL, mZ)
        y = (X - col(mu)) / col(sd)
        return y, norm_bound(y, col(dm), col(ds), col(sd)), None, None
    if norm_type == "tnorm":                                                           # :537, :552
        mu, sd, dm, ds = stats_with_bounds(T, 1, mode, pH, pL, mT)
        y = (X - row(mu)) / row(sd)
        return y, norm_bound(y, row(dm), row(ds), row(sd)), None, None
    selZ = slice(None) if mZ is None else (np.asarray(mZ) != 0)
    selT = slice(None) if mT is None else (np.asarray(mT) != 0)
    if norm_type == "ztnorm":
        ma, sa, dma, dsa = stats_with_bounds(ZT, 1, mode, pH, pL, mT)                  # :618
        mt, st, dmt, dst = stats_with_bounds(T, 1, mode, pH, pL, mT)                   # :623
        Zn = (Z - row(ma)) / row(sa)                                                   # :480
        En = norm_bound(Zn, row(dma), row(dsa), row(sa))[:, selZ].max(axis=1)
        mz, sz, dmz, dsz = stats_with_bounds(Z, 0, mode, pH, pL, mZ, (ma, sa), En)     # :629
        x1 = (X - row(mt)) / row(st)                                                   # :647
        e1 = norm_bound(x1, row(dmt), row(dst), row(st))
        y = (x1 - col(mz)) / col(sz)                                                   # :654
        return y, norm_bound(y, col(dmz), col(dsz), col(sz), e1), x1, e1
    mz, sz, dmz, dsz = stats_with_bounds(Z, 0, mode, pH, pL, mZ)                       # :690
    ma, sa, dma, dsa = stats_with_bounds(ZT, 0, mode, pH, pL, mZ)                      # :697
    Tn = (T - col(ma)) / col(sa)                                                       # :480 through :704
    En = norm_bound(Tn, col(dma), col(dsa), col(sa))[selT, :].max(axis=0)
    mt, st, dmt, dst = stats_with_bounds(T, 1, mode, pH, pL, mT, (ma, sa), En)         # :704
    x1 = (X - col(mz)) / col(sz)                                                       # :730
    e1 = norm_bound(x1, col(dmz), col(dsz), col(sz))
    y = (x1 - row(mt)) / row(st)                                                       # :736
    return y, norm_bound(y, row(dmt), row(dst), row(st), e1), x1, e1


@pytest.mark.parametrize("rule", ["cosine", "plda"])
def test_chains_end_to_end_through_the_host_layer(ctx, rule):
    import torch
    from lia_ral_amd import host_capi
    rng = np.random.default_rng(21)
    dim, M, S, Nt, Nz = 400, 120, 150, 300, 500
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    models, segs, cohort, imps = [dev(rng.normal(0.2, 1.0, size=(dim, n))) for n in (M, S, Nt, Nz)]
    if rule == "cosine":
        score = lambda a, b: ctx.score_cosine(a, b, out=torch.empty((a.shape[1], b.shape[1]), dtype=torch.float64, device="cuda"))
    else:                                                   # asymmetric in models / segments: session counts on the model side
        Q = rng.normal(size=(dim, dim))
        FTJF = dev(Q @ Q.T / dim + np.eye(dim))
        ns = {M: rng.integers(1, 4, M), Nt: rng.integers(1, 4, Nt)}
        score = lambda a, b: ctx.score_plda(a, ns[a.shape[1]], b, FTJF,
                                            out=torch.empty((a.shape[1], b.shape[1]), dtype=torch.float64, device="cuda"))
    X, Z, T, ZT = score(models, segs), score(models, imps), score(cohort, segs), score(cohort, imps)
    torch.cuda.synchronize()
    Xh, Zh, Th, ZTh = [v.cpu().numpy() for v in (X, Z, T, ZT)]
    mT = (rng.random(Nt) < 0.8).astype(np.uint8)
    mZ = (rng.random(Nz) < 0.8).astype(np.uint8)
    for norm_type in ("znorm", "tnorm", "ztnorm", "tznorm"):
        for mode, pH, pL, masks in ((0, 0.0, 0.0, False), (0, 0.05, 0.2, True), (1, 0.1, 0.1, False)):
            Xd, Fd = X.clone(), torch.full_like(X, 99.0)
            torch.cuda.synchronize()
            host_capi.compute_norm(Xd, Z, T, ZT, norm_type, mode, pH, pL, mT if masks else None, mZ if masks else None, first_out=Fd)
            y, by, x1, b1 = chain_ref(Xh, Zh, Th, ZTh, norm_type, mode, pH, pL, mT if masks else None, mZ if masks else None)
            err = np.abs(Xd.cpu().numpy() - y)
            assert np.all(err <= by), (rule, norm_type, mode, pH, pL, err.max(), by.min())
            if x1 is not None:
                e1 = np.abs(Fd.cpu().numpy() - x1)
                assert np.all(e1 <= b1), (rule, norm_type, "first", e1.max(), b1.min())
            else:
                assert bool((Fd == 99.0).all())


# ---- 6. deterministic and asynchronous --------------------------------------------------------------------------------------
def test_device_calls_only_enqueue_and_repeat_bitwise():
    import torch
    from lia_ral_amd import capi
    rng = np.random.default_rng(8)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ctx = capi.Context(0, s.cuda_stream)
        Z = torch.from_numpy(rng.normal(-2.0, 1.5, size=(3000, 1000))).cuda()
        T = torch.from_numpy(rng.normal(-2.0, 1.5, size=(1000, 3000))).cuda()
        X0 = torch.from_numpy(rng.normal(-2.0, 1.5, size=(3000, 3000))).cuda()
        sel = torch.from_numpy((rng.random(1000) < 0.8).astype(np.uint8)).cuda()
        new = lambda n: torch.empty(n, dtype=torch.float64, device="cuda")
        zm, zs, tm, ts = new(3000), new(3000), new(3000), new(3000)
        X, F = X0.clone(), torch.empty_like(X0)

        def run():
            ctx.score_cohort_stats(Z, 0, select=sel, percent_h=0.05, percent_l=0.2, out_mean=zm, out_std=zs)
            ctx.score_cohort_stats(T, 1, select=sel, percent_h=0.05, percent_l=0.2, out_mean=tm, out_std=ts)
            ctx.score_normalize(X, capi.NORM_ZT, zm, zs, tm, ts, first_out=F)
        run()
        torch.cuda.synchronize()                                 # warm-up: whatever is allocated exists now
        first = [v.clone() for v in (zm, zs, tm, ts, X, F)]
        ws = [ctx.workspace_bytes(i) for i in range(64)]
        X.copy_(X0)
        torch.cuda.synchronize()
        torch.cuda._sleep(int(2.0e9))                            # ~1 s of spinning on this stream
        t0 = time.perf_counter()
        run()
        dt = time.perf_counter() - t0
        still_busy = not s.query()
        torch.cuda.synchronize()
        assert still_busy and dt < 0.25, (still_busy, dt)        # three calls enqueued behind the spin kernel
        for a, b in zip(first, (zm, zs, tm, ts, X, F)):
            assert torch.equal(a, b) or same(a.cpu().numpy(), b.cpu().numpy())
        assert ws == [ctx.workspace_bytes(i) for i in range(64)]
        rm, rs, _ = ref_stats(Z.cpu().numpy()[:50], 0, 0, 0.05, 0.2, sel.cpu().numpy())
        check_within(zm.cpu().numpy()[:50], zs.cpu().numpy()[:50], (rm, rs, _), 0, "async z")
        ctx.close()


# ---- 7. no growth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
def test_scratch_is_the_formula_and_does_not_grow(axis):
    import torch
    from lia_ral_amd import capi
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    A = torch.randn((20000, 2000), dtype=torch.float64, device="cuda")
    nd = A.shape[axis]
    L = A.shape[1 - axis]
    m = torch.empty(nd, dtype=torch.float64, device="cuda"); s = torch.empty_like(m)
    sel = torch.ones(L, dtype=torch.uint8, device="cuda")
    pre = (torch.zeros(L, dtype=torch.float64, device="cuda"), torch.ones(L, dtype=torch.float64, device="cuda"))

    def run():
        ctx.score_cohort_stats(A, axis, out_mean=m, out_std=s)
        ctx.score_cohort_stats(A, axis, select=sel, pre_mean=pre[0], pre_std=pre[1], mean_mode=1, percent_h=0.05, percent_l=0.2,
                               out_mean=m, out_std=s)
    run()
    torch.cuda.synchronize()
    ws = [ctx.workspace_bytes(i) for i in range(64)]
    formula = capi.norm_scratch_bytes(nd)                        # GMMIV_SCORE_NORM_SCRATCH_BYTES(nd) = 512 nd + 64
    assert sum(ws) == ctx.workspace_bytes() and 0 < ctx.workspace_bytes() <= formula + formula // 8, (ws, formula)
    assert ctx.workspace_bytes() < A.numel() * 8 // 100          # nowhere near the matrix
    run()
    torch.cuda.synchronize()
    assert ws == [ctx.workspace_bytes(i) for i in range(64)]     # the second call of the same shape allocated nothing
    ctx.close()
