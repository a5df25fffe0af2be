"""k_dgemm (lia_ral_amd/csrc/tv_kernels.hip) called directly through gmmiv_dgemm, on every dispatch path, element by element.

Every case of dgemm_ref.CASES (the table tests/test_cpu_dgemm_ref.py holds against the dispatch mirror) runs with its operands
embedded in larger buffers: NaN around A and B, a finite sentinel around C, NaN inside C when beta == 0.
  exact form   small integers: the WHOLE buffer of C -- interior and surroundings -- must equal the reference bit for bit.
  real form    |got - ref|_ij <= (K + 8) 2^-53 S_ij per element against a long double reference (dgemm_ref.real_case); the
               surroundings of C bit for bit.
A failure names the case, the first offending (batch, i, j), the value got and the reference (for real cases the ratio to the
bound).  Set DGEMM_ERRORS_JSON to a path to have the largest ratio of every real case written there (profiles/r12/dgemm_errors.json).
"""
import contextlib
import ctypes as ct
import json
import os

import numpy as np
import pytest

import dgemm_ref as dr

pytestmark = pytest.mark.gpu
needs_ld = pytest.mark.skipif(not dr.HAVE_LONGDOUBLE, reason=dr.SKIP_MESSAGE)
RATIOS = {}


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lia_ral_amd import capi
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()
    path = os.environ.get("DGEMM_ERRORS_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"bound": "(K + 8) 2^-53 S_ij, S = |alpha| |op A| |op B| + |beta| |C_in| (+ epilogue terms)", "max_ratio": max(RATIOS.values()),
                       "cases": {k: float("%.4g" % v) for k, v in RATIOS.items()}}, f, indent=1)


@contextlib.contextmanager
def options(ctx, opts):
    """set, run, restore (as tools/chol_family_errors.options): set_option hands back what was there"""
    try:
        for k, v in opts.items():
            prev = ctx.set_option(k, v)
            assert prev == dr.DEFAULT_OPTS[k], "option %s was %r, expected the default %r" % (k, prev, dr.DEFAULT_OPTS[k])
        yield
    finally:
        for k, v in opts.items():
            back = ctx.set_option(k, dr.DEFAULT_OPTS[k])
            assert back == v, "option %s read back %r after it was set to %r" % (k, back, v)


def device_view(case, key, x, fill):
    """-> (flat device buffer, the operand as a strided view of it)"""
    import torch
    flat, _, (s, ld) = dr.embed_case(case, key, x, fill)
    (b, r, c), _, off = dr.layouts(case)[key]
    t = torch.from_numpy(flat).cuda()
    return t, t.as_strided((b, r, c), (s, ld, 1), dr.MARGIN + off)


def where(case, idx):
    """a flat index of C's buffer as (batch, i, j), or a description of where outside C it lies"""
    (b, r, c), (s, ld), off = dr.layouts(case)["C"]
    e = idx - dr.MARGIN - off
    if e < 0 or e >= b * s:
        return "buffer margin (flat %d)" % idx
    bi, rem = divmod(e, s)
    i, j = divmod(rem, ld)
    return "(%d, %d, %d)" % (bi, i, j) if i < r and j < c else "padding beside (%d, %d, %d)" % (bi, i, j)


def run(ctx, case, d):
    """one call of gmmiv_dgemm on embedded operands -> the flat buffer of C as a device tensor"""
    import torch
    _, A = device_view(case, "A", d["A"], np.nan)
    _, B = device_view(case, "B", d["B"], np.nan)
    cin = d["C"] if case.beta != 0 else np.full(d["C"].shape, np.nan)
    flat, C = device_view(case, "C", cin, dr.SENTINEL)
    rv = None if d["rv"] is None else torch.from_numpy(d["rv"]).cuda()
    cv = None if d["cv"] is None else torch.from_numpy(d["cv"]).cuda()
    with options(ctx, dict(case.opts)):
        ctx.dgemm(case.ta, case.tb, case.alpha, A[0] if case.batch == 1 else A, B[0] if case.batch == 1 else B, case.beta,
                  C[0] if case.batch == 1 else C, nz=case.nz, epi_mode=case.epi, rv=rv, cv=cv, br=d["br"], bc=d["bc"], cst=d["cst"])
        ctx.sync()
    return flat


def check_exact(ctx, case):
    """-> None, or the failure message"""
    import torch
    d = dr.exact_case(case)
    got = run(ctx, case, d)
    exp = dr.embed_case(case, "C", d["ref"], dr.SENTINEL)[0]
    if torch.equal(got.view(torch.int64), torch.from_numpy(exp).cuda().view(torch.int64)):
        return None
    g = got.cpu().numpy()
    bad = np.flatnonzero(g.view(np.int64) != exp.view(np.int64))
    i = int(bad[0])
    return "%s: %d of %d doubles differ, first at %s: got %r (%s), reference %r (%s)" % (
        case.name, bad.size, g.size, where(case, i), float(g[i]), float(g[i]).hex(), float(exp[i]), float(exp[i]).hex())


def check_real(ctx, case, same_bits_as=None):
    d = dr.real_case(case)
    got = run(ctx, case, d).cpu().numpy()
    marker = dr.embed_case(case, "C", np.zeros((case.batch, case.M, case.N)), dr.SENTINEL)[0]
    outside = np.flatnonzero((marker == dr.SENTINEL) & (got.view(np.int64) != marker.view(np.int64)))
    if outside.size:
        return "%s: %d doubles outside C were written, first at %s: %r" % (case.name, outside.size, where(case, int(outside[0])), float(got[outside[0]]))
    (b, r, c), (s, ld), off = dr.layouts(case)["C"]
    view = np.lib.stride_tricks.as_strided(got[dr.MARGIN + off:], (b, r, c), (8 * s, 8 * ld, 8))
    ratio = (np.abs(view.astype(dr.LD) - d["ref"]) / d["bound"]).astype(np.float64)
    RATIOS[case.name] = float(np.nanmax(ratio)) if np.isfinite(view).all() else float("inf")
    ok = ratio <= 1.0                                      # a NaN fails
    if not ok.all():
        bi, i, j = (int(v) for v in np.argwhere(~ok)[0])
        return "%s: %d of %d elements outside the bound, first at (%d, %d, %d): got %r, reference %r, |error| / bound = %.3g (largest %.3g)" % (
            case.name, (~ok).sum(), ok.size, bi, i, j, float(view[bi, i, j]), float(d["ref"][bi, i, j]), ratio[bi, i, j], np.nanmax(ratio))
    if same_bits_as is not None and not np.array_equal(view.view(np.int64), same_bits_as.view(np.int64)):
        bi, i, j = (int(v) for v in np.argwhere(view.view(np.int64) != same_bits_as.view(np.int64))[0])
        return "%s: not the bits of the aligned call, first at (%d, %d, %d): %r against %r" % (case.name, bi, i, j, float(view[bi, i, j]), float(same_bits_as[bi, i, j]))
    return view.copy()


def cases(group, real, **kw):
    out = [c for c in dr.CASES if c.group == group and c.real == real and all(getattr(c, k) == v for k, v in kw.items())]
    assert out
    return out


def run_all(ctx, cs):
    bad = []
    for c in cs:
        r = check_real(ctx, c) if c.real else check_exact(ctx, c)
        if isinstance(r, str):
            bad.append(r)
    assert not bad, "%d of %d cases failed:\n" % (len(bad), len(cs)) + "\n".join(bad[:40])


# ---------------------------------------------------------------- tiles and k-tails
@pytest.mark.parametrize("ta,tb", dr.PAIRS, ids=[dr.pair_name(*p) for p in dr.PAIRS])
def test_tiles_and_k_tails_exact(ctx, ta, tb):
    """8 shapes (narrow strips both ways, two strip tiles, wide strips, no full tile, 32-row tiles, odd extents) x K in 2 .. 60 and
    1, 17, 33 (no tail / a tail with nkt 1, even, odd / odd K) x alpha in 1, -0.5 x beta in 0, 1, -2: 480 calls, bitwise."""
    cs = cases("tiles", False, ta=ta, tb=tb)
    assert len(cs) == 480
    run_all(ctx, cs)


@needs_ld
@pytest.mark.parametrize("ta,tb", dr.PAIRS, ids=[dr.pair_name(*p) for p in dr.PAIRS])
def test_tiles_and_k_tails_real(ctx, ta, tb):
    """the same shapes at K = 18, 33, 60 with log-normally scaled rows and columns, per element against the gamma bound"""
    run_all(ctx, cases("tiles", True, ta=ta, tb=tb))


# ---------------------------------------------------------------- options
@pytest.mark.parametrize("opt", [o[0][0] for o in dr.OPTION_SETS])
def test_gemm_clamp_0_and_gemm_narrow_0_exact(ctx, opt):
    """(130, 160) and (194, 200) over the whole K / alpha / beta table with the option at 0: bit-identical to the reference, which the
    default route of the same call is held to in test_tiles_and_k_tails_exact -- so both routes give the same bits."""
    cs = cases("options", False, opts=((opt, 0),))
    assert len(cs) == 480
    run_all(ctx, cs)
    assert ctx.set_option(opt, dr.DEFAULT_OPTS[opt]) == dr.DEFAULT_OPTS[opt]           # restored


@needs_ld
def test_gemm_clamp_0_and_gemm_narrow_0_real(ctx):
    run_all(ctx, cases("options", True))


# ---------------------------------------------------------------- alignment
def _align_base(c):
    return c.aoff == c.boff == c.ald == c.bld == 0 and c.sa == c.sb == "even"


def test_unaligned_operands_exact(ctx):
    """an A or a B view one double off 16 bytes, an odd lda / ldb, an odd batch stride (the per-element checked loads), two doubles
    off (still aligned): the reference's bits, like the aligned call"""
    run_all(ctx, cases("align", False))


@needs_ld
def test_unaligned_operands_give_the_bits_of_the_aligned_call(ctx):
    """real-valued operands: every element accumulates its k-tiles in the same order whichever loads staged them, so the unaligned
    calls return the aligned call's bits (and each is inside the bound)"""
    cs = cases("align", True)
    bad, base = [], {}
    for c in [c for c in cs if _align_base(c)] + [c for c in cs if not _align_base(c)]:
        key = (c.ta, c.tb, c.M, c.N, c.K, c.batch)
        r = check_real(ctx, c, base.get(key))
        if isinstance(r, str):
            bad.append(r)
        elif _align_base(c):
            base[key] = r
    assert len(base) == 16 and not bad, "\n".join(bad)


# ---------------------------------------------------------------- batch
def test_batches_exact(ctx):
    """batch = 3: padded even strides, a shared B (sB = 0), a shared A, an odd sC with an even and an odd ldc"""
    run_all(ctx, cases("batch", False))


@needs_ld
def test_batches_real(ctx):
    run_all(ctx, cases("batch", True))


# ---------------------------------------------------------------- tile order
@pytest.mark.parametrize("M,N,K", [s[:3] for s in dr.ORDER_SHAPES])
def test_tile_orders_exact(ctx, M, N, K):
    """gemm_remap 0, 1 and 2 on grids with leftover tile columns, a narrower last block column (G = 9) and a shorter last block row
    (Mt = 9): each equal to the reference bit for bit, hence to each other"""
    cs = cases("order", False, M=M, N=N, K=K)
    assert len(cs) % 3 == 0
    run_all(ctx, cs)


# ---------------------------------------------------------------- split-K
def test_split_k_exact(ctx):
    """ranges 48 / 48 / 4 (NT, TN), K = 101 on the checked loads with ksplit, nz = 0 at K = 4096, beta = -2 with ldc > N, the 128 x 80
    tiles with gemm_nt80 1 and 0, and an odd lda that must keep off them"""
    run_all(ctx, cases("splitk", False))


@needs_ld
def test_split_k_real(ctx):
    run_all(ctx, cases("splitk", True))


# ---------------------------------------------------------------- epilogues
def test_epilogues_exact(ctx):
    """modes 1 and 2 (br, bc, cst all non-zero), TN and NN, beta 0 and 1, on strips, wide strips, odd extents and 32-row tiles"""
    run_all(ctx, cases("epi", False))


@needs_ld
def test_epilogues_real(ctx):
    run_all(ctx, cases("epi", True))


# ---------------------------------------------------------------- degenerate calls
def test_k_zero(ctx):
    """K = 0: C = beta C (beta = 3), zeros over NaN (beta = 0); also through the split-K and epilogue arguments"""
    run_all(ctx, cases("degenerate", False))


def raw(ctx, ta=0, tb=0, M=4, N=6, K=8, alpha=1.0, A=None, lda=None, sA=0, B=None, ldb=None, sB=0, beta=0.0, C=None, ldc=None, sC=0,
        batch=1, nz=1, epi=0, rv=None, cv=None):
    """gmmiv_dgemm with every argument as given -> the status"""
    from lia_ral_amd import capi
    p = lambda t: ct.c_void_p(0 if t is None else t.data_ptr())
    lda = (M if ta else K) if lda is None else lda
    ldb = (K if tb else N) if ldb is None else ldb
    ldc = N if ldc is None else ldc
    return capi.lib.gmmiv_dgemm(ctx._h, ta, tb, M, N, K, ct.c_double(alpha), p(A), ct.c_int64(lda), ct.c_int64(sA), p(B), ct.c_int64(ldb),
                                ct.c_int64(sB), ct.c_double(beta), p(C), ct.c_int64(ldc), ct.c_int64(sC), batch, nz, epi, p(rv), p(cv),
                                ct.c_double(0.0), ct.c_double(0.0), ct.c_double(0.0))


def test_empty_calls_and_bad_arguments(ctx):
    """M, N or batch = 0: GMMIV_OK and C untouched.  Every documented misuse: GMMIV_ERR_ARG (-1) and C untouched.  The context then
    serves the next call."""
    import torch
    buf = torch.full((4096,), dr.SENTINEL, dtype=torch.float64, device="cuda")
    A, B, C, v = buf[0:1024], buf[1024:2048], buf[2048:3072], buf[3072:]
    kw = dict(A=A, B=B, C=C)
    for zero in (dict(M=0), dict(N=0), dict(batch=0), dict(M=0, N=0, K=0)):
        assert raw(ctx, **kw, **zero) == 0, zero
    bad = [dict(lda=7), dict(ta=1, lda=3), dict(ldb=5), dict(tb=1, ldb=7), dict(ldc=5),
           dict(M=-1), dict(N=-1), dict(K=-1), dict(batch=-1), dict(nz=-1),
           dict(batch=2, nz=2), dict(batch=2, nz=0), dict(batch=2, epi=1, rv=v, cv=v), dict(batch=2, epi=2, rv=v, cv=v),
           dict(nz=2, epi=1, rv=v, cv=v), dict(nz=0, epi=2, rv=v, cv=v),
           dict(epi=3, rv=v, cv=v), dict(epi=-1, rv=v, cv=v), dict(epi=1, cv=v), dict(epi=1, rv=v), dict(epi=2), dict(sA=-2, batch=2)]
    for b in bad:
        assert raw(ctx, **dict(kw, **b)) == -1, b
    host = torch.zeros(64, dtype=torch.float64)
    assert raw(ctx, **dict(kw, A=host)) == -1 and raw(ctx, **dict(kw, C=None)) == -1
    ctx.sync()
    assert bool((buf == dr.SENTINEL).all())
    assert raw(ctx, **kw) == 0                                               # 4 x 6 x 8 of sentinels: only that it runs
    ctx.sync()
    assert check_exact(ctx, cases("tiles", False, ta=True, tb=True, M=131, N=129, K=34, alpha=-0.5, beta=-2.0)[0]) is None
