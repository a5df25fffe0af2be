"""The estimation side of the i-vector back end -- gmmiv_dev_mahalanobis, gmmiv_dev_wccn_chol, gmmiv_twocov_model,
gmmiv_plda_precompute (governed by an inverse), gmmiv_sym_eigen, gmmiv_dev_efr_matrix, gmmiv_dev_lda, gmmiv_plda_em_iteration (host
eigen / EM code fed by device kernels) and gmmiv_tv_orthonormalize_t -- judged per column, row, eigenpair and vector against the
80-bit references and the bars of tests/estimation_ref.py: err <= 16 max(err_double, 64 u), err_double the error of the float64
restatement of the library's algorithm on the same unit.  Never against the largest entry of an array (that is
tests/test_gpu_tv.py, which stays).

Every case runs on the defaults and under "chol_gemm" 1 (the even orders then take the GEMM-built inverse as the odd ones always do),
with host arrays in and out, and with device tensors in and out, every device result between guard bands that must come back
untouched; host and device results must be the same bits.

What runs here for the first time: an odd order, and an order smaller than the one reserved, through SpdBatch::inverse /
inverse_of (tvk_spd_inverse_batched with nb = 1) from a back-end entry point; twocov_model against numbers at all; plda_precompute
after a call on a larger odd order whose inputs were all NaN (bitwise against a fresh context: the scratch reused at a smaller
order); plda_em_iteration from a non-zero Delta (k_sub_colvec subtracts something, and the centred X must be the bits of
X - Delta), with rf = 1, rg = 1, rg = 0, 257 speakers of ragged counts (k_dev_means strides 256 threads over them), a speaker of
600 sessions, F / G / Sigma / Delta as device tensors; both routes of tv_orthonormalize_t on either side of dmin = 1e-4 dmax, the
step kernels with the zero row first, in the middle and last, and their grid-stride loop on a second trip (SV = 131100 > 512 * 256);
DevOut / store_out on a device pointer for all nine.  (The context's launch counters do not count the kernels of
tv_orthonormalize_t -- no t_begin brackets them -- so the route is told from the 80-bit factor, tests/test_cpu_estimation_ref.py,
and from the result: the zero row, and the bars of the route's own restatement.)

A failure names case, option path, entry point, unit kind, the first offending unit and its ratio to the bar.  With
ESTIMATION_ERRORS_JSON set to a path, the largest ratio per (case, path, entry point, unit kind) is written there with the
restatement's and the oracle's error on that unit (profiles/r17/estimation_errors.json).
"""
import json
import os

import numpy as np
import pytest

import elementwise_judge as ej
import estimation_ref as er
from elementwise_judge import SENTINEL, Guarded, options, path_name

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300), pytest.mark.skipif(not er.HAVE_LONGDOUBLE, reason=er.SKIP_MESSAGE)]

RATIOS = {}
UNITS = {}            # (case, path, entry, kind) -> dict(ratio, unit, err_double, err_oracle) of the worst unit
PATHS = ({}, {"chol_gemm": 1})


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    c = capi.Context(0)
    yield c
    c.close()
    path = os.environ.get("ESTIMATION_ERRORS_JSON")
    if path and RATIOS:
        per = {}
        for (case, p, entry, kind), v in RATIOS.items():
            for key in ("path: " + p, "entry: %s, %s" % (entry, kind)):
                per[key] = max(per.get(key, 0.0), v)
        with open(path, "w") as f:
            json.dump({"bound": "tests/estimation_ref.py: per column / row / eigenpair / vector, |error| <= 16 max(err_double, 64 u), err_double the error "
                                "of the float64 restatement of the library's algorithm on the same unit against the 80-bit reference; "
                                "a-priori kinds: unit norm of an LDA row 4 u, order of the eigenvalues, exact zeros",
                       "max_ratio": float("%.4g" % max(RATIOS.values())), "worst": {k: float("%.4g" % v) for k, v in sorted(per.items())},
                       "entries": {" | ".join(k): UNITS.get(k, {"ratio": float("%.4g" % v)}) for k, v in sorted(RATIOS.items())}}, f, indent=1)


def Judge(case, path="defaults"):
    return ej.Judge(case, path, RATIOS)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, np.float64, order="C")).cuda()              # a copy: the cached inputs are read-only


def sentinel(*shape):
    return np.full(shape, SENTINEL)


def record(j, entry, ratios, dbl, orc):
    for kind, rec in er.worst_units(ratios, dbl, orc).items():
        key = (j.case, j.path, entry, kind.lstrip("!"))
        if rec["ratio"] >= UNITS.get(key, {"ratio": -1.0})["ratio"]:
            UNITS[key] = rec
    for kind, r in ratios.items():
        j(entry, kind.lstrip("!"), r)


def judged(j, entry, key, host, device):
    """host: the result(s) of the call on host arrays; device: the same read back from between the guard bands.  The host result
    is judged; the device result must be its bits (and is then inside the same bars)"""
    hs, ds = (host, device) if isinstance(host, tuple) else ((host,), (device,))
    for i, (h, d) in enumerate(zip(hs, ds)):
        if np.any(h == SENTINEL):
            j.note(entry, "output %d [host]: %d elements were never written" % (i, int((h == SENTINEL).sum())))
        j.same_bits("%s output %d [device]" % (entry, i), d, h, "the call on host arrays")
    record(j, entry, er.judge(entry, key, host), *er.unit_errors(entry, key))


# ---------------------------------------------------------------- governed by an inverse
@pytest.mark.parametrize("opts", PATHS, ids=path_name)
@pytest.mark.parametrize("name", er.INV_DEV_SETS)
def test_dev_mahalanobis_and_wccn_chol_per_column_and_row(ctx, name, opts):
    X, sps = er.dev_set(name)
    dim = X.shape[0]
    j = Judge("dev " + name, path_name(opts))
    with options(ctx, opts):
        for entry, call in (("dev_mahalanobis", ctx.dev_mahalanobis), ("dev_wccn_chol", ctx.dev_wccn_chol)):
            host = call(X, sps, out=sentinel(dim, dim))
            g, Xd = Guarded((dim, dim), None), dev(X)
            call(Xd, sps, out=g.view)
            ctx.sync()
            judged(j, entry, name, host, g.read(j, entry + " [device]"))
    j.finish()


@pytest.mark.parametrize("opts", PATHS, ids=path_name)
@pytest.mark.parametrize("key", er.TWOCOV_CASES, ids=er.case_name)
def test_twocov_model_per_column(ctx, key, opts):
    W, B = er.twocov_inputs(key)
    n = key[0]
    j = Judge("twocov " + er.case_name(key), path_name(opts))
    with options(ctx, opts):
        host = ctx.twocov_model(W, B, out=(sentinel(n, n), sentinel(n, n)))
        gG, gH, Wd, Bd = Guarded((n, n), None), Guarded((n, n), None), dev(W), dev(B)
        ctx.twocov_model(Wd, Bd, out=(gG.view, gH.view))
        ctx.sync()
        judged(j, "twocov_model", key, host, (gG.read(j, "G [device]"), gH.read(j, "H [device]")))
    j.finish()


@pytest.mark.parametrize("opts", PATHS, ids=path_name)
@pytest.mark.parametrize("key", er.PRECOMPUTE_CASES, ids=er.case_name)
def test_plda_precompute_per_column(ctx, key, opts):
    F, G, S = er.precompute_inputs(key)
    dim, rf, rg = key
    j = Judge("precompute " + er.case_name(key), path_name(opts))
    with options(ctx, opts):
        host = ctx.plda_precompute(F, G, S, out=(sentinel(rf, dim), sentinel(rf, rf)))
        gJ, gJF, Fd, Gd, Sd = Guarded((rf, dim), None), Guarded((rf, rf), None), dev(F), (dev(G) if rg else None), dev(S)
        ctx.plda_precompute(Fd, Gd, Sd, out=(gJ.view, gJF.view))
        ctx.sync()
        judged(j, "plda_precompute", key, host, (gJ.read(j, "FTJ [device]"), gJF.read(j, "FTJF [device]")))
    j.finish()


@pytest.mark.parametrize("opts", PATHS, ids=path_name)
@pytest.mark.parametrize("key", er.PRECOMPUTE_CASES, ids=er.case_name)
def test_plda_precompute_does_not_depend_on_what_the_scratch_held(key, opts):
    """the SPD buffers are reserved at max(dim, rg) and reused at the order of every inverse: a call on a larger odd order whose
    inputs are all NaN (it ends in "not positive definite") leaves NaN in all of them; the results after it must be the bits a fresh
    context gives"""
    from lia_ral_amd import capi
    F, G, S = er.precompute_inputs(key)
    bd, bf, bg = er.PRECOMPUTE_DIRTY
    j = Judge("precompute %s after NaN" % er.case_name(key), path_name(opts))
    outs = []
    for dirty in (False, True):
        c = capi.Context(0)
        try:
            for k, v in opts.items():
                c.set_option(k, v)
            if dirty:
                with pytest.raises(capi.GmmivError, match="not positive definite"):
                    c.plda_precompute(np.full((bd, bf), np.nan), np.full((bd, bg), np.nan), np.full((bd, bd), np.nan))
            outs.append(c.plda_precompute(F, G, S))
        finally:
            c.close()
    for i, what in enumerate(("FTJ", "FTJF")):
        j.same_bits("plda_precompute " + what, outs[1][i], outs[0][i], "the same call on a fresh context")
    record(j, "plda_precompute", er.judge("plda_precompute", key, outs[1]), *er.unit_errors("plda_precompute", key))
    j.finish()


# ---------------------------------------------------------------- host eigen code behind device pointers
@pytest.mark.parametrize("opts", PATHS, ids=path_name)
@pytest.mark.parametrize("mkey", er.eigen_matrices(), ids=er.case_name)
def test_sym_eigen_per_pair_and_efr_matrix_per_row(ctx, mkey, opts):
    A = er.eigen_matrix(mkey)
    n = A.shape[0]
    j = Judge("eigen " + er.case_name(mkey), path_name(opts))
    with options(ctx, opts):
        for rank in er.ranks(n):
            host = ctx.sym_eigen(A, rank, out=(sentinel(n, rank), sentinel(rank)))
            gv, gl, Ad = Guarded((n, rank), None), Guarded((rank,), None), dev(A)
            ctx.sym_eigen(Ad, rank, out=(gv.view, gl.view))
            ctx.sync()
            judged(j, "sym_eigen", (mkey, rank), host, (gv.read(j, "vect [device]"), gl.read(j, "val [device]")))
        if mkey in er.EFR_CASES:
            host = ctx.dev_efr_matrix(A, out=sentinel(n, n))
            g, Ad = Guarded((n, n), None), dev(A)
            ctx.dev_efr_matrix(Ad, out=g.view)
            ctx.sync()
            judged(j, "dev_efr_matrix", mkey, host, g.read(j, "dev_efr_matrix [device]"))
    j.finish()


@pytest.mark.parametrize("opts", PATHS, ids=path_name)
@pytest.mark.parametrize("mkey", er.lda_matrices(), ids=er.case_name)
def test_dev_lda_per_row(ctx, mkey, opts):
    W, B = er.lda_inputs(mkey)
    n = W.shape[0]
    j = Judge("lda " + er.case_name(mkey), path_name(opts))
    with options(ctx, opts):
        for rank in er.ranks(n):
            host = ctx.dev_lda(W, B, rank, out=(sentinel(rank, n), sentinel(rank)))
            gm, gl, Wd, Bd = Guarded((rank, n), None), Guarded((rank,), None), dev(W), dev(B)
            ctx.dev_lda(Wd, Bd, rank, out=(gm.view, gl.view))
            ctx.sync()
            judged(j, "dev_lda", (mkey, rank), host, (gm.read(j, "ldaMat [device]"), gl.read(j, "eigval [device]")))
    j.finish()


# ---------------------------------------------------------------- PLDA EM
@pytest.mark.parametrize("opts", PATHS, ids=path_name)
@pytest.mark.parametrize("name", list(er.EM_CASES))
def test_plda_em_iteration_per_column_and_row(ctx, name, opts):
    """two iterations, each judged on its own: the second starts from the library's own doubles after the first, and the reference,
    the restatement and the oracle are recomputed from that state.  Host arrays; then X, F, G, Sigma, Delta as device tensors in
    place between guard bands: the same bits"""
    state = er.em_inputs(name)
    sps = state[1]
    rg = state[3].shape[1]
    j = Judge("em " + name, path_name(opts))
    with options(ctx, opts):
        for it in range(2):
            entry = "plda_em_iteration %d" % (it + 1)
            X, _, F, G, Sg, Dl = (np.array(a) for a in state)
            ctx.plda_em_iteration(X, sps, F, G, Sg, Dl)
            host = (X, F, G, Sg, Dl)
            gs = [Guarded(a.shape, init=np.array(a)) if a.size else None for a in (state[0], state[2], state[3], state[4], state[5])]
            Gd = gs[2].view if rg else np.array(state[3])
            ctx.plda_em_iteration(gs[0].view, sps, gs[1].view, Gd, gs[3].view, gs[4].view)
            ctx.sync()
            for what, h, g in zip(("X", "F", "G", "Sigma", "Delta"), host, gs):
                if g is not None:
                    j.same_bits("%s %s [device]" % (entry, what), g.read(j, "%s %s [device]" % (entry, what)), h, "the call on host arrays")
            j.same_bits(entry + " X", X, er.em_centred(state), "numpy's X - Delta[:, None]")
            ref, dbl, orc = er.em_bars(state)
            record(j, entry, er.em_judge(state, host), dbl, orc)
            state = (X, sps, F, G, Sg, Dl)
    j.finish()


# ---------------------------------------------------------------- tv_orthonormalize_t
@pytest.mark.parametrize("opts", PATHS, ids=path_name)
@pytest.mark.parametrize("key", er.ORTHO_CASES, ids=er.case_name)
def test_tv_orthonormalize_t_per_row(ctx, key, opts):
    T = er.ortho_inputs(key)
    j = Judge("orthonormalize %s (%s route)" % (er.case_name(key), er.ortho_route(key)), path_name(opts))
    with options(ctx, opts):
        host = ctx.tv_orthonormalize_t(np.array(T))
        g = Guarded(T.shape, init=np.array(T))
        ctx.tv_orthonormalize_t(g.view)
        ctx.sync()
        judged(j, "tv_orthonormalize_t", key, host, g.read(j, "tv_orthonormalize_t [device]"))
    j.finish()
