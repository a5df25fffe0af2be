"""The i-vector E- and M-step -- gmmiv_tv_subtract_m(_to), gmmiv_tv_tett, tv_estep behind gmmiv_tv_estimate_w / _a_and_c,
gmmiv_tv_update_t, gmmiv_tv_min_divergence -- judged per element, per utterance, per Gaussian and per column block against the
80-bit restatement and the bars of tests/tv_ref.py, never against the largest entry of an array: an utterance of a few frames is
held to its own i-vector, a Gaussian of 1e-9 of the others' occupancy to its own row of A and its own block of Cmx.

The shapes sit on either side of every number the dispatch cuts on (tv_ref.ESTEP_CASES, TETT_SHAPES below): the 64-utterance
threshold of tvk_colsum_narrow, both conditions of the two-stage batch sum (128 utterances, P >= 4096), odd orders (unpack / pack /
k_batched_matvec, the GEMM-built factorisation), split-K aux (C D >= 2048) with and without the 128 x 80 tile, batches and
super-batches with ragged ends, all 16 instantiations of k_tett_packed and its multi-pass path, the 128-Gaussian chunk of the GEMM
form of tv_tett, the n_cu-Gaussian chunk of tv_update_t.  W, A, Cmx, Rm, r and meanW live inside sentinel-filled device buffers
whose guard bands must come back untouched.

A failure names case, option path, entry point, unit kind, the first offending unit and its ratio to the bar.  With TV_ERRORS_JSON
set to a path the largest ratio per (case, path, entry point, unit kind) is written there, next to each case's cond(L_u) statistics
(profiles/r15/tv_errors.json).
"""
import json
import os

import numpy as np
import pytest

import elementwise_judge as ej
import spd_ref as sr
import tv_ref as tr
from elementwise_judge import DEFAULTS, SENTINEL, Guarded, options, path_name

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300), pytest.mark.skipif(not tr.HAVE_LONGDOUBLE, reason=tr.SKIP_MESSAGE)]

LD = tr.LD
RATIOS = {}
CONDS = {}


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    c = capi.Context(0)
    yield c
    c.close()
    path = os.environ.get("TV_ERRORS_JSON")
    if path and RATIOS:
        per = {}
        for (case, p, entry, kind), v in RATIOS.items():
            for key in ("path: " + p, "entry: " + entry):
                per[key] = max(per.get(key, 0.0), v)
        with open(path, "w") as f:
            json.dump({"bound": "tests/tv_ref.py: W per utterance 16 max(err_oracle_u, 64 u); A, Cmx per Gaussian, Rm, r, meanW: sum of the terms' bars + "
                                "(U + 8) u |sum|; tett (D + 8) u sum|T iv T|; subtract_m 2 u (|F| + |m N|); update_t per Gaussian and 16 columns "
                                "16 max(err_oracle, 64 u); min_divergence as derived there",
                       "max_ratio": float("%.4g" % max(RATIOS.values())), "worst": {k: float("%.4g" % v) for k, v in sorted(per.items())},
                       "cond_L": CONDS, "entries": {" | ".join(k): float("%.4g" % v) for k, v in sorted(RATIOS.items())}}, f, indent=1)


def Judge(case, path):
    """every comparison is a ratio to a bar of tv_ref; the largest per (case, path, entry point, unit kind) goes to RATIOS"""
    return ej.Judge(case, path, RATIOS)


# ---------------------------------------------------------------- the E-step
ACC_KEYS = ("A", "Cmx", "Rm", "r", "meanW")


def acc_shapes(p):
    return {"A": (p.C, p.P), "Cmx": (p.R, p.C * p.D), "Rm": (p.R, p.R), "r": (p.R,), "meanW": (p.R,)}


def run_estep(ctx, j, p, U, device=True):
    """tv_estimate_w, tv_estimate_a_and_c in one call and in two calls that accumulate into one, on utterances [0, U)"""
    C, D, R = p.C, p.D, p.R
    N, F0 = p.N[:U], p.F0[:U]

    def new_acc():
        if device:
            g = {k: Guarded(s) for k, s in acc_shapes(p).items()}
            return g, {k: v.view for k, v in g.items()}
        return None, {k: np.zeros(s) for k, s in acc_shapes(p).items()}

    def call(entry, lo, hi, guards, acc):
        gw = Guarded((hi - lo, R), None) if device else None
        acc["W"] = gw.view if device else np.full((hi - lo, R), SENTINEL)
        ctx.tv_estimate_a_and_c(N[lo:hi], F0[lo:hi], p.Tm, p.invvar, p.te, C, D, acc=acc)
        ctx.sync()
        W = gw.read(j, entry + " W") if device else acc["W"]
        j(entry, "W per utterance", p.w_ratios(W, lo))
        if lo <= tr.EMPTY_UTT < hi and np.any(W[tr.EMPTY_UTT - lo] != 0.0):
            j.note(entry, "the utterance without frames did not return w = 0")

    def judge_acc(entry, guards, acc):
        got = {k: guards[k].read(j, entry + " " + k) for k in ACC_KEYS} if device else acc
        for kind, r in p.judge_acc(got, U).items():
            j(entry, kind + (" per Gaussian" if kind in ("A", "Cmx") else ""), r)

    gw = Guarded((U, R), None) if device else None
    W = ctx.tv_estimate_w(N, F0, p.Tm, p.invvar, p.te, C, D, out=gw.view if device else np.full((U, R), SENTINEL))
    ctx.sync()
    W = gw.read(j, "estimate_w W") if device else W
    j("estimate_w", "W per utterance", p.w_ratios(W))
    if np.any(W[tr.EMPTY_UTT] != 0.0):
        j.note("estimate_w", "the utterance without frames did not return w = 0")
    guards, acc = new_acc()
    call("estimate_a_and_c", 0, U, guards, acc)
    judge_acc("estimate_a_and_c", guards, acc)
    guards, acc = new_acc()
    h = U // 2
    call("estimate_a_and_c 2 calls", 0, h, guards, acc)
    call("estimate_a_and_c 2 calls", h, U, guards, acc)
    judge_acc("estimate_a_and_c 2 calls", guards, acc)


def estep_test(ctx, case, U, opts=None, device=True):
    p = tr.case_problem(case)
    name = "%dx%dx%dx%d" % (case[0], case[1], case[2], U)
    CONDS[name] = p.cond_stats(U)
    opts = opts or {}
    j = Judge(name + ("" if device else " host arrays"), path_name(opts))
    with options(ctx, opts):
        run_estep(ctx, j, p, U, device)
    j.finish()


@pytest.mark.parametrize("case,U", [(c, U) for c in tr.ESTEP_CASES for U in c[3]], ids=lambda v: tr.case_name(v) if isinstance(v, tuple) else "U%d" % v)
def test_estep_per_utterance_and_per_gaussian(ctx, case, U):
    estep_test(ctx, case, U)


@pytest.mark.parametrize("case", [tr.ESTEP_CASES[0], tr.ESTEP_CASES[5]], ids=tr.case_name)
def test_estep_with_host_arrays(ctx, case):
    estep_test(ctx, case, max(case[3]), device=False)


@pytest.mark.parametrize("acc_mb", [0, 8192])
def test_estep_in_batches_of_16(ctx, acc_mb):
    """U = 75 under tv_batch 16: super-batches of 64 + 11 utterances when only one batch's worth of E fits, one of 80 by default"""
    case = tr.ESTEP_CASES[1]
    assert case[:3] == (16, 12, 40) and case[3] == (75,)
    estep_test(ctx, case, 75, {"tv_batch": 16} if acc_mb == DEFAULTS["tv_acc_mb"] else {"tv_batch": 16, "tv_acc_mb": acc_mb})


@pytest.mark.parametrize("case", [tr.ESTEP_CASES[8], tr.ESTEP_CASES[9]], ids=tr.case_name)
def test_estep_without_the_80_wide_tiles(ctx, case):
    assert case[2] % 80 == 0 and case[3] == (128,)
    estep_test(ctx, case, 128, {"gemm_nt80": 0})


# ---------------------------------------------------------------- tv_tett
KS_SHAPES = tuple((3, D, 17) for D in range(1, 65))                       # all 16 k_tett_packed<KS>, D % 4 in {0, 1, 2, 3} in each
TETT_SHAPES = ((3, 66, 17),                                                 # D > 64: the GEMM form either way
               (3, 60, 1), (3, 60, 15), (3, 60, 16), (3, 60, 33), (3, 60, 144), (3, 60, 145), (3, 60, 161),   # JH = 144 at D = 60
               (3, 64, 128), (3, 64, 129),                                  # JH = 128 at D = 64
               (130, 5, 17))                                                # the 128-Gaussian chunk of the GEMM form


def run_tett(ctx, j, C, D, R):
    rng = np.random.default_rng(10000 * C + 100 * D + R)
    P = R * (R + 1) // 2
    il = np.tril_indices(R)
    # exact: integer T in [-4, 4], iv a power of two -> every product and every partial sum is a double
    Ti = rng.integers(-4, 5, (R, C * D))
    e = rng.integers(-2, 3, C * D)
    Tc = Ti.reshape(R, C, D).astype(np.int64)
    iv4 = (4 * 2.0 ** e).astype(np.int64).reshape(C, D)                                   # 4 iv: 1 .. 16
    want = np.stack([((Tc[:, c, :] * iv4[c]) @ Tc[:, c, :].T)[il] for c in range(C)]) / 4.0
    g = Guarded((C, P), None)
    ctx.tv_tett(Ti.astype(np.float64), 2.0 ** e, C, D, out=g.view)
    ctx.sync()
    j.same_bits("tv_tett exact", g.read(j, "tv_tett exact"), want.astype(np.float64), "the int64 product")
    # real: rows of T log-normal (sigma 2), per element against (D + 8) u sum_k |T_ik iv_k T_jk|
    Tm = rng.normal(0.0, 0.3, (R, C * D)) * np.exp(rng.normal(0.0, 2.0, (R, 1)))
    iv = rng.uniform(0.5, 2.0, C * D)
    ref, bar = tr.tett(Tm, iv, C, D)
    j("tv_tett", "packed element", tr.ratio(ctx.tv_tett(Tm, iv, C, D).astype(LD) - ref, bar))


@pytest.mark.parametrize("direct", [1, 0])
def test_tett_every_instantiation_of_the_packed_kernel(ctx, direct):
    opts = {} if direct else {"tv_tett_direct": 0}
    with options(ctx, opts):
        for C, D, R in KS_SHAPES:
            j = Judge("tett %dx%dx%d" % (C, D, R), path_name(opts))
            run_tett(ctx, j, C, D, R)
            j.finish()


@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("shape", TETT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_tett_tile_pass_and_chunk_boundaries(ctx, shape, direct):
    opts = {} if direct else {"tv_tett_direct": 0}
    j = Judge("tett %dx%dx%d" % shape, path_name(opts))
    with options(ctx, opts):
        run_tett(ctx, j, *shape)
    j.finish()


# ---------------------------------------------------------------- tv_subtract_m, tv_subtract_m_to
@pytest.mark.parametrize("C,D", [(3, 1), (3, 2), (5, 13), (4, 60)])
def test_subtract_m_per_element(ctx, C, D):
    """in place and into another array, host and device, odd D and a base one double off 16-byte alignment (both: copy + the in-place
    kernel); exact on integers, 2 u (|F| + |m N|) on real statistics"""
    import torch
    U = 9
    rng = np.random.default_rng(100 * C + D)
    j = Judge("subtract_m %dx%dx%d" % (C, D, U), "defaults")
    Ni = rng.integers(0, 9, (U, C)).astype(np.float64)
    mi = rng.integers(-4, 5, C * D).astype(np.float64)
    Fi = rng.integers(-100, 101, (U, C * D)).astype(np.float64)
    s = tr.statistics(C, D, 2, U)
    for form, N, F, m in (("exact", Ni, Fi, mi), ("real", s["N"], s["F"], s["means"])):
        ref, bar = tr.subtract_m(N, F, m, C, D)

        def judge(entry, got):
            if form == "exact":
                j.same_bits(entry + " exact", got, ref.astype(np.float64), "the integer result")
            else:
                j(entry, "element", tr.ratio(np.asarray(got, LD) - ref, bar))
        judge("subtract_m host", ctx.tv_subtract_m(N, F.copy(), m, C, D))
        judge("subtract_m_to host", ctx.tv_subtract_m_to(N, F, np.full(F.shape, SENTINEL), m, C, D))
        Fh = F.copy()
        judge("subtract_m_to host in place", ctx.tv_subtract_m_to(N, Fh, Fh, m, C, D))
        Nd, md = torch.from_numpy(N).cuda(), torch.from_numpy(m).cuda()
        for shift in (0, 1):
            tag = " base + %d" % shift
            g = Guarded(F.shape, shift=shift, init=F)
            ctx.tv_subtract_m(Nd, g.view, md, C, D)
            ctx.sync()
            judge("subtract_m device" + tag, g.read(j, "subtract_m device" + tag))
            g = Guarded(F.shape, shift=shift, init=F)
            ctx.tv_subtract_m_to(Nd, g.view, g.view, md, C, D)
            ctx.sync()
            judge("subtract_m_to device in place" + tag, g.read(j, "subtract_m_to device in place" + tag))
            src, g = Guarded(F.shape, shift=shift, init=F), Guarded(F.shape, None, shift=shift)
            ctx.tv_subtract_m_to(Nd, src.view, g.view, md, C, D)
            ctx.sync()
            judge("subtract_m_to device" + tag, g.read(j, "subtract_m_to device" + tag))
            j.same_bits("subtract_m_to device" + tag + " source", src.read(j, "source"), F, "the source it was given")
    j.finish()


# ---------------------------------------------------------------- tv_update_t
MSTEP_CASES = {"16x12x40": (16, 12, 40, 75), "258x2x6": (258, 2, 6, 12)}      # the second: chunks of 256 + 2 Gaussians on 256 CUs


@pytest.mark.parametrize("solve", [1, 0])
@pytest.mark.parametrize("which", list(MSTEP_CASES))
def test_update_t_per_gaussian_and_column_block(ctx, which, solve):
    C, D, R, U = MSTEP_CASES[which]
    p = tr.problem(C, D, R, U)
    m = p.mstep(U)
    opts = {} if solve else {"tv_mstep_solve": 0}
    j = Judge("update_t %s" % which, path_name(opts))
    with options(ctx, opts):
        j("update_t host", "Gaussian x 16 columns", p.mstep_ratios(ctx.tv_update_t(m["A"], m["Cmx"], C, D), m))
        g = Guarded((R, C * D), None)
        ctx.tv_update_t(m["A"], m["Cmx"], C, D, out=g.view)
        ctx.sync()
        j("update_t device", "Gaussian x 16 columns", p.mstep_ratios(g.read(j, "update_t device"), m))
    j.finish()


# ---------------------------------------------------------------- tv_min_divergence
@pytest.mark.parametrize("dev_route", [1, 0])
@pytest.mark.parametrize("R", tr.MD_RANKS)
def test_min_divergence_per_element_and_column(ctx, R, dev_route):
    m = tr.md_problem(R)
    opts = {} if dev_route else {"tv_md_device": 0}
    j = Judge("min_divergence R %d" % R, path_name(opts))
    Rg, rg, mg, Tg = m["Rm"].copy(), m["r"].copy(), m["means"].copy(), m["T"].copy()
    with options(ctx, opts):
        ctx.tv_min_divergence(Rg, rg, m["meanW"], mg, Tg, m["n"], tr.MD_C, tr.MD_D)
    for kind, r in tr.md_judge(m, Rg, rg, mg, Tg).items():
        j("min_divergence", kind, r)
    j.finish()
