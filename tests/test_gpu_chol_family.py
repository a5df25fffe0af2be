"""The batched Cholesky family (chol_fused.hip: k_chol_left2, k_chol_left<lds>, k_trinv_left, k_uut, k_chol_solve_multi; tv_kernels.hip:
tvk_chol_batched / tvk_spd_inverse_batched, k_chol_solve) per SYSTEM, on every variant gmmiv_ctx_set_option ships, against the 80-bit
reference of tests/spd_ref.py.  The systems are dense SPD matrices of condition 1e1 .. 1e6 (1e8 in the ladder case) reached through
the public entry points with selector statistics, so every system of a batch is bit-known and judged on its own:
err_gpu <= 16 max(err_oracle, 64 u)  (spd_ref.accept; err_oracle = the double-precision oracle's measured error on the same system).
The normwise backward errors eta are printed, not asserted.  Cases and records: tools/chol_family_errors.py.

Which case reaches which kernel.  The entry points decide nothing: SpdBatch (capi_tv_util.h) is the one owner of the choice -- left()
(even order and chol_gemm 0) takes the left-looking kernels, everything else tvk_unpack_sym + the GEMM-built tvk_chol_batched /
tvk_spd_inverse_batched -- and launch_chol / launch_trinv / launch_uut (chol_fused.hip) pick the kernel variant under it:
  defaults, even order <= 494      k_chol_left2<1>, k_chol_solve, k_trinv_left<true,1>, k_uut<true,2>
  chol_flow 0                      k_chol_left<true>
  chol_lds 0, and orders 496, 530  k_chol_left<false>, k_trinv_left<false,2>, k_uut<false,2>
  chol_waves 16                    k_trinv_left<true,1,16>, k_uut<true,1,16>
  chol_gemm 1, and orders 33, 131  tvk_chol_batched, tvk_spd_inverse_batched + tvk_pack_sym (GEMM-built)
  update_t, even R, D <= 64        SpdBatch::factor + solve_multi: k_chol_solve_multi;  D = 65 or tv_mstep_solve 0: SpdBatch::inverse:
                                   k_chol_left2 + k_trinv_left + k_uut (full inverse) + k_dgemm;  R = 131: tvk_spd_inverse_batched + k_dgemm
"""
import functools
import os
import sys

import numpy as np
import pytest

import spd_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import chol_family_errors as cfe  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not spd_ref.HAVE_LONGDOUBLE, reason=spd_ref.SKIP_MESSAGE)]


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def batch(n):
    return spd_ref.Batch(n)


def test_the_variant_table_is_the_one_the_dispatch_code_implies():
    """Every order x variant of the plan is present: the LDS kernels' options at every order up to 494 (the last whose panel fits LDS
    next to 36 KB of static arrays), the GEMM-built path on request at even orders up to 258, nothing but the defaults past 494."""
    assert cfe.ORDERS == (2, 34, 130, 258, 492, 494, 496, 530, 33, 131)
    fits = lambda n: 32 * (n if n & 2 else n + 2) * 8 + 36 * 1024 <= 160 * 1024
    assert fits(494) and not fits(496) and cfe.LAST_LDS_ORDER == 494
    names = {n: [v[0] for v in cfe.variants(n)] for n in cfe.ORDERS}
    lds = ["defaults", "chol_flow 0", "chol_lds 0", "chol_waves 16"]
    assert names[2] == names[34] == names[130] == names[258] == lds + ["chol_gemm 1"]
    assert names[492] == names[494] == names[33] == names[131] == lds
    assert names[496] == names[530] == ["defaults"]


@pytest.mark.parametrize("n", cfe.ORDERS)
def test_every_system_of_a_batch_on_every_variant(ctx, n):
    """Four systems (cond 1e1, 1e3, 1e6, 1e3; occupations 1, 2, 4, 0.5) in one batch through tv_estimate_w (Cholesky + k_chol_solve) and
    tv_estimate_a_and_c (W, A = inverse + w w^T fold, Rm), once per variant that applies at this order."""
    b = batch(n)
    recs = []
    for name, opts in cfe.variants(n):
        recs += cfe.estep_records(ctx, b, name, opts)[0]
    assert len(recs) == 4 * len(cfe.variants(n))
    bad = cfe.failures(recs)
    assert not bad, "\n".join(bad)


def test_seven_systems_across_batch_and_super_batch_boundaries(ctx):
    """Order 130, U = 7 distinct systems with tv_batch 3 and tv_acc_mb 0 (batches and super-batches of 3 + 3 + 1), every variant: each
    system's W and A are still its own."""
    b7 = spd_ref.Batch(130, cfe.SEVEN_CONDS, cfe.SEVEN_OCCS, seed=1)
    recs = []
    for name, opts in cfe.variants(130):
        recs += cfe.estep_records(ctx, b7, name, dict(opts, **cfe.SEVEN_OPTS), tag=", U=7 tv_batch 3")[0]
    bad = cfe.failures(recs)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", cfe.LADDER_ORDERS)
def test_condition_1e8_on_both_sides_of_the_lds_boundary(ctx, n):
    """The ladder case: cond 1e8 at the largest LDS order and the first per-wave order, default route, same bar."""
    b = spd_ref.Batch(n, (1e8, 1e8), (1.0, 2.0), seed=8)
    bad = cfe.failures(cfe.estep_records(ctx, b, "defaults", {}, tag=", ladder")[0])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("R", cfe.MSTEP_ORDERS)
def test_update_t_per_gaussian_and_column_block(ctx, R):
    """gmmiv_tv_update_t, C = 3 (cond 1e1, 1e3, 1e6), D in 1, 3, 60, 64, 65, tv_mstep_solve 1 and 0, judged per Gaussian and per
    16-column block.  Route: D <= 64 with even R and tv_mstep_solve 1 goes through k_chol_solve_multi, everything else through the
    explicit inverse + GEMM -- so D = 65 gives the same bits with the option on and off, an odd R does at every D, and an even R
    with D <= 64 does NOT (substitution and inverse + GEMM round differently)."""
    m = spd_ref.MStep(R)
    recs = []
    for D in spd_ref.MSTEP_D:
        T = {}
        for ms in (1, 0):
            r, T[ms] = cfe.mstep_records(ctx, m, D, ms)
            recs += r
        explicit_either_way = D > 64 or R % 2 == 1
        assert np.array_equal(T[1], T[0]) == explicit_either_way, (R, D)
    bad = cfe.failures(recs)
    assert not bad, "\n".join(bad)


def test_not_positive_definite_on_every_variant(ctx):
    """Order 130, system 2 of 4 with a negative diagonal at column 129 (the last, ragged panel): GmmivError from both E-step entry
    points on every variant, and the next healthy call returns the bits it returned before."""
    from lia_ral_amd import capi
    b = batch(130)
    bad = b.te.copy()
    bad[2, 129 * 130 // 2 + 129] = -1e6 / b.occs[2]              # L_2[129][129] = 1 - 1e6
    for name, opts in cfe.variants(130):
        with cfe.options(ctx, opts):
            W = ctx.tv_estimate_w(b.N, b.F, b.Tm, b.invvar, b.te, b.C, b.D)
            with pytest.raises(capi.GmmivError):
                ctx.tv_estimate_w(b.N, b.F, b.Tm, b.invvar, bad, b.C, b.D)
            with pytest.raises(capi.GmmivError):
                ctx.tv_estimate_a_and_c(b.N, b.F, b.Tm, b.invvar, bad, b.C, b.D)
            W2 = ctx.tv_estimate_w(b.N, b.F, b.Tm, b.invvar, b.te, b.C, b.D)
        assert np.isfinite(W).all() and np.array_equal(W2, W), name
