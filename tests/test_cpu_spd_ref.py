"""The yardstick of tests/test_gpu_chol_family.py, checked without a GPU: the 80-bit reference routines of tests/spd_ref.py, the
bit-exactness of the selector-statistics harness, the oracle's own error through that harness, and that the acceptance function
rejects a solve with one dropped 32-wide k-chunk."""
import numpy as np
import pytest

import spd_ref
from spd_ref import LD

pytestmark = pytest.mark.skipif(not spd_ref.HAVE_LONGDOUBLE, reason=spd_ref.SKIP_MESSAGE)


def fro(M):
    return np.sqrt(np.sum(np.asarray(M, LD) ** 2))


@pytest.mark.parametrize("n", [2, 33, 34, 130])
def test_the_80_bit_factor_reproduces_the_matrix(n):
    """L L^T = A to below 1e-17 relative (Frobenius) at cond 1e6; the solve and the inverse through the factor leave residuals of the
    size cond x 2^-64 allows."""
    rng = np.random.default_rng(n)
    A = spd_ref.spd(n, 1e6, rng)
    L = spd_ref.cholesky(A)
    assert L.dtype == LD and not np.triu(L, 1).any()
    Al = np.asarray(A, LD)
    assert fro(L @ L.T - Al) / fro(Al) < 1e-17
    B = rng.normal(size=(n, 5))
    X = spd_ref.solve(L, B)
    assert fro(Al @ X - B) / (fro(Al) * fro(X)) < 1e-17
    assert np.array_equal(spd_ref.solve(L, B[:, 0]), X[:, 0])
    E = spd_ref.inverse(L)
    assert fro(E - E.T) == 0 and fro(Al @ E - np.eye(n)) / fro(Al) / fro(E) < 1e-17
    with pytest.raises(np.linalg.LinAlgError):
        spd_ref.cholesky(A - 2.0 * np.eye(n))            # smallest eigenvalue 1 -> -1


def test_spd_has_the_spectrum_it_promises_and_is_nothing_like_identity_plus_small():
    A = spd_ref.spd(130, 1e6, np.random.default_rng(0))
    ev = np.linalg.eigvalsh(A)
    assert np.array_equal(A, A.T) and abs(ev[0] - 1) < 1e-6 and abs(ev[-1] / 1e6 - 1) < 1e-9
    off = A - np.diag(np.diag(A))
    assert np.linalg.norm(off) > 0.5 * np.linalg.norm(np.diag(A))


def test_selector_statistics_are_bit_exact_in_numpy():
    """What the entry points compute before they factor, redone in numpy double: L_u = (N TETt)_u + I is the matrix the reference
    factors, aux_u = Tm[:, u], and the accumulators of tv_estimate_a_and_c come apart per system -- bit for bit."""
    b = spd_ref.Batch(34)
    n, U = b.n, b.U
    Lp = b.N @ b.te                                                  # the k_dgemm(L) of the E-step, K = C = U: one non-zero term per entry
    assert np.array_equal(Lp, np.asarray(b.occs)[:, None] * b.te)
    assert np.array_equal(spd_ref.unpack(Lp, n) + np.eye(n), b.Lmat) and np.array_equal(b.Lmat, b.Lmat.transpose(0, 2, 1))
    aux = (b.F * b.invvar) @ b.Tm.T                                  # aux = F Sigma^-1 T^T
    assert np.array_equal(aux, b.Tm.T)
    assert np.array_equal(spd_ref.pack(spd_ref.unpack(b.te, n)), b.te)
    E = np.random.default_rng(1).normal(size=(U, 7))                 # A_c = sum_u N_uc E_u = n_c E_c exactly
    assert np.array_equal((b.N.T @ E) / np.asarray(b.occs)[:, None], E)
    for u in range(U):                                               # n_u (A_u - I) / n_u + I: one rounding, in the + I
        assert abs(np.linalg.cond(b.Lmat[u]) / b.conds[u] - 1) < 1e-3


@pytest.mark.parametrize("n", [34, 66])
def test_the_oracle_through_the_harness_is_forward_accurate_to_cond_u(n):
    """The oracle's w_u, A_u and Rm through the selector statistics against the 80-bit reference: forward error <= cond x u
    (u = 2^-53) for cond 1e1, 1e3, 1e6; eta is printed.  The bound carries no factor for the order, and at cond 10 the error is a
    few roundings per entry that grow with it: measured over twelve seeds 0.24 - 0.53 cond u at order 34, 0.45 - 0.60 at 66,
    0.58 - 0.87 at 130, and 1.4 cond u (1.6e-15) at 496, where cond 1e3 / 1e6 sit at 0.27 / 0.11 cond u.  So it is asserted at
    orders 34 and 66; what the GPU tests compare with at the larger orders is the oracle's MEASURED error, not this bound."""
    from oracle import oracle as orc
    b = spd_ref.Batch(n)
    assert np.array_equal(orc.tv_estimate_w(b.N, b.F, b.Tm, b.invvar, b.te_full), b.oracle_W)    # same loops in both oracle entry points
    for u, cond in enumerate(b.conds):
        ew, ea = b.err_oracle["estimate_w/W"][u], b.err_oracle["estimate_a_and_c/A"][u]
        eta = b.eta_oracle["estimate_w/W"][u]
        print("order %d cond %.0e: oracle forward error W %.2e (%.3f cond u)  A %.2e  eta %.2e" % (n, cond, ew, ew / (cond * spd_ref.U_DOUBLE), ea, eta))
        assert ew <= cond * spd_ref.U_DOUBLE
        assert eta < 16 * spd_ref.U_DOUBLE
        assert spd_ref.accept(ew, ew) and spd_ref.accept(ea, ea)
    ms = spd_ref.MStep(n)
    eo, ho = ms.oracle_errors(65)
    for (c, j0, j1), e, h in zip(ms.blocks(65), eo, ho):
        print("update_t order %d cond %.0e columns %d:%d: oracle forward error %.2e eta %.2e" % (n, ms.conds[c], j0, j1, e, h))
        assert e <= ms.conds[c] * spd_ref.U_DOUBLE
    assert len(eo) == 3 * 5


@pytest.mark.parametrize("n,cond", [(34, 1e1), (130, 1e1), (130, 1e6), (494, 1e1)])
def test_a_dropped_k_chunk_is_rejected_by_the_acceptance_function(n, cond):
    """The yardstick bites: a double-precision solve passes the bar; the same solve with ONE 32-wide k-chunk of row 33 of the factor
    zeroed (what a wave that skips a chunk of its panel would compute) misses it by orders of magnitude, at cond 10 and at 1e6."""
    rng = np.random.default_rng(n)
    A = spd_ref.spd(n, cond, rng)
    b = rng.normal(size=n)
    x = spd_ref.solve(spd_ref.cholesky(A), b)
    err_oracle = spd_ref.forward_error(np.linalg.solve(A, b), x)        # a sound double-precision solve as the yardstick's anchor
    Ld = np.linalg.cholesky(A)
    sub = lambda Lf: np.asarray(spd_ref.solve(np.asarray(Lf, LD), b), np.float64)
    good = spd_ref.forward_error(sub(Ld), x)
    assert spd_ref.accept(good, err_oracle), (good, err_oracle)
    Lb = Ld.copy()
    Lb[33, 0:32] = 0.0                                                   # row 33's only off-diagonal chunk: columns 0 .. 31
    broken = spd_ref.forward_error(sub(Lb), x)
    print("order %d cond %.0e: sound %.2e  dropped chunk %.2e  bar %.2e" % (n, cond, good, broken, spd_ref.bar(err_oracle)))
    assert not spd_ref.accept(broken, err_oracle) and broken > 1e3 * spd_ref.bar(err_oracle)
    assert not spd_ref.accept(float("nan"), err_oracle)
