"""MLLR mean adaptation, the parts that need no GPU: the C ABI is declared and exported, and the host layer's computeMLLR
(host_capi.compute_mllr) against the 80-bit reference of tests/mllr_ref.py, per dimension, judged by spd_ref.accept against the
double restatement's own error."""
import ctypes as ct
import functools
import os
import re

import numpy as np
import pytest

import mllr_ref
import spd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 1), (9, 2), (16, 3), (70, 15), (130, 31), (256, 60), (130, 62)]
needs_ld = pytest.mark.skipif(not spd_ref.HAVE_LONGDOUBLE, reason=spd_ref.SKIP_MESSAGE)


def test_entry_points_are_declared_and_exported():
    from lia_ral_amd import capi, host_capi
    header = open(os.path.join(ROOT, "include", "gmmiv.h")).read()
    assert re.search(r"\bint\s+gmmiv_mllr_adapt_models\s*\(", header)
    assert hasattr(capi.lib, "gmmiv_mllr_adapt_models") and hasattr(host_capi.lib, "liagpu_compute_mllr")
    a = np.zeros(4)
    p = a.ctypes.data_as(ct.c_void_p)
    assert capi.lib.gmmiv_mllr_adapt_models(ct.c_void_p(0), 1, 1, 1, p, p, p, p, p, p, ct.c_void_p(0)) == -1     # GMMIV_ERR_ARG: no context


def ml_estimate(k, g):
    """what the EM pass hands computeMLLR for client g: weights N / count, means F / N (NaN for the unoccupied Gaussian), count"""
    N = k["N"][g]
    count = float(int(N.sum()))
    return N / N.sum(), k["m"][g], count


@functools.lru_cache(maxsize=None)
def case(C, D):
    k = mllr_ref.generate(1, C, D, seed=100 * C + D)
    w, m, count = ml_estimate(k, 0)
    occ = w * count
    W_np, m_np = mllr_ref.restate(k["mean0"], k["cov0"], occ, m)
    W_ref, m_ref = mllr_ref.exact(k["mean0"], k["cov0"], occ, m)
    return k, (w, m, count), (W_np, m_np), (W_ref, m_ref)


def test_affine_recovery():
    """ML means that ARE an affine image of the a-priori means, m_j = A mean0_j + b (rounded to double): W = [b | A] and means = m, to
    the bar of the per-system test -- computeMLLR's error against [b | A] judged against the double restatement's error against it"""
    from lia_ral_amd import host_capi as h
    rng = np.random.default_rng(5)
    C, D = 70, 15
    k = mllr_ref.generate(1, C, D, seed=7)
    A = np.eye(D) + 0.2 * rng.normal(size=(D, D)) / np.sqrt(D)          # singular values within [0.6, 1.4]: well conditioned
    b = rng.normal(size=D)
    m = k["mean0"] @ A.T + b
    w = k["N"][0] / k["N"][0].sum()
    W, (wo, mo, co) = h.compute_mllr((w, k["mean0"], k["cov0"]), (w, m), 5000.0)
    W_np, m_np = mllr_ref.restate(k["mean0"], k["cov0"], w * 5000.0, m)
    Wt = np.concatenate([b[:, None], A], axis=1).astype(spd_ref.LD)
    failures = []
    mllr_ref.check_client(W, mo, Wt, m.astype(spd_ref.LD), W_np, m_np, "affine", failures)
    assert not failures, "\n".join(failures)


@needs_ld
@pytest.mark.parametrize("C,D", SHAPES)
def test_compute_mllr_per_system(C, D):
    from lia_ral_amd import host_capi as h
    k, (w, m, count), (W_np, m_np), (W_ref, m_ref) = case(C, D)
    W, (wo, mo, co) = h.compute_mllr((w, k["mean0"], k["cov0"]), (w, m), count)
    failures = []
    worst = mllr_ref.check_client(W, mo, W_ref, m_ref, W_np, m_np, "(%d, %d)" % (C, D), failures)
    print("(%d, %d): worst err / bar = %.3g" % (C, D, worst))
    assert not failures, "\n".join(failures)


def test_weights_and_variances_are_the_a_priori_models():
    from lia_ral_amd import host_capi as h
    k = mllr_ref.generate(1, 16, 3, seed=3)
    w0 = np.random.default_rng(1).dirichlet(np.ones(16))
    w = k["N"][0] / k["N"][0].sum()
    W, (wo, mo, co), ci = h.compute_mllr((w0, k["mean0"], k["cov0"]), (w, k["m"][0]), 1234.0, return_covinv=True)
    assert np.array_equal(wo, w0) and np.array_equal(co, k["cov0"]) and np.array_equal(ci, 1.0 / k["cov0"])


def test_compute_map_does_not_know_mllr():
    """the branch lives in adaptModel, as in the reference: computeMAP leaves the ML estimate alone"""
    from lia_ral_amd import host_capi as h
    k = mllr_ref.generate(1, 9, 2, seed=4)
    w = k["N"][0] / k["N"][0].sum()
    m = np.where(np.isnan(k["m"][0]), 0.0, k["m"][0])
    c = k["cov0"] * 1.5
    wo, mo, co = h.compute_map("MLLR", (np.full(9, 1 / 9), k["mean0"], k["cov0"]), (w, m, c), 500.0)
    assert np.array_equal(wo, w) and np.array_equal(mo, m) and np.array_equal(co, c)


def test_a_client_without_occupation_raises():
    from lia_ral_amd import host_capi as h
    k = mllr_ref.generate(1, 9, 2, seed=4)
    with pytest.raises(h.HostError):
        h.compute_mllr((np.full(9, 1 / 9), k["mean0"], k["cov0"]), (np.zeros(9), k["mean0"]), 500.0)
