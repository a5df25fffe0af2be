"""References for MLLR mean adaptation (computeMLLR, TrainTools.cpp:788-866), shared by tests/test_cpu_mllr.py and
tests/test_gpu_mllr.py.  No GPU.

    restate     the reference restated in numpy, in double, Gaussian after Gaussian in its order of operations, with np.linalg.inv
                for the explicit inverse -- the double-precision yardstick whose own error sets the bar (spd_ref.accept)
    exact       the same systems formed and solved in 80-bit long double on tests/spd_ref.py (cholesky, solve)
    generate    seeded inputs: unit-scale centred a-priori means, variances in U(0.3, 3), gamma-distributed occupations with one
                unoccupied Gaussian per client whose F row is NaN, ML means = a-priori means + 0.3 noise

Per dimension p:  G_p = sum_j (occ_j / cov0_jp) xi_j xi_j^T,  z_p = sum_j (occ_j m_jp / cov0_jp) xi_j,  xi_j = [1, mean0_j],
W[p] = G_p^-1 z_p,  new mean_j = W[:, 0] + W[:, 1:] mean0_j.  A Gaussian with occ_j = 0 is left out.
"""
import numpy as np

import spd_ref
from spd_ref import LD


def generate(G, C, D, seed, scale=1.0, shift=0.0):
    """-> dict(mean0 [C, D], cov0 [C, D], N [G, C], F [G, C*D], m [G, C, D]); client g has N[g, z_g] = 0 and F[g, z_g] = NaN"""
    rng = np.random.default_rng(seed)
    mean0 = rng.normal(size=(C, D))
    mean0 = (mean0 - mean0.mean(0)) * scale + shift
    cov0 = rng.uniform(0.3, 3.0, (C, D))
    N = rng.gamma(2.0, 40.0, (G, C))
    m = mean0[None] + 0.3 * rng.normal(size=(G, C, D))
    zero = rng.integers(0, C, G)
    F = N[:, :, None] * m
    for g in range(G):
        N[g, zero[g]] = 0.0
        F[g, zero[g]] = np.nan
        m[g, zero[g]] = np.nan
    out = dict(mean0=mean0, cov0=cov0, N=N, F=np.ascontiguousarray(F.reshape(G, C * D)), m=m, zero=zero)
    for v in out.values():
        v.setflags(write=False)
    return out


def restate(mean0, cov0, occ, m):
    """one client, double: -> (W [D, D+1], means [C, D]).  Loop order and operation order of the reference."""
    C, D = mean0.shape
    n = D + 1
    Z = np.zeros((D, n))
    Gm = np.zeros((D, n, n))
    for j in range(C):
        if occ[j] == 0.0:
            continue
        xi = np.concatenate([[1.0], mean0[j]])
        Z += ((m[j] * occ[j])[:, None] * xi[None, :]) / cov0[j][:, None]
        Gm += ((occ[j] * xi)[:, None] * xi[None, :])[None] / cov0[j][:, None, None]
    W = np.zeros((D, n))
    for p in range(D):
        Ginv = np.linalg.inv(Gm[p])
        for k in range(n):                      # W(p, c) += Ginv(c, k) Z(p, k), k innermost in the reference: the same sums per c
            W[p] += Ginv[:, k] * Z[p, k]
    means = np.empty((C, D))
    for i in range(D):
        acc = np.full(C, W[i, 0])
        for k in range(D):
            acc = acc + W[i, k + 1] * mean0[:, k]
        means[:, i] = acc
    return W, means


def systems_ld(mean0, cov0, occ, m):
    """the D systems of one client in long double: -> (G [D, n, n], z [D, n])"""
    C, D = mean0.shape
    keep = occ != 0.0
    Xi = np.concatenate([np.ones((C, 1)), mean0], axis=1)[keep].astype(LD)
    a = occ[keep].astype(LD)[:, None] / cov0[keep].astype(LD)          # [C', D]
    am = a * m[keep].astype(LD)
    XiT = np.ascontiguousarray(Xi.T)
    Gs = np.empty((D, D + 1, D + 1), LD)
    for p in range(D):
        Gs[p] = XiT @ (a[:, p:p + 1] * Xi)
    z = (XiT @ am).T                                                   # [D, n]
    return Gs, np.ascontiguousarray(z)


def exact(mean0, cov0, occ, m, keep_systems=False):
    """one client, 80-bit: -> (W [D, D+1] long double, means [C, D] long double[, G, z])"""
    Gs, z = systems_ld(mean0, cov0, occ, m)
    D = mean0.shape[1]
    W = np.empty((D, D + 1), LD)
    for p in range(D):
        W[p] = spd_ref.solve(spd_ref.cholesky(Gs[p]), z[p])
    means = W[:, 0][None, :] + mean0.astype(LD) @ W[:, 1:].T
    return (W, means, Gs, z) if keep_systems else (W, means)


def mean_error(mh, m_ref):
    """max |error| of a client's means over max |reference|"""
    return float(np.max(np.abs(np.asarray(mh, LD) - m_ref)) / np.max(np.abs(m_ref)))


def check_client(Wh, mh, W_ref, m_ref, W_np, m_np, label, failures):
    """forward error of every row of W and the error of the means against the 80-bit reference, each judged by spd_ref.accept against
    the double restatement's error on the same system; appends a line per miss, returns the worst ratio err / bar"""
    worst = 0.0
    for p in range(W_ref.shape[0]):
        e, e0 = spd_ref.forward_error(Wh[p], W_ref[p]), spd_ref.forward_error(W_np[p], W_ref[p])
        worst = max(worst, e / spd_ref.bar(e0))
        if not spd_ref.accept(e, e0):
            failures.append("%s p=%d: forward error %.3e, restatement %.3e, bar %.3e" % (label, p, e, e0, spd_ref.bar(e0)))
    e, e0 = mean_error(mh, m_ref), mean_error(m_np, m_ref)
    worst = max(worst, e / spd_ref.bar(e0))
    if not spd_ref.accept(e, e0):
        failures.append("%s means: error %.3e, restatement %.3e, bar %.3e" % (label, e, e0, spd_ref.bar(e0)))
    return worst
