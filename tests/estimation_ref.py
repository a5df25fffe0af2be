"""References, cases and bars for the back-end ESTIMATION entry points -- the nine that tests/test_gpu_tv.py judged by
`max|a - b| / max|b|` over a whole array alone: gmmiv_dev_mahalanobis, gmmiv_dev_wccn_chol, gmmiv_plda_precompute,
gmmiv_twocov_model (governed by an inverse), gmmiv_sym_eigen, gmmiv_dev_efr_matrix, gmmiv_dev_lda, gmmiv_plda_em_iteration (host
eigen / EM code fed by device kernels) and gmmiv_tv_orthonormalize_t.  Shared by tests/test_cpu_estimation_ref.py and
tests/test_gpu_estimation_elementwise.py.  No test lives here, and no GPU.

For every entry point `e` (ENTRIES):
    reference(e, key)   the operation in np.longdouble from the same double inputs (tests/spd_ref.py for Cholesky and inverse; the
                        eigen problems by a cyclic Jacobi in long double run until the off-diagonal is below 2^-60 of the norm; LDA
                        through the symmetric form L^-1 B L^-T)
    restate(e, key)     a float64 numpy restatement of the LIBRARY's algorithm at the level of its steps (Gram matrix, Cholesky,
                        triangular inverse, product; the cyclic Jacobi of host_linalg.cpp rotation by rotation; the host sequence of
                        gmmiv_plda_em_iteration with its per-session-count cache; Gram / Cholesky / L^-1 / product or the classical
                        Gram-Schmidt steps of tv_orthonormalize_t, chosen by ITS OWN dmin > 1e-4 dmax), with an optional planted `defect`
    oracle(e, key)      the project's fp64 oracle on the same inputs
    errors(e, key, got) the error of every unit of `got`, evaluated in long double -> {unit kind: array}
    judge(e, key, got)  every error over its bar -> {unit kind: ratios}

The bar (one rule, tests/spd_ref.py: accept): err <= 16 max(err_double, 64 u), err_double = the error of the float64 restatement on
the SAME unit against the 80-bit reference; the oracle's error on that unit is recorded next to it (err_oracle).  The library's own
output never sets a bar.  A unit is a vector -- a column, a row, an eigenpair -- wherever the bar is a measured error: the float64
error of one element can vanish by accident.  Kinds that start with "!" are a-priori and arrive as ratios already (unit norm of an
LDA row to 4 u).

Units
    inverses            per column, forward error against the reference scaled by that column of the reference (dev_mahalanobis; G, H
                        of twocov_model; FTJ, FTJF of plda_precompute); dev_mahalanobis also per column the backward error
                        ||e_j - W x^_j|| / (||W||_2 ||x^_j|| + 1), W formed in 80-bit; dev_wccn_chol per row of the upper factor
    sym_eigen           per pair ||A v^ - l^ v^|| / ||A||_2, per value |l^ - l| / ||A||_2, every row of V^T V - I; never component
                        by component (signs, and close pairs, are not defined)
    dev_efr_matrix      rows of M S M^T - I (S in 80-bit); per row ||S m_j^T / l_j - m_j^T|| / ||m_j||
    dev_lda             values relative to the largest; per row ||B l - l^ W l|| / (||B||_2 ||l||); unit norm to 4 u
    plda_em_iteration   F, G per column, Delta as one vector, Sigma per row after scaling both sides by the reference's diag^-1/2
    tv_orthonormalize_t with L = T Q^T in 80-bit: per row ||t_j - (tril L Q^)_j|| / ||t_j||, per row the strictly upper part of L over
                        ||t_j||, every row of Q^ Q^T - I over the non-zero rows, per row the forward error against the 80-bit
                        Gram-Schmidt

err_oracle against err_double, both floored at 64 u (test_cpu_estimation_ref.py prints the range per entry point and kind).  The
expected gap did not show: on tv_orthonormalize_t the oracle's classical Gram-Schmidt and the restatement's Cholesky-QR lose the
same cond(T)^2 u of orthogonality, and at dmin / dmax = 2e-4 (Gram route) the oracle's rows of `Q Q^T - I` and of `T - L Q` read at
most 1.5 times the restatement's; the two inverse routes (the oracle's Gauss-Jordan, the restatement's Cholesky) differ by 0.1 ...
6.5 on the columns of twocov_model at cond 1e6 and by nothing above the floor elsewhere.  The one place beyond the factor 16 is a
unit that is a single number: one eigenvalue of dev_lda (0.014 ... 42 times).  There err_double is not the error on that one value
but the root mean square over all the values of the matrix (unit_err_double) -- a correction of the bar's derivation, not of the
factor: with it the restatement and the oracle read at most 0.35.

Two things the EM iteration taught the references.  Its per-speaker sums are taken session after session (k_dev_spk_sums), so the
restatement takes them so (seq_sum): numpy's pairwise sum of 600 sessions is an order more exact than the library can be.  And the
state of the second iteration is the library's own output, whose Sigma is symmetric only to rounding: the library's host
factorisations read the upper triangle, so the restatement does (upper_sym), and the reference takes the symmetric part.  Reading
the lower triangle instead moves the G columns of the [600, 1, 2] case by 3e-13, 200 times the restatement's own error there.
"""
import functools
import math

import numpy as np

import backend_ref as br
import spd_ref as sr
from backend_ref import LD, f64, ld, mm

u = sr.U_DOUBLE
HAVE_LONGDOUBLE = sr.HAVE_LONGDOUBLE
SKIP_MESSAGE = sr.SKIP_MESSAGE
CONDS = (1e1, 1e3, 1e6)
ROUTE_THRESHOLD = 1e-4            # gmmiv_tv_orthonormalize_t: the Gram route when dmin > 1e-4 dmax


# ================================================================ small tools
def nrm(v, axis=None):
    v = ld(v)
    return np.sqrt(np.sum(v * v, axis=axis))


def safe_div(a, b):
    """a / b where b > 0, else 0 where a == 0 (a zero row against a zero row), else inf"""
    a, b = ld(a), ld(b)
    out = np.where(a == 0, LD(0), LD(np.inf))
    np.divide(a, b, out=out, where=b > 0)
    return out


def col_err(Xh, X):
    return f64(safe_div(nrm(ld(Xh) - X, 0), nrm(X, 0)))


def row_err(Xh, X):
    return f64(safe_div(nrm(ld(Xh) - X, 1), nrm(X, 1)))


def bar(err_double):
    return 16.0 * np.maximum(np.asarray(err_double, np.float64), 64.0 * u)


def seq_sum(Y):
    """row sums taken left to right, one session after the other, as k_dev_spk_sums takes them (numpy's .sum is pairwise)"""
    return np.cumsum(Y, axis=1)[:, -1]


def inv_ld(A):
    return sr.inverse(sr.cholesky(A))


def tri_inv64(L):
    """L^-1 of a lower factor, float64, row by row (host_lower_inverse / the substitution inside host_spd_inverse)"""
    n = L.shape[0]
    Li = np.zeros((n, n))
    for i in range(n):
        Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
        Li[i, i] = 1.0 / L[i, i]
    return Li


INVERSE_DEFECT = "the last column of the ragged 32-wide tail dropped from the product for the faint column"


def upper_sym(A):
    """the symmetric matrix the library's host factorisations see: they read the UPPER triangle (host_cholesky_upper).  It matters
    for the second EM iteration, whose Sigma is the library's own output and symmetric only to rounding: read through the other
    triangle, the same state gives G columns that differ by 3e-13 where the restatement's own error is 1e-15"""
    return np.triu(A) + np.triu(A, 1).T


def inv64(A, defect=None):
    """SPD inverse the way the library forms it: Cholesky factor, its triangular inverse, the product L^-T L^-1.  The defect: the
    k-loop of that product in 32-wide tiles loses the last column of its ragged tail (k = n - 1) for output row / column 0"""
    Li = tri_inv64(np.linalg.cholesky(upper_sym(A)))
    E = Li.T @ Li
    if defect == INVERSE_DEFECT:
        n = A.shape[0]
        assert n % 32, "no ragged tail at order %d" % n
        miss = Li[n - 1, 0] * Li[n - 1, :]
        E[0, :] -= miss
        E[1:, 0] -= miss[1:]
    return E


def chol_upper64(A):
    return np.ascontiguousarray(np.linalg.cholesky(upper_sym(A)).T)


# ================================================================ cyclic Jacobi (host_linalg.cpp: host_sym_eigen), any precision
def jacobi(A, dtype, max_sweeps=100):
    """-> (values descending, vectors as columns).  float64: the library's loop, rotation by rotation (columns p, q of a, rows p, q
    of a, columns p, q of v), its stopping rule off <= 1e-30 (dg + off) over squares and its stable descending sort; long double:
    until the off-diagonal is below 2^-60 of the Frobenius norm"""
    n = A.shape[0]
    exact = dtype is not np.float64
    W = np.empty((2 * n, n), dtype)                 # a on top of v: one column rotation serves both (v never feeds back into a)
    a, v = W[:n], W[n:]
    a[:] = A
    v[:] = np.eye(n)
    skip = 0
    if exact and n > 2:
        # the long-double run starts from numpy's float64 basis, made orthogonal in long double (two Cholesky passes on V^T V): the
        # same eigenvalues, two sweeps instead of ten, and rotations below 2^-70 of the norm are left out
        V0 = ld(np.linalg.eigh(np.asarray(A, np.float64))[1])
        for _ in range(2):
            V0 = sr.forward_subst(sr.cholesky(mm(V0.T, V0)), V0.T).T
        a[:] = mm(mm(V0.T, ld(A)), V0)
        a[:] = (a + a.T) / 2
        v[:] = V0
        skip = LD(2.0) ** -70 * np.sqrt(np.sum(a * a)) / n
    sqrt = np.sqrt if exact else math.sqrt
    one = dtype(1) if exact else 1.0
    for sweep in range(max_sweeps):
        d = np.diag(a)
        dg = np.sum(d * d)
        off = np.sum(np.triu(a, 1) ** 2)
        if exact:
            if np.sqrt(2 * off) <= LD(2.0) ** -60 * np.sqrt(dg + 2 * off):
                break
        elif off <= 1e-30 * (dg + off):
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = a[p, q] if exact else a.item(p, q)
                if apq == 0 or abs(apq) <= skip:
                    continue
                th = ((a[q, q] - a[p, p]) if exact else (a.item(q, q) - a.item(p, p))) / (2 * apq)
                t = (one if th >= 0 else -one) / (abs(th) + sqrt(th * th + one))
                cs = one / sqrt(t * t + one)
                sn = t * cs
                x, y = W[:, p].copy(), W[:, q]
                W[:, p] = cs * x - sn * y
                W[:, q] = sn * x + cs * y
                x, y = a[p].copy(), a[q]
                a[p] = cs * x - sn * y
                a[q] = sn * x + cs * y
    else:
        raise AssertionError("Jacobi did not converge in %d sweeps" % max_sweeps)
    d = np.diag(a).copy()
    order = np.argsort(-d, kind="stable")
    return d[order], np.ascontiguousarray(v[:, order])


# ================================================================ development sets
def _gen_dev(dim, sps):
    sps = np.asarray(sps, np.int64)
    rng = np.random.default_rng(100 * dim + len(sps))
    k, n = len(sps), int(sps.sum())
    cls = np.repeat(np.arange(k), sps)
    return np.ascontiguousarray((rng.normal(size=(dim, k)) * 1.5)[:, cls] + rng.normal(size=(dim, n))), sps


OWN_DEV = {"1x[2,3,1]": (1, (2, 3, 1)), "2x[3,2,2]": (2, (3, 2, 2)), "5x[4,3,5,2]": (5, (4, 3, 5, 2)), "34x[3]*40": (34, (3,) * 40),
           "65x[2]*100": (65, (2,) * 100)}
SHARED_DEV = ("3x[1,2,1]", "33x257", "8x[600,1,2]", "33x257 scaled")            # of backend_ref.DEV_CASES
DEV_SETS = tuple(OWN_DEV)[:3] + SHARED_DEV + tuple(OWN_DEV)[3:]


@functools.lru_cache(maxsize=None)
def dev_set(name):
    X, sps = _gen_dev(*OWN_DEV[name]) if name in OWN_DEV else br.dev_inputs(name)
    X.setflags(write=False)
    return X, np.asarray(sps, np.int64)


def invertible(name):
    X, _ = dev_set(name)
    return X.shape[1] > 2 * X.shape[0]


INV_DEV_SETS = tuple(s for s in DEV_SETS if s != "3x[1,2,1]")       # n > 2 dim: the sets that go to the inverse-governed calls


def _dev_parts(X, sps, dtype):
    """centred-per-speaker data in `dtype`: -> (Yw, counts per session)"""
    k = len(sps)
    off = np.concatenate([[0], np.cumsum(sps)])
    cls = np.repeat(np.arange(k), sps)
    Xl = np.asarray(X, dtype)
    sm = np.stack([seq_sum(Xl[:, off[c]:off[c + 1]]) / dtype(sps[c]) for c in range(k)], 1)
    return Xl - sm[:, cls], np.asarray(sps, dtype)[cls]


@functools.lru_cache(maxsize=None)
def dev_cov(name):
    """float64 (Sigma, W, B) of a dev set: the INPUTS of sym_eigen / efr / lda, from numpy"""
    r = br.dev_restate(name) if name in br.DEV_CASES else None
    if r is None:
        X, sps = dev_set(name)
        n = X.shape[1]
        cls = np.repeat(np.arange(len(sps)), sps)
        off = np.concatenate([[0], np.cumsum(sps)])
        mean = X.mean(1)
        sm = np.stack([X[:, off[c]:off[c + 1]].mean(1) for c in range(len(sps))], 1)
        Y, Yw, Yb = X - mean[:, None], X - sm[:, cls], (sm - mean[:, None]) * np.sqrt(sps)
        r = {"Sigma": Y @ Y.T / n, "W": Yw @ Yw.T / n, "B": Yb @ Yb.T / n}
    return tuple(np.ascontiguousarray((r[q] + r[q].T) / 2) for q in ("Sigma", "W", "B"))


# ================================================================ dev_mahalanobis, dev_wccn_chol
@functools.lru_cache(maxsize=None)
def mahalanobis_reference(name):
    X, sps = dev_set(name)
    Yw, _ = _dev_parts(X, sps, LD)
    W = mm(Yw, Yw.T) / X.shape[1]
    return {"W": W, "norm2": float(np.linalg.norm(f64(W), 2)), "M": inv_ld(W)}


def mahalanobis_restate(name, defect=None):
    X, sps = dev_set(name)
    Yw, _ = _dev_parts(X, sps, np.float64)
    return inv64(Yw @ Yw.T / X.shape[1], defect)


def mahalanobis_oracle(name):
    from oracle import oracle as orc
    X, sps = dev_set(name)
    return orc.invert(orc.dev_cov_mat(X, sps)[1])


def mahalanobis_errors(name, got):
    r = mahalanobis_reference(name)
    Xh = ld(got)
    res = np.eye(Xh.shape[0], dtype=LD) - mm(r["W"], Xh)
    return {"forward column": col_err(got, r["M"]), "backward column": f64(nrm(res, 0) / (LD(r["norm2"]) * nrm(Xh, 0) + 1))}


@functools.lru_cache(maxsize=None)
def wccn_reference(name):
    X, sps = dev_set(name)
    Yw, cnt = _dev_parts(X, sps, LD)
    Y = Yw / np.sqrt(cnt)
    return sr.cholesky(inv_ld(mm(Y, Y.T) / len(sps))).T


def wccn_restate(name, defect=None):
    X, sps = dev_set(name)
    Yw, cnt = _dev_parts(X, sps, np.float64)
    Y = Yw / np.sqrt(cnt)
    return chol_upper64(inv64(Y @ Y.T / len(sps), defect))


def wccn_oracle(name):
    from oracle import oracle as orc
    return orc.dev_wccn_chol(*dev_set(name))


def wccn_errors(name, got):
    low = np.tril(np.asarray(got), -1)
    return {"factor row": row_err(got, wccn_reference(name)), "!zeros below the diagonal": np.where(low != 0.0, np.inf, 0.0).max(1, initial=0.0)}


# ================================================================ twocov_model
TWOCOV_CASES = tuple((n, c) for n in (1, 2, 33, 34, 65) for c in CONDS)


@functools.lru_cache(maxsize=None)
def twocov_inputs(key):
    n, cond = key
    rng = np.random.default_rng(int(31 * n + np.log10(cond)))
    W, B = sr.spd(n, cond, rng), sr.spd(n, cond, rng)
    W.setflags(write=False)
    B.setflags(write=False)
    return W, B


@functools.lru_cache(maxsize=None)
def twocov_reference(key):
    W, B = twocov_inputs(key)
    iW, iB = inv_ld(W), inv_ld(B)
    return tuple(mm(mm(iW, inv_ld(iB + a * iW)), iW) for a in (2, 1))


def twocov_restate(key, defect=None):
    W, B = twocov_inputs(key)
    iW, iB = inv64(W, defect), inv64(B)
    return tuple(iW @ inv64(iB + a * iW) @ iW for a in (2.0, 1.0))


def twocov_oracle(key):
    from oracle import oracle as orc
    return orc.twocov_model(*twocov_inputs(key))


def twocov_errors(key, got):
    G, H = twocov_reference(key)
    return {"G column": col_err(got[0], G), "H column": col_err(got[1], H)}


# ================================================================ plda_precompute
PRECOMPUTE_CASES = ((1, 1, 0), (5, 2, 1), (33, 7, 3), (34, 5, 5), (6, 2, 9), (65, 9, 4), (34, 33, 0))
PRECOMPUTE_DIRTY = (67, 9, 11)                       # the larger odd order of the NaN call that goes before


@functools.lru_cache(maxsize=None)
def precompute_inputs(key):
    dim, rf, rg = key
    rng = np.random.default_rng(1000 * dim + 10 * rf + rg)
    F = rng.normal(size=(dim, rf)) / np.sqrt(dim)
    G = rng.normal(size=(dim, rg)) / np.sqrt(dim) if rg else None
    A = rng.normal(size=(dim, dim))
    out = (np.ascontiguousarray(F), G, np.ascontiguousarray(A @ A.T / dim + np.eye(dim)))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def _precompute(F, G, S, inv, mul):
    Si = inv(S)
    Ftw = mul(F.T, Si)
    FTJ = Ftw
    if G is not None:
        Gtw = mul(G.T, Si)
        GG = mul(Gtw, G)
        GG = GG + np.eye(GG.shape[0], dtype=GG.dtype)
        FTJ = Ftw - mul(mul(mul(Ftw, G), inv(GG)), Gtw)
    return FTJ, mul(FTJ, F)


@functools.lru_cache(maxsize=None)
def precompute_reference(key):
    F, G, S = precompute_inputs(key)
    return _precompute(ld(F), None if G is None else ld(G), ld(S), inv_ld, mm)


def precompute_restate(key, defect=None):
    F, G, S = precompute_inputs(key)
    return _precompute(F, G, S, lambda A: inv64(A, defect if A.shape[0] % 32 else None), np.matmul)


def precompute_oracle(key):
    from oracle import oracle as orc
    return orc.plda_precompute(*precompute_inputs(key))


def precompute_errors(key, got):
    FTJ, FTJF = precompute_reference(key)
    return {"FTJ column": col_err(got[0], FTJ), "FTJF column": col_err(got[1], FTJF)}


# ================================================================ sym_eigen, dev_efr_matrix, dev_lda
EIGEN_ORDERS = (1, 2, 33, 64, 65)
REPEATED = "diag(2,2,1) rotated"


def eigen_matrices():
    return tuple(("spd", n, c) for n in EIGEN_ORDERS for c in CONDS) + tuple(("dev", s, "Sigma") for s in DEV_SETS) + (("repeated", 3, 0),)


def ranks(n):
    return tuple(sorted({n, max(n // 2, 1), 1}, reverse=True))


@functools.lru_cache(maxsize=None)
def eigen_matrix(mkey):
    kind, a, b = mkey
    if kind == "spd":
        A = sr.spd(a, b, np.random.default_rng(int(1000 * a + np.log10(b))))
    elif kind == "dev":
        A = dev_cov(a)[0].copy()
    else:
        Q = np.linalg.qr(np.random.default_rng(3).normal(size=(3, 3)))[0]
        A = (Q * np.array([2.0, 2.0, 1.0])) @ Q.T
        A = (A + A.T) / 2
    A = np.ascontiguousarray(A)
    A.setflags(write=False)
    return A


EIGEN_CASES = tuple((m, r) for m in eigen_matrices() for r in ranks(eigen_matrix(m).shape[0]))
EFR_CASES = tuple(m for m in eigen_matrices() if m[0] != "repeated")


@functools.lru_cache(maxsize=None)
def eigen_full(mkey, exact):
    return jacobi(eigen_matrix(mkey), LD if exact else np.float64)


def eigen_reference(key):
    val, vect = eigen_full(key[0], True)
    return vect[:, :key[1]], val[:key[1]]


EIGEN_DEFECT = "an eigenpair swapped without its value"


def eigen_restate(key, defect=None):
    val, vect = eigen_full(key[0], False)
    vect, val = vect[:, :key[1]].copy(), val[:key[1]].copy()
    if defect == EIGEN_DEFECT:
        assert key[1] >= 2
        vect[:, [0, 1]] = vect[:, [1, 0]]
    return vect, val


def eigen_oracle(key):
    from oracle import oracle as orc
    return orc.sym_eigen(eigen_matrix(key[0]), key[1])


def eigen_errors_of(A, val_ref, vect, val):
    """the judgement of (vect [n x rank], val [rank]) as an eigen decomposition of A -- shared with tests/test_cpu_host_linalg.py"""
    A, V, l = ld(A), ld(vect), ld(val)
    scale = np.max(np.abs(val_ref))
    rank = V.shape[1]
    out = {"pair": f64(nrm(mm(A, V) - V * l, 0) / scale), "value": f64(np.abs(l - val_ref[:rank]) / scale),
           "orthonormality row": f64(nrm(mm(V.T, V) - np.eye(rank, dtype=LD), 1)),
           "!descending": np.where(np.diff(np.asarray(val, np.float64)) > 0, np.inf, 0.0)}
    return out


def eigen_errors(key, got):
    out = eigen_errors_of(eigen_matrix(key[0]), eigen_full(key[0], True)[0], *got)
    if key[0][0] == "repeated":
        del out["orthonormality row"]            # inside the repeated pair only values and residuals are judged
    return out


def efr_reference(mkey):
    val, vect = eigen_full(mkey, True)
    return (vect / np.sqrt(val)).T


def efr_restate(mkey, defect=None):
    val, vect = eigen_full(mkey, False)
    return np.ascontiguousarray((vect / np.sqrt(val)).T)


def efr_oracle(mkey):
    from oracle import oracle as orc
    return orc.dev_efr_matrix(eigen_matrix(mkey))


def efr_errors(mkey, got):
    S, M = ld(eigen_matrix(mkey)), ld(got)
    val = eigen_full(mkey, True)[0]
    n = S.shape[0]
    return {"whitening row": f64(nrm(mm(mm(M, S), M.T) - np.eye(n, dtype=LD), 1)),
            "eigen row": f64(nrm(mm(M, S) / val[:, None] - M, 1) / nrm(M, 1))}


def lda_matrices():
    return tuple(("spd", n, c) for n in EIGEN_ORDERS for c in CONDS) + tuple(("dev", s, "W,B") for s in INV_DEV_SETS)


@functools.lru_cache(maxsize=None)
def lda_inputs(mkey):
    kind, a, b = mkey
    if kind == "spd":
        rng = np.random.default_rng(int(77 * a + np.log10(b)))
        W, B = sr.spd(a, b, rng), sr.spd(a, 1e1, rng)
    else:
        _, W, B = dev_cov(a)
    W, B = np.ascontiguousarray(W), np.ascontiguousarray(B)
    W.setflags(write=False)
    B.setflags(write=False)
    return W, B


LDA_CASES = tuple((m, r) for m in lda_matrices() for r in ranks(lda_inputs(m)[0].shape[0]))


@functools.lru_cache(maxsize=None)
def lda_full(mkey, exact):
    """-> (values descending, unit-norm generalised eigenvectors as ROWS), all of them"""
    W, B = lda_inputs(mkey)
    n = W.shape[0]
    if exact:
        L = sr.cholesky(W)
        Cm = sr.forward_subst(L, sr.forward_subst(L, ld(B)).T).T                  # L^-1 B L^-T
        val, Y = jacobi((Cm + Cm.T) / 2, LD)
        rows = sr.backward_subst(L, Y).T                                           # l = L^-T y
        return val, rows / nrm(rows, 1)[:, None]
    U = chol_upper64(W)                                                            # W = U^T U, L = U^T
    T1 = np.empty((n, n))
    for i in range(n):                                                             # host_upper_tsolve_cols: T1 = U^-T B
        T1[i] = (B[i] - U[:i, i] @ T1[:i]) / U[i, i]
    Cm = np.empty((n, n))
    for i in range(n):                                                             # host_upper_rsolve_rows: Cm = T1 U^-1
        Cm[:, i] = (T1[:, i] - Cm[:, :i] @ U[:i, i]) / U[i, i]
    val, Y = jacobi((Cm + Cm.T) / 2, np.float64)
    rows = np.empty((n, n))
    for j in range(n):                                                             # host_upper_solve_vec, then unit norm by a running sum
        x = np.zeros(n)
        for i in range(n - 1, -1, -1):
            x[i] = (Y[i, j] - U[i, i + 1:] @ x[i + 1:]) / U[i, i]
        s = 0.0
        for t in x:
            s += t * t
        rows[j] = x / np.sqrt(s)
    return val, rows


def lda_reference(key):
    val, rows = lda_full(key[0], True)
    return rows[:key[1]], val[:key[1]]


def lda_restate(key, defect=None):
    val, rows = lda_full(key[0], False)
    return rows[:key[1]].copy(), val[:key[1]].copy()


def lda_oracle(key):
    from oracle import oracle as orc
    return orc.dev_lda(*lda_inputs(key[0]), key[1])


def lda_errors(key, got):
    W, B = lda_inputs(key[0])
    val_ref = lda_full(key[0], True)[0]
    Lm, l = ld(got[0]), ld(got[1])
    nB = LD(np.linalg.norm(B, 2))
    res = mm(Lm, ld(B).T) - l[:, None] * mm(Lm, ld(W).T)                          # rows: (B l - lambda W l)^T
    return {"value": f64(np.abs(l - val_ref[:key[1]]) / np.max(np.abs(val_ref))), "pair row": f64(nrm(res, 1) / (nB * nrm(Lm, 1))),
            "!unit norm": f64(np.abs(nrm(Lm, 1) - 1) / (4 * u)), "!descending": np.where(np.diff(np.asarray(got[1], np.float64)) > 0, np.inf, 0.0)}


# ================================================================ plda_em_iteration
EM_CASES = {"1x1x0 [1,2,1]": (1, 1, 0, (1, 2, 1)), "2x1x1 [1,2,1]": (2, 1, 1, (1, 2, 1)), "5x2x1 [1,2,1,3]": (5, 2, 1, (1, 2, 1, 3)),
            "5x3x0 [1,2,1,3]": (5, 3, 0, (1, 2, 1, 3)), "33x7x3 257 speakers": (33, 7, 3, None), "8x3x2 [600,1,2]": (8, 3, 2, (600, 1, 2)),
            "34x5x5 [3]*40": (34, 5, 5, (3,) * 40), "65x9x4 [2]*100": (65, 9, 4, (2,) * 100)}
# variants that exist for the planted defects alone (tests/test_cpu_estimation_ref.py): the smallest form in which each defect has a
# meaning -- a 257th speaker whose sessions are those of the 1st but for 1e-9, a last session of the 600-session speaker that sits
# 1e-7 from Delta, a Delta of size 1e-10
EM_VARIANTS = {"33x7x3 257 speakers, 257th a twin of the 1st": ("33x7x3 257 speakers", "twin"),
               "8x3x2 [600,1,2], last of the 600 sessions faint": ("8x3x2 [600,1,2]", "faint session"),
               "5x2x1 [1,2,1,3], Delta 1e-10": ("5x2x1 [1,2,1,3]", "small Delta")}
EM_DEFECTS = ("Eh of the 257th speaker taken from the 1st", "the last session of the 600-session speaker missing from one latent row",
              "Delta not subtracted")


@functools.lru_cache(maxsize=None)
def em_inputs(name):
    """-> (X, sps, F, G, Sigma, Delta): data as in test_plda_em_iterations_match_oracle, with a non-zero initial Delta"""
    base, variant = EM_VARIANTS.get(name, (name, None))
    dim, rf, rg, sps = EM_CASES[base]
    sps = br._sps_257() if sps is None else np.asarray(sps, np.int64)
    if variant == "twin":
        sps = sps.copy()
        sps[256] = sps[0]
    rng = np.random.default_rng(1000 * dim + 10 * rf + rg)
    k, n = len(sps), int(sps.sum())
    cls = np.repeat(np.arange(k), sps)
    Ft, Gt = rng.normal(size=(dim, rf)), 0.5 * rng.normal(size=(dim, rg))
    X = Ft @ rng.normal(size=(rf, k))[:, cls] + Gt @ rng.normal(size=(rg, n)) + 0.3 * rng.normal(size=(dim, n)) + 0.2
    F, G = rng.normal(size=(dim, rf)), 0.5 * rng.normal(size=(dim, rg))
    Sigma = np.atleast_2d(np.cov(X)) + 0.1 * np.eye(dim)
    Delta = 0.1 * rng.normal(size=dim) + 0.05
    if variant == "twin":
        X[:, n - sps[256]:] = X[:, :sps[0]] + 1e-9 * rng.normal(size=(dim, sps[0]))
    elif variant == "faint session":
        X[:, sps[0] - 1] = Delta + 1e-7 * rng.normal(size=dim)
    elif variant == "small Delta":
        Delta = Delta * 1e-9
    out = tuple(np.ascontiguousarray(a) for a in (X, sps, F, G, Sigma, Delta))
    for a in out:
        a.setflags(write=False)
    return out


def em_reference(X, sps, F, G, Sigma, Delta):
    """one PldaModel::em_iteration in long double from the given double state -> (X centred, F, G, Sigma, Delta)"""
    dim, n = X.shape
    rf, rg = F.shape[1], G.shape[1]
    k = len(sps)
    cls = np.repeat(np.arange(k), sps)
    off = np.concatenate([[0], np.cumsum(sps)])
    X, F, G, Sigma, Delta = ld(X), ld(F), ld(G), ld(Sigma), ld(Delta)
    Sigma = (Sigma + Sigma.T) / 2                                    # a state that is symmetric only to rounding: its symmetric part
    Xc = X - Delta[:, None]
    Si = inv_ld(Sigma)
    Ftw, Gtw = mm(F.T, Si), mm(G.T, Si)
    iGG = inv_ld(mm(Gtw, G) + np.eye(rg, dtype=LD)) if rg else np.zeros((0, 0), LD)
    FtwG = mm(Ftw, G)
    S = mm(iGG, FtwG.T)                                              # [rg x rf]
    A = mm(Ftw, F) - mm(mm(FtwG, iGG), FtwG.T)
    fi, gi = mm(Ftw, Xc), mm(Gtw, Xc)
    f = np.stack([fi[:, off[c]:off[c + 1]].sum(1) for c in range(k)], 1)
    g = np.stack([gi[:, off[c]:off[c + 1]].sum(1) for c in range(k)], 1)
    rh = rf + rg
    Ehh = np.zeros((rh, rh), LD)
    H = np.zeros((rf, k), LD)
    memo = {}
    for c in range(k):
        ns = int(sps[c])
        if ns not in memo:
            M = inv_ld(ns * A + np.eye(rf, dtype=LD))
            MsT = mm(M, S.T)
            memo[ns] = (M, np.block([[M, -MsT], [-MsT.T, iGG + mm(S, MsT)]]))
        H[:, c] = memo[ns][0] @ (f[:, c] - S.T @ g[:, c])
        Ehh += ns * memo[ns][1]
    Eh = np.concatenate([H[:, cls], mm(iGG, gi) - mm(S, H)[:, cls]], 0)
    Ehh += mm(Eh, Eh.T)
    xh = mm(Xc, Eh.T)
    Um = Eh.sum(1) / n
    FG = mm(xh, inv_ld(Ehh))
    Sg = (mm(Xc, Xc.T) - mm(FG, xh.T)) / n
    cov = Ehh / n - np.outer(Um, Um)
    Fn = mm(FG[:, :rf], sr.cholesky(cov[:rf, :rf]))                  # FG Rh^T, Rh^T the lower factor
    Gn = mm(FG[:, rf:], sr.cholesky(cov[rf:, rf:])) if rg else np.zeros((dim, 0), LD)
    return Xc, Fn, Gn, Sg, Delta + FG @ Um


def em_restate(X, sps, F, G, Sigma, Delta, defect=None):
    """float64, the host sequence of gmmiv_plda_em_iteration: centre, total second moment, the pre-computation, (Ftw; Gtw) X and its
    per-speaker sums, the per-speaker expectations with the (M, tmpM) cache per session count, the expansion of Eh, its Gram
    matrix and X Eh^T, the M-step"""
    dim, n = X.shape
    rf, rg = F.shape[1], G.shape[1]
    rh, k = rf + rg, len(sps)
    cls = np.repeat(np.arange(k), sps)
    off = np.concatenate([[0], np.cumsum(sps)])
    Xc = X.copy() if defect == EM_DEFECTS[2] else X - Delta[:, None]
    sigObs = Xc @ Xc.T
    Si = inv64(Sigma)
    Ftw, Gtw = F.T @ Si, G.T @ Si
    iGG = inv64(Gtw @ G + np.eye(rg)) if rg else np.zeros((0, 0))
    FtwG = Ftw @ G
    S = iGG @ FtwG.T
    A = Ftw @ F - (FtwG @ iGG) @ FtwG.T
    FGX = np.concatenate([Ftw, Gtw], 0) @ Xc
    fg = np.stack([seq_sum(FGX[:, off[c]:off[c + 1]]) for c in range(k)], 1)
    if defect == EM_DEFECTS[1]:
        c = int(np.argmax(sps))
        fg[rh - 1, c] -= FGX[rh - 1, off[c + 1] - 1]
    Hs, Ehh, Um, gsum, cache = np.zeros((rh, k)), np.zeros((rh, rh)), np.zeros(rh), np.zeros(rg), {}
    for c in range(k):
        ns = int(sps[c])
        if ns not in cache:
            M = inv64(ns * A + np.eye(rf))
            MsT = M @ S.T
            cache[ns] = (M, np.block([[M, -MsT], [-MsT.T, iGG + S @ MsT]]))
        h = cache[ns][0] @ (fg[:rf, c] - S.T @ fg[rf:, c])
        Hs[:rf, c], Hs[rf:, c] = h, S @ h
        Um[:rf] += ns * h
        Um[rf:] -= ns * Hs[rf:, c]
        gsum += fg[rf:, c]
        Ehh += ns * cache[ns][1]
    Um[rf:] += iGG @ gsum
    src = cls.copy()
    if defect == EM_DEFECTS[0]:
        src[cls == 256] = 0
    Eh = np.concatenate([Hs[:rf][:, src], iGG @ FGX[rf:] - Hs[rf:][:, src]], 0)
    Ehh += Eh @ Eh.T
    xh = Xc @ Eh.T
    FG = xh @ inv64(Ehh)
    Sg = (sigObs - FG @ xh.T) / n
    Um /= n
    cov = Ehh / n - np.outer(Um, Um)
    Fn = FG[:, :rf] @ chol_upper64(cov[:rf, :rf]).T
    Gn = FG[:, rf:] @ chol_upper64(cov[rf:, rf:]).T if rg else np.zeros((dim, 0))
    return Xc, Fn, Gn, Sg, Delta + FG @ Um


def em_oracle(X, sps, F, G, Sigma, Delta):
    from oracle import oracle as orc
    return orc.plda_em_iteration(X, sps, F, G, Sigma, Delta)


def em_errors_of(ref, got):
    """ref: em_reference's tuple; got: (X, F, G, Sigma, Delta) -> {kind: errors} (X is judged by its bits, not here)"""
    _, F, G, Sg, Dl = ref
    s = 1 / np.sqrt(np.diag(Sg))
    out = {"F column": col_err(got[1], F), "Delta": np.array([sr.forward_error(got[4], Dl)]),
           "Sigma row": row_err(ld(got[3]) * s[:, None] * s[None, :], Sg * s[:, None] * s[None, :])}
    if G.shape[1]:
        out["G column"] = col_err(got[2], G)
    return out


_EM_MEMO = {}


def em_bars(state):
    """(80-bit reference, err_double, err_oracle) of one iteration from `state` = (X, sps, F, G, Sigma, Delta), memoised on its bits"""
    key = tuple(np.ascontiguousarray(a).tobytes() for a in state)
    if key not in _EM_MEMO:
        ref = em_reference(*state)
        _EM_MEMO[key] = (ref, em_errors_of(ref, em_restate(*state)), em_errors_of(ref, em_oracle(*state)))
    return _EM_MEMO[key]


def em_judge(state, got):
    ref, dbl, _ = em_bars(state)
    return {k: v / bar(dbl[k]) for k, v in em_errors_of(ref, got).items()}


def em_centred(state):
    """the bits the centred X must have: one IEEE subtraction"""
    return state[0] - state[5][:, None]


# ================================================================ tv_orthonormalize_t
ORTHO_SHAPES = ((1, 1), (2, 3), (5, 7), (33, 520), (24, 1000), (3, 131100))
ORTHO_RATIOS = {"row at 2e-4": 2e-4, "row at 5e-5": 5e-5}
ORTHO_DEFECT = "the projection onto row j - 1 skipped in the step route"


def ortho_cases():
    out = []
    for R, SV in ORTHO_SHAPES:
        out.append((R, SV, "plain"))
        out += [(R, SV, v) for v in ORTHO_RATIOS]
        out += [(R, SV, "zero row %d" % z) for z in sorted({0, R // 2, R - 1})]
    return tuple(out)


ORTHO_CASES = ortho_cases()


def gram_schmidt(T, dtype, defect=None):
    """classical Gram-Schmidt over the rows (every coefficient against the ORIGINAL row, as AccumulateTVStat.cpp:1548-1596 and the
    step kernels do); a row of norm zero stays zero -> (Q, diagonal of the factor)"""
    T = np.asarray(T, dtype)
    R = T.shape[0]
    Q = np.zeros_like(T)
    diag = np.zeros(R, dtype)
    for j in range(R):
        upto = j - 1 if (defect == ORTHO_DEFECT and j > 0) else j
        v = T[j] - (Q[:upto] @ T[j]) @ Q[:upto] if upto > 0 else T[j].copy()
        diag[j] = np.sqrt(np.sum(v * v))
        if diag[j] != 0:
            Q[j] = v / diag[j]
    return Q, diag


@functools.lru_cache(maxsize=None)
def ortho_inputs(key):
    R, SV, variant = key
    T = np.random.default_rng(100 * R + SV).normal(size=(R, SV)) * 0.05 + 0.01
    if variant in ORTHO_RATIOS:                                  # the last row scaled so that its pivot is `ratio` of the largest
        d = gram_schmidt(T, LD)[1]
        if R > 1:                                                # (one row: its pivot is the largest, the ratio stays 1)
            T[R - 1] *= float(ORTHO_RATIOS[variant] * d[:R - 1].max() / d[R - 1])
    elif variant.startswith("zero row"):
        T[int(variant.split()[-1])] = 0.0
    T = np.ascontiguousarray(T)
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def ortho_reference(key):
    """-> (Q in 80-bit, dmin / dmax of the 80-bit factor: 0 with a zero row)"""
    Q, d = gram_schmidt(ortho_inputs(key), LD)
    return Q, float(d.min() / d.max()) if d.max() > 0 else 0.0


def ortho_route(key):
    """the route the library must take, from the 80-bit factor: no factor (a zero row) or dmin <= 1e-4 dmax -> the step kernels"""
    return "gram" if ortho_reference(key)[1] > ROUTE_THRESHOLD else "step"


def ortho_restate(key, defect=None):
    T = ortho_inputs(key)
    try:
        L = np.linalg.cholesky(T @ T.T)
        d = np.diag(L)
        if d.min() > ROUTE_THRESHOLD * d.max():
            return tri_inv64(L) @ T
    except np.linalg.LinAlgError:
        pass
    return gram_schmidt(T, np.float64, defect)[0]


def ortho_oracle(key):
    from oracle import oracle as orc
    return orc.tv_orthonormalize_t(ortho_inputs(key))


def ortho_errors(key, got):
    T, Qh = ld(ortho_inputs(key)), ld(got)
    Q = ortho_reference(key)[0]
    tn = nrm(T, 1)
    live = tn > 0
    L = mm(T, Qh.T)
    out = {"residual row": f64(safe_div(nrm(T - mm(np.tril(L), Qh), 1), tn)), "upper row": f64(safe_div(nrm(np.triu(L, 1), 1), tn)),
           "forward row": f64(nrm(Qh - Q, 1)), "!zero row stays zero": np.where(np.any(np.asarray(got)[~live] != 0.0, axis=1), np.inf, 0.0)}
    Ql = Qh[live]
    out["orthonormality row"] = f64(nrm(mm(Ql, Ql.T) - np.eye(len(Ql), dtype=LD), 1)) if len(Ql) else np.zeros(0)
    return out


# ================================================================ the table of entry points with cached inputs
class Entry:
    def __init__(self, cases, restate, oracle, errors, full=None):
        """full: key -> the key of the full-rank decomposition a (matrix, rank) case is the head of"""
        self.cases, self.restate, self.oracle, self.errors, self.full = tuple(cases), restate, oracle, errors, full


ENTRIES = {
    "dev_mahalanobis": Entry(INV_DEV_SETS, mahalanobis_restate, mahalanobis_oracle, mahalanobis_errors),
    "dev_wccn_chol": Entry(INV_DEV_SETS, wccn_restate, wccn_oracle, wccn_errors),
    "twocov_model": Entry(TWOCOV_CASES, twocov_restate, twocov_oracle, twocov_errors),
    "plda_precompute": Entry(PRECOMPUTE_CASES, precompute_restate, precompute_oracle, precompute_errors),
    "sym_eigen": Entry(EIGEN_CASES, eigen_restate, eigen_oracle, eigen_errors, lambda key: (key[0], eigen_matrix(key[0]).shape[0])),
    "dev_efr_matrix": Entry(EFR_CASES, efr_restate, efr_oracle, efr_errors),
    "dev_lda": Entry(LDA_CASES, lda_restate, lda_oracle, lda_errors, lambda key: (key[0], lda_inputs(key[0])[0].shape[0])),
    "tv_orthonormalize_t": Entry(ORTHO_CASES, ortho_restate, ortho_oracle, ortho_errors),
}


def case_name(key):
    return key if isinstance(key, str) else " ".join(case_name(k) if isinstance(k, tuple) else ("%g" % k if isinstance(k, float) else str(k)) for k in key)


@functools.lru_cache(maxsize=None)
def err_double(entry, key):
    e = ENTRIES[entry]
    return e.errors(key, e.restate(key))


@functools.lru_cache(maxsize=None)
def err_oracle(entry, key):
    e = ENTRIES[entry]
    return e.errors(key, e.oracle(key))


SCALAR_KINDS = ("value",)


def unit_err_double(kind, d):
    """err_double of every unit of a kind.  An eigenvalue is one number, and the float64 error of one number can vanish by accident
    (the oracle's LDA value 0 of the order-64 matrix at cond 1e6 read 2.6 bars of the restatement's error on that one value, with
    every other value inside): the restatement's error on the unit is the root mean square over the vector of ALL the values of
    the matrix, at any rank"""
    d = np.asarray(d, np.float64)
    return np.sqrt(np.mean(d * d)) if kind in SCALAR_KINDS and d.size else d


def unit_errors(entry, key):
    """-> ({kind: err_double per unit}, {kind: err_oracle per unit}); an eigenvalue kind holds the errors of ALL the values of the matrix"""
    e = ENTRIES[entry]
    d = dict(err_double(entry, key))
    if e.full:
        d.update({k: v for k, v in err_double(entry, e.full(key)).items() if k in SCALAR_KINDS})
    return d, err_oracle(entry, key)


def judge(entry, key, got):
    """-> {unit kind: |error| / bar per unit}; the bar of a measured kind is 16 max(err_double, 64 u) of the same unit"""
    d = unit_errors(entry, key)[0]
    return {k: (v if k.startswith("!") else v / bar(unit_err_double(k, d[k]))) for k, v in ENTRIES[entry].errors(key, got).items()}


def worst_units(ratios, dbl, orc):
    """per unit kind the unit with the largest ratio -> {kind: dict(ratio, unit, err_double, err_oracle)}: what the GPU file records.
    dbl / orc: {kind: errors of the restatement / of the oracle}, as err_double(entry, key) / err_oracle(entry, key) give them"""
    out = {}
    for kind, r in ratios.items():
        if not r.size:
            continue
        i = int(np.argmax(r))
        rec = {"ratio": float("%.4g" % r[i]), "unit": i}
        if not kind.startswith("!"):
            rec["err_double"] = float("%.4g" % np.broadcast_to(unit_err_double(kind, dbl[kind]), r.shape)[i])
            rec["err_oracle"] = float("%.4g" % orc[kind][i])
        out[kind] = rec
    return out
