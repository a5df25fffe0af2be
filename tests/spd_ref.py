"""An 80-bit reference for the batched Cholesky family, and a harness that makes every system of a batch bit-known through
the public i-vector entry points.  Plain numpy on np.longdouble (x87 extended, eps = 2^-63); np.linalg has no long double, so
the factorisation, the substitutions and the inverse are written out here.  No GPU, no LAPACK.

The harness ("selector statistics"): C = U Gaussians of dimension D = 1, N = diag(n_u) with every n_u a power of two,
TETt_c = (A_c - I) / n_c, F = I_U, invvar = 1, Tm random R x U.  Then, with no rounding beyond the one in A_c - I and the one in
the final + I (every other product is by 0, 1 or a power of two):
    L_u   = n_u TETt_u + I                 the matrix both the device and the oracle factor, formed here in double as well
    aux_u = Tm[:, u]
    tv_estimate_w        -> w_u = L_u^-1 Tm[:, u]
    tv_estimate_a_and_c  -> A_u / n_u = E_u = L_u^-1 + w_u w_u^T (packed),  Rm = sum_u E_u,  Cmx[:, u] = w_u
so each system of the batch is checked on its own.  For tv_update_t: A_packed[c] = packed(A_c) (no I is added there), Cmx random
R x (C D), reference T_c = A_c^-1 Cmx_c.

Metrics (all evaluated in long double, per system, never per batch):
    forward   ||x^ - x||_2 / ||x||_2
    inverse   ||E^ - E||_F / ||E||_F
    backward  eta = ||b - A x^|| / (||A||_2 ||x^|| + ||b||)
Acceptance (one function, `accept`): err_gpu <= 16 max(err_oracle, 64 u), u = 2^-53, err_oracle = the double-precision oracle's
error on the SAME system against the 80-bit reference (measured, not assumed).  16 covers the different summation order of the
MFMA k-chunks and the scatter of a single random system (the oracle's own error varies about 3x between systems of equal
conditioning); the floor keeps the cond = 10 cases from asking for better than a few ulps of a 500-term dot product.
"""
import numpy as np

LD = np.longdouble
U_DOUBLE = 2.0 ** -53
HAVE_LONGDOUBLE = bool(np.finfo(LD).eps < 2e-19)
SKIP_MESSAGE = "np.longdouble is not an 80-bit (or wider) type on this platform (eps = %.3g): no reference wider than the code under test" % float(np.finfo(LD).eps)
COL_BLOCK = 16          # right-hand sides per column tile of k_chol_solve_multi


# ---------------------------------------------------------------- 80-bit linear algebra
def cholesky(A):
    """Lower factor of A (column Cholesky, one column at a time from the finished columns to its left), long double."""
    A = np.asarray(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        d = np.sqrt(v[0])
        L[j, j] = d
        L[j + 1:, j] = v[1:] / d
    return L


def forward_subst(L, B):
    """Y with L Y = B; B is n x m (a block of right-hand sides)."""
    Y = np.array(B, LD)
    for i in range(L.shape[0]):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def backward_subst(L, Y):
    """X with L^T X = Y."""
    X = np.array(Y, LD)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def solve(L, B):
    B = np.asarray(B, LD)
    if B.ndim == 1:
        return backward_subst(L, forward_subst(L, B[:, None]))[:, 0]
    return backward_subst(L, forward_subst(L, B))


def inverse(L):
    """A^-1 = L^-T L^-1 through the factor: rows of L^-1 by forward substitution on the identity (row i has i + 1 entries), then
    row i of the product from the rows k >= i of L^-1, lower triangle computed and mirrored."""
    n = L.shape[0]
    Li = np.zeros((n, n), LD)
    for i in range(n):
        Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
        Li[i, i] = 1 / L[i, i]
    Ui = np.ascontiguousarray(Li.T)
    E = np.zeros((n, n), LD)
    for i in range(n):
        E[i, :i + 1] = Ui[i, i:] @ Li[i:, :i + 1]
        E[:i, i] = E[i, :i]
    return E


# ---------------------------------------------------------------- test matrices
def spd(n, cond, rng):
    """Dense Q diag(logspace(0, log10 cond)) Q^T, symmetrised: eigenvalues 1 .. cond, off-diagonals of the size of the diagonal."""
    Q = np.linalg.qr(rng.normal(size=(n, n)))[0]
    A = (Q * np.logspace(0.0, np.log10(cond), n)) @ Q.T
    return (A + A.T) / 2


def pack(M):
    il = np.tril_indices(M.shape[-1])
    return np.ascontiguousarray(M[..., il[0], il[1]])


def unpack(P, n):
    il = np.tril_indices(n)
    M = np.zeros(P.shape[:-1] + (n, n), P.dtype)
    M[..., il[0], il[1]] = P
    M[..., il[1], il[0]] = P
    return M


# ---------------------------------------------------------------- metrics and the bar
def forward_error(xh, x):
    d = np.asarray(xh, LD) - x
    return float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(x * x)))


inverse_error = forward_error      # Frobenius norm of a matrix == 2-norm of its entries


def backward_error(A, norm2_A, xh, b):
    """eta = ||b - A x^|| / (||A||_2 ||x^|| + ||b||); A, x^ in double, the residual in long double.  x^ / b may be column blocks
    (Frobenius norms then)."""
    xh = np.asarray(xh, LD)
    b = np.asarray(b, LD)
    r = b - np.asarray(A, LD) @ xh
    nrm = lambda v: np.sqrt(np.sum(v * v))
    return float(nrm(r) / (LD(norm2_A) * nrm(xh) + nrm(b)))


def bar(err_oracle):
    return 16.0 * max(err_oracle, 64.0 * U_DOUBLE)


def accept(err_gpu, err_oracle):
    """The acceptance function of tests/test_gpu_chol_family.py (and of the CPU test that shows it bites)."""
    return bool(np.isfinite(err_gpu) and err_gpu <= bar(err_oracle))


# ---------------------------------------------------------------- selector statistics: E-step entry points
CONDS = (1e1, 1e3, 1e6, 1e3)
OCCS = (1.0, 2.0, 4.0, 0.5)


class Batch:
    """U systems of order n behind selector statistics, their 80-bit results, and the oracle's errors on them."""

    def __init__(self, n, conds=CONDS, occs=OCCS, seed=0, with_inverse=True):
        from oracle import oracle as orc
        rng = np.random.default_rng(1000 * n + seed)
        U = len(conds)
        assert len(occs) == U and all(np.frexp(o)[0] == 0.5 for o in occs), "occupations must be powers of two"
        self.n, self.U, self.C, self.D, self.conds, self.occs = n, U, U, 1, tuple(conds), tuple(occs)
        eye = np.eye(n)
        self.N = np.diag(np.asarray(occs, np.float64))
        self.te_full = np.stack([(spd(n, c, rng) - eye) / o for c, o in zip(conds, occs)])
        self.te = pack(self.te_full)
        self.F = np.eye(U)
        self.invvar = np.ones(U)
        self.Tm = np.ascontiguousarray(rng.normal(size=(n, U)))
        self.Lmat = np.stack([o * t + eye for o, t in zip(occs, self.te_full)])      # double: what both sides factor
        self.norm2 = [float(np.linalg.norm(M, 2)) for M in self.Lmat]
        # 80-bit results
        self.w, self.E = [], []
        for u in range(U):
            Lf = cholesky(self.Lmat[u])
            w = solve(Lf, self.Tm[:, u])
            self.w.append(w)
            if with_inverse:
                self.E.append(inverse(Lf) + np.outer(w, w))
        self.Rm = sum(self.E) if with_inverse else None
        # the oracle through the same harness, and its errors
        # (its tv_estimate_w runs the loops of tv_estimate_a_and_c -- same W bit for bit, tests/test_cpu_spd_ref.py -- so one
        # Gauss-Jordan pass per system serves both entries when the inverse is wanted anyway)
        o = orc.tv_estimate_a_and_c(self.N, self.F, self.Tm, self.invvar, self.te_full) if with_inverse else None
        self.oracle_W = o["W"] if with_inverse else orc.tv_estimate_w(self.N, self.F, self.Tm, self.invvar, self.te_full)
        self.err_oracle = {"estimate_w/W": self.errors_w(self.oracle_W)}
        self.eta_oracle = {"estimate_w/W": self.etas_w(self.oracle_W)}
        if with_inverse:
            self.oracle_acc = dict(W=o["W"], A=pack(o["A"].reshape(U, n, n)), Rm=o["Rm"])
            for k, v in self.errors_acc(self.oracle_acc).items():
                self.err_oracle[k] = v
            self.eta_oracle["estimate_a_and_c/W"] = self.etas_w(o["W"])

    def errors_w(self, W):
        return [forward_error(W[u], self.w[u]) for u in range(self.U)]

    def etas_w(self, W):
        return [backward_error(self.Lmat[u], self.norm2[u], W[u], self.Tm[:, u]) for u in range(self.U)]

    def errors_acc(self, acc):
        """acc: W [U, n], A [U, packed] (the accumulator as returned: n_u E_u), Rm [n, n] -> per-system errors by entry."""
        il = np.tril_indices(self.n)
        eA = [inverse_error(acc["A"][u] / self.occs[u], self.E[u][il]) for u in range(self.U)]
        return {"estimate_a_and_c/W": self.errors_w(acc["W"]), "estimate_a_and_c/A": eA,
                "estimate_a_and_c/Rm": [inverse_error(acc["Rm"], self.Rm)]}


def run_batch(ctx, b, with_inverse=True):
    """The device's results for Batch b under the context's current options -> (per-entry per-system errors, etas, raw outputs)."""
    W = ctx.tv_estimate_w(b.N, b.F, b.Tm, b.invvar, b.te, b.C, b.D)
    err = {"estimate_w/W": b.errors_w(W)}
    eta = {"estimate_w/W": b.etas_w(W)}
    raw = {"W": W}
    if with_inverse:
        g = ctx.tv_estimate_a_and_c(b.N, b.F, b.Tm, b.invvar, b.te, b.C, b.D)
        err.update(b.errors_acc(g))
        eta["estimate_a_and_c/W"] = b.etas_w(g["W"])
        raw["acc"] = g
    return err, eta, raw


# ---------------------------------------------------------------- tv_update_t
MSTEP_D = (1, 3, 60, 64, 65)
MSTEP_CONDS = (1e1, 1e3, 1e6)


class MStep:
    """C = 3 systems A_c of order R with D_max right-hand sides each; a call with D <= D_max uses the first D columns of every
    Gaussian's block, so one 80-bit solve and one oracle call serve every D."""

    def __init__(self, R, conds=MSTEP_CONDS, Dmax=max(MSTEP_D), seed=0):
        from oracle import oracle as orc
        rng = np.random.default_rng(7000 * R + seed)
        self.R, self.C, self.Dmax, self.conds = R, len(conds), Dmax, tuple(conds)
        self.A = np.stack([spd(R, c, rng) for c in conds])
        self.A_packed = pack(self.A)
        self.norm2 = [float(np.linalg.norm(M, 2)) for M in self.A]
        self.B = rng.normal(size=(self.C, R, Dmax))
        self.T = [solve(cholesky(self.A[c]), self.B[c]) for c in range(self.C)]                   # 80-bit
        To = orc.tv_update_t(self.A.reshape(self.C, R * R), self.cmx(Dmax), self.C, Dmax)
        self.oracle_T = To.reshape(R, self.C, Dmax).transpose(1, 0, 2)

    def cmx(self, D):
        return np.ascontiguousarray(self.B[:, :, :D].transpose(1, 0, 2).reshape(self.R, self.C * D))

    def blocks(self, D):
        return [(c, j0, min(j0 + COL_BLOCK, D)) for c in range(self.C) for j0 in range(0, D, COL_BLOCK)]

    def errors(self, T, D):
        """T [R, C D] from the device (or the oracle's columns) -> forward error per Gaussian and per column block."""
        T = np.asarray(T).reshape(self.R, self.C, D)
        return [forward_error(T[:, c, j0:j1], self.T[c][:, j0:j1]) for c, j0, j1 in self.blocks(D)]

    def etas(self, T, D):
        T = np.asarray(T).reshape(self.R, self.C, D)
        return [backward_error(self.A[c], self.norm2[c], T[:, c, j0:j1], self.B[c][:, j0:j1]) for c, j0, j1 in self.blocks(D)]

    def oracle_errors(self, D):
        To = np.ascontiguousarray(self.oracle_T[:, :, :D].transpose(1, 0, 2)).reshape(self.R, self.C * D)
        return self.errors(To, D), self.etas(To, D)
