"""An 80-bit restatement of the chain that turns statistics into i-vectors and T-matrix accumulators -- gmmiv_tv_subtract_m(_to),
gmmiv_tv_tett, tv_estep behind gmmiv_tv_estimate_w / _a_and_c, gmmiv_tv_update_t, gmmiv_tv_min_divergence -- and the bars each link
is held to, per element, per utterance and per Gaussian, never against the largest entry of an array.  Plain numpy on
np.longdouble; the factorisation, the substitutions and the inverse are spd_ref's.  No GPU, no LAPACK.

Every link takes as input exactly the doubles handed to the library, so a link is judged on its own work:
    F0      = F - m N                                   (subtract_m)
    TETt_c  = T_c diag(iv_c) T_c^T                      (tett; rounded to double, packed: the `te` of the E-step)
    L_u     = I + sum_c N_uc TETt_c,  aux_u = T Sigma^-1 F0_u,  w_u = L_u^-1 aux_u,  E_u = L_u^-1 + w_u w_u^T
    A_c     = sum_u N_uc E_u,  Cmx = sum_u w_u F0_u^T,  Rm = sum_u E_u,  r = meanW = sum_u w_u
    T_c     = A_c^-1 Cmx_c                              (update_t, on the doubles nearest to A and Cmx)
    Rn = Rm / n - (r / n)(r / n)^T,  Ch = upper factor of Rn,  mean += T^T meanW,  T <- Ch T      (min_divergence)

Bars (u = 2^-53; every error is evaluated in long double):
    subtract_m      per element          2 u (|F| + |m N|)                       (with or without fma contraction)
    tett            per packed element   (D + 8) u sum_k |T_ik iv_k T_jk|        (the dot-product bound of dgemm_ref)
    W               per utterance        ||w^ - w|| / ||w|| <= spd_ref.bar(err_oracle_u) = 16 max(err_oracle_u, 64 u); err_oracle_u is
                                         the double oracle's error on the SAME utterance; an utterance without frames returns w = 0
    E_u             (not returned)       b^E_u = spd_ref.bar(the oracle's inverse error on that utterance: a one-utterance call, Rm = E_u)
    A_c             per Gaussian, Frobenius over the packed row:  sum_u N_uc b^E_u ||E_u|| + (U + 8) u || sum_u N_uc |E_u| ||
    Cmx block c     per Gaussian (R x D):                          sum_u b^W_u ||w_u|| ||F0_uc|| + (U + 8) u || sum_u |w_u| |F0_uc|^T ||
    Rm, r / meanW   one unit each, likewise
    update_t        per Gaussian and 16-column block: spd_ref.accept against the oracle's error on the same A_c, Cmx_c
    min_divergence  Rn per element 4 u (|Rm_ij| / n + |r_i r_j| / n^2); r / n per element 1 u;
                    mean per element (R + 8) u (|mean_j| + sum_k |meanW_k T_kj|);
                    Ch T per column j: ||dT'_j|| <= 16 max(err_oracle_j, 64 u) || |Ch| |T_j| ||
A sum's bar is the sum of its terms' bars plus the summation bound: cancellation cannot inflate it, and a Gaussian of 10^-9 of the
others' occupancy is judged on its own scale.  Nothing here is fitted to what the code under test returns.

The statistics (`statistics`) have the dynamic range that conftest-style problems lack: log-normal occupancies (sigma 3), 30 % exact
zeros, a per-utterance scale over 6 decades, one Gaussian at 1e-9 of the others, one utterance without frames, F_uc = N_uc xbar_uc.
"""
import functools

import numpy as np

import spd_ref as sr

LD = sr.LD
U_DOUBLE = sr.U_DOUBLE
HAVE_LONGDOUBLE = sr.HAVE_LONGDOUBLE
SKIP_MESSAGE = sr.SKIP_MESSAGE
COL_BLOCK = sr.COL_BLOCK
FAINT_SCALE = 1e-9
EMPTY_UTT = 2                       # the utterance without frames (inside every prefix a case uses)
CARRIER_ROWS = (0, 1, 3, 4)         # Gaussian c has frames in utterance CARRIER_ROWS[c % 4]: no Gaussian is empty in any prefix >= 5

# C, D, R, the utterance counts that run on it (prefixes of one problem of max(U) utterances)[, the seed of the inputs when not 0:
# the float64 restatement through np.linalg.inv has to stay within 0.25 of every bar (tests/test_cpu_tv_ref.py), a condition on the
# inputs -- with seed 0 one utterance of the R = 90 case has the LAPACK inverse ten times further off than Gauss-Jordan (0.63 of its bar)]
ESTEP_CASES = (
    (5, 3, 2, (7,)),                       # the smallest
    (16, 12, 40, (75,)),                   # tv_batch 16: batches of 16, super-batches 64 + 11 (tv_acc_mb 0) against one of 80
    (6, 4, 70, (63, 64, 65, 71)),          # k_colsum_narrow_part from 64 utterances on: slab and wave tails, R no multiple of 64
    (8, 12, 90, (128,), 1),                # P = 4095: the one-stage batch sum at 128 utterances
    (8, 12, 92, (127, 128, 129)),          # P = 4278: two-stage from 128 utterances on; a last slab shorter than a 4-row unroll
    (8, 12, 35, (20,)),                    # odd R: unpack / pack / k_batched_matvec, the GEMM-built factorisation
    (8, 12, 91, (129,)),                   # odd R with both two-stage sums
    (36, 60, 92, (129,)),                  # C D = 2160: split-K aux with a short last slab
    (4, 12, 160, (128,)),                  # aux with N = 160 = 2 x 80 columns on a full row tile -- but C D = 48 is one K layer, and only
                                           # the split-K product has the 128 x 80 tile ("gemm_nt80"): this shape runs 128 x 128 + strip
    (36, 60, 80, (128,)),                  # C D = 2160 (4 K layers), N = 80: the smallest shape that does run the 128 x 80 tile
)


def case_name(case):
    return "%dx%dx%dx%d" % (case[0], case[1], case[2], max(case[3]))


def faint_gaussian(C):
    return C // 2


# ---------------------------------------------------------------- inputs
def statistics(C, D, R, U, seed=0):
    """-> dict(N [U, C], F [U, C D], means [C D], invvar [C D], Tm [R, C D]) in double"""
    rng = np.random.default_rng(100003 * C + 1009 * D + 31 * R + U + seed)
    occ = np.exp(rng.normal(0.0, 3.0, (U, C)))
    occ[rng.random((U, C)) < 0.3] = 0.0
    for c in range(C):
        if occ[CARRIER_ROWS[c % 4], c] == 0.0:
            occ[CARRIER_ROWS[c % 4], c] = np.exp(rng.normal(0.0, 3.0))
    decades = rng.uniform(-4.0, 2.0, U)
    decades[0], decades[1] = -4.0, 2.0                        # every prefix spans the 6 decades
    gscale = np.ones(C)
    gscale[faint_gaussian(C)] = FAINT_SCALE
    N = occ * (10.0 ** decades)[:, None] * gscale[None, :]
    N[EMPTY_UTT] = 0.0
    means = rng.normal(0.0, 2.0, (C, D))
    invvar = 1.0 / np.exp(rng.normal(0.0, 0.5, (C, D)))
    xbar = means[None] + rng.normal(0.0, 1.0, (U, C, D)) / np.sqrt(invvar)[None] / np.sqrt(1.0 + N[:, :, None])
    F = (N[:, :, None] * xbar).reshape(U, C * D)
    Tm = rng.normal(0.0, 0.05, (R, C * D))
    return dict(N=np.ascontiguousarray(N), F=np.ascontiguousarray(F), means=means.ravel().copy(), invvar=invvar.ravel().copy(), Tm=Tm)


# ---------------------------------------------------------------- the links, one by one
def subtract_m(N, F, means, C, D):
    """-> (F - m N in long double, the bar per element)"""
    mn = np.repeat(np.asarray(N, LD), D, axis=1) * np.asarray(means, LD)[None, :]
    Fl = np.asarray(F, LD)
    return Fl - mn, 2 * U_DOUBLE * (np.abs(Fl) + np.abs(mn))


def tett(Tm, invvar, C, D):
    """-> (packed TETt [C, P] in long double, the bar per packed element)"""
    R = Tm.shape[0]
    T = np.asarray(Tm, LD).reshape(R, C, D)
    iv = np.asarray(invvar, LD).reshape(C, D)
    il = np.tril_indices(R)
    ref, bar = np.empty((C, len(il[0])), LD), np.empty((C, len(il[0])), LD)
    for c in range(C):
        ref[c] = ((T[:, c, :] * iv[c]) @ T[:, c, :].T)[il]
        bar[c] = (D + 8) * U_DOUBLE * ((np.abs(T[:, c, :]) * iv[c]) @ np.abs(T[:, c, :]).T)[il]
    return ref, bar


def norm2(a, axis=None):
    a = np.asarray(a, LD)
    return np.sqrt(np.sum(a * a, axis=axis))


def ratio(err, bar):
    """|err| / bar, elementwise; 0 / 0 = 0, x / 0 = inf, nan -> inf"""
    err, bar = np.abs(np.asarray(err, LD)), np.asarray(bar, LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    return np.where(np.isnan(r), np.inf, r).astype(np.float64)


class Problem:
    """One (C, D, R) with U utterances: the inputs, the 80-bit result of every link, the oracle's error per utterance."""

    def __init__(self, C, D, R, U, seed=0, with_oracle=True):
        self.C, self.D, self.R, self.U, self.P = C, D, R, U, R * (R + 1) // 2
        s = statistics(C, D, R, U, seed)
        self.N, self.F, self.means, self.invvar, self.Tm = s["N"], s["F"], s["means"], s["invvar"], s["Tm"]
        self.faint = faint_gaussian(C)
        self.F0_ref, self.F0_bar = subtract_m(self.N, self.F, self.means, C, D)
        self.F0 = np.ascontiguousarray(self.F0_ref.astype(np.float64))              # what the E-step is handed
        self.te_ref, self.te_bar = tett(self.Tm, self.invvar, C, D)
        self.te = np.ascontiguousarray(self.te_ref.astype(np.float64))              # packed [C, P], what the E-step is handed
        self.te_full = sr.unpack(self.te, R)                                        # the same doubles, full: what the oracle is handed
        te_ld = self.te_full.astype(LD).reshape(C, R * R)
        aux = self.F0.astype(LD) @ (self.Tm.astype(LD) * self.invvar.astype(LD)[None, :]).T
        il = np.tril_indices(R)
        self.w = np.zeros((U, R), LD)
        self.Ep = np.zeros((U, self.P), LD)
        self.cond = np.zeros(U)
        eye = np.eye(R, dtype=LD)
        for u in range(U):
            L = eye + (self.N[u].astype(LD) @ te_ld).reshape(R, R)
            self.cond[u] = np.linalg.cond(L.astype(np.float64))
            Lf = sr.cholesky(L)
            self.w[u] = sr.solve(Lf, aux[u])
            self.Ep[u] = (sr.inverse(Lf) + np.outer(self.w[u], self.w[u]))[il]
        self.wn = norm2(self.w, 1)
        self.En = norm2(self.Ep, 1)
        assert self.wn[EMPTY_UTT] == 0 and all(self.wn[u] > 0 for u in range(U) if u != EMPTY_UTT)
        if with_oracle:
            self._oracle()

    def _oracle(self):
        """the double oracle, one utterance at a time (its Rm is then E_u): its i-vector and inverse errors -> b^W_u, b^E_u"""
        from oracle import oracle as orc
        U = self.U
        self.oracle_W = np.zeros((U, self.R))
        self.oracle_Ep = np.zeros((U, self.P))
        for u in range(U):
            o = orc.tv_estimate_a_and_c(self.N[u:u + 1], self.F0[u:u + 1], self.Tm, self.invvar, self.te_full)
            self.oracle_W[u] = o["W"][0]
            self.oracle_Ep[u] = sr.pack(o["Rm"])
        self.err_oracle_w = self.w_errors(self.oracle_W)
        self.err_oracle_e = np.array([sr.inverse_error(self.oracle_Ep[u], self.Ep[u]) for u in range(U)])
        self.bW = np.array([sr.bar(e) for e in self.err_oracle_w], LD)
        self.bE = np.array([sr.bar(e) for e in self.err_oracle_e], LD)

    def cond_stats(self, U=None):
        c = self.cond[:U or self.U]
        return {"median": float("%.3g" % np.median(c)), "max": float("%.3g" % c.max())}

    # ---- W
    def w_errors(self, W, lo=0):
        """forward error per utterance of W [n, R] = utterances lo .. lo + n; 0 for an exact zero where the reference is zero, inf otherwise"""
        out = np.zeros(len(W))
        for k in range(len(W)):
            u = lo + k
            if self.wn[u] == 0:
                out[k] = 0.0 if not np.any(W[k]) else np.inf
            else:
                out[k] = sr.forward_error(W[k], self.w[u])
        return out

    def w_ratios(self, W, lo=0):
        """per utterance: error / bar; the utterance without frames: 0 iff w = 0 exactly"""
        e = self.w_errors(W, lo)
        return ratio(e, self.bW[lo:lo + len(W)])

    # ---- the sums over utterances [0, U)
    @functools.lru_cache(maxsize=None)
    def sums(self, U):
        C, D, R = self.C, self.D, self.R
        Nl, w, Ep, F0 = self.N[:U].astype(LD), self.w[:U], self.Ep[:U], self.F0[:U].astype(LD)
        k = (U + 8) * U_DOUBLE
        A = Nl.T @ Ep
        A_bar = Nl.T @ (self.bE[:U] * self.En[:U]) + k * norm2(Nl.T @ np.abs(Ep), 1)
        Cmx = w.T @ F0
        Fn = norm2(F0.reshape(U, C, D), 2)                                            # ||F0_uc||  [U, C]
        Cabs = (np.abs(w).T @ np.abs(F0)).reshape(R, C, D)
        Cmx_bar = (self.bW[:U] * self.wn[:U]) @ Fn + k * np.sqrt(np.sum(Cabs * Cabs, axis=(0, 2)))
        Rm = Ep.sum(0)
        Rm_bar = np.sum(self.bE[:U] * self.En[:U]) + k * norm2(np.abs(Ep).sum(0))
        r = w.sum(0)
        r_bar = np.sum(self.bW[:U] * self.wn[:U]) + k * norm2(np.abs(w).sum(0))
        return dict(A=A, A_bar=A_bar, Cmx=Cmx, Cmx_bar=Cmx_bar, Rm=Rm, Rm_bar=Rm_bar, r=r, r_bar=r_bar)

    def judge_acc(self, acc, U):
        """acc: A [C, P], Cmx [R, C D], Rm [R, R], r [R], meanW [R] (sums, as the library returns them) over utterances [0, U)
        -> {unit kind: ratios}: A and Cmx per Gaussian, Rm (lower and upper triangle), r, meanW one unit each"""
        s = self.sums(U)
        C, D, R = self.C, self.D, self.R
        out = {"A": ratio(norm2(np.asarray(acc["A"], LD) - s["A"], 1), s["A_bar"])}
        dC = (np.asarray(acc["Cmx"], LD) - s["Cmx"]).reshape(R, C, D)
        out["Cmx"] = ratio(np.sqrt(np.sum(dC * dC, axis=(0, 2))), s["Cmx_bar"])
        Rg = np.asarray(acc["Rm"], LD)
        out["Rm"] = ratio(np.array([norm2(sr.pack(Rg) - s["Rm"]), norm2(sr.pack(Rg.T) - s["Rm"])]), s["Rm_bar"])
        out["r"] = ratio(np.array([norm2(np.asarray(acc["r"], LD) - s["r"])]), s["r_bar"])
        out["meanW"] = ratio(np.array([norm2(np.asarray(acc["meanW"], LD) - s["r"])]), s["r_bar"])
        return out

    # ---- the M-step on the doubles nearest to the accumulators of utterances [0, U)
    @functools.lru_cache(maxsize=None)
    def mstep(self, U):
        from oracle import oracle as orc
        C, D, R = self.C, self.D, self.R
        s = self.sums(U)
        A = np.ascontiguousarray(s["A"].astype(np.float64))
        Cmx = np.ascontiguousarray(s["Cmx"].astype(np.float64))
        A_full = sr.unpack(A, R)
        Cb = Cmx.astype(LD).reshape(R, C, D)
        T = np.empty((R, C, D), LD)
        for c in range(C):
            T[:, c, :] = sr.solve(sr.cholesky(A_full[c]), Cb[:, c, :])
        To = orc.tv_update_t(A_full.reshape(C, R * R), Cmx, C, D)
        m = dict(A=A, Cmx=Cmx, T=T)
        m["err_oracle"] = self.mstep_errors(To, m)
        return m

    def mstep_blocks(self):
        return [(c, j0, min(j0 + COL_BLOCK, self.D)) for c in range(self.C) for j0 in range(0, self.D, COL_BLOCK)]

    def mstep_errors(self, Tg, m):
        Tg = np.asarray(Tg).reshape(self.R, self.C, self.D)
        return np.array([sr.forward_error(Tg[:, c, j0:j1], m["T"][:, c, j0:j1]) for c, j0, j1 in self.mstep_blocks()])

    def mstep_ratios(self, Tg, m):
        e = self.mstep_errors(Tg, m)
        return ratio(e, np.array([sr.bar(x) for x in m["err_oracle"]], LD))


@functools.lru_cache(maxsize=None)
def problem(C, D, R, U, seed=0):
    return Problem(C, D, R, U, seed)


def case_problem(case):
    return problem(case[0], case[1], case[2], max(case[3]), case[4] if len(case) > 4 else 0)


# ---------------------------------------------------------------- a float64 restatement through another algorithm, and defects of it
def restate(p, U, defect=None):
    """The chain from (N, F0, Tm, invvar, te) in float64 numpy: np.linalg.inv (LU, LAPACK) instead of Gauss-Jordan or Cholesky,
    BLAS sums in BLAS order.  defect: None or a name of DEFECTS (value-only: no index, bound or shape changes)."""
    C, D, R = p.C, p.D, p.R
    N, F0 = p.N[:U], p.F0[:U]
    te = p.te_full.copy()
    f = p.faint
    if defect == "tett k-term":                                   # TETt of the faint Gaussian without its last k term
        Tf = p.Tm.reshape(R, C, D)[:, f, :]
        te[f] -= np.outer(Tf[:, -1] * p.invvar.reshape(C, D)[f, -1], Tf[:, -1])
    L = np.eye(R)[None] + np.einsum("uc,cij->uij", N, te)
    aux = F0 @ (p.Tm * p.invvar[None, :]).T
    Li = np.linalg.inv(L)
    w = np.einsum("uij,uj->ui", Li, aux)
    if defect == "quiet w":                                       # 1e-6 relative on the i-vector of the quietest utterance
        w[quiet_utterance(p, U)] *= 1.0 + 1e-6
    Ep = sr.pack(Li + w[:, :, None] * w[:, None, :])
    NA = N.copy()
    if defect == "A neighbour":                                   # A += N^T E reads the faint Gaussian's weights one utterance off
        NA[:, f] = np.roll(N[:, f], 1)
    A = NA.T @ Ep
    Cmx = w.T @ F0
    if defect == "Cmx utterance":                                 # the faint Gaussian's block of Cmx misses one utterance
        u = dropped_utterance(p, U)
        Cmx.reshape(R, C, D)[:, f, :] -= np.outer(w[u], F0[u].reshape(C, D)[f])
    return dict(te=sr.pack(te), W=w, A=A, Cmx=Cmx, Rm=sr.unpack(Ep.sum(0), R), r=w.sum(0), meanW=w.sum(0))


DEFECTS = ("A neighbour", "quiet w", "tett k-term", "Cmx utterance")


def quiet_utterance(p, U):
    wn = p.wn[:U].astype(np.float64)
    wn[EMPTY_UTT] = np.inf
    return int(np.argmin(wn))


def dropped_utterance(p, U):
    """an utterance that carries the faint Gaussian, not the one that carries most of it"""
    n = p.N[:U, p.faint]
    order = [int(u) for u in np.argsort(n) if n[u] > 0]
    return order[len(order) // 2]


def judge(p, got, U):
    """-> {unit kind: worst ratio} of a restatement's W and accumulators"""
    out = {"W": float(p.w_ratios(got["W"]).max())}
    for k, v in p.judge_acc(got, U).items():
        out[k] = float(v.max())
    return out


def relerr(a, b):
    """the criterion the suite held this chain to before: the largest error over the largest entry of the whole array"""
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(np.max(np.abs(b)), 1e-300))


def old_criteria(p, got, U):
    """-> {array: (relerr, threshold)} as tests/test_gpu_tv.py reads them: 1e-9 on W, A, Cmx, Rm, r and 1e-12 on TETt"""
    s = p.sums(U)
    out = {"te": (relerr(got["te"], p.te_ref), 1e-12), "W": (relerr(got["W"], p.w[:U]), 1e-9)}
    for k in ("A", "Cmx", "r"):
        out[k] = (relerr(got[k], s[k]), 1e-9)
    out["Rm"] = (relerr(sr.pack(got["Rm"]), s["Rm"]), 1e-9)
    return out


# ---------------------------------------------------------------- minimum divergence
MD_RANKS = (24, 66, 25)
MD_C, MD_D, MD_SESSIONS = 6, 10, 50


@functools.lru_cache(maxsize=None)
def md_problem(R):
    """-> dict: the inputs of one minDivergence call (double), its 80-bit results, the bars, the oracle's errors"""
    from oracle import oracle as orc
    rng = np.random.default_rng(11 + R)
    n, SV = MD_SESSIONS, MD_C * MD_D
    W = rng.normal(size=(n, R)) * np.exp(rng.normal(0.0, 1.0, R))[None, :] + 0.3
    Rm = W.T @ W + 0.1 * n * np.eye(R)
    Rm = (Rm + Rm.T) / 2
    r = W.sum(0)
    meanW = r / n
    means = rng.normal(size=SV)
    T = rng.normal(size=(R, SV)) * np.exp(rng.normal(0.0, 1.0, (R, 1)))
    u = U_DOUBLE
    nl = LD(n)
    rn = r.astype(LD) / nl
    Rn = Rm.astype(LD) / nl - np.outer(rn, rn)
    Ch = sr.cholesky(Rn).T                                       # upper factor: Rn = Ch^T Ch
    Tl = T.astype(LD)
    mean = means.astype(LD) + meanW.astype(LD) @ Tl
    Tn = Ch @ Tl
    m = dict(R=R, Rm=Rm, r=r, meanW=meanW, means=means, T=T, n=n,
             rn=rn, rn_bar=u * np.abs(rn), Rn=Rn, Rn_bar=4 * u * (np.abs(Rm.astype(LD)) / nl + np.abs(np.outer(r.astype(LD), r.astype(LD))) / (nl * nl)),
             mean=mean, mean_bar=(R + 8) * u * (np.abs(means.astype(LD)) + np.abs(meanW.astype(LD)) @ np.abs(Tl)),
             Tn=Tn, Tn_scale=norm2(np.abs(Ch) @ np.abs(Tl), 0))
    _, To = orc.tv_min_divergence(Rm.copy(), r.copy(), meanW, means.copy(), T.copy(), n, MD_C, MD_D)
    m["err_oracle"] = md_column_errors(m, To)
    return m


def md_column_errors(m, Tg):
    return (norm2(np.asarray(Tg, LD) - m["Tn"], 0) / m["Tn_scale"]).astype(np.float64)


def md_judge(m, Rg, rg, mg, Tg):
    """the four outputs of a minDivergence call -> {unit kind: ratios}"""
    return {"Rn": ratio(np.asarray(Rg, LD) - m["Rn"], m["Rn_bar"]), "r/n": ratio(np.asarray(rg, LD) - m["rn"], m["rn_bar"]),
            "mean": ratio(np.asarray(mg, LD) - m["mean"], m["mean_bar"]),
            "Ch T": ratio(md_column_errors(m, Tg), np.array([sr.bar(e) for e in m["err_oracle"]], LD))}
