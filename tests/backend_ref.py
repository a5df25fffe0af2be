"""80-bit restatements of everything downstream of the i-vector -- the scoring rules (cosine, Mahalanobis, two-covariance, its
accumulating mix part, PLDA), iv_normalize, the development-set statistics (dev_means, dev_cov_mat, dev_scatter_mat), the JFA steps
and the approximate extractors -- and the bar each result is held to, per trial, per element or per utterance, never against the
largest entry of an array.  Plain numpy on np.longdouble; the Cholesky factor, the solve and the inverse are spd_ref's.

The reference of a quantity is the reference project's own formula in 80 bits, NOT the expansion the device evaluates:
    Mahalanobis     -1/2 (m - s)^T Q (m - s)
    two-covariance  (m + s)^T G (m + s) - m^T H m - s^T H s          mix part: C_in + (m + s)^T G (m + s)
    PLDA            1/2 [(s + m)^T K_{L+1} (s + m) - m^T K_L m - s^T K_1 s] + 1/2 (a_{L+1} - a_L - a_1),
                    K_n = (n FTJF + I)^-1 and a_n = log det K_n from the 80-bit Cholesky factor
    means, covariances, scatter matrices: plain sums

Bars (u = 2^-53).  Each is an a-priori bound on the device's formulation in terms of the operands of that element:
  scoring, per trial (m, s).  The device evaluates ccross m^T (Q + Q^T) s + bm m^T Q_m m + bs s^T Q_s s + cst + beta C_in with two
    GEMM stages (Y = (Q + Q^T) s, then m^T Y), each (dim + 8) u as in dgemm_ref:
        bar = 2 (dim + 8) u S_ms,   S_ms = |ccross| |m|^T (|Q| + |Q^T|) |s| + |bm| |m|^T |Q_m| |m| + |bs| |s|^T |Q_s| |s| + |cst| + |beta| |C_in|
    relative to S_ms, not to the score: for a target trial (s ~ m) the expansion cancels and the bar says so.  Two-covariance runs
    on Q_m = Q_s = G - H, bounded by |G| + |H| (which also carries the rounding of the difference).  Cosine: Q = I, ccross = 1/2,
    the whole over |m| |s|, plus 4 u for the two reciprocal square roots.
  PLDA.  K_n and log det come from a double Cholesky factorisation on the host.  A + dA = L L^T with ||dA|| <= c rf u ||A||, and
    A = n FTJF + I has its smallest eigenvalue >= 1, so kappa = cond(A) = ||A|| and ||K|| <= 1:  dK = K dA K gives
    |x^T dK y| <= c rf u kappa ||K x|| ||K y|| <= c rf u kappa sqrt(x^T K x  y^T K y) <= c rf u kappa * (the |.| forms of S_q); the log
    determinant moves by tr(K dA) and the sum of rf logarithms by rf u sum|log|; at rf = 1 three logarithms of a
    quotient of three roundings each are 6 u on their own.  With c = 4 on K and 8 on the constant:
        bar = (2 (rf + 8) + 4 rf kappa) u S_q + 8 rf u max(S_c, 1)
    S_q the three forms with |K_{L+1}| + |K_{L+1}^T|, |K_{L+1}| + |K_L|, |K_{L+1}| + |K_1|; S_c = 1/2 sum|a|; kappa the largest
    cond(n FTJF + I) of the call.  The cases keep kappa <= 1e3.
  iv_normalize, per element: centring u (|x| + |mu|); rotation (dim_in + 8) u sum_k |M_ik| |x_k - mu_k| plus the centring error
    through |M|; length normalisation (dim_out + 4) u |y| plus the error dz of the unnormalised column through 1 / ||z||:
    |dz_i| / ||z|| + |z_i| sum_k |z_k| |dz_k| / ||z||^3.
  dev set, per element: a mean over `count` vectors (count + 2) u sum|x| / count; a covariance element (i, j) over m summands
    (m + 8) u sum_s a_is a_js / norm with a_ks = |x_ks| + |mu_k| (bounds the centred value, carries the rounding of the mean); B has
    the sqrt(count) weights of the device and the oracle, SW the reference's n_last rule.  For Sigma and W the m = n summands
    outnumber the vectors of any mean, so (m + 8) u a a covers the means' error.  B, SB and SW sum over nspk speakers or n_last
    sessions only, while a mean in them may be one of 600 vectors: they get the term that form misses, the means' own bars e
    through the product, sum_s (e_is a_js + a_is e_js) / norm (with it the oracle's SB of the [600, 1, 2] set is at 0.04 of its
    bar, without it at 0.72).
  JFA, per element: jfa_subtract u |F| + (R + 8) u N (|m| + sum_r |W_r| |T_r| + |D| |Z|); jfa_subtract_sessions the same with the sum
    over the speaker's sessions; estimate_z 8 u |z|; D[k] of estimate_z_and_d (nspk + 8) u (sum|z f| + |sum z f|) / a1.
  approximate extractors, per element: norm_statistics 4 u (|F| + |m N|) sqrt(iv) (the bound of four roundings); subtract_m_plus_tw
    as jfa_subtract; norm_t 8 u |T| sqrt(iv); weighted_cov (C D + 8) u sum|w T_i T_j|; approximate_tctc u |Dm_in| +
    (2 (R + 8) + D + 8) u sum_k (sum_j |T_jk| |Q_ji|)^2.  estimate_w_ubm_weight / _eigen per utterance: ||w^ - w|| / ||w|| <=
    16 max(err_oracle_u, 64 u) (spd_ref.bar).  A call that accumulates onto a non-zero start adds one rounding of start + w, which
    that bar, relative to ||w|| alone, does not carry: the accumulating calls get u ||start + w|| / ||w|| more (and then say little
    about the solve, which the calls from a zero start judge).
An element whose bar is 0 must match exactly (tv_ref.ratio).  Nothing here is fitted to what the code under test returns:
tests/test_cpu_backend_ref.py holds a float64 restatement of the device's formulation and the double oracle to a quarter of every
bar -- bars that ARE the count of the roundings of a pointwise formula (centring, a short mean, estimate_z, norm_statistics) to
the share of the bar those roundings can reach --
and shows value-only defects that the whole-array criteria of tests/test_gpu_tv.py let through.
"""
import functools

import numpy as np

import spd_ref as sr
import tv_ref as tr

LD = sr.LD
U_DOUBLE = sr.U_DOUBLE
HAVE_LONGDOUBLE = sr.HAVE_LONGDOUBLE
SKIP_MESSAGE = sr.SKIP_MESSAGE
ratio = tr.ratio
relerr = tr.relerr
norm2 = tr.norm2
u = U_DOUBLE


def ld(a):
    return np.asarray(a, LD)


def mm(A, B):
    """long-double matrix product (einsum: numpy's matmul loop for long double is five times slower)"""
    return np.einsum("ik,kj->ij", ld(A), ld(B))


def f64(a):
    return np.ascontiguousarray(np.asarray(a, LD).astype(np.float64))


# ================================================================ scoring
SCORE_DIMS = (1, 5, 33, 64, 130)
SCORE_COUNTS = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 7), (33, 31), (34, 130), (131, 129))
RULES = ("cosine", "mahalanobis", "twocov", "mix_part", "plda")
FAINT = 1e-5
TARGET_DISTANCE = 1e-3
PLDA_PATTERN = (1, 1, 1, 3, 3, 1, 7, 7, 7, 7)
PLDA_COUNTS = {"one": (1,), "runs": PLDA_PATTERN, "distinct": (1, 2, 3, 4, 5, 6, 7, 8, 9), "odd run at odd index": (2, 4, 4, 4, 2, 2),
               "n 50": (50, 50, 1)}
KAPPA_MAX = 1e3
PLDA_C_K, PLDA_C_LOGDET = 4, 8


def faint_model(M):
    return M // 2 if M >= 2 else None


def faint_segment(S):
    return S // 2 if S >= 3 else None          # never the last segment: the column next to the pad keeps its scale


@functools.lru_cache(maxsize=None)
def plda_matrices(dim):
    """FTJF and a second model of the same size; one pair per rank, so that K_n is factored once per rank and n"""
    rng = np.random.default_rng(977 * dim + 5)
    k = max(2 * dim, 60)
    Fm = rng.normal(size=(k, dim))
    FTJF = Fm.T @ Fm / k
    return FTJF, FTJF + 0.5 * np.diag(rng.uniform(0.5, 1.5, dim))


_PLDA_K = {}


def score_inputs(dim, M, S, faint=True, quiet_last=None, nsess=None, seed=0):
    """models [dim, M], segments [dim, S]: min(M, S) target trials s_i = m_i + 1e-3 noise, trial (0, 0) exact (s = m) when there
    are two or more, one model and one segment scaled by 1e-5 (faint; not for cosine), quiet_last: the scale of the last segment"""
    rng = np.random.default_rng(1000003 * dim + 1009 * M + S + seed)
    m = rng.normal(size=(dim, M))
    s = rng.normal(size=(dim, S))
    nt = min(M, S)
    s[:, :nt] = m[:, :nt] + TARGET_DISTANCE * rng.normal(size=(dim, nt))
    if nt >= 2:
        s[:, 0] = m[:, 0]
    fm, fs = (faint_model(M), faint_segment(S)) if faint else (None, None)
    if fm is not None:
        m[:, fm] *= FAINT
    if fs is not None:
        s[:, fs] *= FAINT
    if quiet_last is not None:
        s[:, S - 1] *= quiet_last
    targets = [i for i in range(nt) if i != fm and i != fs and not (quiet_last is not None and i == S - 1)]
    A = rng.normal(size=(dim, dim))
    Mah = A @ A.T / dim + np.eye(dim)
    G = rng.normal(size=(dim, dim)) / dim
    H = rng.normal(size=(dim, dim)) / dim
    C_in = rng.normal(size=(M, S))
    FTJF, FTJF2 = plda_matrices(dim)
    if nsess is None:
        nsess = [PLDA_PATTERN[i % len(PLDA_PATTERN)] for i in range(M)]
    nsess = np.asarray(nsess, np.int64)
    assert len(nsess) == M
    return dict(dim=dim, M=M, S=S, m=np.ascontiguousarray(m), s=np.ascontiguousarray(s), Mah=Mah, G=G, H=H, C_in=C_in, FTJF=FTJF, FTJF2=FTJF2,
                nsess=nsess, msum=np.ascontiguousarray(m * nsess[None, :]), targets=targets, exact=(0 if nt >= 2 else None), fm=fm, fs=fs)


def quad_pairs(Q, A, B, sign):
    """q[i, j] = (a_i + sign b_j)^T Q (a_i + sign b_j), every pair on its own difference or sum, long double"""
    Q, A, B = ld(Q), ld(A), ld(B)
    out = np.empty((A.shape[1], B.shape[1]), LD)
    for i in range(A.shape[1]):
        d = A[:, i:i + 1] + sign * B
        out[i] = np.sum(d * mm(Q, d), axis=0)
    return out


def quad_cols(Q, A):
    A = ld(A)
    return np.sum(A * mm(Q, A), axis=0)


def abs_cross(Q, A, B):
    """|a_i|^T |Q| |b_j| (float64 is enough for a bar: nothing cancels)"""
    return np.abs(A).T @ np.abs(Q) @ np.abs(B)


def abs_cols(Q, A):
    A = np.abs(A)
    return np.sum(A * (np.abs(Q) @ A), axis=0)


def score_bar(dim, cross, mterm, sterm, cst=0.0, c_in=None):
    S_ms = cross + mterm[:, None] + sterm[None, :] + abs(cst) + (0.0 if c_in is None else np.abs(c_in))
    return 2 * (dim + 8) * u * ld(S_ms)


def plda_model(key, which, nmax):
    """FTJF, the caches of K_n and a_n = log det K_n (long double, filled by plda_k), kappa = cond((nmax + 1) FTJF + I)"""
    FTJF = score_case(*key)[which]
    rf = FTJF.shape[0]
    K, alpha = _PLDA_K.setdefault((rf, which), ({}, {}))
    return FTJF, K, alpha, float(np.linalg.cond((nmax + 1) * FTJF + np.eye(rf)))


def plda_k(FTJF, K, alpha, n):
    if n not in K:
        rf = FTJF.shape[0]
        L = sr.cholesky(LD(n) * ld(FTJF) + np.eye(rf, dtype=LD))
        K[n] = sr.inverse(L)
        alpha[n] = -2 * np.sum(np.log(np.diagonal(L)))
    return K[n], alpha[n]


@functools.lru_cache(maxsize=None)
def score_case(dim, M, S, kind="plain"):
    if kind == "plain":
        return score_inputs(dim, M, S)
    if kind == "cosine":
        return score_inputs(dim, M, S, faint=False)
    if kind == "quiet last":
        return score_inputs(dim, M, S, quiet_last=0.05)
    if kind == "self":
        p = score_inputs(dim, M, S, nsess=[1] * M)                   # one session each: the models' sums are the models
        p["s"] = p["msum"] = p["m"]
        p["targets"], p["exact"] = [], None
        return p
    if kind.startswith("plda "):
        ns = PLDA_COUNTS[kind[5:]]
        assert len(ns) == M
        return score_inputs(dim, M, S, nsess=ns)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _mix_form(key):
    p = score_case(*key)
    return quad_pairs(p["G"], p["m"], p["s"], 1)                     # shared by two-covariance and its mix part


@functools.lru_cache(maxsize=None)
def score_reference(key, rule, which="FTJF"):
    """-> (the rule's scores [M, S] in long double by the reference project's formula, the bar per trial)"""
    p = score_case(*key)
    dim, m, s = p["dim"], p["m"], p["s"]
    if rule == "cosine":
        ml, sl = ld(m), ld(s)
        nm, ns = np.sqrt(np.sum(ml * ml, 0)), np.sqrt(np.sum(sl * sl, 0))
        ref = mm(ml.T, sl) / (nm[:, None] * ns[None, :])
        bar = (2 * (dim + 8) + 4) * u * ld(np.abs(m).T @ np.abs(s)) / (nm[:, None] * ns[None, :])
        return ref, bar
    if rule == "mahalanobis":
        Q = p["Mah"]
        ref = -quad_pairs(Q, m, s, -1) / 2
        return ref, score_bar(dim, 0.5 * (abs_cross(Q, m, s) + abs_cross(Q.T, m, s)), 0.5 * abs_cols(Q, m), 0.5 * abs_cols(Q, s))
    if rule in ("twocov", "mix_part"):
        G, H = p["G"], p["H"]
        mix = _mix_form(key)
        cross = abs_cross(G, m, s) + abs_cross(G.T, m, s)
        if rule == "mix_part":
            return ld(p["C_in"]) + mix, score_bar(dim, cross, abs_cols(G, m), abs_cols(G, s), c_in=p["C_in"])
        ref = mix - quad_cols(H, m)[:, None] - quad_cols(H, s)[None, :]
        GH = np.abs(G) + np.abs(H)
        return ref, score_bar(dim, cross, abs_cols(GH, m), abs_cols(GH, s))
    assert rule == "plda"
    ns, ms = p["nsess"], p["msum"]
    FTJF, K, alpha, kappa = plda_model(key, which, int(ns.max()))
    assert kappa <= KAPPA_MAX, kappa
    K1, a1 = plda_k(FTJF, K, alpha, 1)
    ref, bar = np.empty((p["M"], p["S"]), LD), np.empty((p["M"], p["S"]), LD)
    s1 = quad_cols(K1, s)
    for L in sorted(set(int(v) for v in ns)):
        rows = np.flatnonzero(ns == L)
        KL, aL = plda_k(FTJF, K, alpha, L)
        KL1, aL1 = plda_k(FTJF, K, alpha, L + 1)
        mr = ms[:, rows]
        cst = (aL1 - aL - a1) / 2
        ref[rows] = (quad_pairs(KL1, mr, s, 1) - quad_cols(KL, mr)[:, None] - s1[None, :]) / 2 + cst
        k1, kl, kl1 = (np.abs(f64(x)) for x in (K1, KL, KL1))
        S_q = 0.5 * (abs_cross(kl1, mr, s) + abs_cross(kl1.T, mr, s)) + 0.5 * abs_cols(kl1 + kl, mr)[:, None] + 0.5 * abs_cols(kl1 + k1, s)[None, :]
        S_c = float(abs(aL1) + abs(aL) + abs(a1)) / 2
        bar[rows] = (2 * (dim + 8) + PLDA_C_K * dim * kappa) * u * ld(S_q) + PLDA_C_LOGDET * dim * u * max(S_c, 1.0)
    return ref, bar


SCORE_DEFECTS = ("segment term of the last segment", "cross term of the faint trial")


def score_restate(key, rule, which="FTJF", defect=None):
    """the device's formulation in float64 numpy: the expansion, (Q + Q^T) s first, BLAS sums in BLAS order, K_n and log det through
    LAPACK.  defect: a name of SCORE_DEFECTS (value-only)"""
    p = score_case(*key)
    m, s = p["m"], p["s"]

    def quad(Qc, cc, Qm, bm, Qs, bs, cst=0.0, mv=m, c_in=None):
        qm = np.sum(mv * (Qm @ mv), 0)
        qs = np.sum(s * (Qs @ s), 0)
        cross = mv.T @ ((Qc + Qc.T) @ s)
        if defect == SCORE_DEFECTS[0]:
            qs[-1] *= 1.0 + 1e-9
        if defect == SCORE_DEFECTS[1]:
            cross[p["fm"], p["fs"]] *= 1.0 + 1e-3
        out = cc * cross + bm * qm[:, None] + bs * qs[None, :] + cst
        return out if c_in is None else out + c_in
    if rule == "cosine":
        return (m.T @ s) * (1.0 / np.sqrt(np.sum(m * m, 0)))[:, None] * (1.0 / np.sqrt(np.sum(s * s, 0)))[None, :]
    if rule == "mahalanobis":
        return quad(p["Mah"], 0.5, p["Mah"], -0.5, p["Mah"], -0.5)
    if rule == "twocov":
        return quad(p["G"], 1.0, p["G"] - p["H"], 1.0, p["G"] - p["H"], 1.0)
    if rule == "mix_part":
        return quad(p["G"], 1.0, p["G"], 1.0, p["G"], 1.0, c_in=p["C_in"])
    FTJF, ns = p[which], p["nsess"]
    rf = p["dim"]
    out = np.empty((p["M"], p["S"]))

    def kn(n):
        A = n * FTJF + np.eye(rf)
        return np.linalg.inv(A), -np.linalg.slogdet(A)[1]
    K1, a1 = kn(1)
    for L in sorted(set(int(v) for v in ns)):
        rows = np.flatnonzero(ns == L)
        (KL, aL), (KL1, aL1) = kn(L), kn(L + 1)
        out[rows] = quad(KL1, 0.5, KL1 - KL, 0.5, KL1 - K1, 0.5, (aL1 - aL - a1) / 2.0, mv=p["msum"][:, rows])
    return out


def score_oracle(key, rule, which="FTJF"):
    from oracle import oracle as orc
    p = score_case(*key)
    if rule == "cosine":
        return orc.score_cosine(p["m"], p["s"])
    if rule == "mahalanobis":
        return orc.score_mahalanobis(p["m"], p["s"], p["Mah"])
    if rule == "twocov":
        return orc.score_twocov(p["m"], p["s"], p["G"], p["H"])
    if rule == "mix_part":
        return p["C_in"] + orc.score_twocov(p["m"], p["s"], p["G"], np.zeros_like(p["G"]))
    return orc.score_plda(p["msum"], p["nsess"], p["s"], p[which])


OLD_SCORE_THRESHOLD = {"cosine": 1e-12, "mahalanobis": 1e-11, "twocov": 1e-11, "mix_part": 1e-11, "plda": 1e-10}


def target_accuracy(key, rule, got):
    """the largest |error| / |score| over the target trials of a case (the exact trial s = m apart: its score is the constant)"""
    p = score_case(*key)
    ref, _ = score_reference(key, rule)
    t = [i for i in p["targets"] if i != p["exact"]]
    if not t:
        return 0.0
    e = np.abs(ld(got)[t, t] - ref[t, t]) / np.abs(ref[t, t])
    return float(e.max())


# ================================================================ iv_normalize
IVN_SHAPES = ((1, 1, 1), (5, 3, 7), (60, 40, 33), (33, 33, 130))
IVN_FORMS = (("mean", "M", True), ("mean", None, False), (None, "M", False), (None, None, True), ("mean", None, True))


@functools.lru_cache(maxsize=None)
def ivn_inputs(din, dout, n):
    rng = np.random.default_rng(7919 * din + 31 * dout + n)
    X = rng.normal(size=(din, n)) + 0.5
    return dict(X=np.ascontiguousarray(X), mean=rng.normal(size=din) * 0.5, M=rng.normal(size=(dout, din)))


def ivn_reference(X, mean, M, length_norm):
    """-> (Y in long double, the bar per element)"""
    Xl = ld(X)
    din = X.shape[0]
    z, dz = Xl, np.zeros(X.shape, LD)
    if mean is not None:
        z = Xl - ld(mean)[:, None]
        dz = u * (np.abs(Xl) + np.abs(ld(mean))[:, None])
    if M is not None:
        Ma = np.abs(ld(M))
        dz = mm(Ma, dz) + (din + 8) * u * mm(Ma, np.abs(z))
        z = mm(M, z)
    if not length_norm:
        return z, dz
    dout = z.shape[0]
    nz = np.sqrt(np.sum(z * z, 0))
    y = z / nz
    bar = (dout + 4) * u * np.abs(y) + dz / nz + np.abs(z) * np.sum(np.abs(z) * dz, 0) / (nz * nz * nz)
    return y, bar


def ivn_restate(X, mean, M, length_norm):
    z = X if mean is None else X - mean[:, None]
    if M is not None:
        z = M @ z
    return z / np.sqrt(np.sum(z * z, 0)) if length_norm else z


def ivn_tiny_columns():
    """X [5, 7]: column 3 of norm 1e-150 (its squared norm, 1e-300, is still a normal double), column 5 of norm 1e-170 (its squared
    norm underflows to 0 in double; long double holds it)"""
    rng = np.random.default_rng(5)
    X = rng.normal(size=(5, 7))
    X[:, 3] *= 1e-150 / np.linalg.norm(X[:, 3])
    X[:, 5] *= 1e-170 / np.linalg.norm(X[:, 5])
    return np.ascontiguousarray(X)


# ================================================================ development set
def _sps_257():
    return np.random.default_rng(257).integers(1, 5, 257)


DEV_CASES = {"1x[1]": (1, (1,), None), "3x[1,2,1]": (3, (1, 2, 1), None), "33x257": (33, None, None), "8x[600,1,2]": (8, (600, 1, 2), None),
             "33x257 scaled": (33, None, (1e6, 0.0)), "33x257 scaled + offset": (33, None, (1e6, 1e4))}


@functools.lru_cache(maxsize=None)
def dev_inputs(name):
    dim, sps, mod = DEV_CASES[name]
    sps = _sps_257() if sps is None else np.asarray(sps, np.int64)
    rng = np.random.default_rng(100 * dim + len(sps))
    k, n = len(sps), int(sps.sum())
    cls = np.repeat(np.arange(k), sps)
    X = (rng.normal(size=(dim, k)) * 1.5)[:, cls] + rng.normal(size=(dim, n))
    if mod is not None:
        X[0] *= mod[0]
        X += mod[1]
    return np.ascontiguousarray(X), sps


@functools.lru_cache(maxsize=None)
def dev_reference(name):
    """-> {quantity: (long-double value, bar per element)} for mean, smean, Sigma, W, B, SB, SW"""
    X, sps = dev_inputs(name)
    dim, n = X.shape
    k = len(sps)
    off = np.concatenate([[0], np.cumsum(sps)])
    cls = np.repeat(np.arange(k), sps)
    Xl, Xa = ld(X), np.abs(ld(X))
    cnt = ld(sps)
    mean = Xl.sum(1) / n
    ssum = np.stack([Xl[:, off[c]:off[c + 1]].sum(1) for c in range(k)], 1)
    sabs = np.stack([Xa[:, off[c]:off[c + 1]].sum(1) for c in range(k)], 1)
    sm = ssum / cnt
    out = {"mean": (mean, (n + 2) * u * Xa.sum(1) / n), "smean": (sm, (cnt + 2) * u * sabs / cnt)}

    e_mean, e_sm = out["mean"][1], out["smean"][1]

    def cov(Y, A, m, norm, E=None):
        bar = (m + 8) * u * mm(A, A.T) / norm
        if E is not None:                                         # the means' own error through the product (see the module docstring)
            bar = bar + (mm(E, A.T) + mm(A, E.T)) / norm
        return mm(Y, Y.T) / norm, bar
    out["Sigma"] = cov(Xl - mean[:, None], Xa + np.abs(mean)[:, None], n, n)
    Yw, Aw = Xl - sm[:, cls], Xa + np.abs(sm)[:, cls]
    out["W"] = cov(Yw, Aw, n, n)
    Yb, Ab, Eb = sm - mean[:, None], np.abs(sm) + np.abs(mean)[:, None], e_sm + e_mean[:, None]
    out["B"] = cov(Yb * np.sqrt(cnt), Ab * np.sqrt(cnt), k, n, Eb * np.sqrt(cnt))
    out["SB"] = cov(Yb, Ab, k, 1, Eb)
    nl = int(sps[-1])                                             # the reference's loop: the FIRST n_last sessions of the set, / n_last
    out["SW"] = cov(Yw[:, :nl], Aw[:, :nl], nl, nl, e_sm[:, cls][:, :nl])
    return out


def dev_restate(name, defect=None):
    """float64 numpy in numpy's (pairwise) summation order, the products through BLAS"""
    X, sps = dev_inputs(name)
    dim, n = X.shape
    k = len(sps)
    off = np.concatenate([[0], np.cumsum(sps)])
    cls = np.repeat(np.arange(k), sps)
    mean = X.mean(1)
    sm = np.stack([X[:, off[c]:off[c + 1]].mean(1) for c in range(k)], 1)
    Y, Yw, Yb = X - mean[:, None], X - sm[:, cls], sm - mean[:, None]
    nl = int(sps[-1])
    out = {"mean": mean, "smean": sm, "Sigma": Y @ Y.T / n, "W": Yw @ Yw.T / n, "B": (Yb * np.sqrt(sps)) @ (Yb * np.sqrt(sps)).T / n,
           "SB": Yb @ Yb.T, "SW": Yw[:, :nl] @ Yw[:, :nl].T / nl}
    if defect == DEV_DEFECT:
        out["W"][5, 7] *= 1.0 + 1e-6
    return out


DEV_DEFECT = "one element of W in a faint dimension"
DEV_DEFECT_CASE = "33x257 scaled"


def dev_oracle(name):
    from oracle import oracle as orc
    X, sps = dev_inputs(name)
    mean, sm = orc.dev_means(X, sps)
    S, W, B = orc.dev_cov_mat(X, sps)
    SB, SW = orc.dev_scatter_mat(X, sps)
    return {"mean": mean, "smean": sm, "Sigma": S, "W": W, "B": B, "SB": SB, "SW": SW}


def dev_judge(name, got):
    r = dev_reference(name)
    return {q: ratio(ld(got[q]) - r[q][0], r[q][1]) for q in got}


# ================================================================ JFA
JFA_SHAPES = ((3, 1, 1), (6, 5, 3), (5, 13, 7))
# 24 sessions, begins 0 1 1 4 13 14 16 16 16 21 22.  tv_batch 4: six FULL windows [0,4) .. [20,24), speaker 3 ([4, 13)) spans three,
# speaker 1 is empty in the middle of a window, the run of speakers 6, 7 empty at the front of [16, 20); the 11 speaker rows end
# ragged (4 + 4 + 3).  tv_batch 5: [0,5) .. [15,20) and a SHORT last window [20,24) (h1 clamped to nsess, a GEMM of 4 rows), speaker 3
# still across three windows; the 24-row forms of jfa_subtract end in a batch of 4 rows at r0 = 20, the 11-row forms in one of 1.
JFA_SESSIONS = (1, 0, 3, 9, 1, 2, 0, 0, 5, 1, 2)
JFA_BATCHES = (4, 5)
JFA_FAINT = 1e-9
JFA_LOUD = 1e4
JFA_STRADDLER = 3
JFA_DEFECT = "last session of the straddling speaker dropped for the faint Gaussian"


def jfa_windows_spanned(spk, batch):
    """the windows of `batch` sessions that hold a session of speaker spk"""
    sb = np.concatenate([[0], np.cumsum(JFA_SESSIONS)])
    return sorted(set(int(h) // batch for h in range(sb[spk], sb[spk + 1])))


def jfa_faint(C):
    return C // 2


@functools.lru_cache(maxsize=None)
def jfa_inputs(C, D, R):
    """11 speakers, 24 sessions.  Every factor entry has magnitude in [1, 2] and xbar in [-1, 1], so that the model terms of a bar
    are never small against u |F| (a bar of u |F| alone is the rounding of the last subtraction itself).  One Gaussian at 1e-9 of
    the others, one at 1e4 (C >= 5: what the whole-array criterion is relative to), one session count exactly 0."""
    rng = np.random.default_rng(10007 * C + 101 * D + R)
    SV = C * D
    nses = np.asarray(JFA_SESSIONS, np.int64)
    nspk, nsess = len(nses), int(nses.sum())
    sb = np.concatenate([[0], np.cumsum(nses)]).astype(np.int64)
    owner = np.repeat(np.arange(nspk), nses).astype(np.int64)

    def mag(shape):
        return rng.uniform(1.0, 2.0, shape) * rng.choice([-1.0, 1.0], shape)
    g = np.ones(C)
    g[jfa_faint(C)] = JFA_FAINT
    if C >= 5:
        g[0] = JFA_LOUD
    Nh = rng.uniform(0.2, 8.0, (nsess, C)) * g[None, :]
    Nh[7, C - 1] = 0.0                                        # one count that is exactly 0 (a session of the straddling speaker)
    Fh = (Nh[:, :, None] * rng.uniform(-1.0, 1.0, (nsess, C, D))).reshape(nsess, SV)
    N = np.stack([Nh[sb[i]:sb[i + 1]].sum(0) for i in range(nspk)])
    F = np.stack([Fh[sb[i]:sb[i + 1]].sum(0) for i in range(nspk)])
    return dict(C=C, D=D, R=R, nspk=nspk, nsess=nsess, sb=sb, owner=owner, Nh=np.ascontiguousarray(Nh), Fh=np.ascontiguousarray(Fh),
                N=np.ascontiguousarray(N), F=np.ascontiguousarray(F), m=mag(SV), V=mag((R, SV)), Um=mag((R, SV)), Y=mag((nspk, R)),
                X=mag((nsess, R)), Dm=rng.uniform(1.0, 2.0, SV), Z=mag((nspk, SV)), iv=rng.uniform(0.5, 2.0, SV))


JFA_SUBTRACT_FORMS = ("m + DZ", "m + VY", "m + VY + DZ by owner", "UX")


def jfa_subtract_args(p, form):
    """-> (N, F, keyword arguments of jfa_subtract as tests/test_gpu_tv.py calls it)"""
    if form == "m + DZ":
        return p["N"], p["F"], dict(means=p["m"], Dm=p["Dm"], Z=p["Z"])
    if form == "m + VY":
        return p["N"], p["F"], dict(means=p["m"], T=p["V"], W=p["Y"])
    if form == "m + VY + DZ by owner":                        # rows are sessions, 11 factor rows for 24 statistics rows
        return p["Nh"], p["Fh"], dict(owner=p["owner"], means=p["m"], T=p["V"], W=p["Y"], Dm=p["Dm"], Z=p["Z"])
    return p["Nh"], p["Fh"], dict(T=p["Um"], W=p["X"])


def jfa_subtract_reference(N, F, D, owner=None, means=None, T=None, W=None, Dm=None, Z=None):
    rows, C = N.shape
    o = np.arange(rows) if owner is None else np.asarray(owner)
    Nx = np.repeat(ld(N), D, axis=1)
    v = np.zeros(F.shape, LD)
    a = np.zeros(F.shape, LD)
    R = 0
    if T is not None:
        R = T.shape[0]
        v = v + mm(ld(W)[o], T)
        a = a + mm(np.abs(ld(W))[o], np.abs(ld(T)))
    if means is not None:
        v = v + ld(means)[None, :]
        a = a + np.abs(ld(means))[None, :]
    if Dm is not None:
        v = v + ld(Dm)[None, :] * ld(Z)[o]
        a = a + np.abs(ld(Dm))[None, :] * np.abs(ld(Z))[o]
    return ld(F) - Nx * v, u * np.abs(ld(F)) + (R + 8) * u * Nx * a


def jfa_subtract_restate(N, F, D, owner=None, means=None, T=None, W=None, Dm=None, Z=None):
    o = np.arange(N.shape[0]) if owner is None else np.asarray(owner)
    v = np.zeros(F.shape)
    if means is not None:
        v = v + means[None, :]
    if T is not None:
        v = v + W[o] @ T
    if Dm is not None:
        v = v + Dm[None, :] * Z[o]
    return F - np.repeat(N, D, axis=1) * v


def jfa_sessions_reference(p):
    D, R, sb = p["D"], p["R"], p["sb"]
    ux = np.repeat(ld(p["Nh"]), D, axis=1) * mm(p["X"], p["Um"])
    ua = np.repeat(ld(p["Nh"]), D, axis=1) * mm(np.abs(p["X"]), np.abs(p["Um"]))
    tot = np.stack([ux[sb[i]:sb[i + 1]].sum(0) for i in range(p["nspk"])])
    tota = np.stack([ua[sb[i]:sb[i + 1]].sum(0) for i in range(p["nspk"])])
    return ld(p["F"]) - tot, u * np.abs(ld(p["F"])) + (R + 8) * u * tota


def jfa_sessions_restate(p, defect=None):
    D, sb = p["D"], p["sb"]
    ux = np.repeat(p["Nh"], D, axis=1) * (p["X"] @ p["Um"])
    if defect == JFA_DEFECT:
        f = jfa_faint(p["C"])
        ux[sb[JFA_STRADDLER + 1] - 1, f * D:(f + 1) * D] = 0.0
    return p["F"] - np.stack([ux[sb[i]:sb[i + 1]].sum(0) for i in range(p["nspk"])])


def jfa_z_reference(p, tau):
    D = p["D"]
    n, F, v, d = np.repeat(ld(p["N"]), D, axis=1), ld(p["F"]), ld(p["iv"])[None, :], ld(p["Dm"])[None, :]
    z = F * v * d / (1 + n * v * d * d) if tau < 0 else (LD(tau) / (LD(tau) + n)) * d * v * F
    return z, 8 * u * np.abs(z)


def jfa_z_restate(p, tau):
    D = p["D"]
    n, F, v, d = np.repeat(p["N"], D, axis=1), p["F"], p["iv"][None, :], p["Dm"][None, :]
    return F * v * d / (1.0 + n * v * d * d) if tau < 0 else (tau / (tau + n)) * d * v * F


def jfa_zd_reference(p):
    """-> (Z, its bar, the new D, its bar)"""
    D, nspk = p["D"], p["nspk"]
    z, zbar = jfa_z_reference(p, -1.0)
    n, F, v, d = np.repeat(ld(p["N"]), D, axis=1), ld(p["F"]), ld(p["iv"])[None, :], ld(p["Dm"])[None, :]
    a1 = np.sum((1 / (1 + n * v * d * d) + z * z) * n, 0)
    a2 = np.sum(z * F, 0)
    return z, zbar, a2 / a1, (nspk + 8) * u * (np.sum(np.abs(z * F), 0) + np.abs(a2)) / a1


def jfa_zd_restate(p):
    D = p["D"]
    n, F, v, d = np.repeat(p["N"], D, axis=1), p["F"], p["iv"][None, :], p["Dm"][None, :]
    L = 1.0 + n * v * d * d
    z = F * v * d / L
    return z, np.sum(z * F, 0) / np.sum((1.0 / L + z * z) * n, 0)


# ================================================================ approximate extractors
AX_SHAPES = ((11, 4, 6, 5), (11, 4, 6, 8), (70, 16, 12, 21))


class Approx:
    """One (U, C, D, R): the inputs, the 80-bit result of every link on exactly the doubles the library is handed, the bars."""

    def __init__(self, U, C, D, R):
        from oracle import oracle as orc
        self.U, self.C, self.D, self.R = U, C, D, R
        SV = C * D
        s = tr.statistics(C, D, R, U)
        rng = np.random.default_rng(13 * U + R)
        self.N, self.F, self.means, self.iv, self.T = s["N"], s["F"], s["means"], s["invvar"], s["Tm"]
        self.weight = rng.dirichlet(np.ones(C))
        self.Wv = rng.normal(size=(U, R))
        self.Q = np.ascontiguousarray(np.linalg.qr(rng.normal(size=(R, R)))[0])
        Nx = np.repeat(ld(self.N), D, axis=1)
        Fl, ml, Tl = ld(self.F), ld(self.means)[None, :], ld(self.T)
        siv = np.sqrt(ld(self.iv))[None, :]
        self.Fn_ref = (Fl - ml * Nx) * siv
        self.Fn_bar = 4 * u * (np.abs(Fl) + np.abs(ml * Nx)) * siv
        self.Fn = f64(self.Fn_ref)
        self.Fs_ref = Fl - (ml + mm(self.Wv, Tl)) * Nx
        self.Fs_bar = u * np.abs(Fl) + (R + 8) * u * Nx * (np.abs(ml) + mm(np.abs(self.Wv), np.abs(Tl)))
        self.Tn_ref = Tl * siv
        self.Tn_bar = 8 * u * np.abs(self.Tn_ref)
        self.Tn = f64(self.Tn_ref)
        Tn = ld(self.Tn)
        wx = np.repeat(ld(self.weight), D)[None, :]
        self.Wm_ref = mm(Tn * wx, Tn.T)
        self.Wm_bar = (SV + 8) * u * mm(np.abs(Tn) * wx, np.abs(Tn).T)
        self.Wm = f64(self.Wm_ref)
        A = mm(Tn.T, self.Q).reshape(C, D, R)
        Aa = mm(np.abs(Tn).T, np.abs(self.Q)).reshape(C, D, R)
        self.Dm_ref = np.sum(A * A, 1)
        self.Dm_scale = (2 * (R + 8) + D + 8) * u * np.sum(Aa * Aa, 1)
        self.Dm = f64(self.Dm_ref)
        aux = mm(self.Fn, Tn.T)
        Wml, Dml, Ql = ld(self.Wm), ld(self.Dm), ld(self.Q)
        self.w_ubm = np.zeros((U, R), LD)
        self.cond = np.zeros(U)
        for i in range(U):
            L = np.eye(R, dtype=LD) + ld(self.N[i]).sum() * Wml
            self.cond[i] = np.linalg.cond(L.astype(np.float64))
            self.w_ubm[i] = sr.solve(sr.cholesky(L), aux[i])
        il = 1 / (1 + mm(self.N, Dml))
        self.w_eig = mm(mm(aux, Ql) * il, Ql.T)
        self.err_oracle = {"ubm": self.errors("ubm", orc.tv_estimate_w_ubm_weight(self.N, self.Fn, self.Tn, self.Wm)),
                           "eig": self.errors("eig", orc.tv_estimate_w_eigen(self.N, self.Fn, self.Tn, self.Dm, self.Q))}

    def w(self, which):
        return self.w_ubm if which == "ubm" else self.w_eig

    def errors(self, which, W, start=None):
        """forward error per utterance; the utterance without frames: 0 iff exactly the start value, inf otherwise"""
        w = self.w(which)
        want = w if start is None else w + ld(start)
        out = np.zeros(self.U)
        for i in range(self.U):
            d = norm2(ld(W[i]) - want[i])
            n = norm2(w[i])
            out[i] = (0.0 if d == 0 else np.inf) if n == 0 else float(d / n)
        return out

    def w_ratios(self, which, W, start=None):
        w = self.w(which)
        bar = np.array([sr.bar(e) for e in self.err_oracle[which]], LD)
        if start is not None:
            nw = norm2(w, 1)
            with np.errstate(divide="ignore", invalid="ignore"):
                bar = bar + np.where(nw > 0, u * norm2(w + ld(start), 1) / nw, 0)
        return ratio(self.errors(which, W, start), bar)

    def tctc_bar(self, start=None):
        return self.Dm_scale + (0 if start is None else u * np.abs(ld(start)))

    def restate(self):
        """float64 numpy, LAPACK's solve instead of the Cholesky factor"""
        Nx = np.repeat(self.N, self.D, axis=1)
        siv = np.sqrt(self.iv)[None, :]
        aux = self.Fn @ self.Tn.T
        w_ubm = np.stack([np.linalg.solve(np.eye(self.R) + self.N[i].sum() * self.Wm, aux[i]) for i in range(self.U)])
        A = (self.Tn.T @ self.Q).reshape(self.C, self.D, self.R)
        return dict(Fn=(self.F - self.means[None, :] * Nx) * siv, Fs=self.F - (self.means[None, :] + self.Wv @ self.T) * Nx, Tn=self.T * siv,
                    Wm=(self.Tn * np.repeat(self.weight, self.D)[None, :]) @ self.Tn.T, Dm=np.sum(A * A, 1), ubm=w_ubm,
                    eig=((aux @ self.Q) * (1.0 / (1.0 + self.N @ self.Dm))) @ self.Q.T)

    def oracle(self):
        from oracle import oracle as orc
        return dict(Fn=orc.tv_norm_statistics(self.N, self.F, self.means, self.iv), Fs=orc.tv_subtract_m_plus_tw(self.N, self.F, self.means, self.T, self.Wv),
                    Tn=orc.tv_norm_t(self.T, self.iv, self.C), Wm=orc.tv_weighted_cov(self.Tn, self.weight), Dm=orc.tv_approximate_tctc(self.Tn, self.Q, self.C))

    def judge(self, got):
        """{Fn, Fs, Tn, Wm, Dm: arrays} -> {name: ratios per element}"""
        refs = {"Fn": (self.Fn_ref, self.Fn_bar), "Fs": (self.Fs_ref, self.Fs_bar), "Tn": (self.Tn_ref, self.Tn_bar), "Wm": (self.Wm_ref, self.Wm_bar),
                "Dm": (self.Dm_ref, self.Dm_scale)}
        return {k: ratio(ld(v) - refs[k][0], refs[k][1]) for k, v in got.items() if k in refs}


@functools.lru_cache(maxsize=None)
def approx(U, C, D, R):
    return Approx(U, C, D, R)
