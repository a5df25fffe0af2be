"""References, operand embedding and a dispatch mirror for the fp64 GEMM (k_dgemm, lia_ral_amd/csrc/tv_kernels.hip) as reached through
gmmiv_dgemm.  Plain numpy, no GPU.

exact_case   operands are integers in [-4, 4] and every scale an integer or a power of two: each product and each partial sum of
             up to 4096 of them is an integer below 2^17, exact in fp64 in ANY order, with or without FMA.  The accumulator is an
             int64 matmul; the scales are then applied in float64 in the kernel's own order of operations, which is exact as well
             and also gives the kernel's sign of a zero (a sum is -0 only when every addend is; the MFMA accumulator starts at +0 and
             the split-K sum at 0.0, so neither is ever -0).  The bar is BITWISE equality of the whole buffer C lives in.
real_case    normal entries, rows of op(A) and columns of op(B) scaled log-normally (sigma = 3): the elements of one result differ
             by many orders of magnitude and each is judged on its own,
                 |got - ref|_ij <= (K + 8) 2^-53 S_ij,   S = |alpha| (|op A| |op B|) + |beta| |C_in| (+ |br rv_i| + |bc cv_j| + |cst|),
             in mode 1 S times |rv_i cv_j| -- the gamma bound of a length-K dot product plus the handful of roundings after it
             (alpha, the epilogue terms, beta C, the nz additions of split-K), reference in np.longdouble.  Derived, not tuned:
             float64 numpy sits at 0.002 .. 0.18 of it (tests/test_cpu_dgemm_ref.py), a dropped term or an fp32 step is orders beyond.
embed        an operand as a view inside a larger flat buffer: NaN around A and B (a read outside the operand poisons the result),
             a finite sentinel around C that must come back bit for bit, and NaN INSIDE C when beta == 0 (every element written,
             C never read, side-stream strips joined before the context's stream is).
plan         what launch_dgemm / tvk_dgemm_splitk / k_dgemm do with a call, restated line by line: the list of launches with MODE,
             tile shape, grid, offsets, tile order and the k-tile count / tail of every K layer.  tests/test_cpu_dgemm_ref.py pushes
             CASES through it and names every dispatch path the table does not reach.
"""
import dataclasses
import functools
import itertools

import numpy as np

import spd_ref

LD = np.longdouble
U_DOUBLE = 2.0 ** -53
MARGIN = 64                 # doubles of fill before and after an embedded operand (512 bytes: keeps the 16-byte alignment)
SENTINEL = -7.03125e+77     # finite, not an integer: what surrounds C
PAIRS = ((False, False), (False, True), (True, False), (True, True))
DEFAULT_OPTS = {"gemm_remap": 1, "gemm_clamp": 1, "gemm_narrow": 1, "gemm_nt80": 1}


def pair_name(ta, tb):
    return "NT"[bool(ta)] + "NT"[bool(tb)]


# ---------------------------------------------------------------- the case table
@dataclasses.dataclass(frozen=True)
class Case:
    group: str
    ta: bool
    tb: bool
    M: int
    N: int
    K: int
    alpha: float = 1.0
    beta: float = 0.0
    batch: int = 1
    nz: int = 1
    epi: int = 0
    opts: tuple = ()            # ((option, value), ...) away from DEFAULT_OPTS
    aoff: int = 0               # doubles between the 16-byte aligned buffer and the first element of A / B
    boff: int = 0
    ald: int = 0                # parity of lda / ldb / ldc (0 even, 1 odd); always at least two more than the extent
    bld: int = 0
    cld: int = 0
    sa: str = "even"            # batch stride of A / B: "even", "odd" or "zero" (one shared matrix)
    sb: str = "even"
    sc: str = "even"
    real: bool = False

    @property
    def name(self):
        s = "%s %s %dx%dx%d a=%g b=%g" % (self.group, pair_name(self.ta, self.tb), self.M, self.N, self.K, self.alpha, self.beta)
        if self.batch != 1: s += " batch=%d" % self.batch
        if self.nz != 1: s += " nz=%d" % self.nz
        if self.epi: s += " epi=%d" % self.epi
        for k, v in self.opts: s += " %s=%d" % (k, v)
        if self.aoff or self.boff: s += " off=%d,%d" % (self.aoff, self.boff)
        if self.ald or self.bld or self.cld: s += " ld-odd=%d%d%d" % (self.ald, self.bld, self.cld)
        if (self.sa, self.sb, self.sc) != ("even",) * 3: s += " s=%s,%s,%s" % (self.sa, self.sb, self.sc)
        return s + (" real" if self.real else "")


TILE_SHAPES = ((130, 160), (192, 192), (194, 200), (96, 100), (3, 300), (1, 258), (64, 130), (131, 129))
TILE_KS = (2, 16, 18, 32, 34, 48, 60, 1, 17, 33)
ALPHA_BETA = tuple(itertools.product((1.0, -0.5), (0.0, 1.0, -2.0)))
REAL_KS = (18, 33, 60)
OPTION_SHAPES = ((130, 160), (194, 200))
OPTION_SETS = ((("gemm_clamp", 0),), (("gemm_narrow", 0),))
ORDER_SHAPES = ((1186, 9384, 18, ((True, False), (False, False))), (300, 2448, 16, PAIRS))
EPI_SHAPES = ((130, 160), (194, 200), (131, 129), (3, 300))


def _cases():
    out = []
    # tiles and k-tails: every pair x shape x K x (alpha, beta) in the exact form, three K per shape in the real-valued form
    for (ta, tb), (M, N), K in itertools.product(PAIRS, TILE_SHAPES, TILE_KS):
        for al, be in ALPHA_BETA:
            out.append(Case("tiles", ta, tb, M, N, K, al, be))
        if K in REAL_KS:
            out.append(Case("tiles", ta, tb, M, N, K, -0.5, 1.0, real=True))
            out.append(Case("tiles", ta, tb, M, N, K, 1.0, 0.0, real=True))
    # the same table with the clamped and the narrow instantiations switched off
    for opts, (ta, tb), (M, N), K in itertools.product(OPTION_SETS, PAIRS, OPTION_SHAPES, TILE_KS):
        for al, be in ALPHA_BETA:
            out.append(Case("options", ta, tb, M, N, K, al, be, opts=opts))
        if K in REAL_KS:
            out.append(Case("options", ta, tb, M, N, K, -0.5, 1.0, opts=opts, real=True))
    # alignment: each way out of the 16-byte loads, against the aligned call of the same operands
    for (ta, tb), (M, N, K), real in itertools.product(PAIRS, ((130, 160, 34), (194, 200, 18)), (False, True)):
        for kw in ({}, {"aoff": 1}, {"boff": 1}, {"aoff": 2, "boff": 2}, {"ald": 1}, {"bld": 1}):
            out.append(Case("align", ta, tb, M, N, K, -0.5, 1.0, real=real, **kw))
        for kw in ({}, {"sa": "odd"}, {"sb": "odd"}):
            out.append(Case("align", ta, tb, M, N, K, -0.5, 1.0, batch=2, real=real, **kw))
    # batch
    for (ta, tb), real in itertools.product(PAIRS, (False, True)):
        for kw in ({}, {"sb": "zero"}, {"sa": "zero"}, {"sc": "odd"}, {"sc": "odd", "cld": 1}):
            out.append(Case("batch", ta, tb, 130, 160, 34, -0.5, -2.0, batch=3, real=real, **kw))
            out.append(Case("batch", ta, tb, 64, 130, 16, 1.0, 0.0, batch=3, real=real, **kw))
    # tile order
    for M, N, K, pairs in ORDER_SHAPES:
        for (ta, tb), rm in itertools.product(pairs, (0, 1, 2)):
            out.append(Case("order", ta, tb, M, N, K, 1.0, 0.0, opts=(("gemm_remap", rm),) if rm != 1 else ()))
    # split-K
    for real in (False, True):
        for ta, tb in ((False, True), (True, False)):
            out.append(Case("splitk", ta, tb, 130, 160, 100, 1.0, 0.0, nz=3, real=real))
            out.append(Case("splitk", ta, tb, 130, 160, 100, -0.5, -2.0, nz=3, real=real))
        out.append(Case("splitk", False, True, 130, 160, 101, 1.0, 0.0, nz=3, real=real))
        out.append(Case("splitk", False, True, 130, 160, 101, -0.5, -2.0, nz=3, real=real))
        out.append(Case("splitk", False, True, 64, 64, 4096, 1.0, 0.0, nz=0, real=real))
        out.append(Case("splitk", True, False, 64, 64, 4096, 1.0, 1.0, nz=0, real=real))
        for (M, N), on in itertools.product(((128, 80), (256, 400), (128, 160)), (1, 0)):
            for al, be in ((1.0, 0.0), (-0.5, -2.0)):
                out.append(Case("splitk", False, True, M, N, 96, al, be, nz=2, opts=() if on else (("gemm_nt80", 0),), real=real))
        out.append(Case("splitk", False, True, 128, 80, 96, 1.0, -2.0, nz=2, ald=1, real=real))
    # epilogues
    for (ta, tb), (M, N), mode, be, real in itertools.product(((True, False), (False, False)), EPI_SHAPES, (1, 2), (0.0, 1.0), (False, True)):
        out.append(Case("epi", ta, tb, M, N, 34, -0.5, be, epi=mode, real=real))
    # K = 0
    for (ta, tb), be in itertools.product(PAIRS, (0.0, 3.0)):
        out.append(Case("degenerate", ta, tb, 130, 160, 0, 1.0, be))
    out.append(Case("degenerate", False, True, 130, 160, 0, 1.0, 3.0, nz=3))
    out.append(Case("degenerate", True, False, 130, 160, 0, 1.0, 3.0, epi=2))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


CASES = _cases()


# ---------------------------------------------------------------- operands
def _ld(cols, odd):
    return cols + 2 + (cols + odd) % 2


def layouts(case):
    """-> {"A" | "B" | "C": (shape3, (batch stride, ld), offset)} in doubles, offset from the aligned start of the operand's region"""
    M, N, K, b = case.M, case.N, case.K, case.batch
    out = {}
    for key, (r, c), odd, off, smode in (("A", (K, M) if case.ta else (M, K), case.ald, case.aoff, case.sa),
                                        ("B", (N, K) if case.tb else (K, N), case.bld, case.boff, case.sb),
                                        ("C", (M, N), case.cld, 0, case.sc)):
        ld = _ld(c, odd)
        s = 0 if smode == "zero" else r * ld + 4 + (r * ld + (smode == "odd")) % 2
        out[key] = ((b, r, c), (s, ld), off)
    return out


def embed(x, pad, fill, offset, shared=0):
    """x [b, r, c] (or [r, c]) as a view inside a flat buffer of `fill`: rows pad[0] doubles apart beyond their length, matrices
    pad[1] doubles beyond their rows (shared > 0: x is ONE matrix seen `shared` times with batch stride 0), the first element
    MARGIN + offset doubles into the buffer.  -> (flat, view, (batch stride, ld))"""
    x = np.asarray(x, np.float64)
    if x.ndim == 2:
        x = x[None]
    b, r, c = x.shape
    ld = c + pad[0]
    s = r * ld + pad[1]
    flat = np.full(2 * MARGIN + offset + b * s, fill, np.float64)
    nb = shared if shared else b
    sb = 0 if shared else s
    view = np.lib.stride_tricks.as_strided(flat[MARGIN + offset:], (nb, r, c), (8 * sb, 8 * ld, 8))
    if r and c:
        view[:b] = x
    return flat, view, (sb, ld)


def embed_case(case, key, x, fill):
    (b, r, c), (s, ld), off = layouts(case)[key]
    if s == 0:
        return embed(x[0], (ld - c, 4), fill, off, shared=b)
    return embed(x, (ld - c, s - r * ld), fill, off)


def _shapes(case):
    lay = layouts(case)
    sh = {k: lay[k][0] for k in lay}
    return {k: ((1,) + sh[k][1:] if lay[k][1][0] == 0 else sh[k]) for k in sh}


def _op(case, A, B):
    """op(A) [bA, M, K], op(B) [bB, K, N]"""
    return (A.transpose(0, 2, 1) if case.ta else A), (B.transpose(0, 2, 1) if case.tb else B)


def splits(case, n_cu=256):
    """True when the call goes through the slabs and the reduce kernel (gmmiv_dgemm: nz == 0 asks tvk_splitk_count)"""
    nz = case.nz if case.nz else splitk_count(case.M, case.N, case.K, n_cu)
    return nz > 1 and case.K > 0 and case.epi == 0


@functools.lru_cache(maxsize=6)
def _exact_operands(seed, ta, tb, M, N, K, batch, shA, shB, shC):
    rng = np.random.default_rng([seed, M, N, K, batch])
    A = rng.integers(-4, 5, shA).astype(np.float64)
    B = rng.integers(-4, 5, shB).astype(np.float64)
    C = rng.integers(-4, 5, shC).astype(np.float64)
    oa = A.transpose(0, 2, 1) if ta else A
    ob = B.transpose(0, 2, 1) if tb else B
    acc = np.matmul(oa.astype(np.int64), ob.astype(np.int64))          # int64, broadcast over a shared operand
    assert np.abs(acc).max(initial=0) <= 16 * max(K, 1)
    for x in (A, B, C, acc):
        x.setflags(write=False)
    return A, B, C, acc


def exact_case(case, seed=0):
    """-> dict A, B, C (the input C), rv, cv, br, bc, cst, ref; all float64 holding small integers / powers of two"""
    sh = _shapes(case)
    A, B, C, acc = _exact_operands(seed, case.ta, case.tb, case.M, case.N, case.K, case.batch, sh["A"], sh["B"], sh["C"])
    rng = np.random.default_rng([seed, 7, case.M, case.N])
    d = {"A": A, "B": B, "C": C, "rv": None, "cv": None, "br": 0.0, "bc": 0.0, "cst": 0.0}
    v = case.alpha * acc.astype(np.float64)
    if case.epi == 1:
        d["rv"] = 2.0 ** rng.integers(-3, 4, case.M) * rng.choice([-1.0, 1.0], case.M)
        d["cv"] = 2.0 ** rng.integers(-3, 4, case.N)
        v = v * d["rv"][None, :, None] * d["cv"][None, None, :]
    elif case.epi == 2:
        d["rv"] = rng.integers(-4, 5, case.M).astype(np.float64)
        d["cv"] = rng.integers(-4, 5, case.N).astype(np.float64)
        d["br"], d["bc"], d["cst"] = -2.0, 3.0, 0.5
        v = v + d["br"] * d["rv"][None, :, None] + d["bc"] * d["cv"][None, None, :] + d["cst"]
    if splits(case):
        ref = (case.beta * C if case.beta != 0 else 0.0) + (0.0 + v)         # k_splitk_reduce: s = 0.0 + slabs, then beta C + s
    else:
        ref = v + case.beta * C if case.beta != 0 else v
    d["ref"] = np.broadcast_to(ref, (case.batch, case.M, case.N))
    return d


def real_case(case, seed=0):
    """-> dict like exact_case, `ref` in long double plus `bound` (per element, float64)"""
    rng = np.random.default_rng([seed + 1000, case.M, case.N, case.K, case.batch])
    sh = _shapes(case)
    rs = np.exp(3.0 * rng.normal(size=case.M))
    cs = np.exp(3.0 * rng.normal(size=case.N))
    A = rng.normal(size=sh["A"]) * (rs[None, None, :] if case.ta else rs[None, :, None])
    B = rng.normal(size=sh["B"]) * (cs[None, :, None] if case.tb else cs[None, None, :])
    C = rng.normal(size=sh["C"]) * rs[None, :, None] * cs[None, None, :] * np.sqrt(max(case.K, 1))
    d = {"A": A, "B": B, "C": C, "rv": None, "cv": None, "br": 0.0, "bc": 0.0, "cst": 0.0}
    oa, ob = _op(case, A, B)
    acc = np.matmul(oa.astype(LD), ob.astype(LD))
    S = abs(case.alpha) * np.matmul(np.abs(oa), np.abs(ob))
    v = LD(case.alpha) * acc
    if case.epi == 1:
        d["rv"] = np.exp(rng.normal(size=case.M)) * rng.choice([-1.0, 1.0], case.M)
        d["cv"] = np.exp(rng.normal(size=case.N))
        rc = d["rv"].astype(LD)[None, :, None] * d["cv"].astype(LD)[None, None, :]
        v = v * rc
        S = S * np.abs(rc).astype(np.float64)
    elif case.epi == 2:
        d["rv"] = rng.normal(size=case.M) * rs
        d["cv"] = rng.normal(size=case.N) * cs
        d["br"], d["bc"], d["cst"] = -2.0, 3.0, 0.5
        v = v + LD(d["br"]) * d["rv"].astype(LD)[None, :, None] + LD(d["bc"]) * d["cv"].astype(LD)[None, None, :] + LD(d["cst"])
        S = S + np.abs(d["br"] * d["rv"])[None, :, None] + np.abs(d["bc"] * d["cv"])[None, None, :] + abs(d["cst"])
    if case.beta != 0:
        v = v + LD(case.beta) * C.astype(LD)
        S = S + abs(case.beta) * np.abs(C)
    d["ref"] = np.broadcast_to(v, (case.batch, case.M, case.N))
    d["bound"] = np.broadcast_to(bound(case.K, S), (case.batch, case.M, case.N))
    return d


def bound(K, S):
    return (K + 8) * U_DOUBLE * np.asarray(S, np.float64)


# ---------------------------------------------------------------- the dispatch mirror
@dataclasses.dataclass(frozen=True)
class Launch:
    ta: bool
    tb: bool
    mode: int
    am: int
    an: int
    wm: int
    wn: int
    grid: tuple             # (x, y, z) as launched
    m_off: int
    n_off: int
    remap: int
    layers: tuple           # per K layer (kb, ke, nkt, krem); one layer when the call is not split
    side: bool              # forked to the side stream
    whole: bool             # the only k_dgemm launch of its call

    @property
    def inst(self):
        """the template arguments as a kernel trace prints them"""
        return "k_dgemm<%s, %s, %d, %d, %d, %d, %d>" % (str(self.ta).lower(), str(self.tb).lower(), self.mode, self.am, self.an, self.wm, self.wn)


def splitk_count(M, N, K, n_cu):
    """tvk_splitk_count (tv_kernels.hip, `int tvk_splitk_count`)"""
    tiles = ((N + 127) // 128) * ((M + 127) // 128)
    if tiles >= 2 * n_cu or K < 2048:
        return 1
    nz = (6 * n_cu + tiles - 1) // tiles
    maxz = K // 512 if K // 512 > 1 else 1
    nz = min(nz, maxz)
    return max(nz, 1)


def _layers(mode, K, ksplit, gz):
    """k_dgemm: `kb = blockIdx.z * ksplit; ke = min(kb + ksplit, K)`, `krem = EDGE ? 0 : (ke - kb) & 15`, `nkt = (ke - kb + 15) / 16`"""
    out = []
    for z in range(gz if ksplit > 0 else 1):
        kb, ke = (z * ksplit, min(z * ksplit + ksplit, K)) if ksplit > 0 else (0, K)
        out.append((kb, ke, (ke - kb + 15) // 16 if ke > kb else 0, 0 if mode == 1 else (ke - kb) & 15))
    return tuple(out)


def _launch_dgemm(out, o, ta, tb, grid, M, N, K, lda, sA, ldb, sB, a_off, b_off, ksplit):
    """launch_dgemm (tv_kernels.hip), statement by statement; grid = (x, y, z)"""
    gx, gy, gz = grid
    remap = o["gemm_remap"] if gx >= 16 else 0                                     # epi.remap = grid.x >= 16 ? g_gemm_remap : 0

    def e(mode, am, an, g, m_off, n_off, side, whole=False):                       # launch_dgemm_e: empty grids are not launched
        if 0 in g:
            return
        out.append(Launch(ta, tb, mode, am, an, 2, 2, tuple(g), m_off, n_off, remap, _layers(mode, K, ksplit, g[2]), side, whole))
    kfull = (K % 2 == 0 or (ta and not tb)) and (ksplit <= 0 or ksplit % 16 == 0)
    aligned = a_off % 2 == 0 and b_off % 2 == 0 and lda % 2 == 0 and ldb % 2 == 0 and sA % 2 == 0 and sB % 2 == 0
    clamp_ok = bool(o["gemm_clamp"]) and (not ta or (M % 2 == 0 and M >= 2)) and (tb or (N % 2 == 0 and N >= 2))
    fm, fn = M // 128, N // 128
    if not kfull or not aligned or K <= 0:
        return e(1, 4, 4, grid, 0, 0, False, True)
    if fm == 0 or fn == 0:
        if clamp_ok and o["gemm_narrow"] and M <= 64 and N > 128:
            return e(2, 1, 4, (gx, (M + 31) // 32, gz), 0, 0, False, True)
        if clamp_ok:
            return e(2, 4, 4, grid, 0, 0, False, True)
        return e(1, 4, 4, grid, 0, 0, False, True)
    if clamp_ok:
        rm, rn = M - fm * 128, N - fn * 128
        if gx > fn:
            if o["gemm_narrow"] and rn <= 64: e(2, 4, 1, ((rn + 31) // 32, gy, gz), 0, fn * 128, True)
            else: e(2, 4, 4, (gx - fn, gy, gz), 0, fn * 128, True)
        if gy > fm:
            if o["gemm_narrow"] and rm <= 64: e(2, 1, 4, (fn, (rm + 31) // 32, gz), fm * 128, 0, True)
            else: e(2, 4, 4, (fn, gy - fm, gz), fm * 128, 0, True)
    else:
        if gx > fn: e(1, 4, 4, (gx - fn, gy, gz), 0, fn * 128, True)
        if gy > fm: e(1, 4, 4, (fn, gy - fm, gz), fm * 128, 0, True)
    e(0, 4, 4, (fn, fm, gz), 0, 0, False, not (gx > fn or gy > fm))


def plan(ta, tb, M, N, K, lda, ldb, sA=0, sB=0, a_off=0, b_off=0, batch=1, nz=1, epi=0, opts=None, n_cu=256):
    """The k_dgemm launches of gmmiv_dgemm(ta, tb, M, N, K, ...) and whether k_splitk_reduce follows: (launches, reduce).
    a_off / b_off: the operand bases in doubles past a 16-byte boundary (only their parity matters).
    Mirrors capi_iv_score.hip gmmiv_dgemm (the choice of path), tv_kernels.hip tvk_dgemm / tvk_dgemm_epi / tvk_dgemm_splitk (grid, the kc
    rounding, the nt80 condition), launch_dgemm (MODE / tile shape / strips) and the krem / nkt lines of k_dgemm."""
    o = dict(DEFAULT_OPTS, **(opts or {}))
    out = []
    if M <= 0 or N <= 0 or batch <= 0:
        return out, False
    grid = ((N + 127) // 128, (M + 127) // 128, batch)
    if epi:                                                                        # tvk_dgemm_epi: one matrix, no strides
        _launch_dgemm(out, o, ta, tb, grid[:2] + (1,), M, N, K, lda, 0, ldb, 0, a_off, b_off, 0)
        return out, False
    if nz == 0:
        nz = splitk_count(M, N, K, n_cu)
    if nz > 1 and K > 0:                                                           # tvk_dgemm_splitk (nz >= 2 here)
        kc = ((K + nz - 1) // nz + 15) // 16 * 16
        nz = (K + kc - 1) // kc
        nt80 = (o["gemm_nt80"] and not ta and tb and M % 128 == 0 and N % 80 == 0 and N % 128 != 0 and K % 16 == 0 and
                a_off % 2 == 0 and b_off % 2 == 0 and lda % 2 == 0 and ldb % 2 == 0)
        if nt80:                                                                   # launch_dgemm_nt80: no remap, no strips
            out.append(Launch(False, True, 0, 2, 5, 4, 1, (N // 80, M // 128, nz), 0, 0, 0, _layers(0, K, kc, nz), False, True))
        else:
            _launch_dgemm(out, o, ta, tb, grid[:2] + (nz,), M, N, K, lda, 0, ldb, 0, a_off, b_off, kc)
        return out, True
    _launch_dgemm(out, o, ta, tb, grid, M, N, K, lda, sA, ldb, sB, a_off, b_off, 0)
    return out, False


def plan_case(case, n_cu=256):
    lay = layouts(case)
    (sA, lda), (sB, ldb) = lay["A"][1], lay["B"][1]
    return plan(case.ta, case.tb, case.M, case.N, case.K, lda, ldb, sA if case.batch > 1 else 0, sB if case.batch > 1 else 0,
                case.aoff, case.boff, case.batch, case.nz, case.epi, dict(case.opts), n_cu)


def remap_tile(remap, Nt, Mt, bx, by):
    """k_dgemm's tile order: the (bx, by) a workgroup with blockIdx (bx, by) of an Nt x Mt grid works on (`if (epi.remap) {...}`)"""
    bx, by = np.asarray(bx, np.int64), np.asarray(by, np.int64)   # scalars or arrays of blockIdx values: the branches become selects
    if not remap:
        return bx, by
    G = Nt >> 3
    idx = by * Nt + bx
    xcd, loc = idx & 7, idx >> 3
    inside = idx < G * 8 * Mt
    if remap >= 2:
        bn = loc // (8 * Mt)
        w = np.minimum(G - 8 * bn, 8)
        assert (w[inside] >= 1).all()
        w = np.maximum(w, 1)                                      # (only keeps the unselected lanes from dividing by <= 0)
        r = loc - bn * 8 * Mt
        bm = r // (8 * w)
        h = np.minimum(Mt - 8 * bm, 8)
        assert (h[inside] >= 1).all()
        h = np.maximum(h, 1)
        rr = r - bm * 8 * w
        tx, ty = (8 * bn + rr // h) * 8 + xcd, 8 * bm + rr % h
    else:
        tx, ty = (loc // Mt) * 8 + xcd, loc % Mt
    r = idx - G * 8 * Mt
    return np.where(inside, tx, G * 8 + r // Mt), np.where(inside, ty, r % Mt)


# ---------------------------------------------------------------- what a plan reaches
def features(case, n_cu=256):
    """The dispatch paths (as the target names of tests/test_cpu_dgemm_ref.py) that `case` goes through"""
    launches, reduce = plan_case(case, n_cu)
    p = pair_name(case.ta, case.tb)
    f = set()
    modes = {l.mode for l in launches}
    lay = layouts(case)
    for l in launches:
        t = (l.am, l.an, l.wm, l.wn)
        f.add("inst " + l.inst)
        if t == (2, 5, 4, 1):
            f.add("NT nt80")
        elif l.mode == 0:
            f.add(p + " MODE 0 <4,4>")
        elif l.mode == 1:
            f.add(p + (" MODE 1 whole call" if l.whole else " MODE 1 strips beside MODE 0"))
        elif t[:2] == (4, 4):
            f.add(p + (" MODE 2 <4,4> no full tile" if l.whole else " MODE 2 <4,4> strips"))
        elif t[:2] == (1, 4):
            f.add(p + (" <1,4> M <= 64" if l.whole else " <1,4> bottom strip"))
        elif t[:2] == (4, 1):
            f.add(p + " <4,1> right strip")
        if l.mode != 1:
            for kb, ke, nkt, krem in l.layers:
                if krem:
                    f.add("MODE %d krem nkt %s" % (l.mode, "1" if nkt == 1 else "even" if nkt % 2 == 0 else "odd"))
                elif nkt in (1, 2, 3):
                    f.add("no tail nkt %d" % nkt)
        if case.K % 2 == 1 and not reduce:
            if l.mode != 1 and p == "TN": f.add("TN odd K on the fast path")
            if l.mode == 1 and l.whole and p != "TN": f.add(p + " odd K on MODE 1")
        Nt, Mt = l.grid[0], l.grid[1]
        G = Nt >> 3
        if l.remap == 1 and G >= 1 and Nt > 8 * G:
            f.add("remap 1 with leftover N tiles")
        if l.remap == 2 and G >= 9 and G % 8 != 0: f.add("remap 2 full and narrower block column")
        if l.remap == 2 and G >= 1 and Mt >= 9 and Mt % 8 != 0: f.add("remap 2 full and shorter block row")
    if reduce:
        f.add("inst k_splitk_reduce")
        ls = launches[0].layers
        if len(ls) > 1 and ls[-1][1] - ls[-1][0] < ls[0][1] - ls[0][0]: f.add("split-K ragged last range")
        if case.nz > 1 and (case.K % case.nz != 0 or (case.K // case.nz) % 16 != 0): f.add("split-K K / nz no multiple of 16")
    if case.batch > 1:
        sA, sB = lay["A"][1][0], lay["B"][1][0]
        if sA == 0 or sB == 0: f.add("batch stride 0")
        elif sA % 2 or sB % 2: f.add("batch odd stride")
        else: f.add("batch even strides")
    if modes == {1} and case.K % 2 == 0 and case.K > 0:
        if case.aoff % 2 or case.boff % 2: f.add("unaligned: base offset")
        if lay["A"][1][1] % 2 or lay["B"][1][1] % 2: f.add("unaligned: odd ld")
        if case.batch > 1 and lay["A"][1][0] % 2: f.add("unaligned: odd sA")
    return f


def targets():
    """Every dispatch path the issue of the GEMM's own tests lists; CASES must reach each"""
    t = []
    for p in ("NN", "NT", "TN", "TT"):
        t += [p + s for s in (" MODE 0 <4,4>", " MODE 1 whole call", " MODE 1 strips beside MODE 0", " MODE 2 <4,4> no full tile",
                              " MODE 2 <4,4> strips", " <1,4> bottom strip", " <4,1> right strip", " <1,4> M <= 64")]
        ab = p[0] == "T", p[1] == "T"
        for mode, am, an in ((0, 4, 4), (1, 4, 4), (2, 4, 4), (2, 1, 4), (2, 4, 1)):
            t.append("inst " + Launch(ab[0], ab[1], mode, am, an, 2, 2, (), 0, 0, 0, (), False, False).inst)
        t.append("TN odd K on the fast path" if p == "TN" else p + " odd K on MODE 1")
    t += ["NT nt80", "inst k_dgemm<false, true, 0, 2, 5, 4, 1>", "inst k_splitk_reduce"]
    t += ["MODE %d krem nkt %s" % (m, n) for m in (0, 2) for n in ("1", "even", "odd")]
    t += ["no tail nkt %d" % n for n in (1, 2, 3)]
    t += ["remap 1 with leftover N tiles", "remap 2 full and narrower block column", "remap 2 full and shorter block row",
          "split-K ragged last range", "split-K K / nz no multiple of 16", "batch even strides", "batch odd stride", "batch stride 0",
          "unaligned: base offset", "unaligned: odd ld", "unaligned: odd sA"]
    return t


HAVE_LONGDOUBLE = spd_ref.HAVE_LONGDOUBLE
SKIP_MESSAGE = spd_ref.SKIP_MESSAGE
