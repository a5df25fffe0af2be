"""What the tests of the list form of the i-vector scoring rules (include/gmmiv_iv_trials.h) share: the trial lists, a numpy mirror of
the host planner gmmiv_plan_iv_trial_tiles, and a float64 emulation of the documented summation order.  The scores and the bars per
trial are those of tests/backend_ref.py (score_case / score_reference), unchanged."""
import functools

import numpy as np

import backend_ref as br

DIMS = (1, 2, 5, 33, 64, 127, 128, 129, 130, 257)       # one pair, a tail lane, exactly 64 pairs, one more, more than two passes
LARGE_DIMS = tuple(d for d in DIMS if d >= 127)
COUNTS = tuple(c for c in br.SCORE_COUNTS if c[0] <= 34 and c[1] <= 130)
LIST_RULES = ("cosine", "mahalanobis", "twocov", "plda")
LISTS = ("full shuffled", "sparse", "single", "twice", "one model", "one segment")
PLDA_KINDS = ("runs", "distinct", "odd run at odd index")
ANCHOR_AUTO, ANCHOR_MODEL, ANCHOR_SEG = 0, 1, 2


def cases():
    """(dim, M, S) of the GPU test"""
    out = [(d, M, S) for d in DIMS for (M, S) in COUNTS]
    out += [(d, 7, 5) for d in LARGE_DIMS]
    return out


def case_key(dim, M, S, rule):
    return (dim, M, S, "cosine" if rule == "cosine" else "plain")


def trial_list(kind, M, S, seed=0):
    """-> (trial_model, trial_seg) int32"""
    rng = np.random.default_rng(7919 * M + 31 * S + seed)
    mm, ss = np.meshgrid(np.arange(M), np.arange(S), indexing="ij")
    mm, ss = mm.ravel(), ss.ravel()
    if kind == "full":
        tm, ts = mm, ss
    elif kind == "full shuffled":
        o = rng.permutation(M * S)
        tm, ts = mm[o], ss[o]
    elif kind == "sparse":
        keep = rng.random(M * S) < 0.3
        if not keep.any():
            keep[rng.integers(M * S)] = True
        o = rng.permutation(np.flatnonzero(keep))
        tm, ts = mm[o], ss[o]
    elif kind == "single":
        tm, ts = np.array([M // 2]), np.array([S - 1])
    elif kind == "twice":
        o = np.concatenate([rng.permutation(M * S), rng.permutation(M * S)])
        tm, ts = mm[o], ss[o]
    elif kind == "one model":
        tm, ts = np.full(S, M - 1), rng.permutation(S)
    elif kind == "one segment":
        tm, ts = rng.permutation(M), np.full(M, S // 2)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(tm, np.int32), np.ascontiguousarray(ts, np.int32)


# ---------------------------------------------------------------- the planner, restated
def anchor_rule(tm, ts):
    return ANCHOR_SEG if len(np.unique(ts)) < len(np.unique(tm)) else ANCHOR_MODEL


def plan(tm, ts, anchor, piece):
    """-> (order, tiles [(anchor, lo, hi)]): sorted by (anchor, partner, position), runs of one anchor cut into pieces"""
    tm, ts = np.asarray(tm, np.int64), np.asarray(ts, np.int64)
    if anchor == ANCHOR_AUTO:
        anchor = anchor_rule(tm, ts)
    ta, tp = (ts, tm) if anchor == ANCHOR_SEG else (tm, ts)
    order = np.lexsort((np.arange(len(ta)), tp, ta)).astype(np.int64)
    tiles = []
    i = 0
    while i < len(order):
        e = i
        while e < len(order) and ta[order[e]] == ta[order[i]]:
            e += 1
        for lo in range(i, e, piece):
            tiles.append((int(ta[order[i]]), lo, min(e, lo + piece)))
        i = e
    return order, tiles


# ---------------------------------------------------------------- the documented summation order in float64
def lane_dot(a_rows, b_rows):
    """dot of the row pairs [n x ldr] as k_score_trials adds them: lane j owns the element pairs p = j, j + 64, ... and adds them in
    increasing p, element 2p before 2p + 1; the 64 partials meet in the xor butterfly 32, 16, 8, 4, 2, 1.  (multiply, then add: the
    kernel's fused multiply-add rounds once where this rounds twice)"""
    n, ldr = a_rows.shape
    assert ldr % 2 == 0
    npairs = ldr // 2
    part = np.zeros((n, 64))
    for p0 in range(0, npairs, 64):
        w = min(64, npairs - p0)
        for e in (0, 1):
            cols = 2 * (p0 + np.arange(w)) + e
            part[:, :w] = part[:, :w] + a_rows[:, cols] * b_rows[:, cols]
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ d]
    assert np.array_equal(part, np.repeat(part[:, :1], 64, axis=1))      # every lane ends with the same bits
    return part[:, 0]


def rows(X):
    """[dim x n] columns -> [n x ldr] rows, the pad 0"""
    dim, n = X.shape
    out = np.zeros((n, dim + (dim & 1)))
    out[:, :dim] = X.T
    return out


def emulate(key, rule, tm, ts, which="FTJF"):
    """the list scores by the formulation of include/gmmiv_iv_trials.h in float64 numpy"""
    p = br.score_case(*key)
    m, s = p["m"], p["s"]

    def quad(mv, Qc, cc, Qm, bm, Qs, bs, cst, idx):
        A, B = rows(mv), rows((Qc + Qc.T) @ s)
        qm = np.sum(mv * (Qm @ mv), 0)
        qs = np.sum(s * (Qs @ s), 0)
        dot = lane_dot(A[tm[idx]], B[ts[idx]])
        return cc * dot + (bm * qm[tm[idx]] + (bs * qs[ts[idx]] + cst))
    every = np.arange(len(tm))
    if rule == "cosine":
        qm, qs = 1.0 / np.sqrt(np.sum(m * m, 0)), 1.0 / np.sqrt(np.sum(s * s, 0))
        return (lane_dot(rows(m)[tm], rows(s)[ts]) * qm[tm]) * qs[ts]
    if rule == "mahalanobis":
        return quad(m, p["Mah"], 0.5, p["Mah"], -0.5, p["Mah"], -0.5, 0.0, every)
    if rule == "twocov":
        return quad(m, p["G"], 1.0, p["G"] - p["H"], 1.0, p["G"] - p["H"], 1.0, 0.0, every)
    assert rule == "plda"
    FTJF, ns, rf = p[which], p["nsess"], p["dim"]

    def kn(n):
        A = n * FTJF + np.eye(rf)
        return np.linalg.inv(A), -np.linalg.slogdet(A)[1]
    K1, a1 = kn(1)
    out = np.empty(len(tm))
    for L in sorted(set(int(v) for v in ns[tm])):
        idx = np.flatnonzero(ns[tm] == L)
        (KL, aL), (KL1, aL1) = kn(L), kn(L + 1)
        out[idx] = quad(p["msum"], KL1, 0.5, KL1 - KL, 0.5, KL1 - K1, 0.5, (aL1 - aL - a1) / 2.0, idx)
    return out


@functools.lru_cache(maxsize=None)
def reference(key, rule, which="FTJF"):
    """backend_ref's long-double scores and bars [M x S], computed once per case and left unchanged"""
    return br.score_reference(key, rule, which)


def worst_ratio(got, key, rule, tm, ts, which="FTJF", scale=1.0):
    """-> (the largest |got_i - ref[m_i, s_i]| / (scale bar[m_i, s_i]) over the list, the position of that trial); per trial"""
    ref, bar = reference(key, rule, which)
    r = np.abs(br.ld(got) - ref[tm, ts]) / (scale * bar[tm, ts])
    r = np.where(np.isfinite(np.asarray(got, float)), r, np.inf)
    i = int(np.argmax(r))
    return float(r[i]), i
