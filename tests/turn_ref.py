"""The yardstick of the TurnDetection tests (include/gmmiv_turn.h): restatements of a window position's criterion from its 2 W frames, of
the smoothing / decision / segment loops of TurnDetection.cpp:136-282 as written, and the bar a device value is held to.

value_ld        numpy.longdouble, every sum sequential in the order the reference reads the frames, log domain
value_ref64     fp64 in the reference's own order and domain: FrameAccGD sums frame by frame, det = prod cov, cst = (2 pi)^(-D/2) / sqrt(det),
                lk = cst exp(-0.5 m), log, the clamp, accumulated frame by frame
value_doc64     fp64 in the order include/gmmiv_turn.h documents (blocks of `step` frames)
Each takes defect = None | "unbiased" | "short12" | "logw": the planted defects of tests/test_cpu_turn_ref.py.

THE BAR of a position (nothing in it is fitted to an output):
    bar = k 2^-53 (sum over the 4 W evaluations of |llk_t|  +  W sum_d (1 + mean_d^2 / cov_d) for each of the three windows)
With u = 2^-53, h = the depth of the longest sum of frames (2 W frame by frame, step + ceil(2 W / step) in blocks) and kappa_d = mean_d^2 / cov_d:
  moments    mean carries (h + 1) u, cov = ss / n - mean^2 carries (h + 4) u (ss / n + mean^2) = (h + 4) u cov (1 + 2 kappa): a relative error
             delta_d = (h + 4) u (1 + 2 kappa_d).  LLK(window) moves by at most sum_d delta_d (W / 2 + sum_t (x - mean)^2 / (2 cov)) = W sum_d delta_d
             (sum_t (x_td - mean_d)^2 / cov_d = W by construction), and by sum_d |d mean_d| sum_t |x - mean| / cov <= (h + 1) u W sum_d |mean_d| / std_d
             <= (h + 1) u W sum_d (1 + kappa_d) / 2                                                  -> 2.5 (h + 4) u W sum_d (1 + kappa_d)
  a frame    q_t = sum_d (x - mean)^2 / cov: three roundings per term, D additions: (D + 4) u q_t; sum_t q_t = W D <= W sum_d (1 + kappa_d);
             q enters with 1/2                                                                      -> 0.5 (D + 4) u W sum_d (1 + kappa_d)
             log cst: D logarithms and D additions: (D + 3) u sum_d |log cov_d| / 2, and sum_d |log cov_d| <= 1.4 sum_d (1 + kappa_d)
             (logcov_ratio() checks that the case tables stay inside)                               -> 0.7 (D + 3) u W sum_d (1 + kappa_d)
             llk_t = log cst - q_t / 2: u |llk_t|; the reference's exp and log: 2 u |llk_t|
  the sums   (h + 1) u sum_t |llk_t| per window, 3 u (|LLK1| + |LLK2| + |LLK12|) for g
so k = 1.2 D + 2.5 h + 17 covers both terms (the first needs h + 7 only).  The long double side is 2^11 times finer and is not counted.
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
ZERO_LLK = -745.1332191019412      # log 2^-1075 (csrc/devutil.h)
GLR, DGLR, BIC = 0, 1, 2
BAD_COV, CLAMPED = 1, 2
TURN_NAMES = {"GLR": GLR, "DGLR": DGLR, "BIC": BIC}


def seq_sum(a, axis=0):
    """left to right, one rounding per addition (numpy's sum is pairwise)"""
    a = np.asarray(a)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), a.dtype)
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


def bar_k(D, W, step):
    h = max(2 * W, step + -(-2 * W // step))
    return 1.2 * D + 2.5 * h + 17


def _crit(g, crit, D, W, defect, dtype):
    if crit == GLR:
        return g
    if crit == DGLR:
        return -g
    P = dtype(0.5 * (2 * D + 1)) * dtype(math.log(W if defect == "logw" else 2 * W))
    return -g - P


def _rule(l, min_llk, max_llk):
    """per-frame rule of gmmiv_llk for one Gaussian of weight 1 -> (llk, acted)"""
    l = np.asarray(l)
    zero = ~(l >= ZERO_LLK) | ~np.isfinite(l)
    out = np.where(zero, min_llk, np.minimum(np.maximum(l, min_llk), max_llk)).astype(l.dtype)
    return out, zero | (l < min_llk) | (l > max_llk)


def _windows(x, W, defect):
    c12 = x[:2 * W - 1] if defect == "short12" else x[:2 * W]
    return x[:W], x[W:2 * W], c12


def value_ld(x, W, crit=DGLR, min_llk=-200.0, max_llk=200.0, defect=None):
    """x [2 W, D] (any float dtype) -> dict(value, status, abs_llk, cond, max_l): the long double value, the status bits, the two magnitudes
    of the bar, and the largest per-frame log-likelihood before the clamp"""
    x = np.asarray(x).astype(LD)
    D = x.shape[1]
    llks, bad, acted, abs_llk, cond, max_l = [], False, False, LD(0), LD(0), -np.inf
    for w in _windows(x, W, defect):
        n = LD(w.shape[0])
        s, ss = seq_sum(w), seq_sum(w * w)
        mean = s / n
        cov = ss / n - mean * mean
        if defect == "unbiased":
            cov = cov * n / (n - 1)
        cov64 = cov.astype(np.float64)
        if not (np.all(cov64 > 0) and np.all(np.isfinite(cov64))):
            bad = True
            continue
        lc = LD(-0.5) * (LD(D) * np.log(LD(8) * np.arctan(LD(1))) + seq_sum(np.log(cov)))
        d = w - mean
        q = seq_sum(d * d / cov, axis=1)
        raw = lc - LD(0.5) * q
        max_l = max(max_l, float(raw.max()))
        l, a = _rule(raw, LD(min_llk), LD(max_llk))
        acted |= bool(a.any())
        llks.append(seq_sum(l))
        abs_llk += seq_sum(np.abs(l))
        cond += LD(W) * seq_sum(1 + mean * mean / cov)
    if bad:
        return dict(value=float("nan"), status=BAD_COV, abs_llk=float("nan"), cond=float("nan"), max_l=float("nan"))
    g = llks[2] - (llks[0] + llks[1])
    return dict(value=_crit(g, crit, D, W, defect, LD), status=CLAMPED if acted else 0, abs_llk=float(abs_llk), cond=float(cond), max_l=max_l)


def bar(ref, D, W, step):
    """the bar of a position from value_ld's magnitudes"""
    return bar_k(D, W, step) * U * (ref["abs_llk"] + ref["cond"])


def logcov_ratio(x, W):
    """max over the three windows of sum_d |log cov_d| / sum_d (1 + kappa_d): the derivation takes it to be <= 1.4"""
    x = np.asarray(x, np.float64)
    out = 0.0
    for w in _windows(x, W, None):
        m, c = w.mean(axis=0), w.var(axis=0)
        out = max(out, float(np.abs(np.log(c)).sum() / (1 + m * m / c).sum()))
    return out


def value_ref64(x, W, crit=DGLR, min_llk=-200.0, max_llk=200.0, defect=None):
    """fp64, the reference's order and domain (linear likelihood, then log)"""
    x = np.asarray(x).astype(np.float64)
    D = x.shape[1]
    llks = []
    for w in _windows(x, W, defect):
        n = float(w.shape[0])
        s, ss = seq_sum(w), seq_sum(w * w)
        mean = s / n
        cov = ss / n - mean * mean
        if defect == "unbiased":
            cov = cov * n / (n - 1)
        if not (np.all(cov > 0) and np.all(np.isfinite(cov))):
            return float("nan")
        covinv = 1.0 / cov
        det = np.multiply.accumulate(cov)[-1]
        cst = math.pow(2.0 * math.pi, -0.5 * D) / math.sqrt(det)
        d = w - mean
        m = seq_sum(d * d * covinv, axis=1)
        with np.errstate(divide="ignore"):
            l = np.log(cst * np.exp(-0.5 * m))
        l, _ = _rule(l, min_llk, max_llk)
        llks.append(seq_sum(l))
    g = llks[2] - (llks[0] + llks[1])
    return float(_crit(g, crit, D, W, defect, np.float64))


def _block_sum(a, step):
    """a window's sum in the documented order: blocks of `step` frames from the first frame, each from 0 left to right, the blocks added
    in order"""
    parts = [seq_sum(a[i:i + step]) for i in range(0, a.shape[0], step)]
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


def value_doc64(x, W, step, crit=DGLR, min_llk=-200.0, max_llk=200.0, defect=None):
    """fp64 in the order of include/gmmiv_turn.h (the fused multiply-add of q is made in long double and rounded once)"""
    x = np.asarray(x).astype(np.float64)
    D = x.shape[1]
    llks = []
    for w in _windows(x, W, defect):
        n = float(w.shape[0])
        mean = _block_sum(w, step) / n
        cov = _block_sum(w * w, step) / n - mean * mean
        if defect == "unbiased":
            cov = cov * n / (n - 1)
        if not (np.all(cov > 0) and np.all(np.isfinite(cov))):
            return float("nan")
        iv = 1.0 / cov
        lc = -0.5 * (D * 1.8378770664093454835606594728112 + seq_sum(np.log(cov)))
        t = w - mean
        t2 = t * t
        q = np.zeros(w.shape[0])
        for d in range(D):
            q = (t2[:, d].astype(LD) * iv[d].astype(LD) + q.astype(LD)).astype(np.float64)
        l, _ = _rule(lc - 0.5 * q, min_llk, max_llk)
        llks.append(_block_sum(l, step))
    g = llks[2] - (llks[0] + llks[1])
    return float(_crit(g, crit, D, W, defect, np.float64))


# ---------------------------------------------------------------------------------------------------------------- as written
M64 = (1 << 64) - 1


def positions_as_written(L, W, step, begin=0):
    """the loop of TurnDetection.cpp:142-171 -> the number of criterion values (0: the segment is copied through)"""
    if L <= 2 * W:
        return 0
    end_seg = begin + L - 1
    end2 = begin + 2 * W - 1
    n = 0
    while end2 < end_seg:
        n += 1
        end2 += step
    return n


def pick_as_written(v, alpha, defect=None, dtype=np.float64):
    """:184-263 on one run's curve -> (smoothed, dec, mean, std); unsigned res.size() - 1, the j > 0 stop and the NaN behaviour kept.
    defect: None | "index0" (the left walk looks at index 0) | "ge" (>= for >)"""
    res = [dtype(a) for a in v]
    n = len(res)
    assert n >= 1
    size_m1 = (n - 1) & M64
    buf = [res[0], res[0]]
    i = 1
    while i < size_m1:
        buf[i % 2] = res[i]
        res[i] = dtype(0.25) * buf[(i - 1) % 2] + dtype(0.25) * res[i + 1] + dtype(0.5) * res[i]
        i += 1
    s, s2 = dtype(0), dtype(0)
    for a in res:
        s += a
        s2 += a * a
    mean = s / dtype(n)
    with np.errstate(invalid="ignore"):
        std = np.sqrt(s2 / dtype(n) - mean * mean)
    dec = [False] * n
    thr = dtype(alpha) * std
    over = (lambda a: a >= thr) if defect == "ge" else (lambda a: a > thr)
    i = 1
    while i < size_m1:
        j = i - 1
        mn = res[i]
        ok = True
        while ok and (j >= 0 if defect == "index0" else j > 0):
            if res[j] < mn:
                mn = res[j]
                j -= 1
            else:
                ok = False
        if over(abs(res[i] - mn)):
            j = i + 1
            mr = res[i]
            ok = True
            while ok and j < n:
                if res[j] < mr:
                    mr = res[j]
                    j += 1
                else:
                    ok = False
            dec[i] = bool(over(abs(res[i] - mr)))
        i += 1
    return np.array(res, dtype), np.array(dec, np.uint8), mean, std


def pick_margins(sm, alpha, std, n):
    """per position the smaller of the two margins ||v' - min| - alpha std| and the width 16 2^-53 (|v'| + |min| + alpha std n) inside which
    a decision may be left out of an exact comparison -> (margin, width) arrays (inf margin at the two ends)"""
    sm = np.asarray(sm, np.float64)
    mar, wid = np.full(n, np.inf), np.zeros(n)
    thr = alpha * std
    for i in range(1, n - 1):
        j, mn = i - 1, sm[i]
        while j > 0 and sm[j] < mn:
            mn = sm[j]
            j -= 1
        j, mr = i + 1, sm[i]
        while j < n and sm[j] < mr:
            mr = sm[j]
            j += 1
        for m in (mn, mr):
            a, w = abs(abs(sm[i] - m) - thr), 16 * U * (abs(sm[i]) + abs(m) + thr * n)
            if a - w < mar[i] - wid[i]:
                mar[i], wid[i] = a, w
    return mar, wid


def segments_as_written(begin, L, W, step, dec):
    """:142-145 and :265-279 for one input segment -> [(begin, length)]; dec: the decisions of its positions (empty: copied through)"""
    end_seg = begin + L - 1
    if L <= 2 * W:
        return [(begin, end_seg - begin + 1)]
    out, start = [], begin
    for i, d in enumerate(dec):
        if d:
            frame = begin + W - 1 + i * step          # end1 of position i
            out.append((start, frame - start + 1))
            start = frame + 1
    if start < end_seg:
        out.append((start, end_seg - start + 1))
    return out


def detect_as_written(x, runs, nfiles, W, step, alpha, crit=DGLR, min_llk=-200.0, max_llk=200.0, value=value_ref64):
    """the whole tool on a run table -> per file the list of output segments, and per run (curve, smoothed, dec, mean, std) or None"""
    segs, per_run = [[] for _ in range(nfiles)], []
    for b, L, f in np.asarray(runs).reshape(-1, 3):
        b, L, f = int(b), int(L), int(f)
        n = positions_as_written(L, W, step, b)
        if n == 0:
            per_run.append(None)
            segs[f] += segments_as_written(b, L, W, step, [])
            continue
        v = np.array([value(x[b + k * step:b + k * step + 2 * W], W, crit, min_llk, max_llk) for k in range(n)])
        sm, dec, mean, std = pick_as_written(v, alpha)
        per_run.append((v, sm, dec, mean, std))
        segs[f] += segments_as_written(b, L, W, step, dec)
    return segs, per_run


# ---------------------------------------------------------------------------------------------------------------- the case table
def draw_frames(rng, T, D, dtype=np.float64):
    """frames with 3 <= |mean| / std <= 10 per column and std in [0.7, 1.4]: kappa stays moderate, and large enough for the bar's
    sum |log cov| <= 1.4 sum (1 + kappa) even in a window of 4 frames (a small sample covariance has a large kappa; a large one, 4 times
    the true one, has log cov <= 2.1 against 1.4 (1 + 2.5^2 / 4) = 3.6)"""
    std = rng.uniform(0.7, 1.4, D)
    mean = std * rng.uniform(3, 10, D) * rng.choice((-1.0, 1.0), D)
    return rng.normal(mean, std, (T, D)).astype(dtype)


def speakers(nframes, D, seed, period=300):
    """two synthetic "speakers" -- two Gaussians two standard deviations apart in every column -- that alternate every `period` frames
    -> (float32 frames [nframes, D], the true change points)"""
    rng = np.random.default_rng(seed)
    std = rng.uniform(0.7, 1.4, D)
    mean = std * rng.uniform(3, 8, D)
    who = (np.arange(nframes) // period) % 2
    x = rng.normal(0, 1, (nframes, D)) * std + mean + 2.0 * std * who[:, None]
    return x.astype(np.float32), list(range(period, nframes, period))


CASES = [(D, W, step) for D in (1, 3, 17, 60, 64) for (W, step) in ((4, 1), (4, 3), (5, 5), (8, 3), (50, 5))]


def case_frames(D, W, step, npos=3, seed=0):
    """[npos, 2 W, D]: the 2 W frames of npos positions of case (D, W, step)"""
    rng = np.random.default_rng(100000 * seed + 1000 * D + 10 * W + step)
    x = draw_frames(rng, 2 * W + (npos - 1) * step, D)
    return np.stack([x[k * step:k * step + 2 * W] for k in range(npos)])
