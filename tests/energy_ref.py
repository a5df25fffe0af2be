"""The yardstick of the batched EnergyDetector (include/gmmiv.h: gmmiv_energy_train, gmmiv_energy_select).

chain() restates one file's chain in np.longdouble (80-bit on x86): FrameAccGD's biased variance of the raw column, energyMixtureInit,
nb_train_it x (log-domain full posteriors under the zero-likelihood rule, getEM, varianceControl), the meanStd threshold.  It also records
the MARGIN of every decision that two correct implementations could take differently (floor / ceiling comparisons, the argmax of the
means, x_t > threshold, the zero-likelihood test), so that tests/test_cpu_energy_ref.py can hold every case of the GPU list away from them.

THE BAR of a file, for every output q of (w, mean, cov, threshold):
    bar(q) = max( 8 |q(sequential fp64 restatement) - q(80-bit)| ,  nb_train_it n 2^-53 max(1, max|x|^2) )
The sequential fp64 restatement is tests/test_oracle_kat.py's energy_detector_steps + kat6_oracle_step (the CPU oracle's linear-domain
E-step, one frame after the other), plus 2^-53 |q|: the 80-bit value has to be written down in fp64 (the whole bar of an empty file
and of nb_train_it = 0, where 1 / C in fp64 is not 1 / C in 80 bits).  The factor 8 is the room a correct chain gets for another summation order; the floor is the plain
forward bound of the n-term sums, repeated per iteration.  A wrong formula shows at 1 / n and above.  For the degenerate files (NaN / Inf
energies, zero-likelihood frames -- inputs the oracle's linear-domain E-step has no rule for) the fp64 restatement is chain() itself run in
np.float64: the same rules, sequential rounding.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LD = np.longdouble
ZERO_LLK = -745.1332191019412          # GMMIV_ZERO_LLK
UNUSABLE_BOUND, READ_AS = 1e18, 1e10   # feat_sane (csrc/devutil.h)
EMPTY, NONFINITE, FLOORED, CEILED = 1, 2, 4, 8
TWO_PI = LD(2) * LD("3.141592653589793238462643383279502884")
FLOORING, CEILING = 0.5, 10.0          # the tool's defaults, the same in every case


def init_model(C, dt=LD):
    mean = np.array([-2.0 + c * 4.0 / (C - 1) if C > 1 else -2.0 for c in range(C)], dt)
    return np.full(C, 1.0, dt) / dt(C), mean, np.ones(C, dt)


def chain(x, C, nb_it, alpha, flooring=FLOORING, ceiling=CEILING, dt=LD, margins=None):
    """x: the selection in run order (raw values).  -> dict(w, mean, cov, threshold, status).  margins (a dict, optional) receives the
    smallest distance of every kind of decision: 'cov' (|cov - floor|, |cov - ceiling|), 'mean' (largest mean against the others),
    'llk' (|L - ZERO_LLK| / max(1, |L|)); the x_t > threshold margin is taken by the caller from the threshold."""
    x = np.asarray(x, np.float64).astype(dt)
    n = len(x)
    w, mean, cov = init_model(C, dt)
    if margins is not None:
        margins.update(cov=np.inf, mean=np.inf, llk=np.inf)
    if n == 0:
        return dict(w=w, mean=mean, cov=cov, threshold=dt(np.nan), status=EMPTY)
    with np.errstate(all="ignore"):
        s, ss = x.sum(), (x * x).sum()
        gm = s / dt(n)
        gcov = ss / dt(n) - gm * gm
        xs = np.where(np.abs(x) <= dt(UNUSABLE_BOUND), x, dt(READ_AS))   # a NaN compares false: read as 1e10
        flags = 0
        for it in range(nb_it):
            k = np.log(w) - dt(0.5) * np.log(dt(TWO_PI) * cov)
            d = xs[:, None] - mean[None, :]
            lg = k[None, :] - dt(0.5) * (d * d / cov[None, :])
            bad = np.isnan(lg).any(1)
            L = np.where(np.isnan(lg), -np.inf, lg).max(1)
            keep = ~bad & (L >= dt(ZERO_LLK)) & (L != np.inf)
            if margins is not None:
                lf = L[np.isfinite(L) & ~bad]
                if len(lf):
                    margins["llk"] = min(margins["llk"], float(np.min(np.abs(lf - dt(ZERO_LLK)) / np.maximum(1, np.abs(lf)))))
            e = np.exp(lg[keep] - L[keep, None])
            g = e / e.sum(1, keepdims=True)
            xk = xs[keep]
            occ, sx, sxx, count = g.sum(0), (g * xk[:, None]).sum(0), (g * (xk * xk)[:, None]).sum(0), dt(int(keep.sum()))
            w = occ / count
            live = occ > 0
            m_new = np.where(live, sx / np.where(live, occ, 1), mean)
            c_new = np.where(live, sxx / np.where(live, occ, 1) - m_new * m_new, cov)
            lo, hi = dt(flooring) * gcov, dt(ceiling) * gcov
            if margins is not None and np.isfinite(float(gcov)):
                margins["cov"] = min(margins["cov"], float(np.min(np.abs(c_new - lo))))
            fl = c_new <= lo
            c_new = np.where(fl, lo, c_new)
            if margins is not None and np.isfinite(float(gcov)):
                margins["cov"] = min(margins["cov"], float(np.min(np.abs(c_new - hi))))
            ce = c_new >= hi
            c_new = np.where(ce, hi, c_new)
            mean, cov = m_new, c_new
            if it == nb_it - 1:
                flags = (FLOORED if fl.any() else 0) | (CEILED if ce.any() else 0)
        higher = 0
        for c in range(1, C):
            if mean[c] > mean[higher]:
                higher = c
        if margins is not None and C > 1:
            margins["mean"] = float(np.min(np.abs(np.delete(mean, higher) - mean[higher])))
        th = mean[higher] - dt(alpha) * np.sqrt(cov[higher])
    fin = np.isfinite(float(th)) and all(np.all(np.isfinite(a.astype(np.float64))) for a in (w, mean, cov))
    return dict(w=w, mean=mean, cov=cov, threshold=th, status=flags | (0 if fin else NONFINITE))


def seq64(x, C, nb_it, alpha):
    """the sequential fp64 restatement: energy_detector_steps + kat6_oracle_step (tests/test_oracle_kat.py) on the selection"""
    from test_oracle_kat import energy_detector_steps, kat6_oracle_step
    w, mean, cov = init_model(C, np.float64)
    k = dict(seg_begin=np.array([0]), seg_len=np.array([len(x)]), init_w=w, init_mean=mean, init_cov=cov, nb_train_it=np.array(nb_it),
             alpha=np.array(float(alpha)), variance_flooring=np.array(FLOORING), variance_ceiling=np.array(CEILING))
    w, mean, cov, th = energy_detector_steps(k, np.asarray(x, np.float32), kat6_oracle_step(k))
    return dict(w=w, mean=mean[:, 0], cov=cov[:, 0], threshold=th)


def bars(x, C, nb_it, alpha, r80, degenerate=False):
    """-> dict(w, mean, cov, threshold) of bars for the file (see the module docstring); an empty file keeps the representation term alone"""
    n = len(x)
    rep = {q: 2.0 ** -53 * np.abs(np.nan_to_num(np.asarray(r80[q], np.float64), nan=0.0, posinf=0.0, neginf=0.0)) for q in ("w", "mean", "cov", "threshold")}
    if n == 0:
        return rep
    xf = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        xf = xf[np.abs(xf) <= UNUSABLE_BOUND]                 # an unusable value adds nothing to any sum: it buys no room either
    floor = nb_it * n * 2.0 ** -53 * max(1.0, float(np.max(xf * xf)) if len(xf) else 1.0)
    r64 = chain(x, C, nb_it, alpha, dt=np.float64) if degenerate else seq64(x, C, nb_it, alpha)
    out = {}
    with np.errstate(all="ignore"):
        for q in ("w", "mean", "cov", "threshold"):
            d = np.abs(np.asarray(r64[q], LD) - np.asarray(r80[q], LD)).astype(np.float64)
            out[q] = np.maximum(8.0 * np.where(np.isfinite(d), d, 0.0), floor) + rep[q]
    return out


def ratios(got, r80, bar):
    """error / bar of every output of one file: got = dict(w, mean, cov, threshold) in float64.  A non-finite reference value must be
    reproduced as it is (ratio 0 when it is, inf when not)."""
    out = {}
    with np.errstate(all="ignore"):
        for q in ("w", "mean", "cov", "threshold"):
            g, r, b = np.atleast_1d(np.asarray(got[q], np.float64)), np.atleast_1d(np.asarray(r80[q], LD)), np.atleast_1d(bar[q])
            rf = r.astype(np.float64)
            same = (np.isnan(g) & np.isnan(rf)) | (g == rf)
            fin = np.isfinite(g) & np.isfinite(rf)
            err = np.abs(g.astype(LD) - r).astype(np.float64)
            out[q] = float(np.max(np.where(same, 0.0, np.where(fin, err / np.where(b > 0, b, 1.0) + np.where(b > 0, 0.0, np.inf), np.inf))))
    return out


# ---- the GPU list: files, grouped by the call that evaluates them ---------------------------------------------------------------------
def energy_like(n, seed):
    """a normalised energy column: silence near -1, speech near +1, float32 values"""
    r = np.random.default_rng(seed)
    speech = r.random(n) < 0.45
    return np.where(speech, r.normal(1.0, 0.55, n), r.normal(-0.9, 0.3, n)).astype(np.float32)


def split_runs(n, k, seed):
    """k input segments of n frames together (every one >= 1 frame when n >= k)"""
    if k <= 1 or n < k:
        return [n]
    cuts = np.sort(np.random.default_rng(seed).choice(np.arange(1, n), k - 1, replace=False))
    return [int(v) for v in np.diff(np.r_[0, cuts, n])]


def groups(stage32, stage64):
    """The list: every group is one call (dtype, ldx, column, C, nb_train_it, alpha) on its files; a file = (n, seed, input segments).
    stage32 / stage64: gmmiv_energy_stage_frames of the two dtypes (the tests ask the library, the CPU test passes the same query)."""
    return [
        dict(name="A", dtype=np.float32, ldx=1, col=0, C=3, nb_it=10, alpha=0.25,
             files=[(2, 1, 1), (3, 2, 1), (63, 3, 1), (64, 4, 2), (0, 0, 1), (65, 5, 3), (255, 6, 1), (256, 7, 4), (257, 8, 1), (1000, 9, 7),
                    (5000, 10, 1), (stage32 - 1, 11, 1), (stage32, 12, 3), (stage32 + 1, 13, 2)]),
        dict(name="B", dtype=np.float64, ldx=34, col=16, C=2, nb_it=10, alpha=0.0,
             files=[(64, 21, 1), (257, 22, 5), (0, 0, 1), (1000, 23, 3), (stage64 - 1, 24, 2), (stage64, 25, 1), (stage64 + 1, 26, 4)]),
        dict(name="C", dtype=np.float32, ldx=34, col=5, C=8, nb_it=1, alpha=2.0, files=[(257, 31, 2), (1000, 32, 1), (5000, 33, 6), (65, 34, 1)]),
        dict(name="D", dtype=np.float64, ldx=1, col=0, C=1, nb_it=10, alpha=2.0, files=[(3, 41, 1), (65, 42, 2), (1000, 43, 1), (255, 44, 3)]),
        dict(name="E", dtype=np.float32, ldx=1, col=0, C=3, nb_it=0, alpha=0.25, files=[(0, 0, 1), (1, 51, 1), (2, 52, 1), (5000, 53, 4), (256, 54, 1)]),
        dict(name="F", dtype=np.float32, ldx=1, col=0, C=2, nb_it=1, alpha=0.0, files=[(2, 61, 1), (3, 62, 2), (64, 63, 1), (1000, 64, 2), (63, 65, 3), (256, 66, 1)]),
    ]


def layout(group):
    """-> (buffer [T, ldx] of the group's dtype, runs [nrun, 3] int64, selections: the column values of every file in run order).  The
    input segments of a file are NOT adjacent and lie in another order in the buffer than in the table; the gaps hold other energies and
    every other column 1e30."""
    rng = np.random.default_rng(1000 + ord(group["name"]))
    pieces, sels = [], []
    for f, (n, seed, k) in enumerate(group["files"]):
        x = energy_like(n, seed)
        sels.append(x)
        o = 0
        for ln in split_runs(n, k, seed + 500):
            pieces.append((f, len(pieces), x[o:o + ln]))
            o += ln
    order = rng.permutation(len(pieces)) if pieces else []
    pos, t, chunks = {}, 0, []
    for p in order:
        gap = energy_like(int(rng.integers(1, 9)), 7000 + int(p))
        chunks.append(gap); t += len(gap)
        pos[p] = t
        chunks.append(pieces[p][2]); t += len(pieces[p][2])
    col = np.concatenate(chunks + [energy_like(3, 7999)]) if chunks else energy_like(3, 7999)
    buf = np.full((len(col), group["ldx"]), 1e30, group["dtype"])
    buf[:, group["col"]] = col
    runs = np.array([(pos[i], len(pieces[i][2]), pieces[i][0]) for i in range(len(pieces)) if len(pieces[i][2]) > 0], np.int64).reshape(-1, 3)
    return buf, runs, sels


_REF = {}


def reference(stage32, stage64):
    """every group with its layout, the 80-bit results, the bars and the decision margins of every file -- computed once, read-only"""
    key = (stage32, stage64)
    if key not in _REF:
        out = []
        for g in groups(stage32, stage64):
            buf, runs, sels = layout(g)
            files = []
            for x in sels:
                m = {}
                r80 = chain(x, g["C"], g["nb_it"], g["alpha"], margins=m)
                files.append(dict(x=x, r80=r80, bar=bars(x, g["C"], g["nb_it"], g["alpha"], r80), margins=m))
            buf.setflags(write=False); runs.setflags(write=False)
            out.append(dict(g, buf=buf, runs=runs, ref=files))
        _REF[key] = out
    return _REF[key]


def file_runs(runs, f):
    r = runs[runs[:, 2] == f]
    return r[:, 0], r[:, 1]
