"""NormFeat's windowMode (LIA_SpkDet/NormFeat/src/NormFeat.cpp:88-186, 372-447) restated -- a yardstick, no product code.

  schedule()     the loop of :384-446 kept in the reference's structure: the window is a list of segment COPIES, the current segment
                 a pointer (here an index into the cluster, None for NULL), nextSeg's exception a raise.  It returns EVERY step, the
                 ones that normalise nothing included.
  longdouble()   the whole mode on plain sequential sums in long double, the buffer kept in its own type (a store rounds), together
                 with a propagated error bar for an fp64 implementation (below).
  emulate()      the documented fp64 order of include/gmmiv_feat_window.h: 16 interleaved row sums per run, runs in table order,
                 the four operations of the statistics, the blend term by term.  Its `defect` argument plants one of four mistakes.

The bar.  u = 2^-53.  For a set of n frames with stored values x_t that the two computations know up to E_t (0 for a frame nobody has
rewritten yet -- both start from the same bytes):
    dS  = (n - 1) u sum|x| + sum E                      any order of n - 1 additions against any other (tests/test_gpu_feat_norm.py)
    dQ  = n u sum x^2 + sum (2 |x| E + E^2)             one more rounding per product
    dm  = dS / n + u |m|        dq = dQ / n + u q       dvar = dq + (2 |m| dm + dm^2 + u m^2) + u |var|       dsd = dvar / sd + u sd
(the square root's first-order factor 1 / (2 sd) is doubled for the higher orders), the blend term by term with one u per rounding,
    do  = dm' / s'_lo + |o| ds' / s'_lo + 3 u |o| + one ulp of the buffer type at o,      s'_lo = s' - ds'
and E_t = do for the frames the step rewrote.  The bar of a frame therefore carries the bars of every step its parameters depend on:
the steps that rewrote frames of its window, and theirs.  Nothing in it is fitted to any output."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def T(i, frame_length, trunc=True):
    """frameIdxToTime (SegTools.cpp:143-148); trunc=False is the planted defect"""
    if not trunc:
        return float(i) * frame_length
    return float(int(float(int(i) * 1000) * frame_length)) / 1000.0


class ScheduleError(Exception):
    pass


def schedule(begin, length, window_duration, window_comp, frame_length, cap=True, trunc=True):
    """-> [(window lo, window hi, apply lo, apply hi, alpha)] for every step, in order; indices into the cluster, hi exclusive.  Raises
    ScheduleError where the reference throws, AssertionError where a window or an apply range is not contiguous."""
    nseg = len(begin)
    window = []                                    # indices of the copies, in the order they were added
    steps = []

    def tm(i):
        return T(i, frame_length, trunc)

    def empty_window():
        return len(window) == 0

    def window_length():
        first, last = window[0], window[-1]
        return tm(begin[last] + length[last]) - tm(begin[first])

    def in_window(seg):
        if empty_window():
            window.append(seg)
            return True
        if window_length() <= window_duration:
            window.append(seg)
            return True
        return False

    def suppress_first():
        if window:
            window.pop(0)

    def move_window(seg, cur):
        window.append(seg)
        while True:
            suppress_first()
            f = window[0]
            if not (cur is not None and begin[f] < begin[cur] and window_length() > window_duration):
                break
        return seg if cur is None else cur

    def window_param():
        duration = window_length()
        alpha = tm(sum(length[s] for s in window))
        with np.errstate(all="ignore"):
            alpha = float(np.float64(alpha) / np.float64(duration))
        if cap and alpha > 1:
            alpha = 1.0
        return alpha * window_comp

    def in_middle(cur):
        return tm(begin[cur]) <= tm(begin[window[0]]) + window_duration / 2.0

    def next_seg(cur):
        for k, s in enumerate(window):
            if begin[s] == begin[cur]:
                return window[k + 1] if k + 1 < len(window) else None
        raise ScheduleError("currentSeg is not in the window")

    def emit(applied, alpha):
        w = list(window)
        assert w == list(range(w[0], w[-1] + 1)), "the window is not contiguous"
        if applied:
            assert applied == list(range(applied[0], applied[-1] + 1)), "the apply range is not contiguous"
            assert w[0] <= applied[0] and applied[-1] <= w[-1], "the apply range leaves the window"
            steps.append((w[0], w[-1] + 1, applied[0], applied[-1] + 1, alpha))
        else:
            steps.append((w[0], w[-1] + 1, w[0], w[0], alpha))

    cur = None
    for seg in range(nseg):
        if in_window(seg):
            if cur is None:
                cur = seg
        else:
            alpha = window_param()
            applied, ok = [], True
            while ok and in_middle(cur):
                applied.append(cur)
                cur = next_seg(cur)
                ok = cur is not None
            emit(applied, alpha)
            cur = move_window(seg, cur)
    if not empty_window():
        alpha = window_param()
        applied = []
        while True:
            applied.append(cur)
            cur = next_seg(cur)
            if cur is None:
                break
        emit(applied, alpha)
    return steps


def emitted(steps):
    """the steps that normalise something -- what gmmiv_plan_norm_windows returns"""
    return [s for s in steps if s[3] > s[2]]


def plan(runs, nfiles, file_first, window_duration, window_comp, frame_length, **kw):
    """the planner's output from schedule(): (step_off [nfiles + 1], steps [n, 4] as GLOBAL run indices, alpha [n])"""
    runs = np.asarray(runs, np.int64).reshape(-1, 3)
    off, st, al = [0], [], []
    for f in range(nfiles):
        idx = np.nonzero(runs[:, 2] == f)[0]
        if len(idx):
            r0 = int(idx[0])
            b = [int(v) - int(file_first[f]) for v in runs[idx, 0]]
            l = [int(v) for v in runs[idx, 1]]
            for wlo, whi, alo, ahi, a in emitted(schedule(b, l, window_duration, window_comp, frame_length, **kw)):
                st.append((r0 + wlo, r0 + whi, r0 + alo, r0 + ahi))
                al.append(a)
        off.append(len(st))
    return np.array(off, np.int64), np.array(st, np.int64).reshape(-1, 4), np.array(al, np.float64)


def _rows(runs, lo, hi):
    return np.concatenate([np.arange(runs[r, 0], runs[r, 0] + runs[r, 1]) for r in range(lo, hi)] or [np.zeros(0, np.int64)])


# ---------------------------------------------------------------------------------------------------------------- long double
def _ld_stats(X, E):
    """X [n, D] long double, E [n, D] float64 -> (m, sd, dm, dsd): FrameAccGD mean / biased std and their bars"""
    n = X.shape[0]
    with np.errstate(all="ignore"):
        S = np.cumsum(X, axis=0)[-1]
        Q = np.cumsum(X * X, axis=0)[-1]
        m = S / n
        q = Q / n
        var = q - m * m
        sd = np.sqrt(var)
        ax = np.abs(X).astype(np.float64)
        dS = (n - 1) * U * ax.sum(0) + E.sum(0)
        dQ = n * U * (ax * ax).sum(0) + (2 * ax * E + E * E).sum(0)
        am, aq = np.abs(m).astype(np.float64), np.abs(q).astype(np.float64)
        dm = dS / n + U * am
        dq = dQ / n + U * aq
        dvar = dq + (2 * am * dm + dm * dm + U * am * am) + U * np.abs(var).astype(np.float64)
        dsd = dvar / sd.astype(np.float64) + U * sd.astype(np.float64)
    return m, sd, dm, dsd


def longdouble(x, runs, nfiles, step_off, steps, alpha, cms=False, var=False):
    """x [T, D] float32 / float64 (not modified) -> dict(out [T, D] of x's type, gstat [nfiles, 2 D], step_stat [nsteps, 2 D] (float64
    of the long double values), bar [T, D], gbar, sbar).  Sums are sequential in frame order, every operation in long double."""
    runs = np.asarray(runs, np.int64).reshape(-1, 3)
    Tn, D = x.shape
    buf = x.copy()
    E = np.zeros((Tn, D))
    ulp = 2.0 ** -23 if x.dtype == np.float32 else 2.0 ** -52
    gstat, gbar = np.full((nfiles, 2 * D), np.nan), np.full((nfiles, 2 * D), np.nan)
    sstat, sbar = np.zeros((len(alpha), 2 * D)), np.zeros((len(alpha), 2 * D))
    for f in range(nfiles):
        idx = np.nonzero(runs[:, 2] == f)[0]
        if not len(idx):
            continue
        R = _rows(runs, int(idx[0]), int(idx[-1]) + 1)
        gm, gs, dgm, dgs = _ld_stats(buf[R].astype(LD), E[R])
        gstat[f], gbar[f] = np.concatenate([gm, gs]).astype(np.float64), np.concatenate([dgm, dgs])
        for s in range(int(step_off[f]), int(step_off[f + 1])):
            wlo, whi, alo, ahi = [int(v) for v in steps[s]]
            R = _rows(runs, wlo, whi)
            m, sd, dm, dsd = _ld_stats(buf[R].astype(LD), E[R])
            a = LD(alpha[s])
            na = LD(1) - a
            fa, fna = abs(float(a)), abs(float(na))
            with np.errstate(all="ignore"):
                mp = a * m + na * gm
                dmp = fa * dm + fna * dgm + 4 * U * (np.abs(a * m) + np.abs(na * gm)).astype(np.float64)
                t0, t1, d = a * sd * sd, na * gs * gs, mp - gm
                t2 = na * a * d * d
                f64 = lambda v: np.abs(v).astype(np.float64)
                dt0 = fa * (2 * f64(sd) * dsd + dsd * dsd) + 3 * U * f64(t0)
                dt1 = fna * (2 * f64(gs) * dgs + dgs * dgs) + 4 * U * f64(t1)
                dd = dmp + dgm + U * f64(d)
                dt2 = fna * fa * (2 * f64(d) * dd + dd * dd) + 5 * U * f64(t2)
                v = t0 + t1 + t2
                dv = dt0 + dt1 + dt2 + 2 * U * (f64(t0) + f64(t1) + f64(t2))
                sp = np.sqrt(v)
                dsp = dv / f64(sp) + U * f64(sp)
            if cms:
                sp, dsp = np.ones(D, LD), np.zeros(D)
            if var:
                mp, dmp = np.zeros(D, LD), np.zeros(D)
            sstat[s], sbar[s] = np.concatenate([mp, sp]).astype(np.float64), np.concatenate([dmp, dsp])
            A = _rows(runs, alo, ahi)
            with np.errstate(all="ignore"):
                o = (buf[A].astype(LD) - mp) / sp
                splo = f64(sp) - dsp
                ao = f64(o)
                E[A] = dmp / splo + ao * dsp / splo + 3 * U * ao + ulp * ao
            buf[A] = o.astype(x.dtype)
    return dict(out=buf, gstat=gstat, step_stat=sstat, bar=E, gbar=gbar, sbar=sbar)


# ---------------------------------------------------------------------------------------------------------------- the fp64 order
def run_partial(X):
    """X [len, D] float64 -> (sum, sum of squares): 16 interleaved row sums, each left to right, added in order"""
    n, D = X.shape
    k = (n + 15) // 16
    P = np.zeros((k * 16, D))
    P[:n] = X
    P = P.reshape(k, 16, D)
    lanes = np.cumsum(P, axis=0)[-1]                     # [16, D]: lane j = x[j] + x[j + 16] + ...  (a padded +0 changes nothing)
    lanes2 = np.cumsum(P * P, axis=0)[-1]
    return np.cumsum(lanes, axis=0)[-1], np.cumsum(lanes2, axis=0)[-1]


def group_stats(buf, runs, lo, hi):
    """the bits of gmmiv_frame_moments_groups (zeroed accumulator, one group of the runs [lo, hi)) and gmmiv_frame_moments_stats"""
    D = buf.shape[1]
    S = Q = n = None
    for r in range(lo, hi):
        s, q = run_partial(buf[runs[r, 0]:runs[r, 0] + runs[r, 1]].astype(np.float64))
        S, Q, n = (s, q, float(runs[r, 1])) if S is None else (S + s, Q + q, n + float(runs[r, 1]))
    if S is None:
        S, Q, n = np.zeros(D), np.zeros(D), 0.0
    S, Q, n = 0.0 + S, 0.0 + Q, 0.0 + n
    with np.errstate(all="ignore"):
        m = S / n
        q = Q / n
        return m, np.sqrt(q - m * m)


def blend(m, s, gm, gs, a, defect=None):
    """computeWindowParam :166-171 in float64, every product and sum rounded on its own -> (m', s') before the flags"""
    na = 1.0 - a
    with np.errstate(all="ignore"):
        mp = (a * m) + (na * gm)
        d = (m if defect == "unblended" else mp) - gm
        sp = np.sqrt(((a * s) * s + (na * gs) * gs) + (na * a) * (d * d))
    return mp, sp


def emulate(x, runs, nfiles, step_off, steps, alpha, cms=False, var=False, defect=None):
    """the documented order in float64 -> dict(out, gstat, step_stat).  defect: None, "unblended" (m instead of m' in the last term) or
    "original" (window statistics from the buffer as it came)"""
    runs = np.asarray(runs, np.int64).reshape(-1, 3)
    D = x.shape[1]
    buf = x.copy()
    gstat, sstat = np.full((nfiles, 2 * D), np.nan), np.zeros((len(alpha), 2 * D))
    for f in range(nfiles):
        idx = np.nonzero(runs[:, 2] == f)[0]
        if not len(idx):
            continue
        gm, gs = group_stats(x, runs, int(idx[0]), int(idx[-1]) + 1)
        gstat[f] = np.concatenate([gm, gs])
        for s in range(int(step_off[f]), int(step_off[f + 1])):
            wlo, whi, alo, ahi = [int(v) for v in steps[s]]
            m, sd = group_stats(x if defect == "original" else buf, runs, wlo, whi)
            mp, sp = blend(m, sd, gm, gs, float(alpha[s]), defect)
            if cms:
                sp = np.ones(D)
            if var:
                mp = np.zeros(D)
            sstat[s] = np.concatenate([mp, sp])
            for r in range(alo, ahi):
                b, n = int(runs[r, 0]), int(runs[r, 1])
                with np.errstate(all="ignore"):
                    buf[b:b + n] = ((buf[b:b + n].astype(np.float64) - mp) / sp).astype(x.dtype)
    return dict(out=buf, gstat=gstat, step_stat=sstat)


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar over the finite bars (0 / 0 counts as 0); the bar must be finite wherever the reference is"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    return float(np.nanmax(r)) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- tables
LENGTHS = (1, 2, 7, 30, 120, 700)
GAPS = (0, 1, 5, 40, 300)
DURATIONS = (0.0, 0.05, 0.5, 1.0, 3.0, 5.0)


def random_table(rng, nfiles, max_runs=12):
    """a run table [nrun, 3] of nfiles files (some without runs, some starting at a non-zero buffer frame) -> (runs, file_first, T)"""
    runs, first, pos = [], [], 0
    for f in range(nfiles):
        pos += int(rng.integers(0, 4))
        first.append(pos)
        p = pos + int(rng.choice((0, 0, 3, 11)))          # the first segment need not begin at the file's first frame
        for _ in range(int(rng.integers(0, max_runs + 1))):
            n = int(rng.choice(LENGTHS))
            runs.append((p, n, f))
            p += n + int(rng.choice(GAPS))
        pos = max(p, pos) + 1
    return np.array(runs, np.int64).reshape(-1, 3), np.array(first, np.int64), pos
