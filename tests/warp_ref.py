"""Feature warping restated (NormFeat `warp true`): the yardstick of tests/test_cpu_feat_warp.py and tests/test_gpu_feat_warp.py.

What is restated, and from where:
  * areaHisto / linearInterpolation (AccumulateStat.cpp:424-437) and warping() (ScoreWarp.cpp:168-206) AS WRITTEN -- including the
    back-off at :190-198, which subtracts the area of the bin AFTER the one the loop stopped in, and `interval < 1e-21 -> 1`;
  * boxMullerGeneratorInit / boxMullerGenerator / makeGausHisto (ScoreWarp.cpp:68-97) on glibc's rand() from its default seed:
    the chain behind NormFeat/test/01New.histo (KAT-7);
  * Histo::save's text layout (nbBin, nbBin lines "lowerBound<TAB>count", the last upper bound; default ostream precision = %g).
alize-core's Histo itself is not in the reference tree.  Its construction is restated from what the fixtures pin (DESIGN.md section 5,
KAT-7): equal-population bins, bound[i] = d[i k] on the sorted samples d with k = n / nbBin, bound[0] = d[0], bound[nbBin] = d[n - 1],
count = (population / n) / width.  Three of the 19 interior bounds of 01New.histo lie a little BELOW d[i k] (inside the gap to
d[i k - 1]); that parity is carried as "assumed".

This library's own definitions (no fixture shows them): n % nbBin != 0 -- the last bin takes the remainder; status DEGENERATE when a
bin's width is not > 0 and finite (ties, a constant column, n < nbBin, a NaN or infinite bound) -- that column is copied through;
the order of the sort is the total order of `sort_key` (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN).

Every function takes fp = numpy.float64 (the bits the device must give) or numpy.longdouble (the judge of those bits)."""
import numpy as np

PI2 = 3.14159265358979323846 * 2
EPS = 0.000000000000000000001
DEGENERATE = 1


# ---------------------------------------------------------------------------------------------------------------- .histo files
def read_histo(path):
    tok = open(path).read().split()
    nb = int(tok[0])
    if len(tok) != 2 * nb + 2:
        raise ValueError("%s: %d tokens for %d bins" % (path, len(tok), nb))
    bounds = np.array([float(t) for t in tok[1:1 + 2 * nb:2]] + [float(tok[-1])])
    count = np.array([float(t) for t in tok[2:2 + 2 * nb:2]])
    return bounds, count


def write_histo(path, bounds, count):
    with open(path, "w") as f:
        f.write("%d\n" % len(count))
        for b, c in zip(bounds[:-1], count):
            f.write("%g\t%g\n" % (b, c))
        f.write("%g\n" % bounds[-1])


# ---------------------------------------------------------------------------------------------------------- the KAT-7 chain
def glibc_rand(n, seed=1):
    """n draws of glibc's rand() (TYPE_3 additive feedback, r[i] = r[i-3] + r[i-31], 310 discarded); seed 1 is the default."""
    r = [0] * 34
    r[0] = seed
    for i in range(1, 31):
        hi, lo = divmod(r[i - 1], 127773)
        w = 16807 * lo - 2836 * hi
        r[i] = w + 2147483647 if w < 0 else w
    for i in range(31, 34):
        r[i] = r[i - 31]
    for i in range(34, 344):
        r.append((r[i - 31] + r[i - 3]) & 0xFFFFFFFF)
    out = np.empty(n, np.int64)
    for i in range(n):
        v = (r[-31] + r[-3]) & 0xFFFFFFFF
        r.append(v)
        out[i] = v >> 1
    return out


def box_muller_chain(n):
    """The n values makeGausHisto(n, 0, 1, .) accumulates: x1 = rand() / (float)RAND_MAX is a FLOAT quotient (2^31 as a float)."""
    u = (glibc_rand(n + 1).astype(np.float32) / np.float32(2147483648.0)).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u[1:])) * np.cos(PI2 * u[:-1])


# -------------------------------------------------------------------------------------------------------------- the histogram
def sort_key(v):
    """Unsigned keys whose order is the sort's: sign-magnitude bits mapped to an ascending integer."""
    v = np.ascontiguousarray(v)
    ut, top = (np.uint32, np.uint32(1 << 31)) if v.dtype == np.float32 else (np.uint64, np.uint64(1 << 63))
    u = v.view(ut)
    return np.where(u & top, ~u, u | top)


def histo(values, nb, fp=np.float64, bound_shift=0, density=True):
    """(bounds [nb + 1], count [nb], status) of one column's values (float32 or float64; the keys keep that type, the bounds are
    widened).  bound_shift and density=False plant defects for the tests of the yardstick."""
    values = np.ascontiguousarray(values)
    n = len(values)
    if n == 0:
        return np.zeros(nb + 1, fp), np.zeros(nb, fp), DEGENERATE
    d = values[np.argsort(sort_key(values), kind="stable")]
    k = n // nb
    idx = [0] + [min(max(i * k + bound_shift, 0), n - 1) for i in range(1, nb)] + [n - 1]
    b = d[idx].astype(np.float64).astype(fp)
    m = np.array([k] * (nb - 1) + [n - (nb - 1) * k], np.float64).astype(fp)
    with np.errstate(all="ignore"):
        w = b[1:] - b[:-1]
        count = (m / fp(n)) / w if density else m.copy()
        status = 0 if bool(np.all((w > 0) & (w < np.inf))) else DEGENERATE
    return b, count, status


# --------------------------------------------------------------------------------------------------------------- warping()
def area_histo(bounds, count, i):
    return count[i] * (bounds[i + 1] - bounds[i])


def linear_interpolation(val, lower, higher):
    interval = higher - lower
    if interval < EPS:
        return type(interval)(1)
    return (val - lower) / interval


def warping(score, sb, sc, tb, tc, backoff=True):
    """ScoreWarp.cpp:168-206, loop for loop, on scalars of the arrays' type (one value: slow)."""
    nb, nt = len(sc), len(tc)
    fp = sb.dtype.type
    score = fp(score)
    total_warp = fp(0.0)
    idx_w = 0
    while idx_w < nb and sb[idx_w + 1] < score:
        idx_w += 1
    idx_w = min(idx_w, nb - 1)  # the reference reads past the table here; a unit's own values never get there
    for i in range(idx_w):
        total_warp += area_histo(sb, sc, i)
    percent_w = linear_interpolation(score, sb[idx_w], sb[idx_w + 1])
    total_warp += area_histo(sb, sc, idx_w) * percent_w
    idx_d, total_dest = 0, fp(0.0)
    while idx_d < nt and total_dest < total_warp:
        total_dest += area_histo(tb, tc, idx_d)
        idx_d += 1
    if backoff:
        if idx_d == nt:
            idx_d -= 1
            total_dest -= area_histo(tb, tc, idx_d)
        elif idx_d > 0:
            total_dest -= area_histo(tb, tc, idx_d)  # as written: the bin AFTER the last one added
            idx_d -= 1
    else:
        idx_d = min(idx_d, nt - 1)
    ret = tb[idx_d]
    percent_h = linear_interpolation(total_warp, total_dest, area_histo(tb, tc, idx_d) + total_dest)
    ret = ret + (tb[idx_d + 1] - tb[idx_d]) * percent_h
    return ret


def _lin(val, lower, higher):
    interval = higher - lower
    with np.errstate(all="ignore"):
        q = (val - lower) / interval
    return np.where(interval < EPS, np.ones_like(q), q)


def warp_column(x, sb, sc, tb, tc, fp=np.float64, backoff=True, detail=False):
    """warping() on every value of a column at once -- the same operations in the same order (the prefixes are left folds), so the
    same bits as the loop.  The target's areas must be >= 0 (its prefix non-decreasing), as a density's are."""
    x = np.asarray(x).astype(np.float64).astype(fp)
    sb, sc, tb, tc = (np.asarray(a).astype(np.float64).astype(fp) if np.asarray(a).dtype != fp else np.asarray(a) for a in (sb, sc, tb, tc))
    nb, nt = len(sc), len(tc)
    with np.errstate(all="ignore"):
        sa = sc * (sb[1:] - sb[:-1])
        ta = tc * (tb[1:] - tb[:-1])
        P = np.concatenate([np.zeros(1, fp), np.cumsum(sa)])
        T = np.concatenate([np.zeros(1, fp), np.cumsum(ta)])
        assert np.all(T[1:] >= T[:-1]), "the target's areas must be >= 0"
        iw = np.searchsorted(sb[1:], x, side="left")
        iw = np.where(np.isnan(x), 0, np.minimum(iw, nb - 1))
        tw = P[iw] + sa[iw] * _lin(x, sb[iw], sb[iw + 1])
        jd = np.searchsorted(T, tw, side="left")
        jd = np.where(np.isnan(tw), 0, np.minimum(jd, nt))
        if backoff:
            full = jd == nt
            j = np.where(full, nt - 1, np.where(jd > 0, jd - 1, 0))
            td = np.where(full, T[nt] - ta[nt - 1], np.where(jd > 0, T[jd] - ta[np.minimum(jd, nt - 1)], T[0]))
        else:
            j = np.minimum(jd, nt - 1)
            td = T[jd]
        out = tb[j] + (tb[j + 1] - tb[j]) * _lin(tw, td, ta[j] + td)
    return (out, iw, j, tw) if detail else out


# ------------------------------------------------------------------------------------------------------------- a whole buffer
def unit_rows(runs, u):
    """The buffer rows of unit u, in table order."""
    sel = [np.arange(f, f + l) for f, l, uu in runs if uu == u]
    return np.concatenate(sel) if sel else np.zeros(0, np.int64)


def warp_units(x, runs, nunits, nb, tb, tc, fp=np.float64, out_dtype=None):
    """x [T x D] (float32 or float64), runs [(first, length, unit)]: (out, bounds [U x D x (nb + 1)], count [U x D x nb], status [U x D]).
    A DEGENERATE column of a unit is copied through; rows outside the runs keep their values."""
    x = np.asarray(x)
    D = x.shape[1]
    out = x.astype(out_dtype or x.dtype).copy()
    bounds = np.zeros((nunits, D, nb + 1), fp)
    count = np.zeros((nunits, D, nb), fp)
    status = np.zeros((nunits, D), np.int32)
    for u in range(nunits):
        rows = unit_rows(runs, u)
        for c in range(D):
            b, cn, s = histo(x[rows, c], nb, fp)
            bounds[u, c], count[u, c], status[u, c] = b, cn, s
            if s == 0 and len(rows):
                out[rows, c] = warp_column(x[rows, c], b, cn, tb, tc, fp).astype(np.float64).astype(out.dtype)
    return out, bounds, count, status
