"""ComputeNorm on score lists, restated in numpy / Python as the reference runs it (LIA_SpkDet/ComputeNorm/src/ComputeNorm.cpp): one
growing list of scores per name (DistribNorm, :104-118) filled line by line (getAllScores / getAllScoresFirstNormed, :446-489),
DistribNorm::computeMeanStd per list (:121-159: descending sort, truncated discards, the unsorted "median" of meanMode 1 without
discards, sequential sums) and the four chains of :530-751 on dictionaries of lists.

Bounds: those of tests/test_gpu_score_norm.py (its module docstring has the derivation), restated for lists -- no new constant.  Any
summation order satisfies |fl(sum) - sum| <= (n - 1) u sum|x|, u = 2^-53; `bounds` turns that into bounds on mean and std of one
distribution, `norm_bound` carries input and parameter errors through y = (x - mu) / sd, `stats_with_bounds` does a whole list."""
import numpy as np

U = 2.0 ** -53


def seq_sum(v):
    """sum += v[i] for i in order (:140-143, :149-150): np.cumsum accumulates sequentially."""
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


def ref_mean_std(scores, mode, pH, pL):
    """DistribNorm::computeMeanStd, :121-159.  Returns (mean, std, kept scores)."""
    x = np.asarray(scores, dtype=np.float64)
    n = len(x)
    assert n > 0                                                       # :122
    begin, end, size = 0, n, n                                         # :124-126
    if pH != 0 or pL != 0:                                             # :127
        x = np.sort(x, kind="stable")[::-1]                            # :128 descendingSort
        dH, dL = int(float(n) * pH), int(float(n) * pL)                # :129-130 (unsigned long)((double)size * percent)
        size -= dH + dL                                                # :131
        begin, end = dH, n - dL                                        # :132-133
    kept = x[begin:end]
    assert size > 0 and len(kept) == size
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mode == 0:
            s, s2 = seq_sum(kept), seq_sum(kept * kept)                # :140-143
            mean = np.float64(s) / np.float64(size)                    # :144
            std = np.sqrt(np.float64(s2) / np.float64(size) - mean * mean)   # :145
        else:
            mean = kept[size // 2]                                     # :148 (input order when nothing was sorted)
            std = np.float64(seq_sum(np.abs(kept - mean))) / np.float64(size)   # :149-151
    return mean, std, kept


def ulp(v):
    return np.spacing(np.abs(v))


def bounds(mean_ref, std_ref, kept, mode, E=0.0):
    """(bound on |mean - mean_ref|, bound on |std - std_ref|) from the data.  E: what each INPUT score may differ by between the two
    sides (the second-stage lists hold normalised scores whose parameters carry their own error)."""
    size = len(kept)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == 1:
            dev = np.abs(kept - mean_ref)
            return E, 2 * E + 2 * (size - 1) * U * dev.mean() + 2 * ulp(std_ref)
        dm = E + 2 * (size - 1) * U * np.abs(kept).mean() + 2 * ulp(mean_ref)
        msq = (kept * kept).mean()
        dq = E * (2 * np.abs(kept).max() + E) + 2 * (size - 1) * U * msq + 2 * ulp(msq)
        dvar = dq + 2 * abs(mean_ref) * dm + dm * dm + 2 * U * (msq + mean_ref * mean_ref)
        return dm, min(dvar / std_ref if std_ref > 0 else np.inf, np.sqrt(dvar)) + 2 * ulp(std_ref)


def norm_bound(y_ref, dm, ds, sd_ref, e_in=0.0):
    """y = (x - mu) / sd against y_ref = (x_ref - mu_ref) / sd_ref with |x - x_ref| <= e_in, |mu - mu_ref| <= dm, |sd - sd_ref| <= ds."""
    b = (e_in + dm + np.abs(y_ref) * ds) / (sd_ref - ds)
    return b + 4 * U * (np.abs(y_ref) + b)


# ---- lists ------------------------------------------------------------------------------------------------------------------
# a line is (gender, name, seg, score)
def get_all_scores(lines, key, ids=None, first=None):
    """getAllScores (:446-462), and with `first` (name -> (mu, sd, dm, ds)) getAllScoresFirstNormed (:466-489).  key: "name" or "seg"
    (fieldOne); the other field is fieldTwo, which selectImp (:436-445) looks up in ids and the first stage in `first`.
    -> dict in order of first appearance: fieldOne -> ([scores in file order], [bound on each score's error])"""
    out = {}
    for _, name, seg, score in lines:
        one, two = (name, seg) if key == "name" else (seg, name)
        if ids is not None and two not in ids:
            continue
        e = 0.0
        if first is not None:
            if two not in first:
                raise KeyError("distribution for [%s] not found" % two)      # :483
            mu, sd, dm, ds = first[two]
            with np.errstate(invalid="ignore", divide="ignore"):
                score = (np.float64(score) - mu) / sd                        # :480
                e = float(norm_bound(score, dm, ds, sd))
        d = out.setdefault(one, ([], []))
        d[0].append(float(score))
        d[1].append(e)
    return out


def stats_with_bounds(dists, mode, pH, pL):
    """computeMeanStd of every list -> name -> (mu, sd, bound on mu, bound on sd)"""
    out = {}
    for k, (sc, err) in dists.items():
        mu, sd, kept = ref_mean_std(sc, mode, pH, pL)
        dm, ds = bounds(mu, sd, kept, mode, max(err) if err else 0.0)
        out[k] = (mu, sd, dm, ds)
    return out


def chain_ref(test, zlines, tlines, ztlines, norm_type, mode, pH, pL, ids=None):
    """:530-751 -> per test line (score, bound, first score or None, its bound or None)"""
    st = lambda lines, key, first=None: stats_with_bounds(get_all_scores(lines, key, ids, first), mode, pH, pL)
    if norm_type == "znorm":
        z, t = st(zlines, "name"), None                                          # :573
    elif norm_type == "tnorm":
        z, t = None, st(tlines, "seg")                                           # :537
    elif norm_type == "ztnorm":
        f = st(ztlines, "seg")                                                   # :618
        t = st(tlines, "seg")                                                    # :623
        z = st(zlines, "name", f)                                                # :629
    elif norm_type == "tznorm":
        z = st(zlines, "name")                                                   # :690
        f = st(ztlines, "name")                                                  # :697
        t = st(tlines, "seg", f)                                                 # :704
    else:
        raise ValueError("unknown normalization mode:" + norm_type)
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for _, name, seg, score in test:
            x = np.float64(score)
            if z is not None and name not in z:
                raise KeyError("znorm distribution not found for id [%s]" % name)
            if t is not None and seg not in t:
                raise KeyError("tnorm distribution not found for seg [%s]" % seg)
            if norm_type == "znorm":
                mu, sd, dm, ds = z[name]
                y = (x - mu) / sd                                                # :587
                out.append((y, norm_bound(y, dm, ds, sd), None, None))
            elif norm_type == "tnorm":
                mu, sd, dm, ds = t[seg]
                y = (x - mu) / sd                                                # :552
                out.append((y, norm_bound(y, dm, ds, sd), None, None))
            else:
                a, b = (t[seg], z[name]) if norm_type == "ztnorm" else (z[name], t[seg])
                x1 = (x - a[0]) / a[1]                                           # :647 / :730
                e1 = norm_bound(x1, a[2], a[3], a[1])
                y = (x1 - b[0]) / b[1]                                           # :654 / :736
                out.append((y, norm_bound(y, b[2], b[3], b[1], e1), x1, e1))
    return out
