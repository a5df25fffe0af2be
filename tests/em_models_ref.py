"""Reference, bars and case table for batched enrolment with variances (gmmiv_em_stats_models, gmmiv_map_adapt_models_full,
gmmiv_normalize_models; lia_ral_amd/csrc/stats_z.hip, gmm_kernels.hip, capi_models.hip).  Plain numpy, no GPU.

statistics   the rows N, F, S of a segment are gmm_ref.Reference.sums over the segment's frames under the segment's model (long double,
             log domain), with its bars occ_b, sx_b, sxx_b: nothing new is derived for them.
cases        gmm_ref.BATCH_CASES and (40, 61, 66) for the walk of vectSize 61-80; segments gmm_ref.ragged_bounds(T) (an empty one,
             bounds that cut 16-frame blocks and 64-frame tiles), the model of a segment from SEG_MODEL; model k has the means of
             gmm_ref.model(case, MODEL_SHIFTS[k]) and, for k > 0, its own variances: covInv scaled by exp(N(0, 0.1)) per entry.
computeMAP   map_ld: long double, from the float64 statistics it is given -- the kernel is element-wise and is judged on the SAME
             device statistics, so its bar is rounding alone: u = 2^-53 times the number of roundings on the path of a term times the
             MAGNITUDE of that term, summed over the terms; not relative to the result, which may be a cancellation.
                 mean_ml = F / N                              one rounding:                                  2u |mean_ml|
                 cov_ml  = S / N - mean_ml^2                  S / N (1), mean_ml (1) squared (2 + 1), the difference (1):
                                                              6u (|S / N| + mean_ml^2)                       -- a cancellation
                 alpha = (N / count) n, a = alpha / (alpha + r): five roundings, |da| <= 6u a, |d(1 - a)| <= 7u
                 mean = (1 - a) m0 + a mean_ml                16u (|m0| + |mean_ml|)
                 cov  = (1 - a) c0 + a cov_ml + (1 - a) a (m0 - mean_ml)^2
                        d(1 - a) c0 <= 8u |c0|;  a cov_ml <= (6 + 7)u (|S / N| + mean_ml^2);  m0 - mean_ml carries u |mean_ml| + u |dm|,
                        its square twice that relative to (|m0| + |mean_ml|)^2, the factor (1 - a) a another 14u, two products, two
                        sums: <= 16u per term:
                                                              16u (|c0| + |S / N| + mean_ml^2 + (|m0| + |mean_ml|)^2)
                 MAPConst / MAPConst2 means                   16u (|m0| + |mean_ml|)
                 weights: a w + (1 - a) w0, then divided by their sum over C terms (all positive):  (C + 16) u |w|
normalize    normalize_ld: one iteration of normalizeMixture towards N(0, 1) in long double.  mixtureFusion is a left fold of C - 1
             steps per dimension; a step puts at most 8 roundings on the mean (magnitude <= M = max_c |mean_c|: a convex combination) and
             12 on the variance (magnitude <= V = max_c cov_c + (2M)^2), and an error already there is carried with a factor <= 1:
                 |d tm| <= 8 C u M,   |d tc| <= 12 C u V                                              -- proportional to C
                 mean' = (mean - tm) / sqrt(tc):   (u |mean - tm| + |d tm|) / sqrt(tc) + |mean'| (|d tc| / (2 tc) + 3u)
                 cov'  = cov / tc:                 cov' (|d tc| / tc + 2u)
             Two iterations are the single iteration applied twice (the kernel keeps no state between them): the tests compare the bits
             of nb_it = 2 with two calls of nb_it = 1 and judge each step on its own input.
Derived, not tuned: a float64 numpy restatement sits well below 1; a dropped (1 - a) a dm^2 term, swapped a-priori / ML variances and
an fp32 table are orders beyond (tests/test_cpu_em_models_ref.py)."""
import functools

import numpy as np

import gmm_ref as gr

LD = gr.LD
U = gr.U
EM_CASES = gr.BATCH_CASES + ((40, 61, 66, 2.0),)
MODEL_SHIFTS = (0, 11, 12)
SEG_MODEL = np.array([1, 2, 0, 2, 1], np.int32)     # ragged_bounds gives five segments for T >= 8; the second one is empty
METHODS = ("MAPOccDep", "MAPModelBased", "MAPConst", "MAPConst2", "ML")   # "ML": an unknown MAPAlgo, the ML estimate
assert all(c in gr.CASES for c in EM_CASES)


def model(case, k):
    """model k of the case: (w, mean, covinv)"""
    w, mean, iv = gr.model(case, MODEL_SHIFTS[k])
    if k:
        iv = iv * np.exp(np.random.default_rng(100 + k).normal(0.0, 0.1, iv.shape))
    return w, mean, iv


def models(case):
    """-> w [3, C], mean [3, C, D], covinv [3, C, D]"""
    ms = [model(case, k) for k in range(len(MODEL_SHIFTS))]
    return tuple(np.stack([m[i] for m in ms]) for i in range(3))


def segments(case):
    sb = gr.ragged_bounds(case[2])
    assert len(sb) == len(SEG_MODEL) + 1
    return sb, SEG_MODEL


@functools.lru_cache(maxsize=None)
def reference(case, dtype_str, k):
    """the cached gmm_ref.Reference of model k on the case's frames; never modified by its users"""
    w, mean, iv = model(case, k)
    return gr.Reference(w, mean, iv, gr.frames(case, np.dtype(dtype_str).type))


@functools.lru_cache(maxsize=None)
def segment_rows(case, dtype_str):
    """per segment the dict of Reference.sums over its frames under its model (None for an empty segment)"""
    sb, sm = segments(case)
    return tuple(reference(case, dtype_str, int(m)).sums(int(sb[s]), int(sb[s + 1])) if sb[s + 1] > sb[s] else None for s, m in enumerate(sm))


def floor_share(case, dtype_str, s):
    """share of the (frame, Gaussian) pairs of segment s that are judged by the floor alone"""
    sb, sm = segments(case)
    g = reference(case, dtype_str, int(sm[s])).gamma[int(sb[s]):int(sb[s + 1])]
    return float((g < gr.FLOOR_ONLY).mean()) if g.size else 0.0


# ---------------------------------------------------------------- computeMAP, all three branches
def map_ld(N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov, method, mean=True, var=False, weight=False, reg=(16.0, 16.0, 16.0), alpha_mean=0.75):
    """N [G, C], F, S [G, C, D], count [G]; w0 [C], mean0, cov0 [C, D]; cur_mean, cur_cov [G, C, D] (float64, as the kernel reads them)
    -> dict mean, cov [G, C, D], w [G, C] (long double) and mean_b, cov_b, w_b (float64 bars)"""
    N, F, S, count, w0, m0, c0, cm, cc = (np.asarray(a, np.float64).astype(LD) for a in (N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov))
    G, C = N.shape
    D = m0.shape[1]
    F, S, cm, cc = (a.reshape(G, C, D) for a in (F, S, cm, cc))
    occ = N > 0
    Ns = np.where(occ, N, LD(1))[:, :, None]
    cnt = count[:, None]
    w = np.where(cnt > 0, N / np.where(cnt > 0, cnt, LD(1)), LD(0))
    ml = np.where(occ[:, :, None], F / Ns, cm)
    s_n = np.where(occ[:, :, None], S / Ns, LD(0))
    cml = np.where(occ[:, :, None], s_n - ml * ml, cc)
    f64 = lambda a: np.abs(a).astype(np.float64)
    ml_b = 2 * U * f64(ml) * occ[:, :, None]
    cml_b = 6 * U * (f64(s_n) + f64(ml * ml)) * occ[:, :, None]
    n = np.floor(count)[:, None]                                   # the reference passes an unsigned long
    alpha = w * n
    known = method in METHODS[:4]
    occdep = method in METHODS[:2]
    out = {}
    if not known:
        out.update(mean=ml, mean_b=ml_b, cov=cml, cov_b=cml_b, w=w, w_b=2 * U * f64(w))
        return out
    mag_m = f64(m0)[None] + f64(ml)
    if not mean:
        out["mean"], out["mean_b"] = np.broadcast_to(m0, ml.shape), np.zeros(ml.shape)
    elif occdep:
        a = (alpha / (alpha + LD(reg[0])))[:, :, None]
        out["mean"], out["mean_b"] = (1 - a) * m0 + a * ml, 16 * U * mag_m
    elif method == "MAPConst":
        out["mean"], out["mean_b"] = LD(alpha_mean) * m0 + (1 - LD(alpha_mean)) * ml, 16 * U * mag_m
    else:
        al = LD(alpha_mean)
        out["mean"] = (al * w0[None, :, None] * m0 + (1 - al) * w[:, :, None] * ml) / (w0[None, :, None] * al + w[:, :, None] * (1 - al))
        out["mean_b"] = 16 * U * mag_m
    if occdep and var:
        a = (alpha / (alpha + LD(reg[1])))[:, :, None]
        dm = m0 - ml
        out["cov"] = (1 - a) * c0 + a * cml + (1 - a) * a * dm * dm
        out["cov_b"] = 16 * U * (f64(c0)[None] + f64(s_n) + f64(ml * ml) + mag_m * mag_m)
    else:
        out["cov"], out["cov_b"] = np.broadcast_to(c0, ml.shape), np.zeros(ml.shape)
    if occdep and weight:
        a = alpha / (alpha + LD(reg[2]))
        r = a * w + (1 - a) * w0
        out["w"] = r / r.sum(1, keepdims=True)
        out["w_b"] = (C + 16) * U * f64(out["w"])
    else:
        out["w"], out["w_b"] = np.broadcast_to(w0, w.shape), np.zeros(w.shape)
    return out


def map_np(N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov, method, mean=True, var=False, weight=False, reg=(16.0, 16.0, 16.0), alpha_mean=0.75,
           defect=None):
    """the kernel's arithmetic restated in float64 numpy -> (mean, cov, w).  defect (tests/test_cpu_em_models_ref.py): "drop" leaves the
    (1 - a) a dm^2 term out, "swap" exchanges the a-priori and the ML variance, "fp32" rounds the a-priori variances to float32"""
    N, F, S, count, w0, m0, c0, cm, cc = (np.asarray(a, np.float64) for a in (N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov))
    G, C = N.shape
    D = m0.shape[1]
    F, S, cm, cc = (a.reshape(G, C, D) for a in (F, S, cm, cc))
    if defect == "fp32":
        c0 = c0.astype(np.float32).astype(np.float64)
    occ = (N > 0)[:, :, None]
    Ns = np.where(N > 0, N, 1.0)[:, :, None]
    w = np.where(count[:, None] > 0, N / np.where(count > 0, count, 1.0)[:, None], 0.0)
    ml = np.where(occ, F / Ns, cm)
    cml = np.where(occ, S / Ns - ml * ml, cc)
    alpha = w * np.floor(count)[:, None]
    if method not in METHODS[:4]:
        return ml, cml, w
    occdep = method in METHODS[:2]
    if not mean:
        mo = np.broadcast_to(m0, ml.shape)
    elif occdep:
        a = (alpha / (alpha + reg[0]))[:, :, None]
        mo = (1 - a) * m0 + a * ml
    elif method == "MAPConst":
        mo = (alpha_mean * m0) + ((1 - alpha_mean) * ml)
    else:
        mo = ((alpha_mean * w0[None, :, None] * m0) + ((1 - alpha_mean) * w[:, :, None] * ml)) / (w0[None, :, None] * alpha_mean + w[:, :, None] * (1 - alpha_mean))
    if occdep and var:
        a = (alpha / (alpha + reg[1]))[:, :, None]
        dm = m0 - ml
        p, q = (cml, c0) if defect == "swap" else (c0, cml)
        co = (1 - a) * p + a * q
        if defect != "drop":
            co = co + (1 - a) * a * dm * dm
    else:
        co = np.broadcast_to(c0, ml.shape)
    if occdep and weight:
        a = alpha / (alpha + reg[2])
        r = a * w + (1 - a) * w0
        wo = r / r.sum(1, keepdims=True)
    else:
        wo = np.broadcast_to(w0, w.shape)
    return mo, co, wo


# ---------------------------------------------------------------- normalizeMixture towards N(0, 1), one iteration
def fusion_ld(w, mean, cov):
    """mixtureFusion in long double: w [C], mean, cov [C, D] -> (tm [D], tc [D])"""
    w, mean, cov = (np.asarray(a, np.float64).astype(LD) for a in (w, mean, cov))
    tm, tc, wt = mean[0].copy(), cov[0].copy(), w[0]
    for i in range(1, len(w)):
        a1 = w[i] / (w[i] + wt)
        a2 = 1 - a1
        d = mean[i] - tm
        tc = a1 * cov[i] + a2 * tc + a1 * a2 * d * d
        tm = a1 * mean[i] + a2 * tm
        wt = w[i] + wt
    return tm, tc


def normalize_ld(w, mean, cov, mean_only=False):
    """one iteration on one model -> (mean', cov' (long double), mean_b, cov_b (float64)); mean_only: cov' = cov, bar 0"""
    C, D = np.shape(mean)
    tm, tc = fusion_ld(w, mean, cov)
    ml, cl = np.asarray(mean, np.float64).astype(LD), np.asarray(cov, np.float64).astype(LD)
    M = np.abs(np.asarray(mean, np.float64)).max(0)
    V = np.asarray(cov, np.float64).max(0) + 4 * M * M
    dtm, dtc = 8 * C * U * M, 12 * C * U * V
    tc64, sd = tc.astype(np.float64), np.sqrt(tc.astype(np.float64))
    nm = (ml - tm) / np.sqrt(tc)
    nm_b = (U * np.abs(ml - tm).astype(np.float64) + dtm) / sd + np.abs(nm).astype(np.float64) * (dtc / (2 * tc64) + 3 * U)
    if mean_only:
        return nm, cl, nm_b, np.zeros((C, D))
    nc = cl / tc
    return nm, nc, nm_b, nc.astype(np.float64) * (dtc / tc64 + 2 * U)


def normalize_np(w, mean, cov, mean_only=False, fp32=False):
    """the kernel's arithmetic in float64 numpy, one iteration (fp32: the fold's variance table rounded to float32)"""
    w, mean, cov = (np.asarray(a, np.float64) for a in (w, mean, cov))
    cv = cov.astype(np.float32).astype(np.float64) if fp32 else cov
    tm, tc, wt = mean[0].copy(), cv[0].copy(), w[0]
    for i in range(1, len(w)):
        a1 = w[i] / (w[i] + wt)
        a2 = 1.0 - a1
        d = mean[i] - tm
        tc = a1 * cv[i] + a2 * tc + a1 * a2 * d * d
        tm = (a1 * mean[i]) + (a2 * tm)
        wt = w[i] + wt
    nm = (mean - tm) / np.sqrt(tc)
    return nm, (cov if mean_only else cov / tc)


class Judge:
    """collects, per result, the largest ratio of an error to its bar and where it is; finish() asserts that none is above 1"""

    def __init__(self, label):
        self.label, self.rows, self.notes = label, [], []

    def __call__(self, name, got, want, bar):
        r = gr.ratio(np.asarray(got).astype(LD) - want, bar)
        worst = float(r.max()) if r.size else 0.0
        where = np.unravel_index(int(np.argmax(r)), r.shape) if r.size else ()
        self.rows.append((name, worst, where))
        return worst

    def same_bits(self, name, got, want):
        if not np.array_equal(np.asarray(got), np.asarray(want)):
            d = np.asarray(got) != np.asarray(want)
            self.notes.append("%s: %d of %d elements differ in their bits" % (name, int(d.sum()), d.size))

    def note(self, text):
        self.notes.append(text)

    def finish(self):
        for name, worst, where in self.rows:
            print("%s | %-34s largest error / bar %.3g at %s" % (self.label, name, worst, where))
        bad = ["%s: %.3g at %s" % r for r in self.rows if not r[1] <= 1.0] + self.notes
        assert not bad, "%s: %s" % (self.label, "; ".join(bad))
