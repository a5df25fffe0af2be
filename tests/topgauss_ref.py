"""Reference, bars and case table for gmmiv_topgauss_compute (k_topgauss_select, lia_ral_amd/csrc/gmm_kernels.hip, on the sorted top
list of gmmiv_llk_determine_top) -- TopGauss::compute of the reference, restated in np.longdouble on gmm_ref.Reference.  Plain
numpy, no GPU.

reference    per frame, with the symbols of gmm_ref (u = 2^-53, rho the error of a logit, B the bar of a log-sum):
                 idx      = the cap largest logits, descending, ties lowest index first           (Reference.top)
                 lk_j     = exp(z_{idx_j}),  bar lkbar_j = rho lk_j + 2^-1074                      (Reference.selected_lk)
                 llk, B   = clamp(Reference.top_llk(idx, complete), lo, hi)       COMPLETE: all Gaussians, PARTIAL: the cap listed
                 tot      = exp(llk),                      bar tot (B + 4u)          (B on the argument, exp and its rounding)
                 cum_j    = lk_1 + .. + lk_j,              bar sum_{i<=j} lkbar_i + j u cum_j          (j additions, in list order)
                 theta    = mass tot,                      bar mass bar(tot) + u theta
                 n_ref    = the smallest n with cum_n > theta, else cap   (the test precedes each addition: the loop stops at the
                            first prefix that has passed); the frame is CAPPED when no prefix passes
                 top_gauss >= 1:  n = (int) top_gauss, nothing is capped
count        n is accepted when it is n_ref, or when the two comparisons that separate it from n_ref lie inside the bars:
                 cum_n + bar(cum_n) > theta - bar(theta)          unless n == cap     (the loop stopped behind n)
                 cum_{n-1} - bar(cum_{n-1}) <= theta + bar(theta)     for n >= 2      (the loop went on behind n - 1)
             A frame accepted at another count than n_ref is AMBIGUOUS, and so is a frame at n_ref = cap whose last comparison
             (capped or not) lies inside the bars.  A condition, not a tolerance: at most 1 % of a case's frames (AMBIGUOUS_SHARE);
             the reference alone has none on these inputs (tests/test_cpu_topgauss_ref.py).
idx          the first n entries by Reference.selection_shortfall -- a selection may differ from the reference's only between
             Gaussians whose logits the kernels cannot tell apart --, inside the model and distinct; entries n .. cap - 1 exactly -1.
             The likelihoods below are the reference's of the Gaussians the library listed.
snsw         1 - sum_{j<n} w[idx_j] in list order, bar (n + 2) u              (every partial result lies in [0, 1])
snsl         max(tot - cum_n, 1e-200), bar bar(tot) + bar(cum_n) + 2u tot, ABSOLUTE: the difference may cancel completely, and a
             bar relative to the result would ask for digits that the operands do not have.  The floor is 1-Lipschitz and keeps
             the bar.  A value below 1e-200 (or NaN) fails whatever the bar: log(snsl) is what TopGauss::get reads.
llk          llk with bar B.
n_capped     the reference's count of capped frames over the frames that are not ambiguous; every ambiguous frame may add one.
zero-likelihood frames (Reference.dead(): a NaN / infinite / absurd feature, or the largest logit not above log 2^-1075) follow the
             rule the code follows today (include/gmmiv.h, "DEGENERATE INPUTS"): llk = lo, lk = 0, idx = 0 .. cap - 1 (cut at n like
             any frame).  In mass mode cum stays 0, so count = cap, the frame IS counted in n_capped, and snsl = exp(lo);
             snsw = 1 - the weights of the Gaussians 0 .. n - 1.
widened      nothing so far: every bar above is the one first derived.
cases        (C, D, T, spread, cap) on gmm_ref.model / gmm_ref.frames.  spread <= 0.5 crowds the Gaussians so that the count varies
             from frame to frame (with spread 2.0 one Gaussian carries every frame of the wider cases); one frame per case
             (PLANT_AT) is replaced by a planted one whose full log-likelihood lies between -745 and lo = -200, so that the
             clamp reaches tot: there tot = exp(lo) is far above every listed likelihood, the frame is capped, snsl = exp(lo).
"""
import functools

import numpy as np

import gmm_ref as gr

LD = gr.LD
U = gr.U
HAVE_LONGDOUBLE = gr.HAVE_LONGDOUBLE
SKIP_MESSAGE = gr.SKIP_MESSAGE
EPS_LK = 1e-200
LO, HI = -200.0, 200.0
AMBIGUOUS_SHARE = 0.01
PLANT_LOGIT = -450.0             # the largest logit of the planted frame: its llk lies in [-450, -450 + log C]

CASES = ((17, 2, 129, 2.0, 16), (33, 16, 257, 0.5, 33), (65, 33, 64, 0.3, 64), (64, 13, 100, 0.3, 64), (512, 60, 200, 0.3, 64),
         (96, 81, 70, 0.3, 40), (1, 1, 17, 2.0, 1))
CAPPED_CASE = (512, 60, 200, 0.3, 64)
MASSES = (0.5, 0.9, 0.999)


def fixed_counts(case):
    return tuple(sorted({1, case[4]}))


def settings(case):
    """every top_gauss of a case: the three masses, then the fixed counts 1 and cap"""
    return MASSES + tuple(float(n) for n in fixed_counts(case))


def case_name(case):
    return "%dx%dx%d s%g cap%d" % case


def plant_at(case):
    return case[2] // 2


def _logits64(w, mean, iv, x):
    D = mean.shape[1]
    a = np.log(w) + 0.5 * np.log(iv).sum(1) - 0.5 * D * gr.LOG_2PI
    d = x[None, :].astype(np.float64) - mean
    return a - 0.5 * (d * d * iv).sum(1)


def planted_frame(case, dtype):
    """a frame of `dtype` whose largest logit is PLANT_LOGIT (+- 1e-2): mu_0 + s v along a fixed direction v, s by bisection (as
    test_gpu_degenerate._frame_at)"""
    w, mean, iv = gr.model(case[:4])
    v = np.random.default_rng(1000 + case[0]).normal(0, 1, case[1]) / np.sqrt(iv[0])
    lo, hi = 0.0, 1e3
    for _ in range(200):
        s = 0.5 * (lo + hi)
        if _logits64(w, mean, iv, (mean[0] + s * v).astype(dtype)).max() > PLANT_LOGIT:
            lo = s
        else:
            hi = s
    x = (mean[0] + lo * v).astype(dtype)
    assert abs(_logits64(w, mean, iv, x).max() - PLANT_LOGIT) < 1e-2
    return x


@functools.lru_cache(maxsize=None)
def _frames(case, dtype_str):
    dtype = np.dtype(dtype_str).type
    x = gr.frames(case[:4], dtype).copy()
    x[plant_at(case)] = planted_frame(case, dtype)
    x.setflags(write=False)
    return x


def frames(case, dtype):
    """the case's frames with the planted one; read-only, shared"""
    return _frames(case, np.dtype(dtype).name)


@functools.lru_cache(maxsize=None)
def reference(case, dtype_str, shift=0):
    """the cached gmm_ref.Reference of the case's model (shift != 0: a client of it) on frames(case); never modified"""
    return gr.Reference(*gr.model(case[:4], shift), frames(case, dtype_str))


class Expected:
    """what TopGauss::compute gives on one Reference: n_ref, capped [T]; llk, B, tot, totbar, theta, thbar [T]; top [T, cap]"""

    def __init__(self, ref, cap, top_gauss, complete=True, lo=LO, hi=HI):
        self.ref, self.cap, self.complete, self.lo = ref, cap, complete, lo
        self.fixed = int(top_gauss) if top_gauss >= 1 else 0
        self.mass = float(top_gauss)
        T = ref.T
        self.dead = ref.dead()
        self.top = np.where(self.dead[:, None], np.arange(cap)[None, :], ref.top(cap))
        with np.errstate(invalid="ignore", over="ignore"):
            raw, rawbar = ref.top_llk(self.top, complete)
            llk, B = gr.clamp(raw, lo, hi, rawbar)
        self.llk = np.where(self.dead, LD(lo), llk)
        self.B = np.where(self.dead, 0.0, B)
        self.tot = np.exp(self.llk)
        self.totbar = self.tot.astype(np.float64) * (self.B + 4 * U)
        self.theta = LD(self.mass) * self.tot
        self.thbar = self.mass * self.totbar + U * self.theta.astype(np.float64)
        cum, _ = self.cumulative(self.top)
        if self.fixed:
            self.n_ref, self.capped = np.full(T, self.fixed), np.zeros(T, bool)
        else:
            passed = cum > self.theta[:, None]
            self.capped = ~passed.any(1)
            self.n_ref = np.where(self.capped, cap, passed.argmax(1) + 1)

    def cumulative(self, idx):
        """cum [T, cap] (long double) and its bar over the listed Gaussians idx (dead frames: zeros, bar 0)"""
        lk, lkbar = self.ref.selected_lk(idx)
        lk = np.where(self.dead[:, None], LD(0), lk)
        lkbar = np.where(self.dead[:, None], 0.0, lkbar)
        cum = np.cumsum(lk, axis=1)
        return cum, np.cumsum(lkbar, axis=1) + np.arange(1, idx.shape[1] + 1)[None, :] * U * cum.astype(np.float64)


def judge(j, e, got, w):
    """hold one call's results (dict idx [T, cap], count, snsw, snsl, llk [T], n_capped) to Expected `e`; w: the model's weights.
    j: an elementwise_judge.Judge.  -> the share of ambiguous frames (None when the structure of the result is already wrong)"""
    ref, cap, T = e.ref, e.cap, e.ref.T
    n = np.asarray(got["count"]).astype(np.int64)
    idx = np.asarray(got["idx"]).astype(np.int64)
    rows = np.arange(T)
    if n.shape != (T,) or idx.shape != (T, cap) or n.min(initial=1) < 1 or n.max(initial=1) > cap:
        j.note("count", "counts outside 1 .. cap: %r .. %r" % (n.min(initial=1), n.max(initial=1)))
        return None
    live = np.arange(cap)[None, :] < n[:, None]
    if not np.all(idx[~live] == -1):
        j.note("idx", "%d entries behind the count are not -1" % int((idx[~live] != -1).sum()))
    sel = np.where(live, idx, -1)
    if sel[live].min() < 0 or sel[live].max() >= ref.C or any(len(set(r[:k])) != k for r, k in zip(sel.tolist(), n.tolist())):
        j.note("idx", "selected indices outside the model or repeated in a row")
        return None
    if not np.array_equal(sel[e.dead], np.where(live, np.arange(cap)[None, :], -1)[e.dead]):
        j.note("idx", "a zero-likelihood frame does not list the Gaussians 0 .. n - 1")
        return None
    full = np.where(live, idx, e.top)                     # behind the count: the reference's own list (never judged)
    short, slack = ref.selection_shortfall(full)
    j("idx", "shortfall", np.where(live & ~e.dead[:, None], gr.ratio(short, slack), 0.0))
    cum, cumbar = e.cumulative(full)
    cum_n, cumbar_n = cum[rows, n - 1], cumbar[rows, n - 1]
    theta, thbar = e.theta, e.thbar
    # ---- count
    if e.fixed:
        ok, amb = n == e.fixed, np.zeros(T, bool)
    else:
        stop = (n == cap) | (cum_n.astype(np.float64) + cumbar_n > (theta.astype(np.float64) - thbar))
        prev = np.maximum(n - 2, 0)
        went = (n < 2) | (cum[rows, prev].astype(np.float64) - cumbar[rows, prev] <= theta.astype(np.float64) + thbar)
        exact = n == e.n_ref
        ok = exact | (stop & went)
        last = np.abs((cum[:, -1] - theta).astype(np.float64)) <= cumbar[:, -1] + thbar
        amb = (ok & ~exact) | (exact & (n == cap) & last)
    j("count", "frames", np.where(ok, 0.0, np.inf))
    share = float(amb.mean()) if T else 0.0
    if share > AMBIGUOUS_SHARE:
        j.note("count", "%d of %d frames are ambiguous, more than %g" % (int(amb.sum()), T, AMBIGUOUS_SHARE))
    # ---- snsw, snsl, llk
    wl = np.asarray(w, np.float64).astype(LD)
    sw = LD(1) - np.where(live, wl[np.where(live, idx, 0)], LD(0)).sum(1)
    j("snsw", "frames", gr.ratio(np.asarray(got["snsw"]).astype(LD) - sw, (n + 2) * U))
    snsl = np.asarray(got["snsl"], np.float64)
    if not np.all(snsl >= EPS_LK):
        j.note("snsl", "%d values below the floor %g (or NaN), first at frame %d: %r"
               % (int((~(snsl >= EPS_LK)).sum()), EPS_LK, int(np.argwhere(~(snsl >= EPS_LK))[0, 0]), float(snsl[~(snsl >= EPS_LK)][0])))
    want = np.maximum(e.tot - cum_n, LD(EPS_LK))
    j("snsl", "frames", gr.ratio(snsl.astype(LD) - want, e.totbar + cumbar_n + 2 * U * e.tot.astype(np.float64)))
    if got.get("llk") is not None:
        j("llk", "frames", gr.ratio(np.asarray(got["llk"]).astype(LD) - e.llk, e.B))
    # ---- n_capped
    if got.get("n_capped") is not None:
        sure = int((e.capped & ~amb).sum())
        if not sure <= got["n_capped"] <= sure + int(amb.sum()):
            j.note("n_capped", "%d, the reference caps %d frames (+ %d ambiguous)" % (got["n_capped"], sure, int(amb.sum())))
    return share


# ---------------------------------------------------------------- a float64 restatement of the library's arithmetic
def restate_compute(w, mean, iv, x, cap, top_gauss, complete=True, lo=LO, hi=HI, defect=None):
    """gmmiv_topgauss_compute in float64 numpy: the logits in the expanded form (gmm_ref.restate) with an unusable feature read as
    1e10, the cap largest per frame (ties lowest index first), lk = exp(z), the log-sum over all Gaussians (COMPLETE) or the listed
    ones (PARTIAL) relative to the largest logit, a frame whose largest logit is not above log 2^-1075 given lo, lk = 0 and the
    list 0 .. cap - 1, the clamp; then k_topgauss_select statement by statement.  -> the dict of capi.Gmm.topgauss_compute.
    defect (tests/test_cpu_topgauss_ref.py): "test_behind_addition" tests the mass behind the addition and before the count, so the
    Gaussian that passes it is not counted; "snsl_not_floored"; "snsw_by_position" subtracts w[j] instead of w[idx_j]."""
    w = np.asarray(w, np.float64)
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        x = np.where(np.abs(x) <= gr.UNUSABLE, x, gr.READ_AS)
    z = gr.restate(w, mean, iv, x)["z"]
    T, C = z.shape
    M = z.max(1)
    dead = ~(M > gr.ZERO_LLK)
    order = np.lexsort((np.broadcast_to(np.arange(C), z.shape), -z), axis=1)[:, :cap]
    order = np.where(dead[:, None], np.arange(cap)[None, :], order)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        zs = np.take_along_axis(z, order, axis=1)
        lk = np.where(dead[:, None], 0.0, np.exp(zs))
        s = np.exp((z if complete else zs) - M[:, None]).sum(1)
        llk = np.where(dead, lo, np.fmin(np.fmax(M + np.log(s), lo), hi))
    fixed = int(top_gauss) if top_gauss >= 1 else 0
    idx = order.astype(np.int32)
    count, snsw, snsl = np.zeros(T, np.int32), np.zeros(T), np.zeros(T)
    n_capped = 0
    for t in range(T):
        lk_tot = np.exp(llk[t])
        n = 0
        if fixed:
            n = fixed
        else:
            val = 0.0
            for jj in range(cap):
                if defect == "test_behind_addition":
                    val += lk[t, jj]
                    if val > top_gauss * lk_tot:
                        break
                    n += 1
                else:
                    if val > top_gauss * lk_tot:
                        break
                    val += lk[t, jj]
                    n += 1
            if n == cap and not val > top_gauss * lk_tot:
                n_capped += 1
        sw, sl = 1.0, lk_tot
        for jj in range(n):
            sw -= w[jj] if defect == "snsw_by_position" else w[idx[t, jj]]
            sl -= lk[t, jj]
        idx[t, n:] = -1
        count[t], snsw[t] = n, sw
        snsl[t] = sl if defect == "snsl_not_floored" or not sl < EPS_LK else EPS_LK
    return dict(idx=idx, count=count, snsw=snsw, snsl=snsl, llk=llk, n_capped=n_capped)
