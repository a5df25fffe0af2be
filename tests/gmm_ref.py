"""Reference, per-pair error bound and case table for the GMM kernels (k_llk_mfma, k_stats_z, k_stats_mfma, k_posteriors, the top-C
family; lia_ral_amd/csrc/gmm_kernels.hip, stats_z.hip, topc_z.hip).  Plain numpy, no GPU.

reference    np.longdouble, log domain, frame by frame, on exactly the doubles / floats handed to the library:
                 z_tc  = log w_c - D/2 log 2pi + 1/2 sum_d log iv_cd - 1/2 sum_d (x_td - mu_cd)^2 iv_cd
                 llk_t = max_c z + log sum_c exp(z - max),      gamma_tc = exp(z_tc - llk_t)
             and the sums  s sum_t gamma_tc [1, x_td, x_td^2]  over any range of frames (Reference.sums).
bound        derived from what the kernels do, per pair (t, c), u = 2^-53.  The MFMA kernels evaluate the expanded form
             a_c + sum x (mu iv) + sum x^2 (-iv/2), a_c = log w + ... - 1/2 sum mu^2 iv summed in D terms (gmm_const_one), and
             exponentiate the raw logit with a one-fma argument reduction that puts <= 1.1e-16 |z| on the argument
             (gexp_tab_reduce, devutil.h):
                 S_tc   = |log w_c| + D/2 log 2pi + 1/2 sum |log iv| + 1/2 sum mu^2 iv + sum |x mu iv| + 1/2 sum x^2 iv
                 rho_tc = (2D + 16) u S_tc              the error of a logit = the relative error of exp(z)
                 B_t    = sum_c gamma_tc rho_tc + 4u |llk_t| + 4u                       the bar of a per-frame log-likelihood
                 |d gamma_tc| <= gamma_tc (rho_tc + B_t + 8u) + phi,   phi = 2^-960     the bar of a posterior
             (phi: the stored-likelihood path keeps exp(z) 2^-E in fp64 against a running exponent, so a posterior some 1000
             binades below its row's largest underflows -- as it does in the linear-domain oracle; with prune_log2 = p, phi = 2^-p).
             A sum of n frames with values v_t in {1, x_td, x_td^2} and weight s:
                 |d| <= |s| sum_t [gamma_tc (rho_tc + B_t + 8u) + phi] |v_t| + (n + 8) u |s| sum_t gamma_tc |v_t|.
             The direct-form kernels (top-C family, vectSize > 80) are inside the same expression: 1/2 sum (x - mu)^2 iv <= 2 S.
             The linear likelihood w_c lk_c of a selected Gaussian gets rho_tc relative.
             The top-C chain in both modes (top_llk, use_top): a log-sum over a SUBSET of the logits -- the selected ones, and in
             COMPLETE mode the world's remainder -- carries the share-weighted rho of the terms in the sum + 4u |llk| + 4u, the
             form of B_t; PARTIAL is that expression without the remainder term.  clamp() is 1-Lipschitz and keeps a bar; a
             value that is NaN (a NaN feature) or -inf (every term 0) becomes exactly lo with bar 0, and a zero-likelihood frame
             (dead(): largest logit not above log 2^-1075) is lo, remainder -inf, selection 0 .. ctop - 1 by definition.
             Derived, not tuned: a float64 numpy restatement of the expanded form (restate) sits well below 1 on every case,
             a dropped term or an fp32 table is orders beyond (tests/test_cpu_gmm_ref.py).
cases        (C, D, T, spread): the smallest shapes at which the structure of the kernels changes -- the KS instantiations 4 / 8 /
             15 / 20 / generic at D <= 16 / 32 / 60 / 80 / above, Gaussian tiles of 16, stages of 32, workgroup groups of 256 (EM)
             and 512 (N / F), 16-frame blocks, 64-frame tiles, 128- and 256-frame workgroups.  In every case at most 1 % of the
             pairs are judged by the floor alone (reference gamma < 2^-900).
the rule     RuleReference: the same reference on frames that hold unusable values, with the zero-likelihood rule of include/gmmiv.h
             applied (a dead frame: llk = lo, posteriors, bars and B exactly 0).  planted(): DEAD_CASES with dead frames of eight kinds
             at 0, T - 1, both sides of the 16 / 64 / 128 / 256 frame boundaries and over the block 32 .. 47, and alive frames at
             largest logit -700 next to them; planted_conditions() asserts what the cases rest on; restate_rule / judge_rule are the
             float64 restatement with the rule and its planted defects (tests/test_cpu_gmm_dead_ref.py,
             tests/test_gpu_gmm_dead_frames.py).
"""
import functools

import numpy as np

import spd_ref
from conftest import make_frames, make_gmm

LD = np.longdouble
HAVE_LONGDOUBLE = spd_ref.HAVE_LONGDOUBLE
SKIP_MESSAGE = spd_ref.SKIP_MESSAGE
U = 2.0 ** -53
PHI = 2.0 ** -960
FLOOR_ONLY = 2.0 ** -900          # a pair whose reference posterior is below this is judged by phi alone
LOG_2PI = float(np.log(2.0 * np.pi))
ZERO_LLK = -745.1332191019412     # log 2^-1075 (GMMIV_ZERO_LLK): a frame whose largest logit is not above it has likelihood 0 in fp64
UNUSABLE, READ_AS = 1e18, 1e10    # a feature that is NaN, infinite or beyond 1e18 in magnitude is read as 1e10 (feat_sane, devutil.h)

CASES = ((1, 1, 17, 2.0), (2, 1, 65, 2.0), (17, 2, 129, 2.0), (16, 13, 16, 2.0), (33, 16, 257, 2.0), (37, 17, 300, 2.0),
         (64, 32, 255, 2.0), (65, 33, 64, 2.0), (129, 60, 256, 2.0), (300, 60, 130, 2.0), (530, 60, 70, 2.0), (2048, 60, 40, 2.0),
         (40, 61, 66, 2.0), (64, 80, 100, 2.0), (512, 60, 200, 0.3), (96, 81, 70, 0.5), (40, 97, 66, 0.5))
PATH_CASES = ((129, 60, 256, 2.0), (300, 60, 130, 2.0), (37, 17, 300, 2.0), (512, 60, 200, 0.3))
BATCH_CASES = ((37, 17, 300, 2.0), (129, 60, 256, 2.0), (40, 97, 66, 0.5))
WIDE_CASE = (129, 60, 256, 2.0)   # also run with the frames as rows of a wider device matrix (ldx > D)
DTYPES = (np.float32, np.float64)


def case_name(case):
    return "%dx%dx%d s%g" % case


def dtype_name(dtype):
    return np.dtype(dtype).name


def model(case, shift=0):
    """the case's mixture; shift != 0: a client of it (means moved by N(0, 0.1), as ComputeTest's adapted models are)"""
    C, D, T, spread = case
    w, mean, iv = make_gmm(C, D, seed=C + D, spread=spread)
    if shift:
        mean = mean + np.random.default_rng(shift).normal(0.0, 0.1, mean.shape)
    return w, mean, iv


def frames(case, dtype):
    C, D, T, spread = case
    w, mean, iv = model(case)
    return make_frames(w, mean, iv, T, seed=T + C, dtype=dtype)


def _ld_pi():
    return LD(4) * np.arctan(LD(1))


def ratio(err, bound):
    """|error| / bound, element by element, in float64; a bound of 0 (an empty sum) admits only an error of 0; NaN -> inf"""
    err = np.abs(np.asarray(err)).astype(LD)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0).astype(LD), np.where(err == 0, LD(0), LD(np.inf)))
    r = r.astype(np.float64)
    return np.where(np.isnan(r), np.inf, r)


class Reference:
    """z, llk, gamma (long double) and S, rho, B, dgamma (float64) of one model on one frame matrix"""

    def __init__(self, w, mean, iv, x, floor=PHI):
        w, mean, iv = (np.ascontiguousarray(a, np.float64) for a in (w, mean, iv))
        assert x.dtype in (np.float32, np.float64)
        self.C, self.D = mean.shape
        self.T = x.shape[0]
        self.x = x.astype(np.float64)                       # exact for float32 frames
        C, D, T = self.C, self.D, self.T
        wl, ml, il, xl = w.astype(LD), mean.astype(LD), iv.astype(LD), x.astype(LD)
        lc = np.log(wl) - LD(D) / 2 * np.log(2 * _ld_pi()) + np.log(il).sum(1) / 2
        self.z = np.empty((T, C), LD)
        for t in range(T):                                  # frame by frame: no T x C x D temporary
            d = xl[t][None, :] - ml
            self.z[t] = lc - np.einsum("cd,cd,cd->c", d, d, il) / 2
        zmax = self.z.max(1, keepdims=True) if C else self.z
        self.llk = (zmax[:, 0] + np.log(np.exp(self.z - zmax).sum(1)))
        self.gamma = np.exp(self.z - self.llk[:, None])
        ax = np.abs(self.x)
        self.S = ((np.abs(np.log(w)) + 0.5 * D * LOG_2PI + 0.5 * np.abs(np.log(iv)).sum(1) + 0.5 * (mean * mean * iv).sum(1))[None, :]
                  + ax @ np.abs(mean * iv).T + 0.5 * (self.x * self.x) @ iv.T)
        self.rho = (2 * D + 16) * U * self.S
        self.g64 = self.gamma.astype(np.float64)            # below 2^-1074: 0, and phi carries the bound
        self.B = (self.g64 * self.rho).sum(1) + 4 * U * np.abs(self.llk.astype(np.float64)) + 4 * U
        self.floor = floor
        self.dgamma = self.g64 * (self.rho + self.B[:, None] + 8 * U) + floor

    def lk(self):
        """w_c lk_c(x_t) = exp(z_tc), linear, long double"""
        return np.exp(self.z)

    def floor_share(self):
        return float((self.gamma < FLOOR_ONLY).mean())

    def sums(self, lo=0, hi=None, s=1.0, keys=("occ", "sx", "sxx")):
        """s sum_{lo <= t < hi} gamma_tc [1, x_td, x_td^2] -> dict occ [C], sx, sxx [C, D] (long double) and occ_b, sx_b, sxx_b
        (float64 bounds)"""
        hi = self.T if hi is None else hi
        n = hi - lo
        g, g64, e, x = self.gamma[lo:hi], self.g64[lo:hi], self.dgamma[lo:hi], self.x[lo:hi]
        xl = x.astype(LD)
        sl, sa = LD(s), abs(s)
        k = (n + 8) * U
        out = {}
        for key, v in (("occ", None), ("sx", xl), ("sxx", xl * xl)):
            if key not in keys:
                continue
            if v is None:
                out["occ"], out["occ_b"] = sl * g.sum(0), sa * (e.sum(0) + k * g64.sum(0))
            else:
                av = np.abs(v).astype(np.float64)
                out[key] = sl * np.einsum("tc,td->cd", g, v)          # (einsum: three times as fast as matmul on long double)
                out[key + "_b"] = sa * (e.T @ av + k * (g64.T @ av))
        return out

    def llk_sum(self, lo=0, hi=None, s=1.0):
        """s sum_t llk_t and its bar |s| sum B_t + (n + 8) u |s| sum |llk_t|"""
        hi = self.T if hi is None else hi
        l = self.llk[lo:hi]
        return LD(s) * l.sum(), abs(s) * (self.B[lo:hi].sum() + (hi - lo + 8) * U * float(np.abs(l).sum()))

    def utt_stats(self, ub):
        """N [U, C], F [U, C, D] (long double) and their bounds for utterances [ub[u], ub[u + 1])"""
        nu = len(ub) - 1
        N, F = np.zeros((nu, self.C), LD), np.zeros((nu, self.C, self.D), LD)
        Nb, Fb = np.zeros((nu, self.C)), np.zeros((nu, self.C, self.D))
        for u in range(nu):
            if ub[u + 1] > ub[u]:
                r = self.sums(int(ub[u]), int(ub[u + 1]), keys=("occ", "sx"))
                N[u], F[u], Nb[u], Fb[u] = r["occ"], r["sx"], r["occ_b"], r["sx_b"]
        return N, F, Nb, Fb

    def count_bar(self, weights):
        """the frame count of an accumulator that holds one call per weight: sum of weights x T, summed in n steps"""
        n = float(sum(weights)) * self.T
        return n, (self.T + 8) * U * n

    def selected_lk(self, idx):
        """w_c lk_c of the selected pairs idx [T, ctop] (long double) and their bar: rho_tc relative, plus one step of the fp64
        denormal grid (a likelihood below the smallest normal double cannot carry a relative error)"""
        lk = np.exp(np.take_along_axis(self.z, idx, axis=1))
        return lk, np.take_along_axis(self.rho, idx, axis=1) * lk.astype(np.float64) + 2.0 ** -1074

    def selection_shortfall(self, idx):
        """how far the logit of the j-th Gaussian selected lies BELOW the j-th largest logit of its frame (0 where it does not), and
        what is allowed: the errors of the two logits compared -- a selection may differ from the reference's only between
        Gaussians the kernels cannot tell apart"""
        want = self.top(idx.shape[1])
        short = np.take_along_axis(self.z, idx, axis=1) - np.take_along_axis(self.z, want, axis=1)
        slack = np.take_along_axis(self.rho, idx, axis=1) + np.take_along_axis(self.rho, want, axis=1)
        return np.minimum(short.astype(np.float64), 0.0), slack

    def top(self, ctop):
        """per frame the ctop largest logits, descending, ties lowest index first: idx [T, ctop]"""
        order = np.lexsort((np.broadcast_to(np.arange(self.C), self.z.shape), -self.z), axis=1)
        return order[:, :ctop]

    def nontop(self, idx, dead=None):
        """log of sum_{c not in idx[t]} exp(z_tc) (-inf when nothing is left) and the share-weighted rho of that sum; dead [T]: the
        zero-likelihood frames (self.dead()), whose remainder is -inf by definition (include/gmmiv.h, "DEGENERATE INPUTS")"""
        mask = np.ones((self.T, self.C), bool)
        np.put_along_axis(mask, idx, False, axis=1)
        if dead is not None:
            mask &= ~dead[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            ln = np.log(np.where(mask, self.gamma, LD(0)).sum(1)) + self.llk
        if dead is not None:
            ln = np.where(dead, LD(-np.inf), ln)
        return ln, mask

    def dead(self):
        """the zero-likelihood frames of include/gmmiv.h: a NaN feature, or the largest logit not above log 2^-1075"""
        with np.errstate(invalid="ignore"):
            return ~(self.z.max(1) > LD(ZERO_LLK)) if self.C else np.ones(self.T, bool)

    def top_llk(self, idx, complete=True):
        """DETERMINE_TOP_DISTRIBS' per-frame value before the clamp and its bar.  COMPLETE: the full log-likelihood, bar B_t.
        PARTIAL: log sum_{c in idx[t]} exp(z_tc), bar = the share-weighted rho of the selected logits + 4u |llk| + 4u."""
        if complete:
            return self.llk, self.B
        z = np.take_along_axis(self.z, idx, axis=1)
        llk = log_sum_exp(z)
        with np.errstate(invalid="ignore"):
            share = np.exp(z - llk[:, None]).astype(np.float64)
            return llk, (share * np.take_along_axis(self.rho, idx, axis=1)).sum(1) + 4 * U * np.abs(llk.astype(np.float64)) + 4 * U


def log_sum_exp(z):
    """log sum_j exp(z[t, j]) in long double; a row of -inf gives -inf, a row with a NaN gives NaN"""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = z.max(1, keepdims=True)
        m = np.where(np.isfinite(m), m, LD(0))
        return m[:, 0] + np.log(np.exp(z - m).sum(1))


def clamp(v, lo, hi, bar=None):
    """fmin(fmax(v, lo), hi) on long double: NaN and -inf give lo.  Clamping is 1-Lipschitz, so a frame's bar does not change under
    it -- except where the value is NaN (a NaN feature) or -inf (every term 0): there the result is lo by definition, bar 0.
    -> clamped values, or (clamped values, bars) when `bar` is given"""
    v = np.asarray(v, LD)
    none = np.isnan(v) | (v == -np.inf)
    with np.errstate(invalid="ignore"):
        c = np.where(none, LD(lo), np.minimum(np.maximum(v, LD(lo)), LD(hi)))
    return c if bar is None else (c, np.where(none, 0.0, np.asarray(bar, np.float64)))


def use_top(client, idx, world_nontop_log, world, mask, complete=True, count=None):
    """USE_TOP_DISTRIBS.  COMPLETE: llk_t = log(sum_{c in idx[t]} exp(z^client_tc) + nontop^world_t) in long double, and its bar:
    the share-weighted logit errors of the terms (the client's for the selected Gaussians, the world's for the remainder, which
    also goes through a log and an exp: 4u |log nontop| more) + 4u |llk| + 4u, as B_t.  PARTIAL (complete=False): the same
    expression without the remainder term, log sum_{c in idx[t]} exp(z^client_tc) and the share-weighted rho of the selected
    logits + 4u |llk| + 4u.  Before the clamp; a frame with a NaN feature comes back NaN (clamp() makes it lo, bar 0).
    count [T] (a stored selection of variable length, TopGauss::get): only the first count[t] entries of idx[t] are terms of the
    sum, what stands behind them (-1) is never read.  world = None: the remainder is a number the caller handed to the library
    (log of a stored snsl), judged from that same double -- it carries no logit error, only the 4u |log nontop| of its log / exp."""
    if count is not None:
        live = np.arange(idx.shape[1])[None, :] < np.asarray(count)[:, None]
        idx = np.where(live, idx, 0)
    zc = np.take_along_axis(client.z, idx, axis=1)
    rc = np.take_along_axis(client.rho, idx, axis=1)
    if count is not None:
        zc, rc = np.where(live, zc, LD(-np.inf)), np.where(live, rc, 0.0)
    if not complete:
        llk = log_sum_exp(zc)
        with np.errstate(invalid="ignore"):
            share = np.exp(zc - llk[:, None]).astype(np.float64)
            return llk, (share * rc).sum(1) + 4 * U * np.abs(llk.astype(np.float64)) + 4 * U
    allz = np.concatenate([zc, world_nontop_log[:, None]], axis=1)
    llk = log_sum_exp(allz)
    with np.errstate(invalid="ignore"):
        share = np.exp(allz - llk[:, None]).astype(np.float64)
    if world is None:
        rn = 0.0
    else:
        tot = np.where(mask, world.g64, 0.0).sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            rn = np.where(tot > 0, (np.where(mask, world.g64 * world.rho, 0.0).sum(1)) / np.where(tot > 0, tot, 1.0), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.where(np.isfinite(world_nontop_log), np.abs(world_nontop_log), LD(0)).astype(np.float64)
    bar = (share[:, :-1] * rc).sum(1) + share[:, -1] * (rn + 4 * U * ln) + 4 * U * np.abs(llk.astype(np.float64)) + 4 * U
    return llk, bar


@functools.lru_cache(maxsize=None)
def reference(case, dtype_str, shift=0, floor=PHI):
    """the cached Reference of a case (dtype_str: numpy dtype name); never modified by its users"""
    w, mean, iv = model(case, shift)
    return Reference(w, mean, iv, frames(case, np.dtype(dtype_str).type), floor)


# ---------------------------------------------------------------- a float64 restatement of the kernels' arithmetic
def restate(w, mean, iv, x, defect=None):
    """The expanded form in float64 numpy, as the MFMA kernels evaluate it: tables mu iv and -iv/2, a_c summed in D terms, logits
    by two products, posteriors exp(z - llk), statistics gamma^T [1 | x | x^2].  -> dict llk [T], gamma [T, C], occ, sx, sxx.
    defect (value-only, for tests/test_cpu_gmm_ref.py): a function (tables dict) -> None called on {"mu_iv", "neg_half_iv"} before
    the logits, or ("gamma", f) with f(gamma) -> gamma called on the posteriors before the statistics."""
    w, mean, iv = (np.asarray(a, np.float64) for a in (w, mean, iv))
    x = x.astype(np.float64)
    C, D = mean.shape
    sl = np.zeros(C)
    sm = np.zeros(C)
    for d in range(D):                                       # gmm_const_one: D terms, in order
        sl += np.log(iv[:, d])
        sm += mean[:, d] * mean[:, d] * iv[:, d]
    a = (np.log(w) - 0.5 * D * 1.8378770664093454836 + 0.5 * sl) - 0.5 * sm
    tab = {"mu_iv": mean * iv, "neg_half_iv": -0.5 * iv}
    if callable(defect):
        defect(tab)
    z = a[None, :] + x @ tab["mu_iv"].T + (x * x) @ tab["neg_half_iv"].T
    zmax = z.max(1, keepdims=True)
    llk = zmax[:, 0] + np.log(np.exp(z - zmax).sum(1))
    gamma = np.exp(z - llk[:, None])
    if isinstance(defect, tuple) and defect[0] == "gamma":
        gamma = defect[1](gamma)
    return {"llk": llk, "gamma": gamma, "occ": gamma.sum(0), "sx": gamma.T @ x, "sxx": gamma.T @ (x * x), "z": z}


def restate_top(world, clients, x, idx, complete=True, lo=-1e9, hi=1e9, defect=None):
    """The top-C chain in float64 numpy, as the kernels evaluate it: the world's logits in the expanded form (restate), its log-sum
    relative to the largest logit over the selected Gaussians plus -- COMPLETE -- the remainder; the clients' selected logits in
    the direct form lwc - 1/2 sum (x - mu)^2 iv, their log-sum with the world's remainder (COMPLETE) or alone (PARTIAL); an
    unusable feature read as 1e10, a frame whose largest world logit is not above log 2^-1075 given lo and remainder -inf; the
    clamp as fmin(fmax(., lo), hi).  clients: a list of (w, mean, iv).  -> (world llk [T], client llk [G, T]).
    defect (tests/test_cpu_trials.py): "drop_small_remainder" leaves the remainder out of a COMPLETE frame where its share is
    below 1e-10; "partial_with_remainder" adds it in PARTIAL mode."""
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        x = np.where(np.abs(x) <= UNUSABLE, x, READ_AS)
    z = restate(*world, x)["z"]
    T, C = z.shape
    M = z.max(1)
    dead = ~(M > ZERO_LLK)
    sel = np.zeros((T, C), bool)
    np.put_along_axis(sel, idx, True, axis=1)
    rest = complete or defect == "partial_with_remainder"
    drop = defect == "drop_small_remainder"
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.exp(z - M[:, None])
        st, srel = np.where(sel, e, 0.0).sum(1), np.where(sel, 0.0, e).sum(1)
        tot = st + srel if rest else st
        if drop:
            tot = np.where(srel < 1e-10 * tot, st, tot)
        wl = np.where(dead, lo, np.fmin(np.fmax(M + np.log(tot), lo), hi))
        nontop = np.where((srel > 0) & ~dead, M + np.log(srel), -np.inf)
        out = []
        for w, mean, iv in clients:
            w, mean, iv = (np.asarray(a, np.float64) for a in (w, mean, iv))
            D = mean.shape[1]
            lwc = np.log(w) - 0.5 * D * 1.8378770664093454836 + 0.5 * np.log(iv).sum(1)
            d = x[:, None, :] - mean[idx]
            zc = lwc[idx] - 0.5 * (d * d * iv[idx]).sum(2)
            allz = np.concatenate([zc, nontop[:, None]], axis=1) if rest else zc
            Mc = allz.max(1)
            ec = np.exp(allz - Mc[:, None])
            s = ec.sum(1)
            if drop and rest:
                s = np.where(ec[:, -1] < 1e-10 * s, ec[:, :-1].sum(1), s)
            out.append(np.fmin(np.fmax(Mc + np.log(s), lo), hi))
    return wl, np.stack(out)


def judge(ref, got, s=1.0):
    """the largest ratio to its bar of every result in `got` (keys llk, gamma, occ, sx, sxx): dict key -> float"""
    out = {}
    if "llk" in got:
        out["llk"] = float(ratio(got["llk"].astype(LD) - ref.llk, ref.B).max())
    if "gamma" in got:
        out["gamma"] = float(ratio(got["gamma"].astype(LD) - ref.gamma, ref.dgamma).max())
    r = ref.sums(s=s)
    for k in ("occ", "sx", "sxx"):
        if k in got:
            out[k] = float(ratio(got[k].astype(LD) - r[k], r[k + "_b"]).max())
    return out


def ragged_bounds(T):
    """utterance bounds in the style of [70, 0, 131, 64, 1], scaled to T frames: an empty utterance, bounds that cut 16-frame
    blocks, a one-frame utterance at the end"""
    if T < 8:
        return np.array([0, 0, T], np.int64) if T < 3 else np.array([0, 1, 1, T - 1, T], np.int64)
    a = max(1, (70 * T) // 266)
    b = a + max(1, (131 * T) // 266)
    return np.array([0, a, a, min(b, T - 2), T - 1, T], np.int64)


# ---------------------------------------------------------------- the zero-likelihood rule (include/gmmiv.h, "DEGENERATE INPUTS")
DEAD_LO, DEAD_HI = -1000.0, 1e9   # the clamp of the dead-frame calls: -1e9 as lo would swamp the bar of a sum of log-likelihoods, -200 would clamp the alive far frames
DEAD_CASES = ((1, 1, 17, 2.0), (2, 1, 65, 2.0), (17, 2, 129, 2.0), (33, 16, 257, 2.0), (37, 17, 300, 2.0), (65, 33, 64, 2.0), (129, 60, 256, 2.0),
              (300, 60, 130, 2.0), (530, 60, 70, 2.0), (40, 61, 66, 2.0), (96, 81, 70, 0.5))
DEAD_PATH_CASES = ((129, 60, 256, 2.0), (37, 17, 300, 2.0), (300, 60, 130, 2.0))
DEAD_CANDIDATES = (-1, 0, 16, 15, 64, 63, 128, 127, 256, 255) + tuple(range(32, 48))    # -1: T - 1; then the whole 16-frame block 32 .. 47
FAR_CANDIDATES = (1, -2, 17, 65)                                                        # -2: T - 2
DEAD_LOGIT, FAR_LOGIT = -800.0, -700.0
KIND_NAMES = ("NaN in one dimension", "+Inf in one dimension", "-Inf in one dimension", "1e30 in one dimension", "-2e18 in the last dimension",
              "every dimension 3e17", "every dimension NaN", "largest logit -800")
KINDS_SCREENED = (0, 1, 2, 3, 4, 6)     # kind (1) of the header: an unusable value; the other two are kind (2), finite and usable
assert all(c in CASES for c in DEAD_CASES) and all(c in DEAD_CASES for c in DEAD_PATH_CASES)


class RuleReference(Reference):
    """Reference on frames that may hold unusable values, with the zero-likelihood rule applied: a value that is NaN, infinite or
    beyond UNUSABLE in magnitude is read as READ_AS; a frame that had one, or whose largest logit is not above ZERO_LLK, is dead():
    gamma, g64, dgamma exactly 0 (bar 0: only 0 passes), B 0, llk = lo.  sums() and utt_stats() then leave the dead frames out with no
    further code.  The two things the header counts differently: gmmiv_llk's sums count EVERY frame, the dead ones with lo
    (llk_sum(every=True)); gmmiv_em_accumulate's llk and count, the N / F rows and seg_llk count the ALIVE frames only (llk_sum(),
    count_bar(), alive_count())."""

    def __init__(self, w, mean, iv, x, floor=PHI, lo=DEAD_LO):
        with np.errstate(invalid="ignore"):
            unusable = ~(np.abs(x) <= UNUSABLE)             # a NaN compares false: unusable
        super().__init__(w, mean, iv, np.where(unusable, x.dtype.type(READ_AS), x), floor)
        self.unusable = unusable.any(1)                     # kind (1): what "screened_frames" counts
        self.lo = lo
        d = self._dead = self.unusable | Reference.dead(self)
        self.gamma[d], self.g64[d], self.dgamma[d], self.B[d], self.llk[d] = 0, 0.0, 0.0, 0.0, lo

    def dead(self):
        return self._dead

    def alive_count(self, lo=0, hi=None):
        return int((~self._dead[lo:self.T if hi is None else hi]).sum())

    def llk_sum(self, lo=0, hi=None, s=1.0, every=False):
        """s sum_t llk_t over the alive frames -- with every=True over all frames, a dead one entering with self.lo -- and its bar, the
        one of Reference.llk_sum (B_t is 0 on a dead frame; the summation term counts every step of the range)"""
        hi = self.T if hi is None else hi
        l = self.llk[lo:hi] if every else np.where(self._dead[lo:hi], LD(0), self.llk[lo:hi])
        return LD(s) * l.sum(), abs(s) * (self.B[lo:hi].sum() + (hi - lo + 8) * U * float(np.abs(l).sum()))

    def count_bar(self, weights):
        n = float(sum(weights)) * self.alive_count()
        return n, (self.T + 8) * U * n


def largest_logit(w, mean, iv, x):
    """the largest logit of every frame in float64, direct form (for placing a frame: +- 1e-2 is asked of it)"""
    x = np.asarray(x, np.float64)
    a = np.log(w) + 0.5 * np.log(iv).sum(1) - 0.5 * mean.shape[1] * LOG_2PI
    d = x[:, None, :] - mean[None]
    return (a[None] - 0.5 * np.einsum("tcd,tcd,cd->tc", d, d, iv)).max(1)


def frame_at(w, mean, iv, c0, target, seed, dtype):
    """a frame mean[c0] + s u of `dtype` whose LARGEST logit is `target` (+- 1e-2): u a random direction scaled by the Gaussian's
    standard deviations, s by bisection (the method of _frame_at in tests/test_gpu_degenerate.py)"""
    u = np.random.default_rng(seed).normal(0.0, 1.0, mean.shape[1]) / np.sqrt(iv[c0])
    at = lambda s: float(largest_logit(w, mean, iv, (mean[c0] + s * u).astype(dtype)[None])[0])
    lo, hi = 0.0, 1e3
    while at(hi) > target:
        hi *= 2.0
    assert at(lo) > target
    for _ in range(200):
        s = 0.5 * (lo + hi)
        lo, hi = (s, hi) if at(s) > target else (lo, s)
    xf = (mean[c0] + lo * u).astype(dtype)
    assert abs(at(lo) - target) < 1e-2, (c0, target, at(lo))
    return xf


def _positions(T, candidates):
    out = []
    for p in candidates:
        p = p + T if p < 0 else p
        if 0 <= p < T and p not in out:
            out.append(p)
    return out


@functools.lru_cache(maxsize=None)
def planted(case, dtype_str):
    """frames(case, dtype) with dead and alive far frames planted -> dict x [T, D] (read-only), dead (positions, in planting order),
    kind (position -> index into KIND_NAMES), far (positions of the alive far frames).
    Dead: the first max(1, T // 3) of DEAD_CANDIDATES that lie inside the call, the i-th of kind i mod 8.  Far: up to two of
    FAR_CANDIDATES that are free, built like kind 7 at FAR_LOGIT."""
    C, D, T, _ = case
    dtype = np.dtype(dtype_str).type
    w, mean, iv = model(case)
    x = frames(case, dtype).copy()
    dead = _positions(T, DEAD_CANDIDATES)[:max(1, T // 3)]
    kind = {}
    for i, t in enumerate(dead):
        k = kind[t] = i % 8
        d = (7 * t) % D
        if k < 4:
            x[t, d] = (np.nan, np.inf, -np.inf, 1e30)[k]
        elif k == 4:
            x[t, D - 1] = -2e18
        elif k == 5:
            x[t, :] = 3e17
        elif k == 6:
            x[t, :] = np.nan
        else:
            x[t] = frame_at(w, mean, iv, t % C, DEAD_LOGIT, 1000 + t, dtype)
    far = [t for t in _positions(T, FAR_CANDIDATES) if t not in dead][:2]
    for t in far:
        x[t] = frame_at(w, mean, iv, t % C, FAR_LOGIT, 2000 + t, dtype)
    x.setflags(write=False)
    return {"x": x, "dead": tuple(dead), "kind": kind, "far": tuple(far)}


@functools.lru_cache(maxsize=None)
def rule_reference(case, dtype_str, shift=0, floor=PHI):
    """the cached RuleReference of model(case, shift) on the planted frames; never modified by its users"""
    return RuleReference(*model(case, shift), planted(case, dtype_str)["x"], floor)


def planted_conditions(case, dtype_str, shifts=(0,)):
    """what the planted cases rest on, asserted from the references alone -> dict of the figures.  The planted set is dead() under the
    world model; under EVERY model that reads the frames (shifts) no largest logit lies within 20 of ZERO_LLK and the dead set is the
    same; at least half of the frames are ordinary; at most 1 % of the pairs of ordinary frames are judged by the floor alone; every
    alive far frame has its largest posterior under a bar above the floor."""
    p = planted(case, dtype_str)
    T = case[2]
    planted_mask = np.zeros(T, bool)
    planted_mask[list(p["dead"])] = True
    out = {"dead": len(p["dead"]), "far": len(p["far"]), "margin": np.inf}
    for s in shifts:
        r = rule_reference(case, dtype_str, s)
        assert np.array_equal(r.dead(), planted_mask), (case, dtype_str, s, np.flatnonzero(r.dead() != planted_mask))
        margin = float(np.abs(r.z.max(1).astype(np.float64) - ZERO_LLK).min())
        assert margin > 20.0, (case, dtype_str, s, margin)
        out["margin"] = min(out["margin"], margin)
    r = rule_reference(case, dtype_str)
    screened = sorted(t for t, k in p["kind"].items() if k in KINDS_SCREENED)
    assert np.flatnonzero(r.unusable).tolist() == screened, (case, dtype_str)
    ordinary = ~planted_mask
    ordinary[list(p["far"])] = False
    out["ordinary"] = int(ordinary.sum())
    assert 2 * out["ordinary"] >= T, (case, out)
    out["floor_share"] = float((r.gamma[ordinary] < FLOOR_ONLY).mean())
    assert out["floor_share"] <= 0.01, (case, dtype_str, out)
    zmax = r.z.max(1).astype(np.float64)
    for t in p["far"]:
        c = int(np.argmax(r.gamma[t]))
        assert abs(zmax[t] - FAR_LOGIT) < 1e-2 and r.g64[t, c] > 0.5 and r.dgamma[t, c] > 2 * r.floor, (case, dtype_str, t, zmax[t], r.g64[t, c])
    for t, k in p["kind"].items():
        assert k != 7 or abs(zmax[t] - DEAD_LOGIT) < 1e-2, (case, dtype_str, t, zmax[t])
    return out


def dead_layouts(T):
    """utterance bounds for the planted cases: (a) one frame per utterance -- every dead frame a zero row of N and F; (b)
    ragged_bounds with one more bound at 40, inside the dead 16-frame block 32 .. 47; (c) one utterance"""
    b = ragged_bounds(T)
    if T > 41:
        b = np.sort(np.append(b, 40))
    return (("a", np.arange(T + 1, dtype=np.int64)), ("b", b.astype(np.int64)), ("c", np.array([0, T], np.int64)))


RULE_DEFECTS = ("uniform posterior on a dead frame", "lo of a dead frame in the EM llk sum", "dead frame in the EM frame count",
                "unusable value read as 0, frame kept alive", "-700 frame dropped as dead", "-800 frame kept alive",
                "dead frame keeps the reference's top list")


def restate_rule(w, mean, iv, x, ctop, lo=DEAD_LO, defect=None):
    """restate() with the rule applied as the kernels apply it, float64: unusable values read as READ_AS, a frame dead where its
    largest logit is not above ZERO_LLK (a frame read at 1e10 is one by its logits), dead rows of zero posteriors, llk = lo,
    idx = 0 .. ctop - 1.  -> dict llk, gamma, occ, sx, sxx, z, dead, em_llk, em_count (alive frames), llk_every (all frames), idx.
    defect: one of RULE_DEFECTS (tests/test_cpu_gmm_dead_ref.py)."""
    assert defect is None or defect in RULE_DEFECTS
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        x = np.where(np.abs(x) <= UNUSABLE, x, 0.0 if defect == RULE_DEFECTS[3] else READ_AS)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        r = restate(w, mean, iv, x)
    zmax = r["z"].max(1)
    cut = {RULE_DEFECTS[4]: -650.0, RULE_DEFECTS[5]: -850.0}.get(defect, ZERO_LLK)
    dead = ~(zmax > cut)
    C = r["z"].shape[1]
    gamma = np.where(dead[:, None], 1.0 / C if defect == RULE_DEFECTS[0] else 0.0, r["gamma"])
    llk = np.where(dead, lo, r["llk"])
    order = np.argsort(-r["z"], axis=1, kind="stable")[:, :ctop]
    idx = order if defect == RULE_DEFECTS[6] else np.where(dead[:, None], np.arange(ctop)[None, :], order)
    return {"llk": llk, "gamma": gamma, "occ": gamma.sum(0), "sx": gamma.T @ x, "sxx": gamma.T @ (x * x), "z": r["z"], "dead": dead, "idx": idx,
            "em_llk": (llk if defect == RULE_DEFECTS[1] else llk[~dead]).sum(), "em_count": float(len(llk) if defect == RULE_DEFECTS[2] else (~dead).sum()),
            "llk_every": llk.sum()}


def judge_rule(ref, got):
    """the largest ratio to its bar of everything the dead-frame module judges on the single-model entry points, for a restatement
    `got` (restate_rule): dict name -> float.  "idx dead" is 0 or inf: a dead frame selects 0 .. ctop - 1."""
    out = judge(ref, got)
    s, sb = ref.llk_sum()
    out["em llk"] = float(ratio(np.array([got["em_llk"]]).astype(LD) - s, sb).max())
    n, nb = ref.count_bar((1.0,))
    out["em count"] = float(ratio(np.array([got["em_count"] - n]), nb).max())
    s, sb = ref.llk_sum(every=True)
    out["llk sums"] = float(ratio(np.array([got["llk_every"]]).astype(LD) - s, sb).max())
    d = ref.dead()
    ctop = got["idx"].shape[1]
    out["idx dead"] = 0.0 if np.array_equal(got["idx"][d], np.broadcast_to(np.arange(ctop), (int(d.sum()), ctop))) else np.inf
    short, slack = ref.selection_shortfall(np.where(d[:, None], ref.top(ctop), got["idx"]))
    out["idx alive"] = float(ratio(np.where(d[:, None], 0.0, short), slack).max())
    x = ref.x
    for name, ub in dead_layouts(ref.T):
        N, F, Nb, Fb = ref.utt_stats(ub)
        seg = np.add.reduceat(got["gamma"], ub[:-1][np.diff(ub) > 0], axis=0)
        out["tv(%s) N" % name] = float(ratio(seg.astype(LD) - N[np.diff(ub) > 0], Nb[np.diff(ub) > 0]).max())
        if name != "a":
            Fg = np.stack([got["gamma"][ub[u]:ub[u + 1]].T @ x[ub[u]:ub[u + 1]] for u in range(len(ub) - 1)])
            out["tv(%s) F" % name] = float(ratio(Fg.astype(LD) - F, Fb).max())
    return out


def clamp_below(v, bar, lo, hi):
    """clamp() with bars, and: a value that lies below lo by more than its bar is lo whatever the admitted error, so its bar is 0
    (a frame read at 1e10 has a log-sum near -1e19 with a bar of thousands; its clamped value is exactly lo)"""
    c, b = clamp(v, lo, hi, bar)
    with np.errstate(invalid="ignore"):
        sure = np.asarray(v, LD) + b < LD(lo)
    return c, np.where(sure, 0.0, b)
