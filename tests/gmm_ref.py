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
