// capi_tv.hip -- C ABI (include/gmmiv.h): total-variability (i-vector) and JFA steps, the approximate extractors, orthonormalize_t.
// I-vector normalisation and scoring: capi_iv_score.hip; the PldaDev / PLDA back end: capi_backend.hip.
#include <string.h>

#include "capi_tv_util.h"
#include "host_linalg.h"

int fetch_host(gmmiv_ctx *c, const double *p, size_t n, std::vector<double> &out)
{
    out.resize(n);
    if (n == 0 || !p) return GMMIV_OK;
    if (gmmiv_is_device_ptr(p)) {
        GCHK(hipMemcpyAsync(out.data(), p, n * 8, hipMemcpyDeviceToHost, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
    } else memcpy(out.data(), p, n * 8);
    return GMMIV_OK;
}
int store_out(gmmiv_ctx *c, double *p, const std::vector<double> &v)
{
    if (!p) return GMMIV_OK;
    if (gmmiv_is_device_ptr(p)) {
        GCHK(hipMemcpyAsync(p, v.data(), v.size() * 8, hipMemcpyHostToDevice, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
    } else memcpy(p, v.data(), v.size() * 8);
    return GMMIV_OK;
}

extern "C" {

size_t gmmiv_tv_packed_len(int R) { return (size_t)R * (R + 1) / 2; }

int gmmiv_tv_subtract_m(gmmiv_ctx *c, int64_t U, int C, int D, const double *N, double *F, const double *means)
{
    if (!c || U < 0 || C <= 0 || D <= 0 || !N || !F || !means) { gmmiv_set_error("tv_subtract_m: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D;
    DevIn<double> i_n, i_m;
    DevOut<double> o_f;
    int rc;
    if ((rc = i_n.init(c, WS_T0, N, (size_t)U * C)) || (rc = i_m.init(c, WS_T1, means, SV)) || (rc = o_f.init(c, WS_T2, F, (size_t)U * SV, true))) return rc;
    c->t_begin("k_subtract_m");
    GCHK(tvk_subtract_m(c->stream, U, C, D, i_n.d, o_f.d, i_m.d));
    c->t_end();
    return o_f.finish();
}

// F_dst = F_src - N ubm_means: restoreStats + substractM of a TotalVariability iteration in one pass over the statistics
int gmmiv_tv_subtract_m_to(gmmiv_ctx *c, int64_t U, int C, int D, const double *N, const double *F_src, double *F_dst, const double *means)
{
    if (!c || U < 0 || C <= 0 || D <= 0 || !N || !F_src || !F_dst || !means) { gmmiv_set_error("tv_subtract_m_to: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D;
    DevIn<double> i_n, i_m, i_f;
    DevOut<double> o_f;
    int rc;
    if ((rc = i_n.init(c, WS_T0, N, (size_t)U * C)) || (rc = i_m.init(c, WS_T1, means, SV)) || (rc = i_f.init(c, WS_T3, F_src, (size_t)U * SV)) ||
        (rc = o_f.init(c, WS_T2, F_dst, (size_t)U * SV, false))) return rc;
    c->t_begin("k_subtract_m");
    int krc = tvk_subtract_m_to(c->stream, U, C, D, i_n.d, i_f.d, o_f.d, i_m.d);
    if (krc < 0) { // odd vectSize or unaligned rows: copy, then the in-place kernel
        if (o_f.d != i_f.d) GCHK(hipMemcpyAsync(o_f.d, i_f.d, (size_t)U * SV * 8, hipMemcpyDeviceToDevice, c->stream));
        krc = tvk_subtract_m(c->stream, U, C, D, i_n.d, o_f.d, i_m.d);
    }
    GCHK(krc);
    c->t_end();
    return o_f.finish();
}

int gmmiv_tv_tett(gmmiv_ctx *c, int C, int D, int R, const double *Tm, const double *invvar, double *tett_packed)
{
    if (!c || C <= 0 || D <= 0 || R <= 0 || !Tm || !invvar || !tett_packed) { gmmiv_set_error("tv_tett: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D, P = gmmiv_tv_packed_len(R), RR = (size_t)R * R;
    DevIn<double> i_t, i_iv;
    DevOut<double> o;
    int rc;
    if ((rc = i_t.init(c, WS_T0, Tm, (size_t)R * SV)) || (rc = i_iv.init(c, WS_T1, invvar, SV)) ||
        (rc = o.init(c, WS_T2, tett_packed, (size_t)C * P, false))) return rc;
    if (c->tv_tett_direct) { // one kernel: lower triangle only, written packed (tv_kernels.hip: k_tett_packed); D <= 64
        c->t_begin("k_tett_packed");
        const int krc = tvk_tett_packed(c->stream, C, D, R, i_t.d, i_iv.d, o.d);
        c->t_end();
        if (krc == 0) return o.finish();
        if (krc != -1) GCHK(krc);
    }
    void *p;
    if ((rc = c->scratch(WS_T3, (size_t)R * SV * 8, &p))) return rc;
    double *Tiv = (double *)p;
    GCHK(tvk_scale_cols(c->stream, R, (long)SV, i_t.d, i_iv.d, Tiv));
    const int CH = 128;
    if ((rc = c->scratch(WS_T4, (size_t)CH * RR * 8, &p))) return rc;
    double *G = (double *)p;
    c->t_begin("k_dgemm(tett)");
    for (int c0 = 0; c0 < C; c0 += CH) {
        const int nb = (C - c0) < CH ? (C - c0) : CH;
        GCHK(tvk_dgemm(c->stream, false, true, R, R, D, 1.0, i_t.d + (size_t)c0 * D, (long)SV, D, Tiv + (size_t)c0 * D, (long)SV, D,
                       0.0, G, R, (long)RR, nb));
        GCHK(tvk_pack_sym(c->stream, R, nb, G, (long)RR, nullptr, o.d + (size_t)c0 * P, (long)P));
    }
    c->t_end();
    return o.finish();
}

// shared body of estimateW / estimateAandC
static int tv_estep(gmmiv_ctx *c, int64_t U, int C, int D, int R, const double *N, const double *F, const double *Tm,
                    const double *invvar, const double *tett, double *W, double *A_packed, double *Cmx, double *Rm,
                    double *r, double *meanW, bool accumulate)
{
    GBIND(c);
    const size_t SV = (size_t)C * D, P = gmmiv_tv_packed_len(R), RR = (size_t)R * R;
    int rc;
    DevIn<double> i_n, i_f, i_t, i_iv, i_te;
    DevOut<double> o_w;
    if ((rc = i_n.init(c, WS_T0, N, (size_t)U * C)) || (rc = i_f.init(c, WS_T1, F, (size_t)U * SV)) || (rc = i_t.init(c, WS_T2, Tm, (size_t)R * SV)) ||
        (rc = i_iv.init(c, WS_PART, invvar, SV)) || (rc = i_te.init(c, WS_X, tett, (size_t)C * P)) ||
        (rc = o_w.init(c, WS_LSE, W, (size_t)U * R, false))) return rc;
    // accumulators: keep device-side copies when the caller passed host arrays
    void *p;
    double *d_a = nullptr, *d_c = nullptr, *d_rm = nullptr, *d_r = nullptr, *d_mw = nullptr, *d_rp = nullptr;
    // device copies of HOST accumulators live for this call only; the guard frees them on EVERY return path
    struct Owned {
        gmmiv_ctx *c;
        std::vector<void *> v;
        ~Owned() { if (v.empty()) return; (void)hipStreamSynchronize(c->stream); for (void *q : v) (void)hipFree(q); }
    } owned{c, {}};
    auto dev_acc = [&](double *user, size_t n, double **dev) -> int {
        if (gmmiv_is_device_ptr(user)) { *dev = user; return GMMIV_OK; }
        GCHK(hipMalloc(&p, n * 8));
        owned.v.push_back(p);
        GCHK(hipMemcpyAsync(p, user, n * 8, hipMemcpyHostToDevice, c->stream));
        *dev = (double *)p;
        return GMMIV_OK;
    };
    if (accumulate) {
        if ((rc = dev_acc(A_packed, (size_t)C * P, &d_a)) || (rc = dev_acc(Cmx, (size_t)R * SV, &d_c)) ||
            (rc = dev_acc(Rm, RR, &d_rm)) || (rc = dev_acc(r, R, &d_r)) || (rc = dev_acc(meanW, R, &d_mw))) return rc;
        GCHK(hipMalloc(&p, P * 8));
        owned.v.push_back(p);
        d_rp = (double *)p;
        GCHK(hipMemsetAsync(d_rp, 0, P * 8, c->stream));
    }
    if ((rc = c->scratch(WS_TIV, (size_t)R * SV * 8, &p))) return rc;
    double *Tiv = (double *)p;
    GCHK(tvk_scale_cols(c->stream, R, (long)SV, i_t.d, i_iv.d, Tiv));

    const int BC = tv_batch_size(c, U, 0);
    // T-matrix EM: the E_u of a SUPER-BATCH of utterances stay in HBM (tv_acc_mb, default 8 GiB = 13 k utterances at rank 400) and
    // A += N^T E, Cmx += W^T F run ONCE per super-batch with K = its utterance count, instead of once per tv_batch with the 1.3 GB
    // accumulator read and written back every time (config 4's 6250 utterances per rank: 7 x 5.1 ms -> 30 ms for A alone).
    int64_t SB = BC;
    if (accumulate) {
        const int64_t fit = ((int64_t)(c->tv_acc_mb > 0 ? c->tv_acc_mb : 0) << 20) / (int64_t)(P * 8);
        SB = fit / BC * BC;
        if (SB < BC) SB = BC;
        if (SB > U) SB = (U + BC - 1) / BC * BC;
    }
    if ((rc = c->scratch(WS_LP, (size_t)SB * P * 8, &p))) return rc;
    double *Lp0 = (double *)p;
    if ((rc = c->scratch(WS_AUX, (size_t)BC * R * 8, &p))) return rc;
    double *aux = (double *)p;
    // the split-K slabs of aux are reserved here, not by splitk_gemm: the same buffer also takes the partial sums of sum_u E_u and
    // of sum_u w_u, and its pointer is taken once for the whole call
    const int nz = tvk_splitk_count(BC, R, (int)SV, c->n_cu);
    size_t slab_doubles = (size_t)nz * BC * R;
    if (accumulate && slab_doubles < (size_t)TVK_BATCH_SUM_SLABS * P) slab_doubles = (size_t)TVK_BATCH_SUM_SLABS * P;
    if (accumulate && slab_doubles < TVK_NARROW_SLABS_DOUBLES(R)) slab_doubles = TVK_NARROW_SLABS_DOUBLES(R);
    if ((rc = c->scratch(WS_SLAB, slab_doubles * 8, &p))) return rc;
    double *slabs = (double *)p;
    SpdBatch ws;
    if ((rc = ws.reserve(c, R, BC))) return rc;

    for (int64_t s0 = 0; s0 < U; s0 += SB) {
        const int64_t ns = (U - s0) < SB ? (U - s0) : SB; // utterances of this super-batch
        for (int64_t u0 = s0; u0 < s0 + ns; u0 += BC) {
            const int nb = (int)((s0 + ns - u0) < BC ? (s0 + ns - u0) : BC);
            const double *Nc = i_n.d + (size_t)u0 * C;
            const double *Fc = i_f.d + (size_t)u0 * SV;
            double *Wc = o_w.d + (size_t)u0 * R;
            double *Lp = Lp0 + (size_t)(u0 - s0) * P;
            if ((rc = ws.begin(nb))) return rc;
            // L (packed) = N * TETt ; + I when it is read
            c->t_begin("k_dgemm(L)", u0 == 0); // one event pair per batch of the call, not the last batch alone
            GCHK(tvk_dgemm(c->stream, false, false, nb, (int)P, C, 1.0, Nc, C, 0, i_te.d, (long)P, 0, 0.0, Lp, (long)P, 0, 1));
            c->t_end();
            if ((rc = ws.from_packed(Lp, (long)P, 1.0))) return rc;
            // aux = F Sigma^-1 T^T
            GCHK(tvk_dgemm_splitk(c->stream, false, true, nb, R, (int)SV, 1.0, Fc, (long)SV, Tiv, (long)SV, 0.0, aux, R, nz, slabs));
            if (accumulate) { // the T-matrix EM needs L^-1 itself: E = L^-1 + w w^T, packed, in the super-batch buffer
                if ((rc = ws.inverse_e(aux, Wc, Lp, (long)P, "tv: L"))) return rc;
            } else {          // extraction only needs w = L^-1 aux: Cholesky + two triangular solves
                if ((rc = ws.factor()) || (rc = ws.solve(aux, Wc)) || (rc = ws.check("tv: L"))) return rc;
            }
        }
        if (accumulate) {
            // A += N^T E ; Cmx += W^T F ; R += sum E ; r, meanW += sum w    over the ns utterances of the super-batch
            const double *Ns = i_n.d + (size_t)s0 * C, *Fs = i_f.d + (size_t)s0 * SV, *Ws = o_w.d + (size_t)s0 * R;
            GCHK(tvk_dgemm(c->stream, true, false, C, (int)P, (int)ns, 1.0, Ns, C, 0, Lp0, (long)P, 0, 1.0, d_a, (long)P, 0, 1));
            // A is complete once the last super-batch's GEMM is enqueued: a caller that shards the M-step starts its exchange here,
            // under the Cmx GEMM and the batch sums below (gmmiv_ctx_set_hook "tv_a_ready"; device accumulators only)
            if (s0 + SB >= U && d_a == A_packed) { c->hook_tv_a_ready.call(); GBIND(c); } // the hook may have driven another context on this thread: bind ours again
            GCHK(tvk_dgemm(c->stream, true, false, R, (int)SV, (int)ns, 1.0, Ws, R, 0, Fs, (long)SV, 0, 1.0, d_c, (long)SV, 0, 1));
            GCHK(tvk_batch_sum(c->stream, (long)P, (int)ns, Lp0, (long)P, d_rp, slabs)); // slabs (split-K workspace of aux) is free again
            GCHK(tvk_colsum_narrow(c->stream, R, (int)ns, Ws, R, d_r, d_mw, slabs)); // r and meanW both accumulate sum_u w_u; slabs is free again (stream order)
        }
    }
    if (accumulate) {
        GCHK(tvk_add_unpacked(c->stream, R, d_rp, d_rm));
        auto back = [&](double *user, double *dev, size_t n) -> int {
            if (dev != user) GCHK(hipMemcpyAsync(user, dev, n * 8, hipMemcpyDeviceToHost, c->stream));
            return GMMIV_OK;
        };
        if ((rc = back(A_packed, d_a, (size_t)C * P)) || (rc = back(Cmx, d_c, (size_t)R * SV)) || (rc = back(Rm, d_rm, RR)) ||
            (rc = back(r, d_r, R)) || (rc = back(meanW, d_mw, R))) return rc;
    }
    return o_w.finish(); // `owned` releases the device copies after this: synchronise, then free, as before
}

int gmmiv_tv_estimate_w(gmmiv_ctx *c, int64_t U, int C, int D, int R, const double *N, const double *F, const double *Tm,
                        const double *invvar, const double *tett_packed, double *W)
{
    if (!c || U < 0 || C <= 0 || D <= 0 || R <= 0 || !N || !F || !Tm || !invvar || !tett_packed || !W) { gmmiv_set_error("tv_estimate_w: bad argument"); return GMMIV_ERR_ARG; }
    if (U == 0) return GMMIV_OK;
    return tv_estep(c, U, C, D, R, N, F, Tm, invvar, tett_packed, W, nullptr, nullptr, nullptr, nullptr, nullptr, false);
}

int gmmiv_tv_estimate_a_and_c(gmmiv_ctx *c, int64_t U, int C, int D, int R, const double *N, const double *F,
                              const double *Tm, const double *invvar, const double *tett_packed, double *W,
                              double *A_packed, double *Cmx, double *Rm, double *r, double *meanW)
{
    if (!c || U < 0 || C <= 0 || D <= 0 || R <= 0 || !N || !F || !Tm || !invvar || !tett_packed || !W || !A_packed || !Cmx || !Rm || !r || !meanW) { gmmiv_set_error("tv_estimate_a_and_c: bad argument"); return GMMIV_ERR_ARG; }
    if (U == 0) return GMMIV_OK;
    return tv_estep(c, U, C, D, R, N, F, Tm, invvar, tett_packed, W, A_packed, Cmx, Rm, r, meanW, true);
}

int gmmiv_tv_update_t(gmmiv_ctx *c, int C, int D, int R, const double *A_packed, const double *Cmx, double *Tm)
{
    if (!c || C <= 0 || D <= 0 || R <= 0 || !A_packed || !Cmx || !Tm) { gmmiv_set_error("tv_update_t: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D, P = gmmiv_tv_packed_len(R), RR = (size_t)R * R;
    int rc;
    DevIn<double> i_a, i_c;
    DevOut<double> o_t;
    if ((rc = i_a.init(c, WS_T0, A_packed, (size_t)C * P)) || (rc = i_c.init(c, WS_T1, Cmx, (size_t)R * SV)) ||
        (rc = o_t.init(c, WS_T2, Tm, (size_t)R * SV, false))) return rc;
    int CH = c->n_cu > 128 ? c->n_cu : 128; // one workgroup per matrix in the batched inverse: a batch fills the chip
    if (C < CH) CH = C;
    SpdBatch ws;
    if ((rc = ws.reserve(c, R, CH))) return rc;
    for (int c0 = 0; c0 < C; c0 += CH) {
        const int nb = (C - c0) < CH ? (C - c0) : CH;
        if ((rc = ws.begin(nb)) || (rc = ws.from_packed(i_a.d + (size_t)c0 * P, (long)P, 0.0))) return rc;
        if (ws.left() && D <= 64 && c->tv_mstep_solve) {
            // T_c = A_c^-1 Cmx_c by substitution through the Cholesky factor: 60 right-hand sides per Gaussian, no explicit inverse
            // (the reference inverts, :981-1000 -- same result to rounding, a third of the work)
            if ((rc = ws.factor()) ||
                (rc = ws.solve_multi(D, i_c.d + (size_t)c0 * D, (long)SV, D, o_t.d + (size_t)c0 * D, (long)SV, D))) return rc;
        } else {
            if ((rc = ws.inverse(ws.inv))) return rc;
            // T_c = A_c^-1 Cmx_c
            GCHK(tvk_dgemm(c->stream, false, false, R, D, R, 1.0, ws.inv, R, (long)RR, i_c.d + (size_t)c0 * D, (long)SV, D, 0.0,
                           o_t.d + (size_t)c0 * D, (long)SV, D, nb));
        }
        if ((rc = ws.check("tv_update_t: A_c"))) return rc;
    }
    return o_t.finish();
}

int gmmiv_tv_min_divergence(gmmiv_ctx *c, int C, int D, int R, double n_sessions, double *Rm, double *r,
                            const double *meanW, double *ubm_means, double *Tm)
{
    if (!c || C <= 0 || D <= 0 || R <= 0 || !(n_sessions > 0) || !Rm || !r || !meanW || !ubm_means || !Tm) { gmmiv_set_error("tv_min_divergence: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D, RR = (size_t)R * R;
    int rc;
    DevOut<double> o_rm, o_r, o_mean, o_t;
    DevIn<double> i_mw;
    if ((rc = o_rm.init(c, WS_T0, Rm, RR, true)) || (rc = o_r.init(c, WS_T1, r, R, true)) || (rc = i_mw.init(c, WS_T2, meanW, R)) ||
        (rc = o_mean.init(c, WS_T3, ubm_means, SV, true)) || (rc = o_t.init(c, WS_T4, Tm, (size_t)R * SV, true))) return rc;
    void *p;
    if ((rc = c->scratch(WS_T5, RR * 8, &p))) return rc;
    double *dCh = (double *)p;
    if (SpdBatch::left(R) && c->tv_md_device) {
        // R <- R / n - r r^T and its factor on the device: one workgroup of k_chol_left (R = L L^T, Ch = L^T); the host only sees the
        // status word.  (The host route below cost 4-5 ms of a 130 ms iteration at R = 400: two 1.28 MB copies each way and a scalar
        // O(R^3) loop.)
        SpdSlots slots; // WS_T0 .. WS_T4 hold the staged arguments, WS_T5 the factor: the matrix goes to WS_T8, and nothing else is needed
        slots.full = WS_T8;
        slots.inv = slots.X = slots.panel = -1;
        SpdBatch ws;
        if ((rc = ws.reserve(c, R, 1, slots)) || (rc = ws.begin(1))) return rc;
        GCHK(tvk_md_normalize(c->stream, R, n_sessions, o_rm.d, o_r.d, ws.full));
        if ((rc = ws.factor())) return rc;
        GCHK(tvk_lower_to_upper(c->stream, R, ws.full, dCh));
        if (ws.check("tv_min_divergence: R")) { gmmiv_set_error("tv_min_divergence: R is not positive definite"); return GMMIV_ERR_NUMERIC; }
    } else {
        // R x R normalisation + Cholesky on the host (odd R: the device factorisation wants 16-byte rows)
        std::vector<double> hR(RR), hr(R), ch;
        GCHK(hipMemcpyAsync(hR.data(), o_rm.d, RR * 8, hipMemcpyDeviceToHost, c->stream));
        GCHK(hipMemcpyAsync(hr.data(), o_r.d, R * 8, hipMemcpyDeviceToHost, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < R; ++i) hr[i] /= n_sessions;
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < R; ++j) hR[(size_t)i * R + j] = hR[(size_t)i * R + j] / n_sessions - hr[i] * hr[j];
        if (!host_cholesky_upper(R, hR, ch)) { gmmiv_set_error("tv_min_divergence: R is not positive definite"); return GMMIV_ERR_NUMERIC; }
        GCHK(hipMemcpyAsync(o_rm.d, hR.data(), RR * 8, hipMemcpyHostToDevice, c->stream));
        GCHK(hipMemcpyAsync(o_r.d, hr.data(), R * 8, hipMemcpyHostToDevice, c->stream));
        GCHK(hipMemcpyAsync(dCh, ch.data(), RR * 8, hipMemcpyHostToDevice, c->stream));
        GCHK(hipStreamSynchronize(c->stream)); // the host vectors go out of scope
    }
    // R is factored, T has not been read yet: a caller whose T is still arriving (all-gather begun before the call) joins it here
    if (o_t.d == Tm) { c->hook_md_factored.call(); GBIND(c); } // (see tv_a_ready)
    // mean += T^T meanW (old T), then T <- Ch T
    GCHK(tvk_vecmat_add(c->stream, R, (long)SV, i_mw.d, o_t.d, o_mean.d));
    if ((rc = c->scratch(WS_T6, (size_t)R * SV * 8, &p))) return rc;
    double *Tn = (double *)p;
    GCHK(tvk_dgemm(c->stream, false, false, R, (int)SV, R, 1.0, dCh, R, 0, o_t.d, (long)SV, 0, 0.0, Tn, (long)SV, 0, 1));
    GCHK(hipMemcpyAsync(o_t.d, Tn, (size_t)R * SV * 8, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = o_rm.finish()) || (rc = o_r.finish()) || (rc = o_mean.finish())) return rc;
    return o_t.finish();
}

// ---- approximate extractors ------------------------------------------------------------------
int gmmiv_tv_norm_statistics(gmmiv_ctx *c, int64_t U, int C, int D, const double *N, double *F, const double *means,
                             const double *invvar)
{
    if (!c || U < 0 || C <= 0 || D <= 0 || !N || !F || !means || !invvar) { gmmiv_set_error("tv_norm_statistics: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D;
    DevIn<double> i_n, i_m, i_v;
    DevOut<double> o_f;
    int rc;
    if ((rc = i_n.init(c, WS_T0, N, (size_t)U * C)) || (rc = i_m.init(c, WS_T2, means, SV)) || (rc = i_v.init(c, WS_T3, invvar, SV)) ||
        (rc = o_f.init(c, WS_T1, F, (size_t)U * SV, true))) return rc;
    GCHK(tvk_norm_stats(c->stream, (long)U, C, D, i_n.d, o_f.d, i_m.d, i_v.d));
    return o_f.finish();
}

int gmmiv_tv_subtract_m_plus_tw(gmmiv_ctx *c, int64_t U, int C, int D, int R, const double *N, double *F, const double *means,
                                const double *Tm, const double *W)
{
    if (!c || U < 0 || C <= 0 || D <= 0 || R <= 0 || !N || !F || !means || !Tm || !W) { gmmiv_set_error("tv_subtract_m_plus_tw: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D;
    DevIn<double> i_n, i_m, i_t, i_w;
    DevOut<double> o_f;
    int rc;
    if ((rc = i_n.init(c, WS_T0, N, (size_t)U * C)) || (rc = i_m.init(c, WS_T2, means, SV)) || (rc = i_t.init(c, WS_T3, Tm, (size_t)R * SV)) ||
        (rc = i_w.init(c, WS_LSE, W, (size_t)U * R)) || (rc = o_f.init(c, WS_T1, F, (size_t)U * SV, true))) return rc;
    const int BC = tv_batch_size(c, U);
    void *p;
    if ((rc = c->scratch(WS_TIV, (size_t)BC * SV * 8, &p))) return rc;
    double *TW = (double *)p;
    for (int64_t u0 = 0; u0 < U; u0 += BC) {
        const int nb = (int)((U - u0) < BC ? (U - u0) : BC);
        GCHK(tvk_dgemm(c->stream, false, false, nb, (int)SV, R, 1.0, i_w.d + (size_t)u0 * R, R, 0, i_t.d, (long)SV, 0, 0.0, TW, (long)SV, 0, 1));
        GCHK(tvk_sub_mtw(c->stream, nb, C, D, i_n.d + (size_t)u0 * C, o_f.d + (size_t)u0 * SV, i_m.d, TW));
    }
    return o_f.finish();
}

// ---- JFA (LIA_SpkTools/src/AccumulateJFAStat.cpp).  The factor steps themselves are the TV functions above under other
// names: estimateVEVT / estimateUEUT = gmmiv_tv_tett, estimateAndInverseL_E{V,C} + estimate{YandV,XandU} =
// gmmiv_tv_estimate_a_and_c, estimateY / estimateX = gmmiv_tv_estimate_w, update{V,U}estimate = gmmiv_tv_update_t. ----
int gmmiv_jfa_subtract(gmmiv_ctx *c, int64_t rows, int C, int D, const double *N, double *F, const int64_t *owner, int64_t nfact,
                       const double *means, int R, const double *Tm, const double *W, const double *Dm, const double *Z)
{
    if (!c || rows < 0 || C <= 0 || D <= 0 || !N || !F || nfact < 0 || (Tm && (R <= 0 || !W)) || (Dm && !Z)) { gmmiv_set_error("jfa_subtract: bad argument"); return GMMIV_ERR_ARG; }
    if (rows == 0) return GMMIV_OK;
    GBIND(c);
    const size_t SV = (size_t)C * D;
    if (!owner && nfact < rows && (Tm || Dm)) { gmmiv_set_error("jfa_subtract: %lld factor rows for %lld statistics rows and no owner map", (long long)nfact, (long long)rows); return GMMIV_ERR_ARG; }
    if (owner && !gmmiv_is_device_ptr(owner))
        for (int64_t r = 0; r < rows; ++r)
            if (owner[r] < 0 || owner[r] >= nfact) { gmmiv_set_error("jfa_subtract: owner[%lld] = %lld out of range", (long long)r, (long long)owner[r]); return GMMIV_ERR_ARG; }
    DevIn<double> i_n, i_m, i_t, i_w, i_d, i_z;
    DevIn<int64_t> i_o;
    DevOut<double> o_f;
    int rc;
    if ((rc = i_n.init(c, WS_T0, N, (size_t)rows * C)) || (rc = i_m.init(c, WS_T2, means, SV)) || (rc = i_t.init(c, WS_T3, Tm, Tm ? (size_t)R * SV : 0)) ||
        (rc = i_w.init(c, WS_LSE, Tm ? W : nullptr, Tm ? (size_t)nfact * R : 0)) || (rc = i_d.init(c, WS_T4, Dm, SV)) ||
        (rc = i_z.init(c, WS_T5, Dm ? Z : nullptr, Dm ? (size_t)nfact * SV : 0)) || (rc = i_o.init(c, WS_SEG, owner, (size_t)rows)) ||
        (rc = o_f.init(c, WS_T1, F, (size_t)rows * SV, true))) return rc;
    const int BC = tv_batch_size(c, rows);
    double *TW = nullptr, *Wg = nullptr;
    void *p;
    if (Tm) {
        if ((rc = c->scratch(WS_TIV, (size_t)BC * SV * 8, &p))) return rc;
        TW = (double *)p;
        if ((rc = c->scratch(WS_AUX, (size_t)BC * R * 8, &p))) return rc;
        Wg = (double *)p;
    }
    for (int64_t r0 = 0; r0 < rows; r0 += BC) {
        const int nb = (int)((rows - r0) < BC ? (rows - r0) : BC);
        if (Tm) {
            GCHK(tvk_gather_rows(c->stream, nb, R, (long)r0, (const long *)i_o.d, i_w.d, Wg));
            GCHK(tvk_dgemm(c->stream, false, false, nb, (int)SV, R, 1.0, Wg, R, 0, i_t.d, (long)SV, 0, 0.0, TW, (long)SV, 0, 1));
        }
        GCHK(tvk_jfa_sub(c->stream, nb, C, D, (long)r0, (const long *)i_o.d, i_n.d, o_f.d, i_m.d, TW, i_d.d, i_z.d));
    }
    return o_f.finish();
}

int gmmiv_jfa_subtract_sessions(gmmiv_ctx *c, int64_t nspk, const int64_t *sess_begin, int C, int D, const double *N_h, double *F_X,
                                int R, const double *Um, const double *X)
{
    if (!c || nspk < 0 || !sess_begin || C <= 0 || D <= 0 || R <= 0 || !N_h || !F_X || !Um || !X) { gmmiv_set_error("jfa_subtract_sessions: bad argument"); return GMMIV_ERR_ARG; }
    if (gmmiv_is_device_ptr(sess_begin)) { gmmiv_set_error("jfa_subtract_sessions: sess_begin must be a host array"); return GMMIV_ERR_ARG; }
    if (nspk == 0) return GMMIV_OK;
    for (int64_t s = 0; s < nspk; ++s)
        if (sess_begin[s + 1] < sess_begin[s] || sess_begin[0] != 0) { gmmiv_set_error("jfa_subtract_sessions: sess_begin must start at 0 and be non-decreasing"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D;
    const int64_t nsess = sess_begin[nspk];
    if (nsess == 0) return GMMIV_OK;
    DevIn<double> i_n, i_u, i_x;
    DevIn<int64_t> i_b;
    DevOut<double> o_f;
    int rc;
    if ((rc = i_n.init(c, WS_T0, N_h, (size_t)nsess * C)) || (rc = i_u.init(c, WS_T3, Um, (size_t)R * SV)) || (rc = i_x.init(c, WS_LSE, X, (size_t)nsess * R)) ||
        (rc = i_b.init(c, WS_SEG, sess_begin, (size_t)nspk + 1)) || (rc = o_f.init(c, WS_T1, F_X, (size_t)nspk * SV, true))) return rc;
    const int BC = tv_batch_size(c, nsess);
    void *p;
    if ((rc = c->scratch(WS_TIV, (size_t)BC * SV * 8, &p))) return rc;
    double *G = (double *)p;
    int64_t s_lo = 0;
    for (int64_t h0 = 0; h0 < nsess; h0 += BC) {
        const int64_t h1 = (h0 + BC) < nsess ? (h0 + BC) : nsess;
        GCHK(tvk_dgemm(c->stream, false, false, (int)(h1 - h0), (int)SV, R, 1.0, i_x.d + (size_t)h0 * R, R, 0, i_u.d, (long)SV, 0, 0.0, G, (long)SV, 0, 1));
        while (s_lo < nspk && sess_begin[s_lo + 1] <= h0) ++s_lo;      // first speaker with a session in [h0, h1)
        int64_t s_hi = s_lo;
        while (s_hi < nspk && sess_begin[s_hi] < h1) ++s_hi;           // one past the last
        GCHK(tvk_jfa_sub_sessions(c->stream, (long)s_lo, (long)(s_hi - s_lo), (long)h0, (long)h1, C, D, (const long *)i_b.d, i_n.d, G, o_f.d));
    }
    return o_f.finish();
}

int gmmiv_jfa_estimate_z(gmmiv_ctx *c, int64_t nspk, int C, int D, const double *N, const double *F, const double *invvar, const double *Dm,
                         double tau, double *Z)
{
    if (!c || nspk < 0 || C <= 0 || D <= 0 || !N || !F || !invvar || !Dm || !Z) { gmmiv_set_error("jfa_estimate_z: bad argument"); return GMMIV_ERR_ARG; }
    if (nspk == 0) return GMMIV_OK;
    GBIND(c);
    const size_t SV = (size_t)C * D;
    DevIn<double> i_n, i_f, i_v, i_d;
    DevOut<double> o_z;
    int rc;
    if ((rc = i_n.init(c, WS_T0, N, (size_t)nspk * C)) || (rc = i_f.init(c, WS_T1, F, (size_t)nspk * SV)) || (rc = i_v.init(c, WS_T2, invvar, SV)) ||
        (rc = i_d.init(c, WS_T4, Dm, SV)) || (rc = o_z.init(c, WS_T5, Z, (size_t)nspk * SV, false))) return rc;
    GCHK(tvk_jfa_z(c->stream, (long)nspk, C, D, i_n.d, i_f.d, i_v.d, i_d.d, tau, o_z.d));
    return o_z.finish();
}

int gmmiv_jfa_estimate_z_and_d(gmmiv_ctx *c, int64_t nspk, int C, int D, const double *N, const double *F, const double *invvar, double *Dm,
                               double *Z)
{
    if (!c || nspk <= 0 || C <= 0 || D <= 0 || !N || !F || !invvar || !Dm || !Z) { gmmiv_set_error("jfa_estimate_z_and_d: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D;
    DevIn<double> i_n, i_f, i_v;
    DevOut<double> o_d, o_z;
    int rc;
    if ((rc = i_n.init(c, WS_T0, N, (size_t)nspk * C)) || (rc = i_f.init(c, WS_T1, F, (size_t)nspk * SV)) || (rc = i_v.init(c, WS_T2, invvar, SV)) ||
        (rc = o_d.init(c, WS_T4, Dm, SV, true)) || (rc = o_z.init(c, WS_T5, Z, (size_t)nspk * SV, false))) return rc;
    GCHK(tvk_jfa_z_and_d(c->stream, (long)nspk, C, D, i_n.d, i_f.d, i_v.d, o_d.d, o_z.d));
    if ((rc = o_d.finish())) return rc;
    return o_z.finish();
}

int gmmiv_tv_norm_t(gmmiv_ctx *c, int C, int D, int R, double *Tm, const double *invvar)
{
    if (!c || C <= 0 || D <= 0 || R <= 0 || !Tm || !invvar) { gmmiv_set_error("tv_norm_t: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D;
    DevIn<double> i_v;
    DevOut<double> o_t;
    int rc;
    if ((rc = i_v.init(c, WS_T0, invvar, SV)) || (rc = o_t.init(c, WS_T1, Tm, (size_t)R * SV, true))) return rc;
    GCHK(tvk_scale_cols_fn(c->stream, R, (long)SV, D, 0, o_t.d, i_v.d, o_t.d));
    return o_t.finish();
}

int gmmiv_tv_weighted_cov(gmmiv_ctx *c, int C, int D, int R, const double *Tm, const double *weight, double *Wm)
{
    if (!c || C <= 0 || D <= 0 || R <= 0 || !Tm || !weight || !Wm) { gmmiv_set_error("tv_weighted_cov: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D;
    DevIn<double> i_t, i_w;
    DevOut<double> o;
    int rc;
    if ((rc = i_t.init(c, WS_T1, Tm, (size_t)R * SV)) || (rc = i_w.init(c, WS_T0, weight, C)) || (rc = o.init(c, WS_T2, Wm, (size_t)R * R, false))) return rc;
    void *p;
    if ((rc = c->scratch(WS_TIV, (size_t)R * SV * 8, &p))) return rc;
    double *Ts = (double *)p;
    GCHK(tvk_scale_cols_fn(c->stream, R, (long)SV, D, 1, i_t.d, i_w.d, Ts));
    if ((rc = splitk_gemm(c, R, false, true, R, R, (int)SV, 1.0, Ts, (long)SV, i_t.d, (long)SV, 0.0, o.d, R))) return rc;
    return o.finish();
}

int gmmiv_tv_approximate_tctc(gmmiv_ctx *c, int C, int D, int R, const double *Tm, const double *Q, double *Dm)
{
    if (!c || C <= 0 || D <= 0 || R <= 0 || !Tm || !Q || !Dm) { gmmiv_set_error("tv_approximate_tctc: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D;
    DevIn<double> i_t, i_q;
    DevOut<double> o;
    int rc;
    if ((rc = i_t.init(c, WS_T1, Tm, (size_t)R * SV)) || (rc = i_q.init(c, WS_T0, Q, (size_t)R * R)) || (rc = o.init(c, WS_T2, Dm, (size_t)C * R, true))) return rc;
    void *p;
    if ((rc = c->scratch(WS_TIV, SV * R * 8, &p))) return rc;
    double *A = (double *)p; // [SV x R] = T^T Q
    GCHK(tvk_dgemm(c->stream, true, false, (int)SV, R, R, 1.0, i_t.d, (long)SV, 0, i_q.d, R, 0, 0.0, A, R, 0, 1));
    GCHK(tvk_block_colnorm(c->stream, C, D, R, A, o.d));
    return o.finish();
}

int gmmiv_tv_estimate_w_ubm_weight(gmmiv_ctx *c, int64_t U, int C, int D, int R, const double *N, const double *F, const double *Tm,
                                   const double *Wm, double *W)
{
    if (!c || U < 0 || C <= 0 || D <= 0 || R <= 0 || !N || !F || !Tm || !Wm || !W) { gmmiv_set_error("tv_estimate_w_ubm_weight: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D;
    DevIn<double> i_n, i_f, i_t, i_w;
    DevOut<double> o;
    int rc;
    if ((rc = i_n.init(c, WS_T0, N, (size_t)U * C)) || (rc = i_f.init(c, WS_T1, F, (size_t)U * SV)) || (rc = i_t.init(c, WS_T2, Tm, (size_t)R * SV)) ||
        (rc = i_w.init(c, WS_T3, Wm, (size_t)R * R)) || (rc = o.init(c, WS_LSE, W, (size_t)U * R, true))) return rc;
    const int BC = tv_batch_size(c, U);
    void *p;
    if ((rc = c->scratch(WS_AUX, (size_t)2 * BC * R * 8, &p))) return rc;
    double *aux = (double *)p, *wc = aux + (size_t)BC * R;
    SpdBatch ws;
    if ((rc = ws.reserve(c, R, BC))) return rc;
    for (int64_t u0 = 0; u0 < U; u0 += BC) {
        const int nb = (int)((U - u0) < BC ? (U - u0) : BC);
        if ((rc = ws.begin(nb))) return rc;
        GCHK(tvk_build_l_ubm(c->stream, R, C, nb, i_n.d + (size_t)u0 * C, i_w.d, ws.full));
        // aux[nb x R] = F_chunk T^T (T and F normalised, no invvar)
        if ((rc = splitk_gemm(c, BC, false, true, nb, R, (int)SV, 1.0, i_f.d + (size_t)u0 * SV, (long)SV, i_t.d, (long)SV, 0.0, aux, R)) ||
            (rc = ws.factor()) || (rc = ws.solve(aux, wc)) || (rc = ws.check("tv_estimate_w_ubm_weight: L"))) return rc;
        GCHK(tvk_axpby(c->stream, (long)nb * R, 1.0, wc, 1.0, o.d + (size_t)u0 * R, o.d + (size_t)u0 * R));
    }
    return o.finish();
}

int gmmiv_tv_estimate_w_eigen(gmmiv_ctx *c, int64_t U, int C, int D, int R, const double *N, const double *F, const double *Tm,
                              const double *Dm, const double *Q, double *W)
{
    if (!c || U < 0 || C <= 0 || D <= 0 || R <= 0 || !N || !F || !Tm || !Dm || !Q || !W) { gmmiv_set_error("tv_estimate_w_eigen: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t SV = (size_t)C * D;
    DevIn<double> i_n, i_f, i_t, i_d, i_q;
    DevOut<double> o;
    int rc;
    if ((rc = i_n.init(c, WS_T0, N, (size_t)U * C)) || (rc = i_f.init(c, WS_T1, F, (size_t)U * SV)) || (rc = i_t.init(c, WS_T2, Tm, (size_t)R * SV)) ||
        (rc = i_d.init(c, WS_T3, Dm, (size_t)C * R)) || (rc = i_q.init(c, WS_T4, Q, (size_t)R * R)) || (rc = o.init(c, WS_LSE, W, (size_t)U * R, true))) return rc;
    const int BC = tv_batch_size(c, U);
    void *p;
    if ((rc = c->scratch(WS_AUX, (size_t)3 * BC * R * 8, &p))) return rc;
    double *aux = (double *)p, *nd = aux + (size_t)BC * R, *b = nd + (size_t)BC * R;
    for (int64_t u0 = 0; u0 < U; u0 += BC) {
        const int nb = (int)((U - u0) < BC ? (U - u0) : BC);
        // aux[nb x R] = F_chunk T^T (T and F normalised, no invvar)
        if ((rc = splitk_gemm(c, BC, false, true, nb, R, (int)SV, 1.0, i_f.d + (size_t)u0 * SV, (long)SV, i_t.d, (long)SV, 0.0, aux, R))) return rc;
        GCHK(tvk_dgemm(c->stream, false, false, nb, R, C, 1.0, i_n.d + (size_t)u0 * C, C, 0, i_d.d, R, 0, 0.0, nd, R, 0, 1));   // N Dm
        GCHK(tvk_dgemm(c->stream, false, false, nb, R, R, 1.0, aux, R, 0, i_q.d, R, 0, 0.0, b, R, 0, 1));                          // (Q^T aux)^T = aux Q
        GCHK(tvk_mul_recip1p(c->stream, (long)nb * R, b, nd));
        GCHK(tvk_dgemm(c->stream, false, true, nb, R, R, 1.0, b, R, 0, i_q.d, R, 0, 1.0, o.d + (size_t)u0 * R, R, 0, 1));         // += b Q^T
    }
    return o.finish();
}

int gmmiv_tv_orthonormalize_t(gmmiv_ctx *c, int R, int64_t SV, double *Tm)
{
    if (!c || R <= 0 || SV <= 0 || !Tm) { gmmiv_set_error("tv_orthonormalize_t: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    DevOut<double> o;
    int rc;
    if ((rc = o.init(c, WS_T0, Tm, (size_t)R * SV, true))) return rc;
    void *p;
    if ((rc = c->scratch(WS_T1, (size_t)R * SV * 8, &p))) return rc;
    double *Q = (double *)p;
    // Gram-Schmidt on the rows of T is T = L Q with L lower triangular, positive diagonal: Q = L^-1 T with L the Cholesky factor
    // of the Gram matrix T T^T -- two GEMMs and an R x R factorisation on the host (3 ms at R = 400, SV = 122 880) instead of R
    // dependent projection steps (116 ms).  Same result as the reference's classical Gram-Schmidt up to cond(T)^2 eps, which is
    // also what the classical scheme itself is good for; zero / dependent rows (no Cholesky factor) and badly conditioned T
    // (diagonal ratio of L below 1e-4) keep the step-by-step kernel, which reproduces the reference's zero-row rule.
    {
        const size_t RR = (size_t)R * R;
        if ((rc = c->scratch(WS_T3, 2 * RR * 8, &p))) return rc;
        double *dG = (double *)p, *dLi = dG + RR;
        if ((rc = splitk_gemm(c, R, false, true, R, R, (int)SV, 1.0, o.d, (long)SV, o.d, (long)SV, 0.0, dG, R))) return rc;
        std::vector<double> G, L, Li;
        if ((rc = fetch_host(c, dG, RR, G))) return rc;
        double dmin, dmax;
        if (host_cholesky_lower(R, G, L, &dmin, &dmax) && dmin > 1e-4 * dmax) {
            host_lower_inverse(R, L, Li);
            GCHK(hipMemcpyAsync(dLi, Li.data(), RR * 8, hipMemcpyHostToDevice, c->stream));
            GCHK(tvk_dgemm(c->stream, false, false, R, (int)SV, R, 1.0, dLi, R, 0, o.d, (long)SV, 0, 0.0, Q, (long)SV, 0, 1));
            GCHK(hipMemcpyAsync(o.d, Q, (size_t)R * SV * 8, hipMemcpyDeviceToDevice, c->stream));
            GCHK(hipStreamSynchronize(c->stream)); // Li is a stack-lifetime vector
            return o.finish();
        }
    }
    if ((rc = c->scratch(WS_T2, ((size_t)SV + R + 512) * 8, &p))) return rc;
    double *v = (double *)p, *rv = v + SV, *partial = rv + R;
    GCHK(tvk_orthonormalize(c->stream, R, (long)SV, o.d, Q, rv, v, partial));
    GCHK(hipMemcpyAsync(o.d, Q, (size_t)R * SV * 8, hipMemcpyDeviceToDevice, c->stream));
    return o.finish();
}

} // extern "C"
