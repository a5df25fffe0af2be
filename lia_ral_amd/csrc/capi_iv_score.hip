// capi_iv_score.hip -- C ABI (include/gmmiv.h): i-vector normalisation, the scoring rules (cosine, Mahalanobis, two-covariance, PLDA)
// and the gmmiv_dgemm pass-through to the fp64 GEMM they all run on.  Score normalisation is capi_score.hip.
#include <string.h>

#include "ctx.h"
#include "host_linalg.h"
#include "tv_kernels.h"

extern "C" {

// ---- i-vector normalisation ------------------------------------------------------------------
int gmmiv_iv_normalize(gmmiv_ctx *c, int dim_in, int dim_out, int64_t n, const double *X, const double *mean,
                       const double *M, int length_norm, double *Y)
{
    if (!c || dim_in <= 0 || dim_out <= 0 || n < 0 || !X || !Y) { gmmiv_set_error("iv_normalize: bad argument"); return GMMIV_ERR_ARG; }
    if (!M && dim_in != dim_out) { gmmiv_set_error("iv_normalize: dim_out must equal dim_in without a rotation matrix"); return GMMIV_ERR_ARG; }
    if (n > 0x7fffffff) { gmmiv_set_error("iv_normalize: too many vectors"); return GMMIV_ERR_UNSUPPORTED; }
    if (n == 0) return GMMIV_OK;
    GBIND(c);
    DevIn<double> i_x, i_mu, i_m;
    DevOut<double> o;
    int rc;
    if ((rc = i_x.init(c, WS_T0, X, (size_t)dim_in * n)) || (rc = i_mu.init(c, WS_T1, mean, dim_in)) ||
        (rc = i_m.init(c, WS_T2, M, (size_t)dim_out * dim_in)) || (rc = o.init(c, WS_T3, Y, (size_t)dim_out * n, false))) return rc;
    const double *cur = i_x.d;
    void *p;
    if (mean) { // PldaTest::center (PldaTools.cpp:3754-3767)
        double *dst = o.d;
        if (M || cur == o.d) {
            if ((rc = c->scratch(WS_T4, (size_t)dim_in * n * 8, &p))) return rc;
            dst = (double *)p;
        }
        GCHK(tvk_sub_colvec(c->stream, dim_in, n, cur, i_mu.d, dst));
        cur = dst;
    }
    if (M) { // PldaTest::rotateLeft (:3770-3790): Y = M X
        GCHK(tvk_dgemm(c->stream, false, false, dim_out, (int)n, dim_in, 1.0, i_m.d, dim_in, 0, cur, n, 0, 0.0, o.d, n, 0, 1));
        cur = o.d;
    }
    if (cur != o.d) GCHK(hipMemcpyAsync(o.d, cur, (size_t)dim_out * n * 8, hipMemcpyDeviceToDevice, c->stream));
    if (length_norm) { // PldaTest::lengthNorm (:3706-3751)
        if ((rc = c->scratch(WS_T5, (size_t)n * 8, &p))) return rc;
        GCHK(tvk_coldot(c->stream, dim_out, n, o.d, o.d, (double *)p));
        GCHK(tvk_scale_cols_rsqrt(c->stream, dim_out, n, o.d, (const double *)p));
    }
    return o.finish();
}

// ---- scoring -----------------------------------------------------------------------------
struct ScoreArgs {
    DevIn<double> m, s;
    DevOut<double> sc;
    double *qm = nullptr, *qs = nullptr;
    // row strides of the vector matrices as the GEMMs see them.  _models [dim x M] / _segments [dim x S] have the vector count as
    // their row stride: with an ODD count no row but the first starts on 16 bytes and every GEMM of the rule would run on the
    // per-element checked instantiation (1.5 x slower); such a matrix is copied once into an even-stride block.
    int64_t ldm = 0, lds = 0;
    static int even_stride(gmmiv_ctx *c, int slot, int dim, int64_t n, DevIn<double> &v, int64_t *ld)
    {
        *ld = n;
        if ((n & 1) == 0 || n < 2) return GMMIV_OK;
        void *p;
        int rc = c->scratch(slot, (size_t)dim * (n + 1) * 8, &p);
        if (rc) return rc;
        GCHK(hipMemcpy2DAsync(p, (n + 1) * 8, v.d, n * 8, n * 8, dim, hipMemcpyDeviceToDevice, c->stream));
        v.d = (const double *)p;
        *ld = n + 1;
        return GMMIV_OK;
    }
    int init(gmmiv_ctx *c, int dim, int64_t M, int64_t S, const double *models, const double *segs, double *scores, bool load = false)
    {
        int rc;
        if ((rc = m.init(c, WS_T0, models, (size_t)dim * M)) || (rc = s.init(c, WS_T1, segs, (size_t)dim * S)) ||
            (rc = even_stride(c, WS_T9, dim, M, m, &ldm)) || (rc = even_stride(c, WS_TIV, dim, S, s, &lds)) ||
            (rc = sc.init(c, WS_T2, scores, (size_t)M * S, load))) return rc;
        void *p;
        if ((rc = c->scratch(WS_T3, (size_t)(M + S) * 8, &p))) return rc;
        qm = (double *)p;
        qs = qm + M;
        return GMMIV_OK;
    }
};

static int score_check(gmmiv_ctx *c, int dim, int64_t M, int64_t S, const void *a, const void *b, const void *o, const char *what)
{
    if (!c || dim <= 0 || M < 0 || S < 0 || !a || !b || !o) { gmmiv_set_error("%s: bad argument", what); return GMMIV_ERR_ARG; }
    if (M > 0x7fffffff || S > 0x7fffffff) { gmmiv_set_error("%s: too many vectors", what); return GMMIV_ERR_UNSUPPORTED; }
    GBIND(c);
    return GMMIV_OK;
}

int gmmiv_score_cosine(gmmiv_ctx *c, int dim, int64_t M, int64_t S, const double *models, const double *segs, double *scores)
{
    int rc = score_check(c, dim, M, S, models, segs, scores, "score_cosine");
    if (rc) return rc;
    if (M == 0 || S == 0) return GMMIV_OK;
    ScoreArgs a;
    if ((rc = a.init(c, dim, M, S, models, segs, scores))) return rc;
    GCHK(tvk_coldot(c->stream, dim, M, a.m.d, a.m.d, a.qm, a.ldm));
    GCHK(tvk_coldot(c->stream, dim, S, a.s.d, a.s.d, a.qs, a.lds));
    c->t_begin("k_dgemm(score)");
    GCHK(tvk_rsqrt_vec(c->stream, M, a.qm));   // the normalisation rides in the GEMM epilogue: x 1/|m| x 1/|s|
    GCHK(tvk_rsqrt_vec(c->stream, S, a.qs));
    GCHK(tvk_dgemm_epi(c->stream, true, false, (int)M, (int)S, dim, 1.0, a.m.d, a.ldm, a.s.d, a.lds, a.sc.d, S, 1, a.qm, a.qs, 0.0, 0.0, 0.0));
    c->t_end();
    return a.sc.finish();
}

// scores = Mt (Q + Q^T) S * half_cross + bm * diag(Mt Qm M) + bs * diag(St Qs S)
// ldm: row stride of the model matrix a.m (0: M) -- a run of models gathered by gmmiv_score_plda has an EVEN stride whatever its length
static int quad_score(gmmiv_ctx *c, ScoreArgs &a, int dim, int64_t M, int64_t S, const double *Qcross, double ccross,
                      const double *Qm, double bm, const double *Qs, double bs, double cst, double beta = 0.0, int64_t ldm = 0)
{
    int rc;
    void *p;
    if (ldm <= 0) ldm = a.ldm > 0 ? a.ldm : M;
    const int64_t lds = a.lds > 0 ? a.lds : S;
    const size_t nn = (size_t)dim * dim;
    if ((rc = c->scratch(WS_T4, nn * 8, &p))) return rc;
    double *Qsym = (double *)p;
    const size_t mx = (size_t)dim * (ldm > lds ? ldm : lds);
    if ((rc = c->scratch(WS_T5, mx * 8, &p))) return rc;
    double *Y = (double *)p;
    GCHK(tvk_dgemm(c->stream, false, false, dim, (int)M, dim, 1.0, Qm, dim, 0, a.m.d, ldm, 0, 0.0, Y, ldm, 0, 1));
    GCHK(tvk_coldot(c->stream, dim, M, a.m.d, Y, a.qm, ldm));
    GCHK(tvk_dgemm(c->stream, false, false, dim, (int)S, dim, 1.0, Qs, dim, 0, a.s.d, lds, 0, 0.0, Y, lds, 0, 1));
    GCHK(tvk_coldot(c->stream, dim, S, a.s.d, Y, a.qs, lds));
    GCHK(tvk_add_transpose(c->stream, dim, Qcross, Qcross, Qsym));
    GCHK(tvk_dgemm(c->stream, false, false, dim, (int)S, dim, 1.0, Qsym, dim, 0, a.s.d, lds, 0, 0.0, Y, lds, 0, 1));
    c->t_begin("k_dgemm(score)");
    // ccross m^T Y s + bm q_m + bs q_s + cst in ONE pass over the M x S matrix (GEMM epilogue)
    GCHK(tvk_dgemm_epi(c->stream, true, false, (int)M, (int)S, dim, ccross, a.m.d, ldm, Y, lds, a.sc.d, S, 2, a.qm, a.qs, bm, bs, cst, beta));
    c->t_end();
    return GMMIV_OK;
}

int gmmiv_score_mahalanobis(gmmiv_ctx *c, int dim, int64_t M, int64_t S, const double *models, const double *segs,
                            const double *Mah, double *scores)
{
    int rc = score_check(c, dim, M, S, models, segs, scores, "score_mahalanobis");
    if (rc) return rc;
    if (!Mah) { gmmiv_set_error("score_mahalanobis: Mah == NULL"); return GMMIV_ERR_ARG; }
    if (M == 0 || S == 0) return GMMIV_OK;
    ScoreArgs a;
    if ((rc = a.init(c, dim, M, S, models, segs, scores))) return rc;
    DevIn<double> q;
    if ((rc = q.init(c, WS_T6, Mah, (size_t)dim * dim))) return rc;
    // -1/2 (m-s)' Q (m-s) = -1/2 m'Qm - 1/2 s'Qs + 1/2 m'(Q+Q')s
    if ((rc = quad_score(c, a, dim, M, S, q.d, 0.5, q.d, -0.5, q.d, -0.5, 0.0))) return rc;
    return a.sc.finish();
}

int gmmiv_score_twocov(gmmiv_ctx *c, int dim, int64_t M, int64_t S, const double *models, const double *segs,
                       const double *G, const double *H, double *scores)
{
    int rc = score_check(c, dim, M, S, models, segs, scores, "score_twocov");
    if (rc) return rc;
    if (!G || !H) { gmmiv_set_error("score_twocov: G/H == NULL"); return GMMIV_ERR_ARG; }
    if (M == 0 || S == 0) return GMMIV_OK;
    ScoreArgs a;
    if ((rc = a.init(c, dim, M, S, models, segs, scores))) return rc;
    DevIn<double> g, h;
    const size_t nn = (size_t)dim * dim;
    if ((rc = g.init(c, WS_T6, G, nn)) || (rc = h.init(c, WS_T7, H, nn))) return rc;
    void *p;
    if ((rc = c->scratch(WS_T8, nn * 8, &p))) return rc;
    double *GmH = (double *)p; // G - H: (m+s)'G(m+s) - m'Hm - s'Hs = m'(G-H)m + s'(G-H)s + m'(G+G')s
    GCHK(tvk_axpby(c->stream, (long)nn, 1.0, g.d, -1.0, h.d, GmH));
    if ((rc = quad_score(c, a, dim, M, S, g.d, 1.0, GmH, 1.0, GmH, 1.0, 0.0))) return rc;
    return a.sc.finish();
}

// PldaTest::twoCovScoringMixPart (PldaTools.cpp:3923-3949): scores[m][s] += (m + s)^T G (m + s) for every pair (ACCUMULATES,
// like the reference's `_scores(m,s) +=`): m'Gm + s'Gs + m'(G + G')s with the model / segment terms in the GEMM epilogue.
int gmmiv_score_twocov_mix_part(gmmiv_ctx *c, int dim, int64_t M, int64_t S, const double *models, const double *segs, const double *G,
                                double *scores)
{
    int rc = score_check(c, dim, M, S, models, segs, scores, "score_twocov_mix_part");
    if (rc) return rc;
    if (!G) { gmmiv_set_error("score_twocov_mix_part: G == NULL"); return GMMIV_ERR_ARG; }
    if (M == 0 || S == 0) return GMMIV_OK;
    ScoreArgs a;
    if ((rc = a.init(c, dim, M, S, models, segs, scores, true))) return rc;
    DevIn<double> g;
    if ((rc = g.init(c, WS_T6, G, (size_t)dim * dim)) || (rc = quad_score(c, a, dim, M, S, g.d, 1.0, g.d, 1.0, g.d, 1.0, 0.0, 1.0))) return rc;
    return a.sc.finish();
}

// PldaTest::_trials (PldaTools.cpp:3437, 3591-3620): cosineDistance / mahalanobisDistance only score the listed trials
// (:3871, :3889), the others keep the initial value of _scores (0).  The device computes the whole M x S block in one GEMM;
// this entry point then writes `fill` into every cell whose trial flag is 0.  trials: [M x S] bytes, host or device.
int gmmiv_score_apply_trials(gmmiv_ctx *c, int64_t M, int64_t S, const unsigned char *trials, double fill, double *scores)
{
    if (!c || M < 0 || S < 0 || !trials || !scores) { gmmiv_set_error("score_apply_trials: bad argument"); return GMMIV_ERR_ARG; }
    if (M == 0 || S == 0) return GMMIV_OK;
    GBIND(c);
    DevIn<unsigned char> t;
    DevOut<double> o;
    int rc;
    if ((rc = t.init(c, WS_T0, trials, (size_t)M * S)) || (rc = o.init(c, WS_T2, scores, (size_t)M * S, true))) return rc;
    GCHK(tvk_mask_trials(c->stream, (long)(M * S), t.d, fill, o.d));
    return o.finish();
}

// The fp64 GEMM under every step above, as it is: C[b] = epilogue(alpha op(A[b]) op(B[b])) + beta C[b] on the context's stream with the
// context's "gemm_*" options bound.  A pass-through to tvk_dgemm / tvk_dgemm_splitk / tvk_dgemm_epi: device pointers only, nothing
// is staged or copied, so the caller's bases, leading dimensions and batch strides reach launch_dgemm unchanged.
int gmmiv_dgemm(gmmiv_ctx *c, int ta, int tb, int M, int N, int K, double alpha, const double *A, int64_t lda, int64_t sA,
                const double *B, int64_t ldb, int64_t sB, double beta, double *C, int64_t ldc, int64_t sC, int batch, int nz,
                int epi_mode, const double *rv, const double *cv, double br, double bc, double cst)
{
    if (!c) { gmmiv_set_error("dgemm: ctx == NULL"); return GMMIV_ERR_ARG; }
    if (M < 0 || N < 0 || K < 0 || batch < 0 || nz < 0) { gmmiv_set_error("dgemm: negative size"); return GMMIV_ERR_ARG; }
    if (epi_mode < 0 || epi_mode > 2) { gmmiv_set_error("dgemm: epi_mode %d is not 0, 1 or 2", epi_mode); return GMMIV_ERR_ARG; }
    if (epi_mode != 0 && (!rv || !cv)) { gmmiv_set_error("dgemm: epi_mode %d needs rv and cv", epi_mode); return GMMIV_ERR_ARG; }
    if (batch > 1 && (nz != 1 || epi_mode != 0)) { gmmiv_set_error("dgemm: a batch takes neither split-K nor an epilogue"); return GMMIV_ERR_ARG; }
    if (nz != 1 && epi_mode != 0) { gmmiv_set_error("dgemm: split-K takes no epilogue"); return GMMIV_ERR_ARG; }
    if (lda < (ta ? M : K) || ldb < (tb ? K : N) || ldc < N) {
        gmmiv_set_error("dgemm: a leading dimension is smaller than its extent (lda %lld, ldb %lld, ldc %lld)", (long long)lda, (long long)ldb, (long long)ldc);
        return GMMIV_ERR_ARG;
    }
    if (sA < 0 || sB < 0 || sC < 0) { gmmiv_set_error("dgemm: negative batch stride"); return GMMIV_ERR_ARG; }
    if (M == 0 || N == 0 || batch == 0) return GMMIV_OK;
    if (!C || (K > 0 && (!A || !B))) { gmmiv_set_error("dgemm: NULL operand"); return GMMIV_ERR_ARG; }
    if (!gmmiv_is_device_ptr(C) || (K > 0 && (!gmmiv_is_device_ptr(A) || !gmmiv_is_device_ptr(B))) ||
        (epi_mode != 0 && (!gmmiv_is_device_ptr(rv) || !gmmiv_is_device_ptr(cv)))) {
        gmmiv_set_error("dgemm: operands must be device pointers");
        return GMMIV_ERR_ARG;
    }
    GBIND(c);
    if (epi_mode != 0) {
        GCHK(tvk_dgemm_epi(c->stream, ta != 0, tb != 0, M, N, K, alpha, A, lda, B, ldb, C, ldc, epi_mode, rv, cv, br, bc, cst, beta));
        return GMMIV_OK;
    }
    if (nz == 0) nz = tvk_splitk_count(M, N, K, c->n_cu);
    if (nz > 1 && K > 0) {
        void *p;
        int rc;
        if ((rc = c->scratch(WS_SLAB, (size_t)nz * M * N * 8, &p))) return rc;
        GCHK(tvk_dgemm_splitk(c->stream, ta != 0, tb != 0, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, nz, (double *)p));
        return GMMIV_OK;
    }
    GCHK(tvk_dgemm(c->stream, ta != 0, tb != 0, M, N, K, alpha, A, lda, sA, B, ldb, sB, beta, C, ldc, sC, batch));
    return GMMIV_OK;
}

int gmmiv_score_plda(gmmiv_ctx *c, int rf, int64_t M, int64_t S, const double *models_sum, const int64_t *nsess,
                     const double *segs, const double *FTJF, double *scores)
{
    int rc = score_check(c, rf, M, S, models_sum, segs, scores, "score_plda");
    if (rc) return rc;
    if (!nsess || !FTJF) { gmmiv_set_error("score_plda: nsess/FTJF == NULL"); return GMMIV_ERR_ARG; }
    if (gmmiv_is_device_ptr(nsess)) { gmmiv_set_error("score_plda: nsess must be a host array"); return GMMIV_ERR_ARG; }
    if (M == 0 || S == 0) return GMMIV_OK;
    ScoreArgs a;
    if ((rc = a.init(c, rf, M, S, models_sum, segs, scores))) return rc;
    const size_t nn = (size_t)rf * rf;
    std::vector<double> hF(nn);
    // a device FTJF is read in the order of the context's stream: the call that wrote it (gmmiv_plda_precompute, gmmiv_dgemm) may still be queued
    if (gmmiv_is_device_ptr(FTJF)) {
        GCHK(hipMemcpyAsync(hF.data(), FTJF, nn * 8, hipMemcpyDeviceToHost, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
    } else memcpy(hF.data(), FTJF, nn * 8);
    // K_n = (n FTJF + I)^-1 and alpha_n = log det K_n on the host, cached per n in the context for as long as FTJF is unchanged
    typedef gmmiv_ctx::PldaK KN;
    if (c->plda_ftjf.size() != nn || memcmp(c->plda_ftjf.data(), hF.data(), nn * 8) != 0) {
        c->plda_ftjf = hF;
        c->plda_k.clear();
    }
    std::map<long, KN> &cache = c->plda_k;
    auto getK = [&](int64_t n) -> const KN * {
        auto it = cache.find((long)n);
        if (it != cache.end()) return &it->second;
        std::vector<double> t(nn);
        for (size_t e = 0; e < nn; ++e) t[e] = (double)n * hF[e];
        for (int i = 0; i < rf; ++i) t[(size_t)i * rf + i] += 1.0;
        KN kn;
        double ld;
        if (!host_spd_inverse(rf, t, kn.K, &ld)) return nullptr;
        kn.alpha = -ld; // log det K = -log det (nFTJF + I)
        return &cache.emplace((long)n, std::move(kn)).first->second;
    };
    const KN *K1 = getK(1);
    if (!K1) { gmmiv_set_error("score_plda: FTJF + I is not positive definite"); return GMMIV_ERR_NUMERIC; }
    void *p;
    if ((rc = c->scratch(WS_T6, 3 * nn * 8, &p))) return rc;
    double *dQc = (double *)p, *dQm = dQc + nn, *dQs = dQm + nn;
    // runs of consecutive models with the same session count (PldaTools.cpp:4186-4250)
    for (int64_t m0 = 0; m0 < M;) {
        int64_t m1 = m0;
        const int64_t L = nsess[m0];
        while (m1 < M && nsess[m1] == L) ++m1;
        if (L < 1) { gmmiv_set_error("score_plda: nsess[%ld] < 1", (long)m0); return GMMIV_ERR_ARG; }
        const KN *KL = getK(L), *KL1 = getK(L + 1);
        if (!KL || !KL1) { gmmiv_set_error("score_plda: K_n not positive definite"); return GMMIV_ERR_NUMERIC; }
        // score = 1/2[(s+m)'K_{L+1}(s+m) - m'K_L m - s'K_1 s] + (a_{L+1} - a_L - a_1)/2
        //       = 1/2 m'(K_{L+1}-K_L)m + 1/2 s'(K_{L+1}-K_1)s + 1/2 m'(K_{L+1}+K_{L+1}')s + cst
        std::vector<double> qm(nn), qs(nn);
        for (size_t e = 0; e < nn; ++e) { qm[e] = KL1->K[e] - KL->K[e]; qs[e] = KL1->K[e] - K1->K[e]; }
        GCHK(hipMemcpyAsync(dQc, KL1->K.data(), nn * 8, hipMemcpyHostToDevice, c->stream));
        GCHK(hipMemcpyAsync(dQm, qm.data(), nn * 8, hipMemcpyHostToDevice, c->stream));
        GCHK(hipMemcpyAsync(dQs, qs.data(), nn * 8, hipMemcpyHostToDevice, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
        const double cst = (KL1->alpha - KL->alpha - K1->alpha) / 2.0;
        // operate on the column range [m0, m1) of models (ld = M) and the row range of scores
        ScoreArgs sub = a;
        const int64_t Mr = m1 - m0;
        // gather the run's columns into a compact block [rf x Mr] with an EVEN row stride: with an odd one (a run of odd length, half of
        // all runs) no row but the first starts on 16 bytes and the whole scoring GEMM fell to the per-element checked instantiation
        // (37 instead of 24 ms per third of 100 k x 100 k trials: 98 G trials/s where 137 are possible)
        void *q;
        const int64_t ldq = Mr + (Mr & 1);
        if ((rc = c->scratch(WS_T7, (size_t)rf * ldq * 8, &q))) return rc;
        GCHK(hipMemcpy2DAsync(q, ldq * 8, a.m.d + m0, a.ldm * 8, Mr * 8, rf, hipMemcpyDeviceToDevice, c->stream));
        sub.m.d = (const double *)q;
        sub.sc.d = a.sc.d + (size_t)m0 * S;
        sub.qm = a.qm + m0;
        if ((rc = quad_score(c, sub, rf, Mr, S, dQc, 0.5, dQm, 0.5, dQs, 0.5, cst, 0.0, ldq))) return rc;
        GCHK(hipStreamSynchronize(c->stream));
        m0 = m1;
    }
    return a.sc.finish();
}

} // extern "C"
