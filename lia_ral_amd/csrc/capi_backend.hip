// capi_backend.hip -- C ABI (include/gmmiv.h): the PldaDev / PLDA back end on a development set of i-vectors: means, covariance and
// scatter matrices, Mahalanobis / WCCN / EFR / LDA matrices, the symmetric eigensolver, PLDA EM and pre-computation, the
// two-covariance model.
#include <math.h>
#include <string.h>

#include "capi_tv_util.h"
#include "host_linalg.h"

extern "C" {

namespace { // (inside extern "C", as it has always been: dev_gram keeps the C name under which the library has exported it)
struct DevSet { // device views shared by the gmmiv_dev_* entry points
    DevIn<double> x;
    long *off = nullptr;   // [nspk + 1] session offsets
    int *cls = nullptr;    // [n] speaker of each session
    double *ssum = nullptr, *mean = nullptr, *smean = nullptr;
    std::vector<long> hoff;
    int init(gmmiv_ctx *c, int dim, int64_t n, const double *X, int64_t nspk, const int64_t *sps, const char *what)
    {
        if (!c || dim <= 0 || n <= 0 || nspk <= 0 || !X || !sps) { gmmiv_set_error("%s: bad argument", what); return GMMIV_ERR_ARG; }
        if (gmmiv_is_device_ptr(sps)) { gmmiv_set_error("%s: sessions_per_speaker must be a host array", what); return GMMIV_ERR_ARG; }
        GBIND(c);
        hoff.assign(nspk + 1, 0);
        for (int64_t i = 0; i < nspk; ++i) {
            if (sps[i] <= 0) { gmmiv_set_error("%s: speaker %ld has no session", what, (long)i); return GMMIV_ERR_ARG; }
            hoff[i + 1] = hoff[i] + (long)sps[i];
        }
        if (hoff[nspk] != n) { gmmiv_set_error("%s: sessions_per_speaker sums to %ld, n = %ld", what, hoff[nspk], (long)n); return GMMIV_ERR_ARG; }
        std::vector<int> hc(n);
        for (int64_t i = 0; i < nspk; ++i) for (long s = hoff[i]; s < hoff[i + 1]; ++s) hc[s] = (int)i;
        int rc;
        if ((rc = x.init(c, WS_T0, X, (size_t)dim * n))) return rc;
        void *p;
        if ((rc = c->scratch(WS_SEG, (nspk + 1) * sizeof(long) + n * sizeof(int), &p))) return rc;
        off = (long *)p; cls = (int *)(off + nspk + 1);
        GCHK(hipMemcpyAsync(off, hoff.data(), (nspk + 1) * sizeof(long), hipMemcpyHostToDevice, c->stream));
        GCHK(hipMemcpyAsync(cls, hc.data(), n * sizeof(int), hipMemcpyHostToDevice, c->stream));
        GCHK(hipStreamSynchronize(c->stream)); // hc is a stack-lifetime vector
        if ((rc = c->scratch(WS_T1, ((size_t)2 * dim * nspk + dim) * 8, &p))) return rc;
        ssum = (double *)p; smean = ssum + (size_t)dim * nspk; mean = smean + (size_t)dim * nspk;
        GCHK(tvk_dev_means(c->stream, dim, (long)n, x.d, (long)nspk, off, ssum, mean, smean));
        return GMMIV_OK;
    }
};
// out[dim x dim] = alpha * Y Y^T for Y [dim x m] (row-major, ld = m)
int dev_gram(gmmiv_ctx *c, int dim, long m, const double *Y, double alpha, double *out)
{
    return splitk_gemm(c, dim, false, true, dim, dim, (int)m, alpha, Y, m, Y, m, 0.0, out, dim);
}
} // namespace

// ---- PldaDev: development-set statistics ---------------------------------------------------------

int gmmiv_dev_means(gmmiv_ctx *c, int dim, int64_t n, const double *X, int64_t nspk, const int64_t *sps, double *mean, double *spk_means)
{
    DevSet ds;
    int rc = ds.init(c, dim, n, X, nspk, sps, "dev_means");
    if (rc) return rc;
    DevOut<double> o_m, o_s;
    if ((rc = o_m.init(c, WS_T2, mean, dim, false)) || (rc = o_s.init(c, WS_T3, spk_means, (size_t)dim * nspk, false))) return rc;
    if (mean) GCHK(hipMemcpyAsync(o_m.d, ds.mean, dim * 8, hipMemcpyDeviceToDevice, c->stream));
    if (spk_means) GCHK(hipMemcpyAsync(o_s.d, ds.smean, (size_t)dim * nspk * 8, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = o_m.finish())) return rc;
    return o_s.finish();
}

int gmmiv_dev_cov_mat(gmmiv_ctx *c, int dim, int64_t n, const double *X, int64_t nspk, const int64_t *sps, double *Sigma, double *W, double *B)
{
    DevSet ds;
    int rc = ds.init(c, dim, n, X, nspk, sps, "dev_cov_mat");
    if (rc) return rc;
    const size_t dd = (size_t)dim * dim;
    DevOut<double> o_s, o_w, o_b;
    if ((rc = o_s.init(c, WS_T2, Sigma, dd, false)) || (rc = o_w.init(c, WS_T3, W, dd, false)) || (rc = o_b.init(c, WS_T4, B, dd, false))) return rc;
    void *p;
    if ((rc = c->scratch(WS_TIV, (size_t)dim * (n > nspk ? n : nspk) * 8, &p))) return rc;
    double *Y = (double *)p;
    const double inv_n = 1.0 / (double)n;
    if (Sigma) {
        GCHK(tvk_dev_center(c->stream, dim, (long)n, 0, ds.x.d, ds.mean, ds.smean, (long)nspk, ds.off, ds.cls, Y));
        if ((rc = dev_gram(c, dim, (long)n, Y, inv_n, o_s.d))) return rc;
    }
    if (W) {
        GCHK(tvk_dev_center(c->stream, dim, (long)n, 1, ds.x.d, ds.mean, ds.smean, (long)nspk, ds.off, ds.cls, Y));
        if ((rc = dev_gram(c, dim, (long)n, Y, inv_n, o_w.d))) return rc;
    }
    if (B) {
        GCHK(tvk_dev_between(c->stream, dim, (long)nspk, 1, ds.mean, ds.smean, ds.off, Y));
        if ((rc = dev_gram(c, dim, (long)nspk, Y, inv_n, o_b.d))) return rc;
    }
    if ((rc = o_s.finish()) || (rc = o_w.finish())) return rc;
    return o_b.finish();
}

int gmmiv_dev_mahalanobis(gmmiv_ctx *c, int dim, int64_t n, const double *X, int64_t nspk, const int64_t *sps, double *M)
{
    if (!M) { gmmiv_set_error("dev_mahalanobis: bad argument"); return GMMIV_ERR_ARG; }
    DevSet ds;
    int rc = ds.init(c, dim, n, X, nspk, sps, "dev_mahalanobis");
    if (rc) return rc;
    DevOut<double> o;
    if ((rc = o.init(c, WS_T2, M, (size_t)dim * dim, false))) return rc;
    void *p;
    if ((rc = c->scratch(WS_TIV, (size_t)dim * n * 8, &p))) return rc;
    SpdBatch ws;
    if ((rc = ws.reserve(c, dim, 1))) return rc;
    GCHK(tvk_dev_center(c->stream, dim, (long)n, 1, ds.x.d, ds.mean, ds.smean, (long)nspk, ds.off, ds.cls, (double *)p));
    if ((rc = dev_gram(c, dim, (long)n, (double *)p, 1.0 / (double)n, ws.full)) ||
        (rc = ws.begin(1)) || (rc = ws.inverse(o.d)) || (rc = ws.check("dev_mahalanobis: W"))) return rc;
    return o.finish();
}

int gmmiv_dev_wccn_chol(gmmiv_ctx *c, int dim, int64_t n, const double *X, int64_t nspk, const int64_t *sps, double *WCCN)
{
    if (!WCCN) { gmmiv_set_error("dev_wccn_chol: bad argument"); return GMMIV_ERR_ARG; }
    DevSet ds;
    int rc = ds.init(c, dim, n, X, nspk, sps, "dev_wccn_chol");
    if (rc) return rc;
    void *p;
    if ((rc = c->scratch(WS_TIV, (size_t)dim * n * 8, &p))) return rc;
    SpdBatch ws;
    if ((rc = ws.reserve(c, dim, 1))) return rc;
    GCHK(tvk_dev_center(c->stream, dim, (long)n, 2, ds.x.d, ds.mean, ds.smean, (long)nspk, ds.off, ds.cls, (double *)p));
    if ((rc = dev_gram(c, dim, (long)n, (double *)p, 1.0 / (double)nspk, ws.full)) ||
        (rc = ws.begin(1)) || (rc = ws.inverse(ws.inv)) || (rc = ws.check("dev_wccn_chol: W"))) return rc;
    std::vector<double> iw, ch; // upperCholesky on the host (O(dim^3) once, like min-divergence)
    if ((rc = fetch_host(c, ws.inv, (size_t)dim * dim, iw))) return rc;
    if (!host_cholesky_upper(dim, iw, ch)) { gmmiv_set_error("dev_wccn_chol: W^-1 is not positive definite"); return GMMIV_ERR_NUMERIC; }
    return store_out(c, WCCN, ch);
}

int gmmiv_dev_scatter_mat(gmmiv_ctx *c, int dim, int64_t n, const double *X, int64_t nspk, const int64_t *sps, double *SB, double *SW)
{
    DevSet ds;
    int rc = ds.init(c, dim, n, X, nspk, sps, "dev_scatter_mat");
    if (rc) return rc;
    const size_t dd = (size_t)dim * dim;
    DevOut<double> o_b, o_w;
    if ((rc = o_b.init(c, WS_T2, SB, dd, false)) || (rc = o_w.init(c, WS_T3, SW, dd, false))) return rc;
    void *p;
    if ((rc = c->scratch(WS_TIV, (size_t)dim * (n > nspk ? n : nspk) * 8, &p))) return rc;
    double *Y = (double *)p;
    if (SB) {
        GCHK(tvk_dev_between(c->stream, dim, (long)nspk, 0, ds.mean, ds.smean, ds.off, Y));
        if ((rc = dev_gram(c, dim, (long)nspk, Y, 1.0, o_b.d))) return rc;
    }
    if (SW) { // the reference's loop: the first n_last sessions of the set, centred per speaker, / n_last
        const long nl = (long)sps[nspk - 1];
        GCHK(tvk_dev_center(c->stream, dim, (long)n, 1, ds.x.d, ds.mean, ds.smean, (long)nspk, ds.off, ds.cls, Y));
        if ((rc = splitk_gemm(c, dim, false, true, dim, dim, (int)nl, 1.0 / (double)nl, Y, (long)n, Y, (long)n, 0.0, o_w.d, dim))) return rc;
    }
    if ((rc = o_b.finish())) return rc;
    return o_w.finish();
}

int gmmiv_sym_eigen(gmmiv_ctx *c, int n, const double *A, int rank, double *vect, double *val)
{
    if (!c || n <= 0 || rank <= 0 || rank > n || !A) { gmmiv_set_error("sym_eigen: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    std::vector<double> a, v, l;
    int rc;
    if ((rc = fetch_host(c, A, (size_t)n * n, a))) return rc;
    host_sym_eigen(n, a, rank, v, l);
    if ((rc = store_out(c, vect, v))) return rc;
    return store_out(c, val, l);
}

int gmmiv_dev_efr_matrix(gmmiv_ctx *c, int dim, const double *Cov, double *M)
{
    if (!c || dim <= 0 || !Cov || !M) { gmmiv_set_error("dev_efr_matrix: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    std::vector<double> a, v, l, m((size_t)dim * dim);
    int rc;
    if ((rc = fetch_host(c, Cov, (size_t)dim * dim, a))) return rc;
    host_sym_eigen(dim, a, dim, v, l);
    for (int j = 0; j < dim; ++j) {
        if (!(l[j] > 0.0)) { gmmiv_set_error("dev_efr_matrix: eigenvalue %d = %g is not positive", j, l[j]); return GMMIV_ERR_NUMERIC; }
        for (int k = 0; k < dim; ++k) m[(size_t)j * dim + k] = v[(size_t)k * dim + j] / sqrt(l[j]);
    }
    return store_out(c, M, m);
}

int gmmiv_dev_lda(gmmiv_ctx *c, int dim, const double *W, const double *B, int rank, double *ldaMat, double *eigval)
{
    if (!c || dim <= 0 || rank <= 0 || rank > dim || !W || !B || !ldaMat) { gmmiv_set_error("dev_lda: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    std::vector<double> w, b, U;
    int rc;
    if ((rc = fetch_host(c, W, (size_t)dim * dim, w)) || (rc = fetch_host(c, B, (size_t)dim * dim, b))) return rc;
    if (!host_cholesky_upper(dim, w, U)) { gmmiv_set_error("dev_lda: W is not positive definite"); return GMMIV_ERR_NUMERIC; }
    // symmetric form of W^-1 B: Cm = L^-1 B L^-T with W = L L^T, L = U^T
    std::vector<double> T1, Cm, vect, val, out((size_t)rank * dim);
    host_upper_tsolve_cols(dim, U, b, T1);
    host_upper_rsolve_rows(dim, U, T1, Cm);
    for (int i = 0; i < dim; ++i)
        for (int j = i + 1; j < dim; ++j) { const double m = 0.5 * (Cm[(size_t)i * dim + j] + Cm[(size_t)j * dim + i]); Cm[(size_t)i * dim + j] = Cm[(size_t)j * dim + i] = m; }
    host_sym_eigen(dim, Cm, rank, vect, val);
    for (int j = 0; j < rank; ++j) { // v = U^-1 y, unit norm (Eigen::EigenSolver normalises its eigenvectors)
        double nrm = 0.0;
        host_upper_solve_vec(dim, U, vect, rank, j, out);
        for (int i = 0; i < dim; ++i) nrm += out[(size_t)j * dim + i] * out[(size_t)j * dim + i];
        nrm = sqrt(nrm);
        for (int i = 0; i < dim; ++i) out[(size_t)j * dim + i] /= nrm;
    }
    if ((rc = store_out(c, ldaMat, out))) return rc;
    return store_out(c, eigval, val);
}

int gmmiv_plda_em_iteration(gmmiv_ctx *c, int dim, int64_t n, double *X, int64_t nspk, const int64_t *sps, int rf, int rg, double *Fm,
                            double *Gm, double *Sigma, double *Delta)
{
    // rg == 0 (pldaEigenChannelNumber 0, the common "simplified PLDA" configuration): every G-sized object is empty
    if (rf <= 0 || rg < 0 || !Fm || (rg > 0 && !Gm) || !Sigma || !Delta) { gmmiv_set_error("plda_em_iteration: bad argument"); return GMMIV_ERR_ARG; }
    DevSet ds; // validates the arguments, uploads X (when it is a host array), builds cls / off
    int rc = ds.init(c, dim, n, X, nspk, sps, "plda_em_iteration");
    if (rc) return rc;
    const int rh = rf + rg;
    const size_t dd = (size_t)dim * dim;
    hipStream_t st = c->stream;
    std::vector<double> F, G, Sg, Dl;
    if ((rc = fetch_host(c, Fm, (size_t)dim * rf, F)) || (rc = fetch_host(c, Gm, (size_t)dim * rg, G)) || (rc = fetch_host(c, Sigma, dd, Sg)) ||
        (rc = fetch_host(c, Delta, dim, Dl))) return rc;
    // device scratch: centred X (in place when X is a device array), small operands, Eh
    void *p;
    double *Xd = const_cast<double *>(ds.x.d); // DevIn's staging copy or the caller's device array
    if ((rc = c->scratch(WS_T2, ((size_t)rh * dim + (size_t)rg * rg + (size_t)rh * nspk + dim + dd + (size_t)rh * rh + (size_t)dim * rh) * 8, &p))) return rc;
    double *dFG = (double *)p, *dIGG = dFG + (size_t)rh * dim, *dH = dIGG + (size_t)rg * rg, *dDelta = dH + (size_t)rh * nspk;
    double *dOut = dDelta + dim; // sigObs [dd] | gram [rh x rh] | xh [dim x rh]
    if ((rc = c->scratch(WS_TIV, (size_t)2 * rh * n * 8, &p))) return rc;
    double *FGX = (double *)p, *Eh = FGX + (size_t)rh * n; // [rh x n] each: (Ftw; Gtw) X, then the expected latent variables
    // 1. centre by Delta, total second moment
    GCHK(hipMemcpyAsync(dDelta, Dl.data(), dim * 8, hipMemcpyHostToDevice, st));
    GCHK(tvk_sub_colvec(st, dim, (long)n, Xd, dDelta, Xd));
    if ((rc = dev_gram(c, dim, (long)n, Xd, 1.0, dOut))) return rc;
    // 2. preComputation on the host (PldaTools.cpp:2950-2972)
    std::vector<double> Si, FGtw((size_t)rh * dim), GtwG((size_t)rg * rg), iGG, FtwG((size_t)rf * rg), FtwF((size_t)rf * rf), S((size_t)rg * rf),
        A((size_t)rf * rf), t1((size_t)rf * rg);
    if (!host_spd_inverse(dim, Sg, Si, nullptr)) { gmmiv_set_error("plda_em_iteration: Sigma is not positive definite"); return GMMIV_ERR_NUMERIC; }
    double *Ftw = FGtw.data(), *Gtw = FGtw.data() + (size_t)rf * dim;
    hmm(rf, dim, dim, F.data(), true, Si.data(), false, Ftw);
    hmm(rg, dim, dim, G.data(), true, Si.data(), false, Gtw);
    hmm(rg, rg, dim, Gtw, false, G.data(), false, GtwG.data());
    hmm(rf, rg, dim, Ftw, false, G.data(), false, FtwG.data());
    for (int i = 0; i < rg; ++i) GtwG[(size_t)i * rg + i] += 1.0;
    if (!host_spd_inverse(rg, GtwG, iGG, nullptr)) { gmmiv_set_error("plda_em_iteration: G^T S^-1 G + I is not positive definite"); return GMMIV_ERR_NUMERIC; }
    hmm(rf, rf, dim, Ftw, false, F.data(), false, FtwF.data());
    hmm(rg, rf, rg, iGG.data(), false, FtwG.data(), true, S.data());
    hmm(rf, rg, rg, FtwG.data(), false, iGG.data(), false, t1.data());
    hmm(rf, rf, rg, t1.data(), false, FtwG.data(), true, A.data());
    for (size_t i = 0; i < A.size(); ++i) A[i] = FtwF[i] - A[i];
    // 3. (Ftw; Gtw) X on the device, per-speaker sums back to the host
    GCHK(hipMemcpyAsync(dFG, FGtw.data(), FGtw.size() * 8, hipMemcpyHostToDevice, st));
    if (rg > 0) GCHK(hipMemcpyAsync(dIGG, iGG.data(), iGG.size() * 8, hipMemcpyHostToDevice, st));
    GCHK(tvk_dgemm(st, false, false, rh, (int)n, dim, 1.0, dFG, dim, 0, Xd, (long)n, 0, 0.0, FGX, (long)n, 0, 1));
    void *q;
    if ((rc = c->scratch(WS_T3, ((size_t)2 * rh * nspk + rh) * 8, &q))) return rc;
    double *dsum = (double *)q, *dsm = dsum + (size_t)rh * nspk, *dmn = dsm + (size_t)rh * nspk;
    GCHK(tvk_dev_means(st, rh, (long)n, FGX, (long)nspk, ds.off, dsum, dmn, dsm));
    std::vector<double> fg;
    if ((rc = fetch_host(c, dsum, (size_t)rh * nspk, fg))) return rc; // rows 0..rf-1: f_s, rows rf..: g_s
    // 4. per-speaker expectations on the host (:2417-2477)
    std::vector<double> Hs((size_t)rh * nspk), Ehh((size_t)rh * rh, 0.0), U(rh, 0.0), M, MsT((size_t)rf * rg), SMsT((size_t)rg * rg), tmpM((size_t)rh * rh),
        J((size_t)rf * rf), v(rf), gsum(rg, 0.0);
    std::map<int64_t, std::pair<std::vector<double>, std::vector<double> > > cache; // session count -> (M, tmpM)
    for (int64_t spk = 0; spk < nspk; ++spk) {
        const int64_t ns = sps[spk];
        auto it = cache.find(ns);
        if (it == cache.end()) {
            for (size_t i = 0; i < J.size(); ++i) J[i] = (double)ns * A[i];
            for (int i = 0; i < rf; ++i) J[(size_t)i * rf + i] += 1.0;
            if (!host_spd_inverse(rf, J, M, nullptr)) { gmmiv_set_error("plda_em_iteration: n A + I is not positive definite"); return GMMIV_ERR_NUMERIC; }
            hmm(rf, rg, rf, M.data(), false, S.data(), true, MsT.data());
            hmm(rg, rg, rf, S.data(), false, MsT.data(), false, SMsT.data());
            for (int i = 0; i < rf; ++i) for (int j = 0; j < rf; ++j) tmpM[(size_t)i * rh + j] = M[(size_t)i * rf + j];
            for (int i = 0; i < rf; ++i) for (int j = 0; j < rg; ++j) { tmpM[(size_t)i * rh + rf + j] = -MsT[(size_t)i * rg + j]; tmpM[(size_t)(rf + j) * rh + i] = -MsT[(size_t)i * rg + j]; }
            for (int i = 0; i < rg; ++i) for (int j = 0; j < rg; ++j) tmpM[(size_t)(rf + i) * rh + rf + j] = iGG[(size_t)i * rg + j] + SMsT[(size_t)i * rg + j];
            it = cache.emplace(ns, std::make_pair(M, tmpM)).first;
        }
        const std::vector<double> &Mn = it->second.first, &Tn = it->second.second;
        for (int r = 0; r < rf; ++r) { double a = fg[(size_t)r * nspk + spk]; for (int k = 0; k < rg; ++k) a -= S[(size_t)k * rf + r] * fg[(size_t)(rf + k) * nspk + spk]; v[r] = a; }
        for (int r = 0; r < rf; ++r) { double a = 0.0; for (int k = 0; k < rf; ++k) a += Mn[(size_t)r * rf + k] * v[k]; Hs[(size_t)r * nspk + spk] = a; U[r] += (double)ns * a; }
        for (int r = 0; r < rg; ++r) { double a = 0.0; for (int k = 0; k < rf; ++k) a += S[(size_t)r * rf + k] * Hs[(size_t)k * nspk + spk]; Hs[(size_t)(rf + r) * nspk + spk] = a; U[rf + r] -= (double)ns * a; gsum[r] += fg[(size_t)(rf + r) * nspk + spk]; }
        for (size_t i = 0; i < Ehh.size(); ++i) Ehh[i] += (double)ns * Tn[i];
    }
    for (int r = 0; r < rg; ++r) { double a = 0.0; for (int k = 0; k < rg; ++k) a += iGG[(size_t)r * rg + k] * gsum[k]; U[rf + r] += a; }
    // 5. Eh = [h_spk ; iGG g_i - S h_spk] per session, its Gram matrix and X Eh^T on the device
    GCHK(hipMemcpyAsync(dH, Hs.data(), Hs.size() * 8, hipMemcpyHostToDevice, st));
    GCHK(tvk_dev_expand(st, rf, (long)n, (long)nspk, dH, ds.cls, Eh));
    if (rg > 0) {
        GCHK(tvk_dgemm(st, false, false, rg, (int)n, rg, 1.0, dIGG, rg, 0, FGX + (size_t)rf * n, (long)n, 0, 0.0, Eh + (size_t)rf * n, (long)n, 0, 1));
        GCHK(tvk_dev_center(st, rg, (long)n, 1, Eh + (size_t)rf * n, nullptr, dH + (size_t)rf * nspk, (long)nspk, ds.off, ds.cls, Eh + (size_t)rf * n));
    }
    double *dGram = dOut + dd, *dXh = dGram + (size_t)rh * rh;
    if ((rc = dev_gram(c, rh, (long)n, Eh, 1.0, dGram)) ||
        (rc = splitk_gemm(c, dim, false, true, dim, rh, (int)n, 1.0, Xd, (long)n, Eh, (long)n, 0.0, dXh, rh))) return rc;
    std::vector<double> outv;
    if ((rc = fetch_host(c, dOut, dd + (size_t)rh * rh + (size_t)dim * rh, outv))) return rc;
    const double *sigObs = outv.data(), *gram = sigObs + dd, *xh = gram + (size_t)rh * rh;
    for (size_t i = 0; i < Ehh.size(); ++i) Ehh[i] += gram[i];
    // 6. mStep on the host (:2790-2815)
    std::vector<double> iE, FG((size_t)dim * rh), SL(dd), cF((size_t)rf * rf), cG((size_t)rg * rg), Rh, Rw;
    if (!host_spd_inverse(rh, Ehh, iE, nullptr)) { gmmiv_set_error("plda_em_iteration: sum E[hh^T] is not positive definite"); return GMMIV_ERR_NUMERIC; }
    hmm(dim, rh, rh, xh, false, iE.data(), false, FG.data());
    hmm(dim, dim, rh, FG.data(), false, xh, true, SL.data());
    for (size_t i = 0; i < dd; ++i) Sg[i] = (sigObs[i] - SL[i]) / (double)n;
    for (int i = 0; i < rh; ++i) U[i] /= (double)n;
    for (int i = 0; i < rf; ++i) for (int j = 0; j < rf; ++j) cF[(size_t)i * rf + j] = Ehh[(size_t)i * rh + j] / (double)n - U[i] * U[j];
    for (int i = 0; i < rg; ++i) for (int j = 0; j < rg; ++j) cG[(size_t)i * rg + j] = Ehh[(size_t)(rf + i) * rh + rf + j] / (double)n - U[rf + i] * U[rf + j];
    if (!host_cholesky_upper(rf, cF, Rh) || !host_cholesky_upper(rg, cG, Rw)) { gmmiv_set_error("plda_em_iteration: minimum-divergence covariance is not positive definite"); return GMMIV_ERR_NUMERIC; }
    for (int i = 0; i < dim; ++i) {
        for (int j = 0; j < rf; ++j) { double a = 0.0; for (int k = 0; k < rf; ++k) a += FG[(size_t)i * rh + k] * Rh[(size_t)j * rf + k]; F[(size_t)i * rf + j] = a; }
        for (int j = 0; j < rg; ++j) { double a = 0.0; for (int k = 0; k < rg; ++k) a += FG[(size_t)i * rh + rf + k] * Rw[(size_t)j * rg + k]; G[(size_t)i * rg + j] = a; }
        double d = 0.0;
        for (int k = 0; k < rh; ++k) d += FG[(size_t)i * rh + k] * U[k];
        Dl[i] += d;
    }
    if ((rc = store_out(c, Fm, F)) || (rc = store_out(c, Gm, G)) || (rc = store_out(c, Sigma, Sg)) || (rc = store_out(c, Delta, Dl))) return rc;
    if (!gmmiv_is_device_ptr(X)) { // the centred data goes back to the caller's host array
        GCHK(hipMemcpyAsync(X, Xd, (size_t)dim * n * 8, hipMemcpyDeviceToHost, st));
        GCHK(hipStreamSynchronize(st));
    }
    return GMMIV_OK;
}

int gmmiv_plda_precompute(gmmiv_ctx *c, int dim, int rf, int rg, const double *Fm, const double *Gm, const double *Sigma, double *FTJ,
                          double *FTJF)
{
    if (!c || dim <= 0 || rf <= 0 || rg < 0 || !Fm || (rg > 0 && !Gm) || !Sigma || !FTJ || !FTJF) { gmmiv_set_error("plda_precompute: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    DevIn<double> i_f, i_g, i_s;
    DevOut<double> o_j, o_jf;
    int rc;
    if ((rc = i_f.init(c, WS_T0, Fm, (size_t)dim * rf)) || (rc = i_g.init(c, WS_T1, Gm, (size_t)dim * rg)) || (rc = i_s.init(c, WS_T2, Sigma, (size_t)dim * dim)) ||
        (rc = o_j.init(c, WS_T3, FTJ, (size_t)rf * dim, false)) || (rc = o_jf.init(c, WS_T9, FTJF, (size_t)rf * rf, false))) return rc;
    const int big = dim > rg ? dim : rg;
    SpdBatch ws;
    if ((rc = ws.reserve(c, big, 1))) return rc;
    void *p;
    const size_t need = (size_t)dim * dim + (size_t)rf * dim + (size_t)rg * dim + (size_t)rg * rg * 2 + (size_t)rf * rg * 2;
    if ((rc = c->scratch(WS_AUX, need * 8, &p))) return rc;
    double *Si = (double *)p, *Ftw = Si + (size_t)dim * dim, *Gtw = Ftw + (size_t)rf * dim, *GG = Gtw + (size_t)rg * dim;
    double *Mi = GG + (size_t)rg * rg, *FtwG = Mi + (size_t)rg * rg, *t1 = FtwG + (size_t)rf * rg;
    hipStream_t st = c->stream;
    // S^-1 (the inverse routine factors its input in place: work on a copy)
    if ((rc = ws.inverse_of(dim, i_s.d, Si, "plda_precompute: Sigma"))) return rc;
    GCHK(tvk_dgemm(st, true, false, rf, dim, dim, 1.0, i_f.d, rf, 0, Si, dim, 0, 0.0, Ftw, dim, 0, 1));          // F^T S^-1
    GCHK(hipMemcpyAsync(o_j.d, Ftw, (size_t)rf * dim * 8, hipMemcpyDeviceToDevice, st));
    if (rg > 0) {
        GCHK(tvk_dgemm(st, true, false, rg, dim, dim, 1.0, i_g.d, rg, 0, Si, dim, 0, 0.0, Gtw, dim, 0, 1));      // G^T S^-1
        GCHK(tvk_dgemm(st, false, false, rg, rg, dim, 1.0, Gtw, dim, 0, i_g.d, rg, 0, 0.0, GG, rg, 0, 1));        // G^T S^-1 G
        GCHK(tvk_add_identity(st, rg, GG));
        GCHK(tvk_dgemm(st, false, false, rf, rg, dim, 1.0, Ftw, dim, 0, i_g.d, rg, 0, 0.0, FtwG, rg, 0, 1));      // F^T S^-1 G
        if ((rc = ws.inverse_of(rg, GG, Mi, "plda_precompute: G^T S^-1 G + I"))) return rc;
        GCHK(tvk_dgemm(st, false, false, rf, rg, rg, 1.0, FtwG, rg, 0, Mi, rg, 0, 0.0, t1, rg, 0, 1));
        GCHK(tvk_dgemm(st, false, false, rf, dim, rg, -1.0, t1, rg, 0, Gtw, dim, 0, 1.0, o_j.d, dim, 0, 1));       // FTJ -= t1 Gtw
    }
    GCHK(tvk_dgemm(st, false, false, rf, rf, dim, 1.0, o_j.d, dim, 0, i_f.d, rf, 0, 0.0, o_jf.d, rf, 0, 1));
    if ((rc = o_j.finish())) return rc;
    return o_jf.finish();
}

int gmmiv_twocov_model(gmmiv_ctx *c, int dim, const double *W, const double *B, double *G, double *H)
{
    if (!c || dim <= 0 || !W || !B || !G || !H) { gmmiv_set_error("twocov_model: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t dd = (size_t)dim * dim;
    DevIn<double> i_w, i_b;
    DevOut<double> o_g, o_h;
    int rc;
    if ((rc = i_w.init(c, WS_T0, W, dd)) || (rc = i_b.init(c, WS_T1, B, dd)) || (rc = o_g.init(c, WS_T2, G, dd, false)) || (rc = o_h.init(c, WS_T3, H, dd, false))) return rc;
    SpdBatch ws;
    if ((rc = ws.reserve(c, dim, 1))) return rc;
    void *p;
    if ((rc = c->scratch(WS_AUX, 5 * dd * 8, &p))) return rc;
    double *iW = (double *)p, *iB = iW + dd, *sm = iB + dd, *ti = sm + dd, *t2 = ti + dd;
    hipStream_t st = c->stream;
    auto inv = [&](const double *src, double *dst, const char *what) { return ws.inverse_of(dim, src, dst, what); };
    if ((rc = inv(i_w.d, iW, "twocov_model: W")) || (rc = inv(i_b.d, iB, "twocov_model: B"))) return rc;
    for (int pass = 0; pass < 2; ++pass) { // G: B^-1 + 2 W^-1 ; H: B^-1 + W^-1
        GCHK(tvk_axpby(st, (long)dd, 1.0, iB, pass == 0 ? 2.0 : 1.0, iW, sm));
        if ((rc = inv(sm, ti, "twocov_model: B^-1 + a W^-1"))) return rc;
        GCHK(tvk_dgemm(st, false, false, dim, dim, dim, 1.0, iW, dim, 0, ti, dim, 0, 0.0, t2, dim, 0, 1));
        GCHK(tvk_dgemm(st, false, false, dim, dim, dim, 1.0, t2, dim, 0, iW, dim, 0, 0.0, pass == 0 ? o_g.d : o_h.d, dim, 0, 1));
    }
    if ((rc = o_g.finish())) return rc;
    return o_h.finish();
}

} // extern "C"
