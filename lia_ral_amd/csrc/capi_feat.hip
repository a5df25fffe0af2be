// capi_feat.hip -- C ABI (include/gmmiv.h): the entry points that read or rewrite FRAMES -- moments, gather / scatter, segment means,
// the unusable-frame count, feature-domain channel compensation and feature mapping, the NormFeat family.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "ctx.h"
#include "gmm_kernels.h"
#include "tv_kernels.h"
#include "capi_gmm_util.h"

extern "C" {

// ---- frame moments -------------------------------------------------------------------------
int gmmiv_frame_moments(gmmiv_ctx *c, const void *x, int dt, int64_t T, int64_t ldx, int D, double *acc)
{
    if (!c || !acc || T < 0 || D <= 0) { gmmiv_set_error("frame_moments: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    XView xv;
    int rc = xv.init(c, x, dt, T, ldx, D);
    if (rc) return rc;
    DevOut<double> o;
    if ((rc = o.init(c, WS_T0, acc, 2 * D + 1, true))) return rc;
    const int maxb = 2048;
    void *part;
    if ((rc = c->scratch(WS_PART, (size_t)maxb * 2 * D * sizeof(double), &part))) return rc;
    c->t_begin("k_frame_moments");
    GCHK(gmmk_frame_moments(c->stream, dt == GMMIV_F64, xv.d, T, xv.ldx, D, (double *)part, maxb, o.d));
    c->t_end();
    GCHK(gmmk_add_scalar(c->stream, o.d + 2 * D, (double)T));
    return o.finish();
}

// ---- frame selection -------------------------------------------------------------------------
int gmmiv_gather_frames(gmmiv_ctx *c, const void *x, int dt, int64_t ldx, int D, const int64_t *frame_idx, int64_t n,
                        void *out)
{
    if (!c || !x || !out || !frame_idx || n < 0 || D <= 0 || ldx < D) { gmmiv_set_error("gather_frames: bad argument"); return GMMIV_ERR_ARG; }
    if (!gmmiv_is_device_ptr(x) || !gmmiv_is_device_ptr(out)) { gmmiv_set_error("gather_frames: x and out must be device arrays"); return GMMIV_ERR_ARG; }
    GBIND(c);
    DevIn<int64_t> i_idx;
    int rc = i_idx.init(c, WS_T0, frame_idx, (size_t)n);
    if (rc) return rc;
    c->t_begin("k_gather_frames");
    GCHK(gmmk_gather_frames(c->stream, dt == GMMIV_F64, x, ldx, D, (const long *)i_idx.d, n, out));
    c->t_end();
    if (!gmmiv_is_device_ptr(frame_idx)) GCHK(hipStreamSynchronize(c->stream)); // host index list may be freed
    return GMMIV_OK;
}

int gmmiv_count_unusable_frames(gmmiv_ctx *c, const void *x, int dt, int64_t T, int64_t ldx, int D, int64_t *count)
{
    if (!c || !count || T < 0 || D <= 0) { gmmiv_set_error("count_unusable_frames: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    *count = 0;
    if (T == 0) return GMMIV_OK;
    XView xv;
    int rc = xv.init(c, x, dt, T, ldx, D);
    if (rc) return rc;
    void *p;
    const size_t fbytes = ((size_t)T + 15) / 16 * 16;
    if ((rc = c->scratch(WS_GFLAG, fbytes + 16, &p))) return rc;
    unsigned char *flag = (unsigned char *)p;
    int *any = (int *)(flag + fbytes);
    GCHK(hipMemsetAsync(flag, 0, fbytes + 16, c->stream));
    GCHK(gmmk_flag_frames(c->stream, dt == GMMIV_F64, xv.d, T, xv.ldx, D, flag, any));
    int h_any = 0;
    GCHK(hipMemcpyAsync(&h_any, any, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    GCHK(hipStreamSynchronize(c->stream));
    if (!h_any) return GMMIV_OK;
    std::vector<unsigned char> hf((size_t)T);
    GCHK(hipMemcpyAsync(hf.data(), flag, (size_t)T, hipMemcpyDeviceToHost, c->stream));
    GCHK(hipStreamSynchronize(c->stream));
    int64_t n = 0;
    for (int64_t t = 0; t < T; ++t) n += hf[t] ? 1 : 0;
    *count = n;
    return GMMIV_OK;
}

int gmmiv_gather_runs(gmmiv_ctx *c, const void *x, int dt, int64_t ldx, int D, const int64_t *runs, int64_t nrun, void *out)
{
    if (!c || !x || !out || (!runs && nrun > 0) || nrun < 0 || D <= 0 || ldx < D) { gmmiv_set_error("gather_runs: bad argument"); return GMMIV_ERR_ARG; }
    if (dt != GMMIV_F32 && dt != GMMIV_F64) { gmmiv_set_error("gather_runs: feature dtype must be GMMIV_F32 or GMMIV_F64"); return GMMIV_ERR_ARG; }
    if (!gmmiv_is_device_ptr(x) || !gmmiv_is_device_ptr(out)) { gmmiv_set_error("gather_runs: x and out must be device arrays"); return GMMIV_ERR_ARG; }
    if (nrun == 0) return GMMIV_OK;
    GBIND(c);
    DevIn<int64_t> i_runs;
    int rc = i_runs.init(c, WS_T0, runs, (size_t)nrun * 3);
    if (rc) return rc;
    c->t_begin("k_gather_runs");
    GCHK(gmmk_gather_runs(c->stream, dt == GMMIV_F64, x, ldx, D, (const long *)i_runs.d, nrun, out));
    c->t_end();
    if (!gmmiv_is_device_ptr(runs)) GCHK(hipStreamSynchronize(c->stream)); // the host table may be freed
    return GMMIV_OK;
}

int gmmiv_segment_means(gmmiv_ctx *c, const double *v, int64_t ld, int nrows, const int64_t *seg_begin, int64_t nseg, double *out)
{
    if (!c || !v || !seg_begin || !out || nrows < 0 || nseg < 0 || ld < 0) { gmmiv_set_error("segment_means: bad argument"); return GMMIV_ERR_ARG; }
    if (!gmmiv_is_device_ptr(v)) { gmmiv_set_error("segment_means: v must be a device array"); return GMMIV_ERR_ARG; }
    if (gmmiv_is_device_ptr(seg_begin)) { gmmiv_set_error("segment_means: seg_begin must be a host array"); return GMMIV_ERR_ARG; }
    for (int64_t s = 0; s < nseg; ++s)
        if (seg_begin[s] < 0 || seg_begin[s + 1] < seg_begin[s]) { gmmiv_set_error("segment_means: seg_begin must be non-negative and non-decreasing"); return GMMIV_ERR_ARG; }
    if (nseg > 0 && nrows > 1 && seg_begin[nseg] > ld) { gmmiv_set_error("segment_means: the last segment ends after the row stride"); return GMMIV_ERR_ARG; }
    const int64_t npair = (int64_t)nrows * nseg;
    if (npair == 0) return GMMIV_OK;
    GBIND(c);
    const int64_t PIECE = 8192;
    std::vector<long> tab; // items [3 x nitem] | pair_off [npair + 1] | pair_len [npair]
    std::vector<long> off(npair + 1, 0), len(npair, 0);
    for (int r = 0; r < nrows; ++r)
        for (int64_t s = 0; s < nseg; ++s) {
            const int64_t p = (int64_t)r * nseg + s;
            len[p] = (long)(seg_begin[s + 1] - seg_begin[s]);
            for (int64_t b = seg_begin[s]; b < seg_begin[s + 1]; b += PIECE) {
                tab.push_back(r); tab.push_back((long)b); tab.push_back((long)(b + PIECE < seg_begin[s + 1] ? b + PIECE : seg_begin[s + 1]));
            }
            off[p + 1] = (long)(tab.size() / 3);
        }
    const size_t nitem = tab.size() / 3;
    tab.insert(tab.end(), off.begin(), off.end());
    tab.insert(tab.end(), len.begin(), len.end());
    void *dtab, *part;
    int rc;
    if ((rc = c->scratch(WS_T8, tab.size() * sizeof(long), &dtab))) return rc;
    if ((rc = c->scratch(WS_T9, (nitem ? nitem : 1) * sizeof(double), &part))) return rc;
    DevOut<double> o;
    if ((rc = o.init(c, WS_T7, out, (size_t)npair, false))) return rc;
    GCHK(hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(long), hipMemcpyHostToDevice, c->stream));
    const long *di = (const long *)dtab;
    GCHK(gmmk_segment_means(c->stream, v, (long)ld, di, (long)nitem, (double *)part, di + 3 * nitem, di + 3 * nitem + npair + 1, (long)npair, o.d));
    GCHK(hipStreamSynchronize(c->stream)); // tab is a stack-lifetime vector
    return o.finish();
}

// ---- frames rewritten from the posteriors: feature-domain channel compensation, feature mapping ----------------------------
// argument checks shared by gmmiv_feat_compensate / gmmiv_feat_map: nothing is enqueued before they pass
static int feat_check_dtype(const char *who, int xdt, int odt)
{
    if ((xdt != GMMIV_F32 && xdt != GMMIV_F64) || (odt != GMMIV_F32 && odt != GMMIV_F64)) { gmmiv_set_error("%s: x_dtype / out_dtype must be GMMIV_F32 or GMMIV_F64", who); return GMMIV_ERR_ARG; }
    return GMMIV_OK;
}
static int feat_check(const char *who, const void *x, int xdt, int64_t T, int64_t ldx, const void *out, int odt, int64_t ldo, int D)
{
    if (T < 0 || ldx < D || ldo < D) { gmmiv_set_error("%s: T < 0 or a row stride below vectSize %d", who, D); return GMMIV_ERR_ARG; }
    if (T == 0) return GMMIV_OK;
    if (!x || !out) { gmmiv_set_error("%s: x or out == NULL", who); return GMMIV_ERR_ARG; }
    const uintptr_t xb = (uintptr_t)x, xe = xb + ((size_t)(T - 1) * ldx + D) * gmmiv_esize(xdt);
    const uintptr_t ob = (uintptr_t)out, oe = ob + ((size_t)(T - 1) * ldo + D) * gmmiv_esize(odt);
    const bool in_place = x == out && xdt == odt && ldx == ldo;
    if (!in_place && xb < oe && ob < xe) { gmmiv_set_error("%s: out overlaps x (only out == x with the same dtype and stride is allowed)", who); return GMMIV_ERR_ARG; }
    return GMMIV_OK;
}

// the same two checks for gmmiv_feat_compensate_models (capi_models.hip)
int gmmiv_feat_check_args(const char *who, const void *x, int xdt, int64_t T, int64_t ldx, const void *out, int odt, int64_t ldo, int D)
{
    const int rc = feat_check_dtype(who, xdt, odt);
    return rc ? rc : feat_check(who, x, xdt, T, ldx, out, odt, ldo, D);
}

int gmmiv_feat_compensate(gmmiv_ctx *c, const gmmiv_gmm *g, const void *x, int dt, int64_t T, int64_t ldx, const double *offset,
                          void *out, int odt, int64_t ldo)
{
    int rc = feat_check_dtype("feat_compensate", dt, odt);
    if (rc) return rc;
    if (!c || !g) { gmmiv_set_error("feat_compensate: NULL context or model"); return GMMIV_ERR_ARG; }
    if ((rc = check_model(c, g))) return rc;
    if (!offset) { gmmiv_set_error("feat_compensate: offset == NULL"); return GMMIV_ERR_ARG; }
    if ((rc = feat_check("feat_compensate", x, dt, T, ldx, out, odt, ldo, g->D))) return rc;
    if (T == 0) return GMMIV_OK;
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, g->D))) return rc;
    FeatOut o;
    if ((rc = o.init(c, out, odt, 0, T, ldo, g->D))) return rc;
    DevIn<double> i_off;
    if ((rc = i_off.init(c, WS_FEAT_M0, offset, (size_t)g->C * g->D))) return rc;
    if ((rc = count_unusable(c, xv, dt, T, g->D))) return rc;
    // Fast path: k_llk_mfma<WZ> leaves the scaled likelihoods of a frame chunk in the scratch, k_feat_comp streams them once,
    // contracts the posteriors against the offsets on the matrix cores and writes D values per frame -- no posterior array
    const int64_t Tcz = g->D <= 64 ? z_chunk_frames(c, g) : 0;
    if (Tcz > 0) {
        gmmk_zview z;
        double *lz;
        void *offp;
        if ((rc = gmmiv_z_reserve(c, g->nct, T < Tcz ? T : Tcz, true, &z, &lz))) return rc;
        if ((rc = c->scratch(WS_FEAT_OFF, gmmk_feat_offset_doubles(g->nct, g->D) * sizeof(double), &offp))) return rc;
        GCHK(gmmk_feat_pack_offset(c->stream, i_off.d, g->C, g->D, g->nct, (double *)offp));
        for (int64_t c0 = 0; c0 < T; c0 += Tcz) {
            const int64_t n = (T - c0) < Tcz ? (T - c0) : Tcz;
            if ((rc = llk_z_run(c, g, xv, dt, c0, n, lz, z, c0 == 0))) return rc;
            GCHK(count_dead(c, lz, n));
            c->t_begin("k_feat_comp", c0 == 0);
            GCHK(gmmk_feat_comp(c->stream, dt == GMMIV_F64, odt == GMMIV_F64, gmmiv_x_at(xv, dt, c0), xv.ldx, n, g->D, g->nct, z, (const double *)offp,
                                o.at(c0), o.ld));
            c->t_end();
        }
        return o.finish();
    }
    // Generic path (vectSize > 60, "stats_z" 0, no likelihood scratch): posteriors of a bounded frame chunk (512 MiB), P = gamma offset on
    // the fp64 GEMM, out = x - P.  The log-sums of ALL frames come first, so an in-place call never evaluates a rewritten frame.
    double *lse;
    if ((rc = run_lse(c, g, xv, dt, T, &lse))) return rc;
    int64_t per = (int64_t)(((size_t)512 << 20) / ((size_t)g->C * sizeof(double))) / 2 * 2;
    if (per < 64) per = 64;
    const int64_t firstg = T < per ? T : per;
    void *gam, *pm;
    if ((rc = c->scratch(WS_Z, (size_t)firstg * g->C * sizeof(double), &gam))) return rc;
    if ((rc = c->scratch(WS_INV, (size_t)firstg * g->D * sizeof(double), &pm))) return rc;
    for (int64_t b = 0; b < T; b += per) {
        const int64_t m = T - b < per ? T - b : per;
        c->t_begin("k_posteriors", b == 0);
        GCHK(gmmk_posteriors(c->stream, dt == GMMIV_F64, gmmiv_x_at(xv, dt, b), (long)m, xv.ldx, g->D, g->C, g->Cp64, g->meanT, g->ivT, g->lwc, lse + b,
                             (double *)gam));
        c->t_end();
        GCHK(tvk_dgemm(c->stream, false, false, (int)m, g->D, g->C, 1.0, (const double *)gam, g->C, 0, i_off.d, g->D, 0, 0.0, (double *)pm, g->D, 0, 1));
        c->t_begin("k_feat_sub", b == 0);
        GCHK(gmmk_feat_sub(c->stream, dt == GMMIV_F64, odt == GMMIV_F64, gmmiv_x_at(xv, dt, b), xv.ldx, (long)m, g->D, (const double *)pm, lse + b, o.at(b), o.ld));
        c->t_end();
    }
    return o.finish();
}

int gmmiv_feat_map(gmmiv_ctx *c, const gmmiv_gmm *cd, const double *cd_mean, const double *cd_cov, const double *ci_mean,
                   const double *ci_cov, const void *x, int dt, int64_t T, int64_t ldx, void *out, int odt, int64_t ldo, int32_t *best)
{
    int rc = feat_check_dtype("feat_map", dt, odt);
    if (rc) return rc;
    if (!c || !cd) { gmmiv_set_error("feat_map: NULL context or model"); return GMMIV_ERR_ARG; }
    if ((rc = check_model(c, cd))) return rc;
    if (!cd_mean || !cd_cov || !ci_mean || !ci_cov) { gmmiv_set_error("feat_map: a model table is NULL"); return GMMIV_ERR_ARG; }
    if ((rc = feat_check("feat_map", x, dt, T, ldx, out, odt, ldo, cd->D))) return rc;
    if (T == 0) return GMMIV_OK;
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, cd->D))) return rc;
    FeatOut o;
    if ((rc = o.init(c, out, odt, 0, T, ldo, cd->D))) return rc;
    const size_t CD = (size_t)cd->C * cd->D;
    DevIn<double> m0, v0, m1, v1;
    if ((rc = m0.init(c, WS_FEAT_M0, cd_mean, CD)) || (rc = v0.init(c, WS_FEAT_M1, cd_cov, CD)) || (rc = m1.init(c, WS_FEAT_M2, ci_mean, CD)) ||
        (rc = v1.init(c, WS_FEAT_M3, ci_cov, CD))) return rc;
    int32_t *bd = best;
    if (!gmmiv_is_device_ptr(best)) {
        void *p;
        if ((rc = c->scratch(WS_FEAT_IDX, (size_t)T * sizeof(int32_t), &p))) return rc;
        bd = (int32_t *)p;
    }
    // getBestGaussian = the top-1 selection (strict `>` from 0: the lowest index on ties, index 0 when every term is 0).  The index
    // array starts at 0: the fused ranking kernel writes no index for a frame whose candidates are all PADDED Gaussians (a frame with an
    // unusable value under a model whose Gaussian count is no multiple of 16) -- 0 is what the rule gives such a frame.
    GCHK(hipMemsetAsync(bd, 0, (size_t)T * sizeof(int32_t), c->stream));
    if ((rc = gmmiv_llk_determine_top(c, cd, xv.d, dt, T, xv.ldx, 1, GMMIV_TOP_COMPLETE, -INFINITY, INFINITY, bd, nullptr, nullptr, nullptr, nullptr,
                                      nullptr))) return rc;
    c->t_begin("k_feat_map");
    GCHK(gmmk_feat_map(c->stream, dt == GMMIV_F64, odt == GMMIV_F64, xv.d, xv.ldx, T, cd->D, cd->C, bd, m0.d, v0.d, m1.d, v1.d, o.d, o.ld));
    c->t_end();
    if (best && bd != best) GCHK(hipMemcpyAsync(best, bd, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if ((rc = o.finish())) return rc;
    if (best && bd != best) GCHK(hipStreamSynchronize(c->stream));
    return GMMIV_OK;
}

int gmmiv_scatter_runs(gmmiv_ctx *c, void *x, int dt, int64_t ldx, int D, const int64_t *runs, int64_t nrun, const void *in)
{
    if (!c || !x || !in || (!runs && nrun > 0) || nrun < 0 || D <= 0 || ldx < D) { gmmiv_set_error("scatter_runs: bad argument"); return GMMIV_ERR_ARG; }
    if (dt != GMMIV_F32 && dt != GMMIV_F64) { gmmiv_set_error("scatter_runs: feature dtype must be GMMIV_F32 or GMMIV_F64"); return GMMIV_ERR_ARG; }
    if (!gmmiv_is_device_ptr(x) || !gmmiv_is_device_ptr(in)) { gmmiv_set_error("scatter_runs: x and in must be device arrays"); return GMMIV_ERR_ARG; }
    if (nrun == 0) return GMMIV_OK;
    GBIND(c);
    DevIn<int64_t> i_runs;
    int rc = i_runs.init(c, WS_T0, runs, (size_t)nrun * 3);
    if (rc) return rc;
    c->t_begin("k_scatter_runs");
    GCHK(gmmk_scatter_runs(c->stream, dt == GMMIV_F64, x, ldx, D, (const long *)i_runs.d, nrun, in));
    c->t_end();
    if (!gmmiv_is_device_ptr(runs)) GCHK(hipStreamSynchronize(c->stream)); // the host table may be freed
    return GMMIV_OK;
}

// ---- cepstral mean / variance normalisation: NormFeat's default mode and NormFeatWindowMode's online mode ---------------------------
// A HOST run table is validated before anything is enqueued (a device table is not read here): lengths >= 0, group ids non-decreasing
// and inside [0, ngroups).  lo / hi (nullable): the frame range the runs cover.
static int norm_check_runs(const char *who, const int64_t *runs, int64_t nrun, int64_t ngroups, int64_t *lo, int64_t *hi)
{
    int64_t prev = 0, a = INT64_MAX, b = 0;
    for (int64_t r = 0; r < nrun; ++r) {
        const int64_t first = runs[3 * r], len = runs[3 * r + 1], g = runs[3 * r + 2];
        if (first < 0 || len < 0) { gmmiv_set_error("%s: run %ld has a negative first frame or length", who, (long)r); return GMMIV_ERR_ARG; }
        if (g < prev || g >= ngroups) { gmmiv_set_error("%s: run %ld: group %ld is below its predecessor's or outside [0, %ld) (group ids must be non-decreasing)", who, (long)r, (long)g, (long)ngroups); return GMMIV_ERR_ARG; }
        prev = g;
        if (len > 0) { if (first < a) a = first; if (first + len > b) b = first + len; }
    }
    if (lo) *lo = a == INT64_MAX ? 0 : a;
    if (hi) *hi = b;
    return GMMIV_OK;
}
// frames [lo, hi) of x and out: out may be exactly x (pointer, dtype, stride), any other overlap is refused (the rule of feat_check)
static int norm_check_overlap(const char *who, const void *x, int xdt, int64_t ldx, const void *out, int odt, int64_t ldo, int D, int64_t lo, int64_t hi)
{
    const bool in_place = x == out && xdt == odt && ldx == ldo;
    if (in_place || hi <= lo) return GMMIV_OK;
    const uintptr_t xb = (uintptr_t)x + (size_t)lo * ldx * gmmiv_esize(xdt), xe = (uintptr_t)x + ((size_t)(hi - 1) * ldx + D) * gmmiv_esize(xdt);
    const uintptr_t ob = (uintptr_t)out + (size_t)lo * ldo * gmmiv_esize(odt), oe = (uintptr_t)out + ((size_t)(hi - 1) * ldo + D) * gmmiv_esize(odt);
    if (xb < oe && ob < xe) { gmmiv_set_error("%s: out overlaps x (only out == x with the same dtype and stride is allowed)", who); return GMMIV_ERR_ARG; }
    return GMMIV_OK;
}

int gmmiv_frame_moments_groups(gmmiv_ctx *c, const void *x, int dt, int64_t ldx, int D, const int64_t *runs, int64_t nrun, int64_t ngroups,
                               double *acc)
{
    if (dt != GMMIV_F32 && dt != GMMIV_F64) { gmmiv_set_error("frame_moments_groups: x_dtype must be GMMIV_F32 or GMMIV_F64"); return GMMIV_ERR_ARG; }
    if (nrun < 0 || ngroups < 0 || D <= 0 || ldx < D || (!runs && nrun > 0)) { gmmiv_set_error("frame_moments_groups: bad argument (nrun, ngroups < 0, D <= 0, ldx < D or runs == NULL)"); return GMMIV_ERR_ARG; }
    const bool host_runs = nrun > 0 && !gmmiv_is_device_ptr(runs);
    int rc;
    if (host_runs && (rc = norm_check_runs("frame_moments_groups", runs, nrun, ngroups, nullptr, nullptr))) return rc;
    if (!c) { gmmiv_set_error("frame_moments_groups: NULL context"); return GMMIV_ERR_ARG; }
    if (nrun == 0 || ngroups == 0) return GMMIV_OK;
    if (!acc || !x) { gmmiv_set_error("frame_moments_groups: x or acc == NULL"); return GMMIV_ERR_ARG; }
    if (!gmmiv_is_device_ptr(x)) { gmmiv_set_error("frame_moments_groups: x must be a device array"); return GMMIV_ERR_ARG; }
    GBIND(c);
    DevIn<int64_t> i_runs;
    if ((rc = i_runs.init(c, WS_T0, runs, (size_t)nrun * 3))) return rc;
    DevOut<double> o;
    if ((rc = o.init(c, WS_T1, acc, (size_t)ngroups * (2 * D + 1), true))) return rc;
    void *part;
    if ((rc = c->scratch(WS_PART, (size_t)nrun * 2 * D * sizeof(double), &part))) return rc;
    c->t_begin("k_moments_groups");
    GCHK(gmmk_moments_groups(c->stream, dt == GMMIV_F64, x, ldx, D, (const long *)i_runs.d, nrun, ngroups, (double *)part, o.d));
    c->t_end();
    if ((rc = o.finish())) return rc;
    if (host_runs && !o.host) GCHK(hipStreamSynchronize(c->stream)); // the host table may be freed
    return GMMIV_OK;
}

int gmmiv_frame_moments_stats(gmmiv_ctx *c, int64_t ngroups, int D, const double *acc, double *mean, double *std)
{
    if (!c) { gmmiv_set_error("frame_moments_stats: NULL context"); return GMMIV_ERR_ARG; }
    if (ngroups < 0 || D <= 0) { gmmiv_set_error("frame_moments_stats: ngroups < 0 or D <= 0"); return GMMIV_ERR_ARG; }
    if (ngroups == 0) return GMMIV_OK;
    if (!acc || !mean || !std) { gmmiv_set_error("frame_moments_stats: acc, mean or std == NULL"); return GMMIV_ERR_ARG; }
    GBIND(c);
    int rc;
    DevIn<double> i_acc;
    if ((rc = i_acc.init(c, WS_T1, acc, (size_t)ngroups * (2 * D + 1)))) return rc;
    DevOut<double> om, os;
    if ((rc = om.init(c, WS_FEAT_M0, mean, (size_t)ngroups * D, false)) || (rc = os.init(c, WS_FEAT_M1, std, (size_t)ngroups * D, false))) return rc;
    c->t_begin("k_moments_stats");
    GCHK(gmmk_moments_stats(c->stream, ngroups, D, i_acc.d, om.d, os.d));
    c->t_end();
    if ((rc = om.finish()) || (rc = os.finish())) return rc;
    if (!gmmiv_is_device_ptr(acc) && !om.host && !os.host) GCHK(hipStreamSynchronize(c->stream)); // the host accumulator may be freed
    return GMMIV_OK;
}

int gmmiv_feat_norm_apply(gmmiv_ctx *c, const void *x, int dt, int64_t ldx, int D, const int64_t *runs, int64_t nrun, int64_t ngroups,
                          const double *mean, const double *std, void *out, int odt, int64_t ldo)
{
    int rc = feat_check_dtype("feat_norm_apply", dt, odt);
    if (rc) return rc;
    if (nrun < 0 || ngroups < 0 || D <= 0 || ldx < D || ldo < D || (!runs && nrun > 0)) { gmmiv_set_error("feat_norm_apply: bad argument (nrun, ngroups < 0, D <= 0, a row stride below D or runs == NULL)"); return GMMIV_ERR_ARG; }
    const bool host_runs = nrun > 0 && !gmmiv_is_device_ptr(runs);
    int64_t lo = 0, hi = 0;
    if (host_runs && (rc = norm_check_runs("feat_norm_apply", runs, nrun, ngroups, &lo, &hi))) return rc;
    if (!c) { gmmiv_set_error("feat_norm_apply: NULL context"); return GMMIV_ERR_ARG; }
    if (nrun == 0) return GMMIV_OK;
    if (!x || !out) { gmmiv_set_error("feat_norm_apply: x or out == NULL"); return GMMIV_ERR_ARG; }
    if (x == out && (dt != odt || ldx != ldo)) { gmmiv_set_error("feat_norm_apply: out overlaps x (only out == x with the same dtype and stride is allowed)"); return GMMIV_ERR_ARG; }
    if (host_runs && (rc = norm_check_overlap("feat_norm_apply", x, dt, ldx, out, odt, ldo, D, lo, hi))) return rc;
    if (!gmmiv_is_device_ptr(x) || !gmmiv_is_device_ptr(out)) { gmmiv_set_error("feat_norm_apply: x and out must be device arrays"); return GMMIV_ERR_ARG; }
    GBIND(c);
    DevIn<int64_t> i_runs;
    if ((rc = i_runs.init(c, WS_T0, runs, (size_t)nrun * 3))) return rc;
    DevIn<double> i_mean, i_std;
    if ((rc = i_mean.init(c, WS_FEAT_M0, mean, (size_t)ngroups * D)) || (rc = i_std.init(c, WS_FEAT_M1, std, (size_t)ngroups * D))) return rc;
    c->t_begin("k_feat_norm_apply");
    GCHK(gmmk_feat_norm_apply(c->stream, dt == GMMIV_F64, odt == GMMIV_F64, x, ldx, D, (const long *)i_runs.d, nrun, ngroups, i_mean.d, i_std.d, out, ldo));
    c->t_end();
    if (host_runs || (mean && !gmmiv_is_device_ptr(mean)) || (std && !gmmiv_is_device_ptr(std))) GCHK(hipStreamSynchronize(c->stream)); // host arrays may be freed
    return GMMIV_OK;
}

int gmmiv_feat_norm_online(gmmiv_ctx *c, const void *x, int dt, int64_t ldx, int D, const int64_t *file_begin, int64_t nfiles, int64_t window,
                           int64_t look_ahead, void *out, int odt, int64_t ldo)
{
    int rc = feat_check_dtype("feat_norm_online", dt, odt);
    if (rc) return rc;
    if (nfiles < 0 || D <= 0 || ldx < D || ldo < D || window < 1 || look_ahead < 0 || (!file_begin && nfiles > 0)) { gmmiv_set_error("feat_norm_online: bad argument (nfiles < 0, D <= 0, a row stride below D, window < 1, look_ahead < 0 or file_begin == NULL)"); return GMMIV_ERR_ARG; }
    const bool host_tab = nfiles > 0 && !gmmiv_is_device_ptr(file_begin);
    if (host_tab)
        for (int64_t f = 0; f < nfiles; ++f)
            if (file_begin[f] < 0 || file_begin[f + 1] < file_begin[f]) { gmmiv_set_error("feat_norm_online: file_begin must be non-negative and non-decreasing (file %ld)", (long)f); return GMMIV_ERR_ARG; }
    if (!c) { gmmiv_set_error("feat_norm_online: NULL context"); return GMMIV_ERR_ARG; }
    if (nfiles == 0 || (host_tab && file_begin[nfiles] == file_begin[0])) return GMMIV_OK;
    if (!x || !out) { gmmiv_set_error("feat_norm_online: x or out == NULL"); return GMMIV_ERR_ARG; }
    if (x == out && (dt != odt || ldx != ldo)) { gmmiv_set_error("feat_norm_online: out overlaps x (only out == x with the same dtype and stride is allowed)"); return GMMIV_ERR_ARG; }
    if (host_tab && (rc = norm_check_overlap("feat_norm_online", x, dt, ldx, out, odt, ldo, D, file_begin[0], file_begin[nfiles]))) return rc;
    if (!gmmiv_is_device_ptr(x) || !gmmiv_is_device_ptr(out)) { gmmiv_set_error("feat_norm_online: x and out must be device arrays"); return GMMIV_ERR_ARG; }
    GBIND(c);
    // The scan's scratch is sized by the number of chunks.  A host table gives it; with a device table (never read back: the call only
    // enqueues) the frames that fit between x and the end of its allocation bound it.
    int64_t frames;
    if (host_tab) frames = file_begin[nfiles] - file_begin[0];
    else {
        void *base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange((hipDeviceptr_t *)&base, &size, (hipDeviceptr_t)x) != hipSuccess) { (void)hipGetLastError(); gmmiv_set_error("feat_norm_online: the allocation of x is unknown to the runtime; pass file_begin as a host array"); return GMMIV_ERR_ARG; }
        frames = (int64_t)(((uintptr_t)base + size - (uintptr_t)x) / ((size_t)ldx * gmmiv_esize(dt))) + 1;
    }
    const long L = (long)(look_ahead < window ? look_ahead : window);
    const size_t units = gmmk_online_units((long)nfiles, (long)frames);
    DevIn<int64_t> i_fb;
    if ((rc = i_fb.init(c, WS_T0, file_begin, (size_t)nfiles + 1))) return rc;
    void *off, *state, *decay;
    if ((rc = c->scratch(WS_NORM_OFF, ((size_t)nfiles + 1) * sizeof(int64_t), &off)) || (rc = c->scratch(WS_NORM_STATE, units * D * 2 * sizeof(double), &state)) ||
        (rc = c->scratch(WS_NORM_DECAY, units * sizeof(double), &decay))) return rc;
    c->t_begin("k_feat_norm_online");
    GCHK(gmmk_feat_norm_online(c->stream, c->n_cu, dt == GMMIV_F64, odt == GMMIV_F64, x, ldx, D, (const long *)i_fb.d, (long)nfiles, (long)window, L, (long)units,
                               (long *)off, (double *)state, (double *)decay, out, ldo));
    c->t_end();
    if (host_tab) GCHK(hipStreamSynchronize(c->stream)); // the host table may be freed
    return GMMIV_OK;
}

// ---- EnergyDetector on resident frames: a model, a threshold and the output segments per file (energy_det.hip) ------------------------
static int energy_check(const char *who, gmmiv_ctx *c, const void *x, int dt, int64_t ldx, const int64_t *runs, int64_t nrun, int64_t nfiles, bool *host_runs)
{
    if (dt != GMMIV_F32 && dt != GMMIV_F64) { gmmiv_set_error("%s: x_dtype must be GMMIV_F32 or GMMIV_F64", who); return GMMIV_ERR_ARG; }
    if (nrun < 0 || nfiles < 0 || ldx < 1 || (!runs && nrun > 0)) { gmmiv_set_error("%s: bad argument (nrun, nfiles < 0, ldx < 1 or runs == NULL)", who); return GMMIV_ERR_ARG; }
    *host_runs = nrun > 0 && !gmmiv_is_device_ptr(runs);
    int rc;
    if (*host_runs && (rc = norm_check_runs(who, runs, nrun, nfiles, nullptr, nullptr))) return rc;
    if (!c) { gmmiv_set_error("%s: NULL context", who); return GMMIV_ERR_ARG; }
    if (nrun > 0 && (!x || !gmmiv_is_device_ptr(x))) { gmmiv_set_error("%s: x must be a device array", who); return GMMIV_ERR_ARG; }
    return GMMIV_OK;
}

int64_t gmmiv_energy_stage_frames(int x_dtype) { return x_dtype == GMMIV_F32 || x_dtype == GMMIV_F64 ? (int64_t)gmmk_energy_stage_frames(x_dtype == GMMIV_F64) : 0; }

int gmmiv_energy_train(gmmiv_ctx *c, const void *x, int dt, int64_t ldx, const int64_t *runs, int64_t nrun, int64_t nfiles, int C, int nb_train_it,
                       double flooring, double ceiling, double alpha, double *model, double *threshold, int32_t *status)
{
    if (C < 1 || C > GMMIV_ENERGY_MAX_C) { gmmiv_set_error("energy_train: C = %d outside 1 .. %d", C, GMMIV_ENERGY_MAX_C); return GMMIV_ERR_ARG; }
    if (nb_train_it < 0) { gmmiv_set_error("energy_train: nb_train_it < 0"); return GMMIV_ERR_ARG; }
    bool host_runs;
    int rc = energy_check("energy_train", c, x, dt, ldx, runs, nrun, nfiles, &host_runs);
    if (rc) return rc;
    if (nfiles == 0) return GMMIV_OK;
    if (!model || !threshold || !status) { gmmiv_set_error("energy_train: model, threshold or status == NULL"); return GMMIV_ERR_ARG; }
    GBIND(c);
    // the host plan: the files longest first (a workgroup is a file), and the longest selection sizes the LDS of the launch.  With a
    // device table neither is known: table order, the whole staging budget.  Neither changes a bit of any file's result.
    std::vector<long> order;
    long max_frames = -1;
    if (host_runs || nrun == 0) {
        std::vector<int64_t> n((size_t)nfiles, 0);
        for (int64_t r = 0; r < nrun; ++r) n[(size_t)runs[3 * r + 2]] += runs[3 * r + 1];
        order.resize((size_t)nfiles);
        for (int64_t f = 0; f < nfiles; ++f) order[(size_t)f] = (long)f;
        std::stable_sort(order.begin(), order.end(), [&](long a, long b) { return n[(size_t)a] > n[(size_t)b]; });
        max_frames = (long)n[(size_t)order[0]];
    }
    DevIn<int64_t> i_runs;
    if ((rc = i_runs.init(c, WS_T0, runs, (size_t)nrun * 3))) return rc;
    DevIn<long> i_order;
    if ((rc = i_order.init(c, WS_T1, order.empty() ? nullptr : order.data(), order.size()))) return rc;
    DevOut<double> o_model, o_th;
    DevOut<int32_t> o_st;
    if ((rc = o_model.init(c, WS_T2, model, (size_t)nfiles * 3 * C, false)) || (rc = o_th.init(c, WS_T3, threshold, (size_t)nfiles, false)) ||
        (rc = o_st.init(c, WS_T4, status, (size_t)nfiles, false))) return rc;
    c->t_begin("k_energy_em");
    GCHK(gmmk_energy_em(c->stream, dt == GMMIV_F64, x, ldx, (const long *)i_runs.d, nrun, nfiles, i_order.d, max_frames, C, nb_train_it, flooring, ceiling, alpha,
                        o_model.d, o_th.d, (int *)o_st.d));
    c->t_end();
    if ((rc = o_model.finish()) || (rc = o_th.finish()) || (rc = o_st.finish())) return rc;
    if (!order.empty() || host_runs) GCHK(hipStreamSynchronize(c->stream)); // the host tables may be freed
    return GMMIV_OK;
}

int gmmiv_energy_select(gmmiv_ctx *c, const void *x, int dt, int64_t ldx, const int64_t *runs, int64_t nrun, int64_t nfiles, const double *threshold,
                        int64_t *n_above, int64_t *seg_count, const int64_t *seg_off, int64_t *seg_begin, int64_t *seg_len)
{
    bool host_runs;
    int rc = energy_check("energy_select", c, x, dt, ldx, runs, nrun, nfiles, &host_runs);
    if (rc) return rc;
    if ((seg_begin == nullptr) != (seg_len == nullptr)) { gmmiv_set_error("energy_select: seg_begin and seg_len go together"); return GMMIV_ERR_ARG; }
    if (nfiles == 0) return GMMIV_OK;
    if (!threshold) { gmmiv_set_error("energy_select: threshold == NULL"); return GMMIV_ERR_ARG; }
    if (seg_begin && !seg_off) { gmmiv_set_error("energy_select: seg_off == NULL with seg_begin"); return GMMIV_ERR_ARG; }
    const bool host_off = seg_begin && !gmmiv_is_device_ptr(seg_off);
    size_t room = 0;
    if (host_off) {
        for (int64_t f = 0; f < nfiles; ++f)
            if (seg_off[f] < 0 || seg_off[f + 1] < seg_off[f]) { gmmiv_set_error("energy_select: seg_off must be non-negative and non-decreasing (file %ld)", (long)f); return GMMIV_ERR_ARG; }
        room = (size_t)seg_off[nfiles];
    } else if (seg_begin && (!gmmiv_is_device_ptr(seg_begin) || !gmmiv_is_device_ptr(seg_len))) { gmmiv_set_error("energy_select: host seg_begin / seg_len need a host seg_off"); return GMMIV_ERR_ARG; }
    GBIND(c);
    DevIn<int64_t> i_runs, i_off;
    DevIn<double> i_th;
    if ((rc = i_runs.init(c, WS_T0, runs, (size_t)nrun * 3)) || (rc = i_th.init(c, WS_T3, threshold, (size_t)nfiles)) ||
        (rc = i_off.init(c, WS_T7, seg_begin ? seg_off : nullptr, (size_t)nfiles + 1))) return rc;
    DevOut<int64_t> o_above, o_cnt, o_beg, o_len;
    if ((rc = o_above.init(c, WS_T5, n_above, (size_t)nfiles, false)) || (rc = o_cnt.init(c, WS_T6, seg_count, (size_t)nfiles, false)) ||
        (rc = o_beg.init(c, WS_T8, seg_begin, room, false)) || (rc = o_len.init(c, WS_T9, seg_len, room, false))) return rc;
    c->t_begin("k_energy_select");
    GCHK(gmmk_energy_select(c->stream, dt == GMMIV_F64, x, ldx, (const long *)i_runs.d, nrun, nfiles, i_th.d, (long *)o_above.d, (long *)o_cnt.d, (const long *)i_off.d,
                            (long *)o_beg.d, (long *)o_len.d));
    c->t_end();
    if ((rc = o_above.finish()) || (rc = o_cnt.finish()) || (rc = o_beg.finish()) || (rc = o_len.finish())) return rc;
    if (host_runs || host_off || !gmmiv_is_device_ptr(threshold)) GCHK(hipStreamSynchronize(c->stream)); // host arrays may be freed
    return GMMIV_OK;
}

} // extern "C"
