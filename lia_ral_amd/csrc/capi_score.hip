// capi_score.hip -- C ABI of the score-normalisation calls (include/gmmiv.h, "score normalisation"); kernels: score_norm.hip.
#include "ctx.h"
#include "score_norm.h"

static int norm_err(const char *fmt, long a = 0, long b = 0, long c = 0)
{
    gmmiv_set_error(fmt, a, b, c);
    return GMMIV_ERR_ARG;
}

int gmmiv_score_cohort_stats(gmmiv_ctx *c, int64_t rows, int64_t cols, const double *scores, int64_t ld, int axis,
                             const unsigned char *select, const double *pre_mean, const double *pre_std, int mean_mode,
                             double percent_h, double percent_l, double *mean, double *std)
{
    if (!c) return norm_err("score_cohort_stats: ctx == NULL");
    if (rows < 0 || cols < 0) return norm_err("score_cohort_stats: negative shape %ld x %ld", (long)rows, (long)cols);
    if (axis != 0 && axis != 1) return norm_err("score_cohort_stats: axis %ld is neither 0 (rows) nor 1 (columns)", axis);
    if (mean_mode != 0 && mean_mode != 1) return norm_err("score_cohort_stats: mean_mode %ld is neither 0 (mean) nor 1 (median)", mean_mode);
    if (!(percent_h >= 0.0 && percent_h < 1.0) || !(percent_l >= 0.0 && percent_l < 1.0)) {
        gmmiv_set_error("score_cohort_stats: percent_h = %g, percent_l = %g must lie in [0, 1)", percent_h, percent_l);
        return GMMIV_ERR_ARG;
    }
    const int64_t ndist = axis == 0 ? rows : cols, L = axis == 0 ? cols : rows;
    if (ndist == 0) return GMMIV_OK;
    if (!mean || !std) return norm_err("score_cohort_stats: mean / std == NULL");
    if (!scores && L > 0) return norm_err("score_cohort_stats: scores == NULL");
    if (ld < cols) return norm_err("score_cohort_stats: ld = %ld is smaller than cols = %ld", (long)ld, (long)cols);
    if ((pre_mean == nullptr) != (pre_std == nullptr)) return norm_err("score_cohort_stats: pre_mean and pre_std go together");
    if (ndist > 0x7fffffff) { gmmiv_set_error("score_cohort_stats: too many distributions"); return GMMIV_ERR_UNSUPPORTED; }
    const bool dev_mask = select && gmmiv_is_device_ptr(select);
    const int sorted = percent_h != 0.0 || percent_l != 0.0; // ComputeNorm.cpp:127: the reference sorts when either is set
    long n = (long)L, dH = 0, dL = 0, qidx = 0;
    if (!dev_mask) {
        if (select) {
            n = 0;
            for (int64_t i = 0; i < L; ++i) n += select[i] != 0;
        }
        dH = (long)(unsigned long)((double)n * percent_h); // :125-126
        dL = (long)(unsigned long)((double)n * percent_l);
        if (n == 0 || dH + dL >= n)
            return norm_err("score_cohort_stats: empty kept range: a distribution of %ld scores with %ld + %ld discarded", n, dH, dL);
        qidx = n / 2;
        if (select) { // position of the (n / 2)-th selected score
            long k = 0;
            for (int64_t i = 0; i < L; ++i)
                if (select[i]) {
                    if (k == n / 2) { qidx = (long)i; break; }
                    ++k;
                }
        }
    } else if (L == 0)
        return norm_err("score_cohort_stats: empty kept range: a distribution of %ld scores", 0);
    GBIND(c);
    int rc;
    DevIn<double> x, pm, ps;
    DevIn<unsigned char> sel;
    DevOut<double> om, os;
    const size_t span = (size_t)(rows - 1) * (size_t)ld + (size_t)cols;
    if ((rc = x.init(c, WS_T2, scores, span)) || (rc = sel.init(c, WS_T0, select, (size_t)L)) ||
        (rc = pm.init(c, WS_T1, pre_mean, (size_t)L)) || (rc = ps.init(c, WS_T3, pre_std, (size_t)L)) ||
        (rc = om.init(c, WS_T4, mean, (size_t)ndist, false)) || (rc = os.init(c, WS_T5, std, (size_t)ndist, false)))
        return rc;
    long *info = nullptr;
    double *part = nullptr;
    const bool slabs = axis == 1 && mean_mode == 0 && !sorted; // the streaming column pass keeps its slab sums in the scratch
    if (dev_mask || slabs) {
        void *p;
        if ((rc = c->scratch(WS_NORM, SNK_INFO_BYTES + (slabs ? (size_t)SNK_PART_BYTES * (size_t)ndist : 0), &p))) return rc;
        if (dev_mask) {
            info = (long *)p;
            GCHK(snk_mask_info(c->stream, sel.d, (long)L, percent_h, percent_l, info));
        }
        if (slabs) part = (double *)((char *)p + SNK_INFO_BYTES);
    }
    c->t_begin("k_norm_stats"); // whichever of k_norm_rowsum / k_norm_colsum + k_norm_colfin / k_norm_select serves the call
    GCHK(snk_cohort_stats(c->stream, axis, (long)rows, (long)cols, x.d, (long)ld, sel.d, pm.d, ps.d, mean_mode, sorted, n, dH, dL, qidx,
                          info, part, om.d, os.d));
    c->t_end();
    if ((rc = om.finish())) return rc;
    return os.finish();
}

int gmmiv_score_normalize(gmmiv_ctx *c, int64_t M, int64_t S, double *scores, int order, const double *row_mean,
                          const double *row_std, const double *col_mean, const double *col_std, double *first_out)
{
    if (!c) return norm_err("score_normalize: ctx == NULL");
    if (M < 0 || S < 0) return norm_err("score_normalize: negative shape %ld x %ld", (long)M, (long)S);
    if (order < GMMIV_NORM_Z || order > GMMIV_NORM_TZ) return norm_err("score_normalize: unknown order %ld", order);
    const bool need_row = order != GMMIV_NORM_T, need_col = order != GMMIV_NORM_Z;
    if (need_row && (!row_mean || !row_std)) return norm_err("score_normalize: order %ld needs row_mean and row_std", order);
    if (need_col && (!col_mean || !col_std)) return norm_err("score_normalize: order %ld needs col_mean and col_std", order);
    if (M == 0 || S == 0) return GMMIV_OK;
    if (!scores) return norm_err("score_normalize: scores == NULL");
    if (M > 0x7fffffff) { gmmiv_set_error("score_normalize: too many rows"); return GMMIV_ERR_UNSUPPORTED; }
    GBIND(c);
    int rc;
    DevIn<double> rm, rs, cm, cs;
    DevOut<double> x, f;
    const bool two = order >= GMMIV_NORM_ZT;
    if ((rc = x.init(c, WS_T2, scores, (size_t)M * S, true)) || (rc = f.init(c, WS_T6, two ? first_out : nullptr, (size_t)M * S, false)) ||
        (rc = rm.init(c, WS_T0, need_row ? row_mean : nullptr, (size_t)M)) || (rc = rs.init(c, WS_T1, need_row ? row_std : nullptr, (size_t)M)) ||
        (rc = cm.init(c, WS_T3, need_col ? col_mean : nullptr, (size_t)S)) || (rc = cs.init(c, WS_T4, need_col ? col_std : nullptr, (size_t)S)))
        return rc;
    c->t_begin("k_norm_apply");
    GCHK(snk_apply(c->stream, (long)M, (long)S, x.d, order, rm.d, rs.d, cm.d, cs.d, f.d));
    c->t_end();
    if ((rc = x.finish())) return rc;
    return f.finish();
}

size_t gmmiv_ctx_workspace_bytes(gmmiv_ctx *c, int slot)
{
    if (!c) return 0;
    if (slot < 0) slot = WS_NORM;
    return slot < WS_COUNT ? c->ws_size[slot] : 0;
}
