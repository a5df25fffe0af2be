// capi_score_lists.hip -- C ABI of score normalisation on lists (include/gmmiv.h, "score normalisation on lists") and its host
// planner gmmiv_plan_score_lists; kernels: score_norm_lists.hip.  DESIGN.md section 3.17.
#include "ctx.h"
#include "score_norm_lists.h"

static int list_err(const char *fmt, long a = 0, long b = 0, long c = 0)
{
    gmmiv_set_error(fmt, a, b, c);
    return GMMIV_ERR_ARG;
}

// The launch shapes of the dense call as a function of the row length (snk_cohort_stats, score_norm.hip): they fix the summation
// order, so a distribution of a list gets the shape of a row of its length.
int gmmiv_score_list_class(int64_t n, int streaming, int *threads, int64_t *stage_scores)
{
    int cls, thr;
    int64_t stage = 0;
    if (streaming) {
        cls = n <= 4096 ? 0 : 1; // SN_WAVE_ROW
        thr = cls ? 256 : 64;
    } else {
        static const int64_t top[GMMIV_SCORE_LIST_CLASSES - 1] = {512, 1024, 2048, 4096, 8192, 16384}; // 8 scores per thread, SN_STAGE
        cls = 0;
        while (cls < GMMIV_SCORE_LIST_CLASSES - 1 && n > top[cls]) ++cls;
        thr = cls >= 4 ? 1024 : 64 << cls;
        stage = cls < GMMIV_SCORE_LIST_CLASSES - 1 ? top[cls] : 0;
    }
    if (threads) *threads = thr;
    if (stage_scores) *stage_scores = stage;
    return cls;
}

int64_t gmmiv_plan_score_lists(int64_t ndist, const int64_t *off, int streaming, int32_t *cls, int32_t *order, int64_t *class_begin)
{
    if (ndist < 0 || ndist > 0x7fffffff || !off || off[0] < 0) return -1;
    int64_t cnt[GMMIV_SCORE_LIST_CLASSES + 1] = {};
    for (int64_t d = 0; d < ndist; ++d) {
        if (off[d + 1] < off[d]) return -1;
        const int k = gmmiv_score_list_class(off[d + 1] - off[d], streaming, nullptr, nullptr);
        if (cls) cls[d] = k;
        cnt[k + 1]++;
    }
    int64_t used = 0;
    for (int k = 0; k < GMMIV_SCORE_LIST_CLASSES; ++k) { used += cnt[k + 1] > 0; cnt[k + 1] += cnt[k]; }
    if (class_begin)
        for (int k = 0; k <= GMMIV_SCORE_LIST_CLASSES; ++k) class_begin[k] = cnt[k];
    if (order) { // table order inside a class
        int64_t at[GMMIV_SCORE_LIST_CLASSES];
        for (int k = 0; k < GMMIV_SCORE_LIST_CLASSES; ++k) at[k] = cnt[k];
        for (int64_t d = 0; d < ndist; ++d)
            order[at[gmmiv_score_list_class(off[d + 1] - off[d], streaming, nullptr, nullptr)]++] = (int32_t)d;
    }
    return used;
}

int gmmiv_score_list_stats(gmmiv_ctx *c, int64_t ndist, const int64_t *off, const int64_t *pos, const double *scores, int64_t nscores,
                           const int32_t *pre_id, const double *pre_mean, const double *pre_std, int64_t npre, int mean_mode,
                           double percent_h, double percent_l, double *mean, double *std)
{
    // the arguments first: nothing here touches the context or a device
    if (ndist < 0 || nscores < 0 || npre < 0) return list_err("score_list_stats: negative count (ndist %ld, nscores %ld, npre %ld)", (long)ndist, (long)nscores, (long)npre);
    if (mean_mode != 0 && mean_mode != 1) return list_err("score_list_stats: mean_mode %ld is neither 0 (mean) nor 1 (median)", mean_mode);
    if (!(percent_h >= 0.0 && percent_h < 1.0) || !(percent_l >= 0.0 && percent_l < 1.0)) {
        gmmiv_set_error("score_list_stats: percent_h = %g, percent_l = %g must lie in [0, 1)", percent_h, percent_l);
        return GMMIV_ERR_ARG;
    }
    if ((pre_mean == nullptr) != (pre_std == nullptr)) return list_err("score_list_stats: pre_mean and pre_std go together");
    if ((pre_id == nullptr) != (pre_mean == nullptr)) return list_err("score_list_stats: pre_id goes with pre_mean and pre_std, and they with it");
    if (ndist > 0x7fffffff) { gmmiv_set_error("score_list_stats: too many distributions"); return GMMIV_ERR_UNSUPPORTED; }
    if (ndist > 0) {
        if (!off) return list_err("score_list_stats: off == NULL");
        if (gmmiv_is_device_ptr(off)) return list_err("score_list_stats: off must be a host array");
        if (off[0] < 0) return list_err("score_list_stats: off[0] = %ld is negative", (long)off[0]);
        const int sorted_ = percent_h != 0.0 || percent_l != 0.0;
        for (int64_t d = 0; d < ndist; ++d) {
            const long n = (long)(off[d + 1] - off[d]);
            if (n < 0) return list_err("score_list_stats: off decreases at distribution %ld (%ld -> %ld)", (long)d, (long)off[d], (long)off[d + 1]);
            if (n == 0) return list_err("score_list_stats: distribution %ld has 0 scores: empty impostor cohort", (long)d);
            if (sorted_) {
                const long dH = (long)(unsigned long)((double)n * percent_h), dL = (long)(unsigned long)((double)n * percent_l); // :129-130
                if (dH + dL >= n) {
                    gmmiv_set_error("score_list_stats: distribution %ld: empty kept range, %ld scores with %ld + %ld discarded: empty impostor cohort",
                                    (long)d, n, dH, dL);
                    return GMMIV_ERR_ARG;
                }
            }
        }
        if (!mean || !std) return list_err("score_list_stats: mean / std == NULL");
        if (!scores) return list_err("score_list_stats: scores == NULL");
        if (!pos && off[ndist] > nscores) return list_err("score_list_stats: the list ends at slot %ld, beyond nscores = %ld", (long)off[ndist], (long)nscores);
        auto dist_of = [&](int64_t k) { // the distribution that owns slot k
            int64_t lo = 0, hi = ndist;
            while (hi - lo > 1) { const int64_t mid = (lo + hi) / 2; (off[mid] <= k ? lo : hi) = mid; }
            return (long)lo;
        };
        if (pos && !gmmiv_is_device_ptr(pos))
            for (int64_t k = off[0]; k < off[ndist]; ++k)
                if (pos[k] < 0 || pos[k] >= nscores) {
                    gmmiv_set_error("score_list_stats: distribution %ld: pos[%ld] = %ld outside [0, %ld)", dist_of(k), (long)k, (long)pos[k], (long)nscores);
                    return GMMIV_ERR_ARG;
                }
        if (pre_id && !gmmiv_is_device_ptr(pre_id))
            for (int64_t k = off[0]; k < off[ndist]; ++k)
                if (pre_id[k] < 0 || pre_id[k] >= npre) {
                    gmmiv_set_error("score_list_stats: distribution %ld: pre_id[%ld] = %ld outside [0, %ld)", dist_of(k), (long)k, (long)pre_id[k], (long)npre);
                    return GMMIV_ERR_ARG;
                }
    }
    if (!c) return list_err("score_list_stats: ctx == NULL");
    if (ndist == 0) return GMMIV_OK;

    const int sorted = percent_h != 0.0 || percent_l != 0.0; // ComputeNorm.cpp:127: the reference sorts when either is set
    const int streaming = mean_mode == 0 && !sorted;
    std::vector<long> h_off((size_t)ndist + 1);
    std::vector<int32_t> h_ids((size_t)ndist);
    int64_t cb[GMMIV_SCORE_LIST_CLASSES + 1];
    for (int64_t d = 0; d <= ndist; ++d) h_off[(size_t)d] = (long)off[d];
    if (gmmiv_plan_score_lists(ndist, off, streaming, nullptr, h_ids.data(), cb) < 0) return list_err("score_list_stats: bad offsets");

    GBIND(c);
    int rc;
    const long k0 = (long)off[0], total = (long)(off[ndist] - off[0]);
    DevIn<double> x, pm, ps;
    DevIn<long> dp;
    DevIn<int> di;
    DevOut<double> om, os;
    const bool host_pos = pos && !gmmiv_is_device_ptr(pos), host_pre = pre_id && !gmmiv_is_device_ptr(pre_id);
    if ((rc = x.init(c, WS_T2, scores, (size_t)nscores)) ||
        (rc = dp.init(c, WS_T0, host_pos ? (const long *)pos + k0 : (const long *)pos, (size_t)total)) ||
        (rc = di.init(c, WS_T1, host_pre ? (const int *)pre_id + k0 : (const int *)pre_id, (size_t)total)) ||
        (rc = pm.init(c, WS_T3, pre_mean, (size_t)npre)) || (rc = ps.init(c, WS_T6, pre_std, (size_t)npre)) ||
        (rc = om.init(c, WS_T4, mean, (size_t)ndist, false)) || (rc = os.init(c, WS_T5, std, (size_t)ndist, false)))
        return rc;
    void *tab;
    if ((rc = c->scratch(WS_NORM, GMMIV_SCORE_LIST_SCRATCH_BYTES(ndist), &tab))) return rc;
    const long *d_off = (const long *)tab;
    const int *d_ids = (const int *)(d_off + ndist + 1);
    GCHK(hipMemcpyAsync(tab, h_off.data(), h_off.size() * sizeof(long), hipMemcpyHostToDevice, c->stream));
    GCHK(hipMemcpyAsync((void *)d_ids, h_ids.data(), h_ids.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    GCHK(hipStreamSynchronize(c->stream)); // the tables live in host vectors of this call
    bool first = true;
    for (int k = 0; k < GMMIV_SCORE_LIST_CLASSES; ++k) { // one launch per length class that occurs
        const long count = (long)(cb[k + 1] - cb[k]);
        if (count == 0) continue;
        c->t_begin("k_norm_stats", first); // k_norm_listsum or k_norm_select_lists, summed over the classes
        first = false;
        if (streaming)
            GCHK(snk_list_sum(c->stream, k, x.d, dp.d, di.d, host_pos ? k0 : 0, host_pre ? k0 : 0, pm.d, ps.d, d_off, d_ids + cb[k], count, om.d, os.d));
        else {
            int threads;
            int64_t stage;
            gmmiv_score_list_class((int64_t)512 << k, 0, &threads, &stage); // the longest length of class k (any length of the last one)
            GCHK(snk_list_select(c->stream, threads, sorted ? (size_t)stage * 8 : 0, x.d, dp.d, di.d, host_pos ? k0 : 0, host_pre ? k0 : 0, pm.d, ps.d,
                                 d_off, d_ids + cb[k], count, mean_mode, sorted, percent_h, percent_l, om.d, os.d));
        }
        c->t_end();
    }
    if ((rc = om.finish())) return rc;
    return os.finish();
}

int gmmiv_score_normalize_list(gmmiv_ctx *c, int64_t n, double *scores, int order, const int32_t *row_id, const double *row_mean,
                               const double *row_std, int64_t nrow, const int32_t *col_id, const double *col_mean, const double *col_std,
                               int64_t ncol, double *first_out)
{
    if (n < 0 || nrow < 0 || ncol < 0) return list_err("score_normalize_list: negative count (n %ld, nrow %ld, ncol %ld)", (long)n, (long)nrow, (long)ncol);
    if (order < GMMIV_NORM_Z || order > GMMIV_NORM_TZ) return list_err("score_normalize_list: unknown order %ld", order);
    const bool need_row = order != GMMIV_NORM_T, need_col = order != GMMIV_NORM_Z;
    if (need_row && (!row_id || !row_mean || !row_std)) return list_err("score_normalize_list: order %ld needs row_id, row_mean and row_std", order);
    if (need_col && (!col_id || !col_mean || !col_std)) return list_err("score_normalize_list: order %ld needs col_id, col_mean and col_std", order);
    if (n > 0 && !scores) return list_err("score_normalize_list: scores == NULL");
    if (need_row && n > 0 && !gmmiv_is_device_ptr(row_id))
        for (int64_t i = 0; i < n; ++i)
            if (row_id[i] < 0 || row_id[i] >= nrow) return list_err("score_normalize_list: row_id[%ld] = %ld outside [0, %ld)", (long)i, (long)row_id[i], (long)nrow);
    if (need_col && n > 0 && !gmmiv_is_device_ptr(col_id))
        for (int64_t i = 0; i < n; ++i)
            if (col_id[i] < 0 || col_id[i] >= ncol) return list_err("score_normalize_list: col_id[%ld] = %ld outside [0, %ld)", (long)i, (long)col_id[i], (long)ncol);
    if (!c) return list_err("score_normalize_list: ctx == NULL");
    if (n == 0) return GMMIV_OK;
    if (n > (int64_t)0x7fffffff * 256) { gmmiv_set_error("score_normalize_list: too many trials"); return GMMIV_ERR_UNSUPPORTED; }
    GBIND(c);
    int rc;
    DevIn<double> rm, rs, cm, cs;
    DevIn<int> ri, ci;
    DevOut<double> x, f;
    const bool two = order >= GMMIV_NORM_ZT;
    if ((rc = x.init(c, WS_T2, scores, (size_t)n, true)) || (rc = f.init(c, WS_T6, two ? first_out : nullptr, (size_t)n, false)) ||
        (rc = ri.init(c, WS_T7, need_row ? (const int *)row_id : nullptr, (size_t)n)) ||
        (rc = rm.init(c, WS_T0, need_row ? row_mean : nullptr, (size_t)nrow)) || (rc = rs.init(c, WS_T1, need_row ? row_std : nullptr, (size_t)nrow)) ||
        (rc = ci.init(c, WS_T8, need_col ? (const int *)col_id : nullptr, (size_t)n)) ||
        (rc = cm.init(c, WS_T3, need_col ? col_mean : nullptr, (size_t)ncol)) || (rc = cs.init(c, WS_T4, need_col ? col_std : nullptr, (size_t)ncol)))
        return rc;
    c->t_begin("k_norm_apply");
    GCHK(snk_apply_list(c->stream, (long)n, x.d, order, ri.d, rm.d, rs.d, ci.d, cm.d, cs.d, f.d));
    c->t_end();
    if ((rc = x.finish())) return rc;
    return f.finish();
}
