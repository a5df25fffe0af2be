// capi_feat_warp.hip -- C ABI (include/ext/gmmiv_feat_warp.h): NormFeat's `warp true` -- the checks on host tables and the two entry
// points that run a list of units in one launch each (feat_warp.hip).
#include <math.h>

#include "ctx.h"
#include "feat_warp.h"
#include "../../include/ext/gmmiv_feat_warp.h"

namespace {

// the checks on a host run table; *max_len: the longest unit, *rows: one past the last frame any run names
bool warp_check_runs(const char *fn, const int64_t *runs, int64_t nrun, int64_t nunits, int64_t *max_len, int64_t *rows)
{
    int64_t prev = 0, cur = 0, mx = 0, end = 0;
    for (int64_t r = 0; r < nrun; ++r) {
        const int64_t first = runs[3 * r], len = runs[3 * r + 1], u = runs[3 * r + 2];
        if (first < 0 || len < 0) { gmmiv_set_error("%s: run %ld has a negative first frame or length", fn, (long)r); return false; }
        if (u < prev || u >= nunits) { gmmiv_set_error("%s: run %ld: unit %ld is below its predecessor's or outside [0, %ld) (unit ids must be non-decreasing)", fn, (long)r, (long)u, (long)nunits); return false; }
        if (r > 0 && u == prev && runs[3 * (r - 1) + 2] == u) {
            if (first < runs[3 * (r - 1)]) { gmmiv_set_error("%s: run %ld of unit %ld begins before the run before it (the runs of a unit must be in frame order)", fn, (long)r, (long)u); return false; }
            if (first < runs[3 * (r - 1)] + runs[3 * (r - 1) + 1]) { gmmiv_set_error("%s: run %ld of unit %ld overlaps the run before it", fn, (long)r, (long)u); return false; }
        } else cur = 0;
        cur += len;
        if (cur > mx) mx = cur;
        if (len > 0 && first + len > end) end = first + len;
        prev = u;
    }
    *max_len = mx;
    *rows = end;
    return true;
}

} // namespace

extern "C" {

int gmmiv_feat_warp_hist(gmmiv_ctx *c, const void *x, int dt, int64_t ldx, int D, const int64_t *runs, int64_t nrun, int64_t nunits, int nbin,
                         int flags, double *bounds, double *count, int32_t *status)
{
    if (dt != GMMIV_F32 && dt != GMMIV_F64) { gmmiv_set_error("feat_warp_hist: x_dtype must be GMMIV_F32 or GMMIV_F64"); return GMMIV_ERR_ARG; }
    if (nrun < 0 || nunits < 0 || D <= 0 || ldx < D || (!runs && nrun > 0)) { gmmiv_set_error("feat_warp_hist: bad argument (nrun, nunits < 0, D <= 0, ldx < D or runs == NULL)"); return GMMIV_ERR_ARG; }
    if (nbin < 1 || nbin > GMMIV_WARP_MAX_BINS) { gmmiv_set_error("feat_warp_hist: nbin = %d is outside [1, %d]", nbin, GMMIV_WARP_MAX_BINS); return GMMIV_ERR_ARG; }
    if (flags & ~GMMIV_WARP_FORCE_SELECT) { gmmiv_set_error("feat_warp_hist: flags must be 0 or GMMIV_WARP_FORCE_SELECT"); return GMMIV_ERR_ARG; }
    if (nunits > 0 && (!bounds || !count || !status)) { gmmiv_set_error("feat_warp_hist: bounds, count or status == NULL"); return GMMIV_ERR_ARG; }
    if (nunits * (int64_t)D > 0x7fffffffLL) { gmmiv_set_error("feat_warp_hist: nunits * D = %ld exceeds 2^31 - 1", (long)(nunits * D)); return GMMIV_ERR_ARG; }
    const bool host_runs = nrun > 0 && !gmmiv_is_device_ptr(runs);
    int64_t max_len = -1, rows = 0;
    if (host_runs && !warp_check_runs("feat_warp_hist", runs, nrun, nunits, &max_len, &rows)) return GMMIV_ERR_ARG;
    if (nrun == 0) max_len = 0;
    if (!c) { gmmiv_set_error("feat_warp_hist: NULL context"); return GMMIV_ERR_ARG; }
    if (nunits == 0) return GMMIV_OK;
    if (nrun > 0 && (!x || !gmmiv_is_device_ptr(x))) { gmmiv_set_error("feat_warp_hist: x must be a device array"); return GMMIV_ERR_ARG; }
    GBIND(c);
    int rc;
    DevIn<int64_t> i_runs;
    if ((rc = i_runs.init(c, WS_T0, runs, (size_t)nrun * 3))) return rc;
    const size_t UD = (size_t)nunits * D;
    DevOut<double> o_b, o_c;
    DevOut<int32_t> o_s;
    if ((rc = o_b.init(c, WS_T1, bounds, UD * ((size_t)nbin + 1), false)) || (rc = o_c.init(c, WS_T2, count, UD * (size_t)nbin, false)) ||
        (rc = o_s.init(c, WS_T3, status, UD, false))) return rc;
    c->t_begin("k_warp_hist");
    GCHK(gmmk_warp_hist(c->stream, dt == GMMIV_F64, x, ldx, D, (const long *)i_runs.d, nrun, nunits, nbin, max_len, flags & GMMIV_WARP_FORCE_SELECT,
                        o_b.d, o_c.d, (int *)o_s.d));
    c->t_end();
    if ((rc = o_b.finish()) || (rc = o_c.finish()) || (rc = o_s.finish())) return rc;
    if (host_runs && !o_b.host && !o_c.host && !o_s.host) GCHK(hipStreamSynchronize(c->stream)); // the host table may be freed
    return GMMIV_OK;
}

int gmmiv_feat_warp_apply(gmmiv_ctx *c, const void *x, int dt, int64_t ldx, void *out, int odt, int64_t ldo, int D, const int64_t *runs, int64_t nrun,
                          int64_t nunits, int nbin, const double *bounds, const double *count, const int32_t *status, int nbin_t, const double *tbounds,
                          const double *tcount)
{
    if ((dt != GMMIV_F32 && dt != GMMIV_F64) || (odt != GMMIV_F32 && odt != GMMIV_F64)) { gmmiv_set_error("feat_warp_apply: x_dtype and out_dtype must be GMMIV_F32 or GMMIV_F64"); return GMMIV_ERR_ARG; }
    if (nrun < 0 || nunits < 0 || D <= 0 || ldx < D || ldo < D || (!runs && nrun > 0)) { gmmiv_set_error("feat_warp_apply: bad argument (nrun, nunits < 0, D <= 0, ldx < D, ldo < D or runs == NULL)"); return GMMIV_ERR_ARG; }
    if (nbin < 1 || nbin > GMMIV_WARP_MAX_BINS) { gmmiv_set_error("feat_warp_apply: nbin = %d is outside [1, %d]", nbin, GMMIV_WARP_MAX_BINS); return GMMIV_ERR_ARG; }
    if (nbin_t < 1 || !tbounds || !tcount) { gmmiv_set_error("feat_warp_apply: the target needs nbin_t >= 1, tbounds and tcount"); return GMMIV_ERR_ARG; }
    if (nunits > 0 && (!bounds || !count || !status)) { gmmiv_set_error("feat_warp_apply: bounds, count or status == NULL"); return GMMIV_ERR_ARG; }
    if (nunits * (int64_t)D > 0x7fffffffLL) { gmmiv_set_error("feat_warp_apply: nunits * D = %ld exceeds 2^31 - 1", (long)(nunits * D)); return GMMIV_ERR_ARG; }
    const bool in_place = out == (const void *)x;
    if (in_place && x && (odt != dt || ldo != ldx)) { gmmiv_set_error("feat_warp_apply: out == x needs the same dtype and stride (in place); any other overlap is refused"); return GMMIV_ERR_ARG; }
    const bool host_runs = nrun > 0 && !gmmiv_is_device_ptr(runs);
    const bool host_tb = !gmmiv_is_device_ptr(tbounds), host_tc = !gmmiv_is_device_ptr(tcount);
    int64_t max_len = -1, rows = 0;
    if (host_runs) {
        if (!warp_check_runs("feat_warp_apply", runs, nrun, nunits, &max_len, &rows)) return GMMIV_ERR_ARG;
        if (!in_place && x && out && rows > 0) {
            const char *x0 = (const char *)x, *x1 = x0 + ((size_t)(rows - 1) * ldx + D) * (dt == GMMIV_F64 ? 8 : 4);
            const char *o0 = (const char *)out, *o1 = o0 + ((size_t)(rows - 1) * ldo + D) * (odt == GMMIV_F64 ? 8 : 4);
            if (x0 < o1 && o0 < x1) { gmmiv_set_error("feat_warp_apply: out overlaps x without being x (the frames up to %ld of both)", (long)rows); return GMMIV_ERR_ARG; }
        }
    }
    if (host_tb)
        for (int i = 0; i < nbin_t; ++i)
            if (!(tbounds[i + 1] >= tbounds[i])) { gmmiv_set_error("feat_warp_apply: target bin %d: its upper bound is not >= its lower bound", i); return GMMIV_ERR_ARG; }
    if (host_tc)
        for (int i = 0; i < nbin_t; ++i)
            if (!(tcount[i] >= 0)) { gmmiv_set_error("feat_warp_apply: target bin %d: its count is not >= 0", i); return GMMIV_ERR_ARG; }
    if (!c) { gmmiv_set_error("feat_warp_apply: NULL context"); return GMMIV_ERR_ARG; }
    if (nunits == 0 || nrun == 0) return GMMIV_OK;
    if (!x || !gmmiv_is_device_ptr(x) || !out || !gmmiv_is_device_ptr(out)) { gmmiv_set_error("feat_warp_apply: x and out must be device arrays"); return GMMIV_ERR_ARG; }
    GBIND(c);
    int rc;
    const size_t UD = (size_t)nunits * D;
    DevIn<int64_t> i_runs;
    DevIn<double> i_b, i_c, i_tb, i_tc;
    DevIn<int32_t> i_s;
    if ((rc = i_runs.init(c, WS_T0, runs, (size_t)nrun * 3)) || (rc = i_b.init(c, WS_T1, bounds, UD * ((size_t)nbin + 1))) ||
        (rc = i_c.init(c, WS_T2, count, UD * (size_t)nbin)) || (rc = i_s.init(c, WS_T3, status, UD)) ||
        (rc = i_tb.init(c, WS_T4, tbounds, (size_t)nbin_t + 1)) || (rc = i_tc.init(c, WS_T5, tcount, (size_t)nbin_t))) return rc;
    void *tw;
    if ((rc = c->scratch(WS_T6, (2 * (size_t)nbin_t + 1) * sizeof(double), &tw))) return rc;
    double *ta = (double *)tw, *tT = ta + nbin_t;
    c->t_begin("k_warp_apply");
    GCHK(gmmk_warp_target(c->stream, nbin_t, i_tb.d, i_tc.d, ta, tT));
    GCHK(gmmk_warp_apply(c->stream, dt == GMMIV_F64, x, ldx, odt == GMMIV_F64, out, ldo, D, (const long *)i_runs.d, nrun, nunits, nbin, i_b.d, i_c.d,
                         (const int *)i_s.d, nbin_t, i_tb.d, ta, tT, c->n_cu));
    c->t_end();
    const bool host_any = host_runs || host_tb || host_tc || !gmmiv_is_device_ptr(bounds) || !gmmiv_is_device_ptr(count) || !gmmiv_is_device_ptr(status);
    if (host_any) GCHK(hipStreamSynchronize(c->stream)); // the host tables may be freed
    return GMMIV_OK;
}

} // extern "C"
