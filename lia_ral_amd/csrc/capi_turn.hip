// capi_turn.hip -- C ABI (include/gmmiv_turn.h): LIA_SpkSeg/TurnDetection on the resident frames -- the position plan, the criterion
// curve, the smoothing and decisions, the output segments (kernels in turn_detect.hip).
#include <math.h>

#include "ctx.h"
#include "turn_detect.h"
#include "../../include/gmmiv_turn.h"

namespace {

// the run table's own rules; false with the message set
bool turn_check_runs(const char *who, const int64_t *runs, int64_t nrun, int64_t nfiles)
{
    int64_t prev = 0;
    for (int64_t r = 0; r < nrun; ++r) {
        const int64_t first = runs[3 * r], len = runs[3 * r + 1], f = runs[3 * r + 2];
        if (first < 0 || len < 0) { gmmiv_set_error("%s: run %ld has a negative first frame or length", who, (long)r); return false; }
        if (f < prev || f >= nfiles) { gmmiv_set_error("%s: run %ld: file %ld is below its predecessor's or outside [0, %ld) (file ids must be non-decreasing)", who, (long)r, (long)f, (long)nfiles); return false; }
        prev = f;
    }
    return true;
}

// host pos_off against the counts; with host runs against the plan of (W, S) too
bool turn_check_off(const char *who, const int64_t *runs, const int64_t *pos_off, int64_t nrun, int64_t npos, int64_t W, int64_t S)
{
    if (pos_off[0] != 0) { gmmiv_set_error("%s: pos_off[0] must be 0", who); return false; }
    for (int64_t r = 0; r < nrun; ++r) {
        const int64_t n = pos_off[r + 1] - pos_off[r];
        if (n < 0) { gmmiv_set_error("%s: pos_off must be non-decreasing (run %ld)", who, (long)r); return false; }
        if (runs && n != turn_run_positions(runs[3 * r + 1], W, S)) { gmmiv_set_error("%s: run %ld of length %ld has %ld positions in pos_off, the plan for W = %ld, step = %ld gives %ld", who, (long)r, (long)runs[3 * r + 1], (long)n, (long)W, (long)S, (long)turn_run_positions(runs[3 * r + 1], W, S)); return false; }
    }
    if (pos_off[nrun] != npos) { gmmiv_set_error("%s: pos_off ends at %ld, not at npos = %ld", who, (long)pos_off[nrun], (long)npos); return false; }
    return true;
}

} // namespace

extern "C" {

int gmmiv_turn_tile_positions(int D, int64_t W, int64_t step)
{
    TurnShape s;
    if (!turn_shape(D, W, step, 1, s) || s.bytes > TURN_LDS_BUDGET) return 0;
    int P = 1;
    while (P < TURN_MAX_TILE && turn_shape(D, W, step, P + 1, s) && s.bytes <= TURN_LDS_BUDGET) ++P;
    return P;
}

int64_t gmmiv_plan_turn_positions(const int64_t *runs, int64_t nrun, int64_t nfiles, int64_t W, int64_t step, int64_t *pos_off)
{
    if (nrun < 0 || nfiles < 0 || (!runs && nrun > 0)) { gmmiv_set_error("plan_turn_positions: bad argument (nrun, nfiles < 0 or runs == NULL)"); return -1; }
    if (W < 1 || step < 1 || W > (1L << 24) || step > (1L << 24)) { gmmiv_set_error("plan_turn_positions: W = %ld and step = %ld must be in [1, 2^24]", (long)W, (long)step); return -1; }
    if (!turn_check_runs("plan_turn_positions", runs, nrun, nfiles)) return -1;
    int64_t tot = 0;
    for (int64_t r = 0; r < nrun; ++r) {
        if (pos_off) pos_off[r] = tot;
        tot += turn_run_positions(runs[3 * r + 1], W, step);
    }
    if (pos_off) pos_off[nrun] = tot;
    return tot;
}

int gmmiv_turn_curve(gmmiv_ctx *c, const void *x, int dt, int64_t ldx, int D, const int64_t *runs, int64_t nrun, int64_t nfiles, const int64_t *pos_off,
                     int64_t npos, int64_t W, int64_t step, int crit, double min_llk, double max_llk, double *value, int32_t *status)
{
    if (dt != GMMIV_F32 && dt != GMMIV_F64) { gmmiv_set_error("turn_curve: x_dtype must be GMMIV_F32 or GMMIV_F64"); return GMMIV_ERR_ARG; }
    if (nrun < 0 || nfiles < 0 || npos < 0 || D <= 0 || ldx < D || (!runs && nrun > 0) || !pos_off) { gmmiv_set_error("turn_curve: bad argument (nrun, nfiles, npos < 0, D <= 0, ldx < D, runs or pos_off == NULL)"); return GMMIV_ERR_ARG; }
    if (W < 1 || step < 1) { gmmiv_set_error("turn_curve: W = %ld and step = %ld must be >= 1", (long)W, (long)step); return GMMIV_ERR_ARG; }
    if (crit != GMMIV_TURN_GLR && crit != GMMIV_TURN_DGLR && crit != GMMIV_TURN_BIC) { gmmiv_set_error("turn_curve: crit must be GMMIV_TURN_GLR, GMMIV_TURN_DGLR or GMMIV_TURN_BIC"); return GMMIV_ERR_ARG; }
    const bool host_runs = nrun > 0 && !gmmiv_is_device_ptr(runs), host_off = !gmmiv_is_device_ptr(pos_off);
    if (host_runs && !turn_check_runs("turn_curve", runs, nrun, nfiles)) return GMMIV_ERR_ARG;
    if (host_off && !turn_check_off("turn_curve", host_runs ? runs : nullptr, pos_off, nrun, npos, W, step)) return GMMIV_ERR_ARG;
    const int P = gmmiv_turn_tile_positions(D, W, step);
    if (P < 1) { gmmiv_set_error("turn_curve: the windows of W = %ld frames of D = %d columns do not fit the LDS even with one position per tile (no streaming path)", (long)W, D); return GMMIV_ERR_ARG; }
    if (!c) { gmmiv_set_error("turn_curve: NULL context"); return GMMIV_ERR_ARG; }
    if (npos == 0 || nrun == 0) return GMMIV_OK;
    if (!value) { gmmiv_set_error("turn_curve: value == NULL"); return GMMIV_ERR_ARG; }
    if (!x || !gmmiv_is_device_ptr(x)) { gmmiv_set_error("turn_curve: x must be a device array"); return GMMIV_ERR_ARG; }
    GBIND(c);
    int rc;
    DevIn<int64_t> i_runs, i_off;
    if ((rc = i_runs.init(c, WS_T0, runs, (size_t)nrun * 3)) || (rc = i_off.init(c, WS_T1, pos_off, (size_t)nrun + 1))) return rc;
    DevOut<double> o_val;
    DevOut<int32_t> o_st;
    if ((rc = o_val.init(c, WS_T5, value, (size_t)npos, false)) || (rc = o_st.init(c, WS_T6, status, (size_t)npos, false))) return rc;
    void *tile_off;
    if ((rc = c->scratch(WS_T2, ((size_t)nrun + 1) * sizeof(int64_t), &tile_off))) return rc;
    // every run with positions ends in at most one short tile
    const int64_t grid = (npos + P - 1) / P + (nrun < npos ? nrun : npos);
    if (grid > 0x7fffffffL) { gmmiv_set_error("turn_curve: %ld tiles exceed one launch", (long)grid); return GMMIV_ERR_ARG; }
    const double penalty = 0.5 * (double)(2 * D + 1) * log((double)(2 * W));
    GCHK(gmmk_turn_tiles(c->stream, (const long *)i_runs.d, nrun, (const long *)i_off.d, W, step, P, (long *)tile_off));
    c->t_begin("k_turn_curve");
    GCHK(gmmk_turn_curve(c->stream, dt == GMMIV_F64, x, ldx, D, (const long *)i_runs.d, nrun, (const long *)i_off.d, npos, W, step, P, grid, (const long *)tile_off,
                         crit, penalty, min_llk, max_llk, o_val.d, (int *)o_st.d));
    c->t_end();
    if ((rc = o_val.finish()) || (rc = o_st.finish())) return rc;
    if ((host_runs || host_off) && !o_val.host && !o_st.host) GCHK(hipStreamSynchronize(c->stream)); // the host tables may be freed
    return GMMIV_OK;
}

int gmmiv_turn_pick(gmmiv_ctx *c, const double *value, const int64_t *pos_off, int64_t nrun, int64_t npos, double alpha, double *smoothed, uint8_t *dec,
                    double *run_stats, int64_t *n_turns)
{
    if (nrun < 0 || npos < 0 || !pos_off) { gmmiv_set_error("turn_pick: bad argument (nrun, npos < 0 or pos_off == NULL)"); return GMMIV_ERR_ARG; }
    const bool host_off = !gmmiv_is_device_ptr(pos_off);
    if (host_off && !turn_check_off("turn_pick", nullptr, pos_off, nrun, npos, 1, 1)) return GMMIV_ERR_ARG;
    if (smoothed && smoothed == value) { gmmiv_set_error("turn_pick: smoothed must not alias value"); return GMMIV_ERR_ARG; }
    if (!c) { gmmiv_set_error("turn_pick: NULL context"); return GMMIV_ERR_ARG; }
    if (nrun == 0) return GMMIV_OK;
    if (npos > 0 && (!value || !dec)) { gmmiv_set_error("turn_pick: value or dec == NULL"); return GMMIV_ERR_ARG; }
    GBIND(c);
    int rc;
    DevIn<double> i_val;
    DevIn<int64_t> i_off;
    if ((rc = i_val.init(c, WS_T0, value, (size_t)npos)) || (rc = i_off.init(c, WS_T1, pos_off, (size_t)nrun + 1))) return rc;
    DevOut<double> o_sm, o_rs;
    DevOut<uint8_t> o_dec;
    DevOut<int64_t> o_nt;
    if ((rc = o_sm.init(c, WS_T5, smoothed, (size_t)npos, false)) || (rc = o_dec.init(c, WS_T6, dec, (size_t)npos, false)) ||
        (rc = o_rs.init(c, WS_T7, run_stats, (size_t)nrun * 2, false)) || (rc = o_nt.init(c, WS_T8, n_turns, (size_t)nrun, false))) return rc;
    double *sm = o_sm.d;
    if (!sm) { // the smoothed curve is needed whether the caller wants it or not
        void *p;
        if ((rc = c->scratch(WS_PART, (size_t)npos * sizeof(double), &p))) return rc;
        sm = (double *)p;
    }
    c->t_begin("k_turn_pick");
    GCHK(gmmk_turn_pick(c->stream, i_val.d, (const long *)i_off.d, nrun, npos, alpha, sm, o_dec.d, o_rs.d, (long *)o_nt.d));
    c->t_end();
    if ((rc = o_sm.finish()) || (rc = o_dec.finish()) || (rc = o_rs.finish()) || (rc = o_nt.finish())) return rc;
    if ((host_off || (npos > 0 && !gmmiv_is_device_ptr(value))) && !o_sm.host && !o_dec.host && !o_rs.host && !o_nt.host) GCHK(hipStreamSynchronize(c->stream));
    return GMMIV_OK;
}

int gmmiv_turn_segments(gmmiv_ctx *c, const int64_t *runs, int64_t nrun, int64_t nfiles, const int64_t *pos_off, int64_t npos, const uint8_t *dec, int64_t W,
                        int64_t step, int64_t *seg_count, const int64_t *seg_off, int64_t *seg_begin, int64_t *seg_len)
{
    if (nrun < 0 || nfiles < 0 || npos < 0 || (!runs && nrun > 0) || !pos_off) { gmmiv_set_error("turn_segments: bad argument (nrun, nfiles, npos < 0, runs or pos_off == NULL)"); return GMMIV_ERR_ARG; }
    if (W < 1 || step < 1) { gmmiv_set_error("turn_segments: W = %ld and step = %ld must be >= 1", (long)W, (long)step); return GMMIV_ERR_ARG; }
    if ((seg_begin == nullptr) != (seg_len == nullptr)) { gmmiv_set_error("turn_segments: seg_begin and seg_len go together"); return GMMIV_ERR_ARG; }
    const bool host_runs = nrun > 0 && !gmmiv_is_device_ptr(runs), host_off = !gmmiv_is_device_ptr(pos_off);
    if (host_runs && !turn_check_runs("turn_segments", runs, nrun, nfiles)) return GMMIV_ERR_ARG;
    if (host_off && !turn_check_off("turn_segments", host_runs ? runs : nullptr, pos_off, nrun, npos, W, step)) return GMMIV_ERR_ARG;
    if (seg_begin && !seg_off) { gmmiv_set_error("turn_segments: seg_off == NULL with seg_begin"); return GMMIV_ERR_ARG; }
    const bool host_soff = seg_begin && !gmmiv_is_device_ptr(seg_off);
    size_t room = 0;
    if (host_soff) {
        for (int64_t f = 0; f < nfiles; ++f)
            if (seg_off[f] < 0 || seg_off[f + 1] < seg_off[f]) { gmmiv_set_error("turn_segments: seg_off must be non-negative and non-decreasing (file %ld)", (long)f); return GMMIV_ERR_ARG; }
        room = (size_t)seg_off[nfiles];
    } else if (seg_begin && (!gmmiv_is_device_ptr(seg_begin) || !gmmiv_is_device_ptr(seg_len))) { gmmiv_set_error("turn_segments: host seg_begin / seg_len need a host seg_off"); return GMMIV_ERR_ARG; }
    if (!c) { gmmiv_set_error("turn_segments: NULL context"); return GMMIV_ERR_ARG; }
    if (nfiles == 0) return GMMIV_OK;
    if (npos > 0 && !dec) { gmmiv_set_error("turn_segments: dec == NULL"); return GMMIV_ERR_ARG; }
    GBIND(c);
    int rc;
    DevIn<int64_t> i_runs, i_off, i_soff;
    DevIn<uint8_t> i_dec;
    if ((rc = i_runs.init(c, WS_T0, runs, (size_t)nrun * 3)) || (rc = i_off.init(c, WS_T1, pos_off, (size_t)nrun + 1)) ||
        (rc = i_dec.init(c, WS_T2, dec, (size_t)npos)) || (rc = i_soff.init(c, WS_T7, seg_begin ? seg_off : nullptr, (size_t)nfiles + 1))) return rc;
    DevOut<int64_t> o_cnt, o_beg, o_len;
    // the room's entries that no segment fills keep their values: host arrays are loaded first
    if ((rc = o_cnt.init(c, WS_T6, seg_count, (size_t)nfiles, false)) || (rc = o_beg.init(c, WS_T8, seg_begin, room, true)) ||
        (rc = o_len.init(c, WS_T9, seg_len, room, true))) return rc;
    void *run_base;
    if ((rc = c->scratch(WS_T3, ((size_t)nrun + 1) * sizeof(int64_t), &run_base))) return rc;
    c->t_begin("k_turn_segments");
    GCHK(gmmk_turn_segments(c->stream, (const long *)i_runs.d, nrun, nfiles, (const long *)i_off.d, npos, i_dec.d, W, step, (long *)run_base, (long *)o_cnt.d,
                            (const long *)i_soff.d, (long *)o_beg.d, (long *)o_len.d));
    c->t_end();
    if ((rc = o_cnt.finish()) || (rc = o_beg.finish()) || (rc = o_len.finish())) return rc;
    if ((host_runs || host_off || host_soff || (npos > 0 && !gmmiv_is_device_ptr(dec))) && !o_cnt.host && !o_beg.host && !o_len.host) GCHK(hipStreamSynchronize(c->stream));
    return GMMIV_OK;
}

} // extern "C"
