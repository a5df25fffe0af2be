// capi_feat_window.hip -- C ABI (include/gmmiv_feat_window.h): NormFeat's windowMode -- the schedule of NormFeat.cpp:384-446 as a host
// plan, and the entry point that runs the plan of a list of files in one launch (feat_norm_window.hip).
#include <math.h>

#include <vector>

#include "ctx.h"
#include "feat_norm_window.h"
#include "../../include/gmmiv_feat_window.h"

namespace {

// frameIdxToTime (SegTools.cpp:143-148): the truncation to whole milliseconds is part of the rule
inline double nw_time(unsigned long idx, double frameLength)
{
    const unsigned long t = (unsigned long)(idx * 1000 * frameLength);
    return (double)t / 1000.0;
}

// The segments of one file: begins b[i] (relative to the file) and lengths l[i], i in [0, n).  The reference's window is a cluster of
// copies and its current segment a pointer; here both are indices -- the window is [wlo, whi), the current segment cur (-1: NULL).
struct NwFile {
    const int64_t *b, *l;
    int64_t n;
    double wd, comp, fl;
    double length(int64_t wlo, int64_t whi) const { return nw_time((unsigned long)(b[whi - 1] + l[whi - 1]), fl) - nw_time((unsigned long)b[wlo], fl); } // windowLength
    double alpha(int64_t wlo, int64_t whi) const                                                                                                    // computeWindowParam :156-164
    {
        unsigned long total = 0;
        for (int64_t i = wlo; i < whi; ++i) total += (unsigned long)l[i];
        double a = nw_time(total, fl);
        a /= length(wlo, whi);
        if (a > 1) a = 1.0;
        a *= comp;
        return a;
    }
};

// the loop of NormFeat.cpp:384-446; emit(wlo, whi, alo, ahi, alpha) per step that normalises something.  false: the reference's
// "currentSeg is not in the window" (cannot happen on a table that passed the checks)
template <typename Emit> bool nw_schedule(const NwFile &F, Emit emit)
{
    int64_t wlo = 0, whi = 0, cur = -1;
    for (int64_t i = 0; i < F.n; ++i) {
        if (wlo == whi) { wlo = i; whi = i + 1; if (cur < 0) cur = i; continue; }             // inWindow: the empty window takes the segment
        if (F.length(wlo, whi) <= F.wd) { whi = i + 1; if (cur < 0) cur = i; continue; }      // inWindow: the length is not reached
        // the window is full: its parameters, the segments up to its middle, then moveWindow
        const int64_t a0 = cur;
        bool ok = true;
        while (ok && nw_time((unsigned long)F.b[cur], F.fl) <= nw_time((unsigned long)F.b[wlo], F.fl) + F.wd / 2.0) {   // inMiddle
            if (cur < wlo || cur >= whi) return false;                                         // nextSeg
            ++cur;
            if (cur >= whi) { cur = -1; ok = false; }
        }
        const int64_t a1 = cur < 0 ? whi : cur;
        if (a1 > a0) emit(wlo, whi, a0, a1, F.alpha(wlo, whi));
        whi = i + 1;                                                                           // moveWindow: addCopy(seg)
        do { ++wlo; } while (cur >= 0 && F.b[wlo] < F.b[cur] && F.length(wlo, whi) > F.wd);    // suppressFirst at least once
        if (cur < 0) cur = i;
    }
    if (wlo < whi) {                                                                           // the last window: from the current segment to its end
        if (cur < wlo || cur >= whi) return false;
        emit(wlo, whi, cur, whi, F.alpha(wlo, whi));
    }
    return true;
}

} // namespace

extern "C" {

int64_t gmmiv_plan_norm_windows(const int64_t *runs, int64_t nrun, int64_t nfiles, const int64_t *file_first, double window_duration,
                                double window_comp, double frame_length, int64_t *step_off, int64_t *steps, double *alpha)
{
    if (nrun < 0 || nfiles < 0 || (!runs && nrun > 0) || (!file_first && nfiles > 0)) { gmmiv_set_error("plan_norm_windows: bad argument (nrun, nfiles < 0 or a missing table)"); return -1; }
    if (!(window_duration >= 0) || !isfinite(window_duration) || !(frame_length > 0) || !isfinite(frame_length)) { gmmiv_set_error("plan_norm_windows: window_duration must be >= 0 and frame_length > 0, both finite"); return -1; }
    std::vector<int64_t> b((size_t)nrun), l((size_t)nrun);
    int64_t prevf = 0;
    for (int64_t r = 0; r < nrun; ++r) {
        const int64_t first = runs[3 * r], len = runs[3 * r + 1], f = runs[3 * r + 2];
        if (f < prevf || f >= nfiles) { gmmiv_set_error("plan_norm_windows: run %ld: file %ld is below its predecessor's or outside [0, %ld) (file ids must be non-decreasing)", (long)r, (long)f, (long)nfiles); return -1; }
        if (len < 1) { gmmiv_set_error("plan_norm_windows: run %ld has length %ld < 1", (long)r, (long)len); return -1; }
        const int64_t beg = first - file_first[f];
        if (beg < 0) { gmmiv_set_error("plan_norm_windows: run %ld begins %ld frames before its file %ld", (long)r, (long)-beg, (long)f); return -1; }
        if (r > 0 && f == prevf && runs[3 * (r - 1) + 2] == f) {
            if (beg <= b[(size_t)r - 1]) { gmmiv_set_error("plan_norm_windows: run %ld of file %ld does not begin after the run before it (begins must be strictly increasing)", (long)r, (long)f); return -1; }
            if (beg < b[(size_t)r - 1] + l[(size_t)r - 1]) { gmmiv_set_error("plan_norm_windows: run %ld of file %ld overlaps the run before it", (long)r, (long)f); return -1; }
        }
        b[(size_t)r] = beg; l[(size_t)r] = len;
        prevf = f;
    }
    int64_t ns = 0, r0 = 0;
    for (int64_t f = 0; f < nfiles; ++f) {
        int64_t r1 = r0;
        while (r1 < nrun && runs[3 * r1 + 2] == f) ++r1;
        if (step_off) step_off[f] = ns;
        const NwFile F = {b.data() + r0, l.data() + r0, r1 - r0, window_duration, window_comp, frame_length};
        const bool ok = nw_schedule(F, [&](int64_t wlo, int64_t whi, int64_t alo, int64_t ahi, double a) {
            if (steps) { steps[4 * ns] = r0 + wlo; steps[4 * ns + 1] = r0 + whi; steps[4 * ns + 2] = r0 + alo; steps[4 * ns + 3] = r0 + ahi; }
            if (alpha) alpha[ns] = a;
            ++ns;
        });
        if (!ok) { gmmiv_set_error("plan_norm_windows: file %ld: the current segment is not in the window", (long)f); return -1; }
        r0 = r1;
    }
    if (step_off) step_off[nfiles] = ns;
    return ns;
}

int gmmiv_feat_norm_window(gmmiv_ctx *c, void *x, int dt, int64_t ldx, int D, const int64_t *runs, int64_t nrun, int64_t nfiles,
                           const int64_t *step_off, const int64_t *steps, const double *alpha, int64_t nsteps, int flags, double *gstat,
                           double *step_stat)
{
    if (dt != GMMIV_F32 && dt != GMMIV_F64) { gmmiv_set_error("feat_norm_window: x_dtype must be GMMIV_F32 or GMMIV_F64"); return GMMIV_ERR_ARG; }
    if (nrun < 0 || nfiles < 0 || nsteps < 0 || D <= 0 || ldx < D || (!runs && nrun > 0)) { gmmiv_set_error("feat_norm_window: bad argument (nrun, nfiles, nsteps < 0, D <= 0, ldx < D or runs == NULL)"); return GMMIV_ERR_ARG; }
    if ((flags & ~(GMMIV_NORMWIN_CMS | GMMIV_NORMWIN_VAR)) || flags == (GMMIV_NORMWIN_CMS | GMMIV_NORMWIN_VAR)) { gmmiv_set_error("feat_norm_window: flags must be 0, GMMIV_NORMWIN_CMS or GMMIV_NORMWIN_VAR (cmsOnly and varOnly are not compatible)"); return GMMIV_ERR_ARG; }
    if ((!step_off && nfiles > 0) || ((!steps || !alpha) && nsteps > 0)) { gmmiv_set_error("feat_norm_window: step_off, steps or alpha == NULL"); return GMMIV_ERR_ARG; }
    const bool host_runs = nrun > 0 && !gmmiv_is_device_ptr(runs), host_off = nfiles > 0 && !gmmiv_is_device_ptr(step_off);
    const bool host_steps = nsteps > 0 && !gmmiv_is_device_ptr(steps), host_alpha = nsteps > 0 && !gmmiv_is_device_ptr(alpha);
    if (host_runs) {
        int64_t prev = 0;
        for (int64_t r = 0; r < nrun; ++r) {
            const int64_t first = runs[3 * r], len = runs[3 * r + 1], f = runs[3 * r + 2];
            if (first < 0 || len < 0) { gmmiv_set_error("feat_norm_window: run %ld has a negative first frame or length", (long)r); return GMMIV_ERR_ARG; }
            if (f < prev || f >= nfiles) { gmmiv_set_error("feat_norm_window: run %ld: file %ld is below its predecessor's or outside [0, %ld) (file ids must be non-decreasing)", (long)r, (long)f, (long)nfiles); return GMMIV_ERR_ARG; }
            prev = f;
        }
    }
    if (host_off) {
        if (step_off[0] != 0) { gmmiv_set_error("feat_norm_window: step_off[0] must be 0"); return GMMIV_ERR_ARG; }
        for (int64_t f = 0; f < nfiles; ++f)
            if (step_off[f + 1] < step_off[f]) { gmmiv_set_error("feat_norm_window: step_off must be non-decreasing (file %ld)", (long)f); return GMMIV_ERR_ARG; }
        if (step_off[nfiles] != nsteps) { gmmiv_set_error("feat_norm_window: step_off ends at %ld, not at nsteps = %ld", (long)step_off[nfiles], (long)nsteps); return GMMIV_ERR_ARG; }
    }
    if (host_steps) {
        int64_t f = 0, r0 = 0, r1 = 0; // with host runs and offsets: the runs [r0, r1) of the file that owns the step
        const bool per_file = host_off && (host_runs || nrun == 0);
        if (per_file) while (r1 < nrun && runs[3 * r1 + 2] == 0) ++r1;
        for (int64_t s = 0; s < nsteps; ++s) {
            const int64_t wlo = steps[4 * s], whi = steps[4 * s + 1], alo = steps[4 * s + 2], ahi = steps[4 * s + 3];
            if (wlo < 0 || whi > nrun || !(wlo <= alo && alo < ahi && ahi <= whi)) { gmmiv_set_error("feat_norm_window: step %ld: (window, apply) = ([%ld, %ld), [%ld, %ld)) is not lo <= apply lo < apply hi <= hi inside the %ld runs", (long)s, (long)wlo, (long)whi, (long)alo, (long)ahi, (long)nrun); return GMMIV_ERR_ARG; }
            if (per_file) {
                while (s >= step_off[f + 1]) { ++f; r0 = r1; while (r1 < nrun && runs[3 * r1 + 2] == f) ++r1; }
                if (wlo < r0 || whi > r1) { gmmiv_set_error("feat_norm_window: step %ld of file %ld names runs outside the file's runs [%ld, %ld)", (long)s, (long)f, (long)r0, (long)r1); return GMMIV_ERR_ARG; }
            }
        }
    }
    if (!c) { gmmiv_set_error("feat_norm_window: NULL context"); return GMMIV_ERR_ARG; }
    if (nfiles == 0) return GMMIV_OK;
    if (nrun > 0 && (!x || !gmmiv_is_device_ptr(x))) { gmmiv_set_error("feat_norm_window: x must be a device array"); return GMMIV_ERR_ARG; }
    GBIND(c);
    int rc;
    DevIn<int64_t> i_runs, i_off, i_steps;
    DevIn<double> i_alpha;
    if ((rc = i_runs.init(c, WS_T0, runs, (size_t)nrun * 3)) || (rc = i_off.init(c, WS_T1, step_off, (size_t)nfiles + 1)) ||
        (rc = i_steps.init(c, WS_T2, steps, (size_t)nsteps * 4)) || (rc = i_alpha.init(c, WS_T3, alpha, (size_t)nsteps))) return rc;
    DevOut<double> o_g, o_s;
    if ((rc = o_g.init(c, WS_T4, gstat, (size_t)nfiles * 2 * D, false)) || (rc = o_s.init(c, WS_T5, step_stat, (size_t)nsteps * 2 * D, false))) return rc;
    void *part;
    if ((rc = c->scratch(WS_PART, (size_t)nrun * 2 * D * sizeof(double), &part))) return rc;
    c->t_begin("k_norm_window");
    GCHK(gmmk_norm_window(c->stream, dt == GMMIV_F64, x, ldx, D, (const long *)i_runs.d, nrun, nfiles, (const long *)i_off.d, (const long *)i_steps.d, i_alpha.d,
                          flags & GMMIV_NORMWIN_CMS, flags & GMMIV_NORMWIN_VAR, (double *)part, o_g.d, o_s.d));
    c->t_end();
    if ((rc = o_g.finish()) || (rc = o_s.finish())) return rc;
    if ((host_runs || host_off || host_steps || host_alpha) && !o_g.host && !o_s.host) GCHK(hipStreamSynchronize(c->stream)); // the host tables may be freed
    return GMMIV_OK;
}

} // extern "C"
