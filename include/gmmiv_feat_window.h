/* gmmiv_feat_window.h -- C ABI: NormFeat's windowMode (NormFeat.cpp:88-186, 372-447) on the resident frames, a list of files per call.
 *
 * The rule.  Per file the selected label segments ("runs", in table order) are normalised by the FrameAccGD mean and biased std of a
 * window of about windowDuration seconds of selected speech around them, blended with the file's global statistics by how full the
 * window is.  A window's statistics read the frames AS THE BUFFER STANDS: segments normalised by an earlier step enter with their
 * rewritten values, so a file is a sequential chain of steps.  The windows are counted in segments and in truncated milliseconds,
 *     T(i) = (double)(unsigned long)(i * 1000 * frameLength) / 1000.0                                       (SegTools.cpp:143-148),
 * with begins counted from the FILE's first frame -- not in frames.
 *
 * Two calls.  gmmiv_plan_norm_windows (pure host, no frame data) restates the loop of NormFeat.cpp:384-446 on the segment table and
 * returns the steps: (window, segments to normalise, alpha).  gmmiv_feat_norm_window runs the steps of every file in ONE launch.
 *
 * A step (computeWindowParam, :147-173), per column, every product and sum rounded on its own:
 *     m, s    mean / std of the window's frames as they stand;  gm, gs  the same over all runs of the file before anything was rewritten
 *     alpha = min(T(frames of the window) / (T(end of the last run) - T(begin of the first run)), 1) * windowComp       (the planner)
 *     m' = alpha m + (1 - alpha) gm
 *     s' = sqrt((alpha s) s + ((1 - alpha) gs) gs + ((1 - alpha) alpha) (m' - gm)^2)        -- the blended m' in the last term, as written
 *     GMMIV_NORMWIN_CMS: s' = 1;  GMMIV_NORMWIN_VAR: m' = 0;   x <- (x - m') / s' on the step's runs (one subtraction, one division)
 *
 * Bits.  The moments of a set of runs are the bits gmmiv_frame_moments_groups gives a zeroed accumulator for one group made of exactly
 * those runs, uncut: per run 16 interleaved row sums, each left to right, added in order; runs added in table order.  Mean and std
 * are the bits of gmmiv_frame_moments_stats, the apply those of gmmiv_feat_norm_apply, the blend the expression above without
 * contraction.  The call therefore equals, bit for bit, the per-step composition of those entry points.  A file's bits depend on its
 * own runs and steps alone -- not on its neighbours or its place in the list.  No atomics.  Columns >= D and frames outside the runs
 * are not touched.  An f32 buffer is rounded once per store, and later windows read the stored value.  Non-finite values are not
 * screened; a zero std divides by zero as the reference does.
 *
 * Limit.  Parallelism is across files only: one workgroup runs the whole chain of a file, so one long file runs on one compute unit.
 * A list of files fills the device.  A window may be of any length (nothing is staged per window: the kernel keeps the 2 D partial
 * sums of every run and renews those of a run when it rewrites it, so every frame is read twice and written once).
 *
 * Tables (host or device; with device pointers throughout, gstat / step_stat included, the call only enqueues on the context's stream):
 *   runs [nrun x 3]       (first frame in the buffer, length, file); file ids non-decreasing.  A run is one label segment, never cut.
 *   step_off [nfiles + 1] CSR: the steps of file f are step_off[f] .. step_off[f + 1]
 *   steps [nsteps x 4]    (window lo, window hi, apply lo, apply hi): indices into `runs`, hi exclusive, lo <= apply lo < apply hi <= hi
 *   alpha [nsteps]
 * HOST tables are validated before the context is looked at (the dtype first, then the tables, then the context): GMMIV_ERR_ARG with a
 * message that names the first offending run, file or step.  Device tables are not read by the host.
 * Workspace: 16 D nrun bytes of run partials (the slot of gmmiv_frame_moments_groups) plus the staging of host tables.
 * Kernel timer: "k_norm_window". */
#ifndef GMMIV_FEAT_WINDOW_H
#define GMMIV_FEAT_WINDOW_H

#include "gmmiv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GMMIV_NORMWIN_CMS 1 /* cmsOnly: the std is replaced by 1 (:401) */
#define GMMIV_NORMWIN_VAR 2 /* varOnly: the mean is replaced by 0 (:402) */

/* The schedule (pure host).  runs as above; file_first [nfiles]: the buffer frame where file f starts (begins are first - file_first[file]).
 * Returns the number of steps; with non-NULL arrays step_off [nfiles + 1], steps [4 x .] and alpha [.] are filled.  Steps that normalise
 * nothing are not emitted (computing a window's parameters has no side effect), which leaves at most one step per run: arrays of nrun
 * steps ALWAYS suffice.  A file without runs has no steps.  -1, with a message (gmmiv_last_error) naming the first offending run, for:
 * file ids decreasing or out of range, a length < 1, a begin < 0, within a file a begin not strictly greater than the previous one
 * (the reference's nextSeg would not terminate), a run that overlaps the previous one (its frames would be rewritten twice); also for
 * a negative count, a missing table, window_duration < 0 or frame_length <= 0 (or either not finite). */
int64_t gmmiv_plan_norm_windows(const int64_t *runs, int64_t nrun, int64_t nfiles, const int64_t *file_first, double window_duration,
                                double window_comp, double frame_length, int64_t *step_off, int64_t *steps, double *alpha);

/* In place on x (GMMIV_F32 or GMMIV_F64, row stride ldx >= D, a device array; a column slice is x + first column with the full stride).
 * flags: 0, GMMIV_NORMWIN_CMS or GMMIV_NORMWIN_VAR (both: GMMIV_ERR_ARG).  gstat (nullable) [nfiles x 2 D] receives gm | gs (NaN for a
 * file without runs), step_stat (nullable) [nsteps x 2 D] receives m' | s' after the flags; host or device.  nfiles == 0, nsteps == 0
 * and files without runs are valid. */
int gmmiv_feat_norm_window(gmmiv_ctx *ctx, void *x, int x_dtype, int64_t ldx, int D, const int64_t *runs, int64_t nrun, int64_t nfiles,
                           const int64_t *step_off, const int64_t *steps, const double *alpha, int64_t nsteps, int flags, double *gstat,
                           double *step_stat);

#ifdef __cplusplus
}
#endif
#endif
