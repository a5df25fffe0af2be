/* gmmiv_turn.h -- C ABI: LIA_SpkSeg/TurnDetection (TurnDetection.cpp:101-287; the criterion of ClusteringCriterion.cpp:104-139 and
 * :807-927 over AccumulateStat.cpp:69-95) on the resident frames, a list of files per call.
 *
 * The rule.  A label segment ("run") of L <= 2 W frames is copied through.  A longer one is walked by two adjacent windows of W frames
 * in steps of S frames: position k of a run that begins at buffer frame b has
 *     c1 = frames [b + k S, b + k S + W),   c2 = the next W frames,   c12 = those 2 W frames in order,
 * for every k with b + k S + 2 W - 1 < b + L - 1 (the strict end2 < endSeg of :154), n = ceil((L - 2 W) / S) positions.  Per window a
 * one-Gaussian diagonal model is built from its own frames -- the FrameAccGD mean s / n and biased covariance ss / n - mean^2 per
 * column, covInv = 1 / cov, det = prod cov, cst = (2 pi)^(-D/2) / sqrt(det) -- and LLK(window) is the sum over the window's frames of the
 * per-frame log-likelihood under the rule gmmiv_llk documents for a model of one Gaussian of weight 1:
 *     l = log cst - 0.5 sum_d (x_d - mean_d)^2 covInv_d             (log domain, as the library's other kernels)
 *     l below log 2^-1075 = -745.1332 (the likelihood is 0 in fp64) or not finite:  llk = min_llk     (the zero-likelihood rule)
 *     otherwise                                                                     llk = min(max(l, min_llk), max_llk)
 * Then g = LLK12 - (LLK1 + LLK2) and value = g (GMMIV_TURN_GLR), -g (GMMIV_TURN_DGLR), -g - P (GMMIV_TURN_BIC) with
 * P = 0.5 (2 D + 1) log(2 W), computed on the host in double.  DELTABIC (a split and two EM iterations per position) has no constant.
 * Feature values are NOT screened, as gmmiv_frame_moments does not screen: a NaN or infinite value goes through the moments and makes the
 * covariance of its windows not finite; a finite value of any size is evaluated as it stands.
 *
 * status [npos] (int32 bit set, nullable):
 *   GMMIV_TURN_BAD_COV   one of the three windows has a covariance that is <= 0 or not finite in some column (a constant column, a NaN
 *                        feature).  value = NaN -- the reference's arithmetic gives 0 x inf there too; no other bit is set.
 *   GMMIV_TURN_CLAMPED   the clamp or the zero-likelihood rule acted on at least one of the position's 4 W frame evaluations.
 *
 * Bits.  The summation order of gmmiv_turn_curve, fp64 throughout, every operation rounded on its own unless said otherwise:
 *   - a window is cut into BLOCKS of S frames counted from the window's first frame, the last block short when the window's length is
 *     no multiple of S.  A block's sum (of x, of x^2, of llk) starts from 0 and adds its frames left to right; a window's sum is its
 *     first block's, the further blocks' added in order.
 *   - mean = s / n, cov = ss / n - mean * mean, covInv = 1 / cov;  log cst = -0.5 (D log(2 pi) + (sum_d log cov_d, from 0, in column order));
 *   - per frame q = fma((x_d - mean_d)^2, covInv_d, q) from 0 in column order (the ONE fused operation), l = log cst - 0.5 q;
 *   - g = LLK12 - (LLK1 + LLK2).
 * A position's value is therefore a function of its own 2 W frames, D, W, S and the options alone -- not of the tile it fell into, its
 * neighbours, its run, its file or the rest of the call.  An f32 buffer is converted exactly.  No atomics.
 *
 * The kernel (csrc/turn_detect.hip).  One workgroup per tile of at most gmmiv_turn_tile_positions(D, W, S) consecutive positions of one
 * run; the tile's 2 W + (P - 1) S frames are staged in LDS once, so a frame leaves HBM about 1 + 2 W / (P S) times.  A window that does
 * not fit the 160 KB of LDS with one position per tile is refused (gmmiv_turn_tile_positions returns 0); there is no streaming path.
 *
 * gmmiv_turn_pick (:184-263, as written) on a curve v of n positions, per run:
 *   smoothing   v'[i] = (0.25 v[i - 1] + 0.25 v[i + 1]) + 0.5 v[i] on the RAW neighbours for i = 1 .. n - 2; v'[0] = v[0], v'[n - 1] = v[n - 1]
 *   mean / std  over v': sum and sum of squares as 256 lane partials (lane j adds v'[j], v'[j + 256], ... in order, from 0), the
 *               min(n, 256) partials added in lane order from the first; mean = sum / n, std = sqrt(sum2 / n - mean * mean).  A NaN
 *               (a NaN value, a negative rounding) is kept: every comparison with it is false.
 *   left min    from v'[i], down the strictly decreasing values at i - 1, i - 2, ...; index 0 is never looked at
 *   right min   the same to the right; the last index may be reached
 *   decision    dec[i] = |v'[i] - minL| > alpha std && |v'[i] - minR| > alpha std for i = 1 .. n - 2; dec[0] = dec[n - 1] = 0
 *
 * gmmiv_turn_segments (:142-145, :265-279): a run without positions yields itself; a run with positions is cut after frame
 * b + W - 1 + i S of every i with dec[i] != 0, and the tail is added when start < b + L - 1, as written.  Segments never cross an input
 * run; begins are buffer frames.
 *
 * Tables.  x is a DEVICE array, GMMIV_F32 or GMMIV_F64, row stride ldx >= D (a column slice is x + first column with the full stride).
 * runs[3 r + 0 .. 2] = (first frame, length, file), file ids non-decreasing and in [0, nfiles); a run is ONE input label segment, never
 * cut.  pos_off [nrun + 1] is the CSR of gmmiv_plan_turn_positions for the same (W, S).  Every array but x is host or device, and with
 * device pointers throughout a call only enqueues on the context's stream.  HOST tables are validated before the context is looked at:
 * GMMIV_ERR_ARG with a message that names the first offending run.  DEVICE tables are not read by the host; the kernels never give a run
 * more positions than its length holds frames for and never write outside [0, npos).  nfiles = 0, nrun = 0, npos = 0 and files without
 * runs are valid.
 * Kernel timers: "k_turn_curve", "k_turn_pick", "k_turn_segments". */
#ifndef GMMIV_TURN_H
#define GMMIV_TURN_H

#include "gmmiv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GMMIV_TURN_GLR 0
#define GMMIV_TURN_DGLR 1
#define GMMIV_TURN_BIC 2

#define GMMIV_TURN_BAD_COV 1
#define GMMIV_TURN_CLAMPED 2

/* Positions per tile of k_turn_curve for (D, W, step): the largest P <= 32 whose frames, block sums, models and partials fit the LDS;
 * 0 when one position does not fit (or an argument is < 1): gmmiv_turn_curve then returns GMMIV_ERR_ARG. */
int gmmiv_turn_tile_positions(int D, int64_t W, int64_t step);

/* Pure host.  pos_off [nrun + 1] (nullable) receives the CSR of the positions per run; returns their total.  -1, with a message
 * (gmmiv_last_error) naming the first offending run, for file ids decreasing or outside [0, nfiles), a length < 0 or a first frame < 0;
 * also for a negative count, a missing table, W < 1 or step < 1. */
int64_t gmmiv_plan_turn_positions(const int64_t *runs, int64_t nrun, int64_t nfiles, int64_t W, int64_t step, int64_t *pos_off);

/* value [npos], status [npos] (nullable): the criterion at every position of every run, one launch over the whole list. */
int gmmiv_turn_curve(gmmiv_ctx *ctx, const void *x, int x_dtype, int64_t ldx, int D, const int64_t *runs, int64_t nrun, int64_t nfiles,
                     const int64_t *pos_off, int64_t npos, int64_t W, int64_t step, int crit, double min_llk, double max_llk, double *value,
                     int32_t *status);

/* value [npos]: the output of gmmiv_turn_curve or any array.  smoothed [npos] (nullable; must not alias value), dec [npos] (uint8),
 * run_stats [nrun x 2] = mean | std (nullable; NaN for a run without positions), n_turns [nrun] (nullable). */
int gmmiv_turn_pick(gmmiv_ctx *ctx, const double *value, const int64_t *pos_off, int64_t nrun, int64_t npos, double alpha, double *smoothed,
                    uint8_t *dec, double *run_stats, int64_t *n_turns);

/* Count-then-fill like gmmiv_energy_select: seg_count [nfiles] (nullable) = output segments per file; seg_begin / seg_len (both or
 * neither) = the segments of file f at [seg_off[f], seg_off[f + 1]), in run order -- seg_off [nfiles + 1] from a first call with
 * seg_begin = seg_len = NULL (counts only; seg_off is then not read).  Segments beyond a file's CSR room are not written; entries of the
 * room that no segment fills keep their values. */
int gmmiv_turn_segments(gmmiv_ctx *ctx, const int64_t *runs, int64_t nrun, int64_t nfiles, const int64_t *pos_off, int64_t npos,
                        const uint8_t *dec, int64_t W, int64_t step, int64_t *seg_count, const int64_t *seg_off, int64_t *seg_begin,
                        int64_t *seg_len);

#ifdef __cplusplus
}
#endif
#endif
