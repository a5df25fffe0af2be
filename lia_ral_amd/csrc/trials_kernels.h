// trials_kernels.h -- host-callable launchers of topc_trials.hip (internal).  All pointers are device pointers; every function returns a
// hipError_t value, or -1 for a shape the kernel does not serve.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gmmiv.h" // gmmiv_trial_tile

// k_topc_use4_trials: tiles[0 .. ntiles) (frame numbers of the call; x row 0 is frame xbase, idx / nllk row 0 is frame base), models at
// mean + g sm, iv + g si, lwc + g sl (0 = shared); the tile's sum goes to part[trial_off[trial] + piece].  -1: ctop > 16 or odd D
int gmmk_topc_use4_trials(hipStream_t st, int x_f64, const void *x, long xbase, long ldx, int D, const double *mean, long sm, const double *iv,
                          long si, const double *lwc, long sl, int C, int ctop, const gmmiv_trial_tile *tiles, long ntiles, const long *trial_off,
                          long base, const int *idx, const double *nllk, int complete, double lo, double hi, double *part);
// the piece sums of v (row 0 = frame base) over the segments [s0, s1): piece k of segment s -> part[seg_off[s] + k]; npiece = their number
int gmmk_piece_sums_segs(hipStream_t st, const double *v, long base, const long *seg_begin, const long *seg_off, long s0, long s1, long npiece, int P,
                         double *part);
int gmmk_piece_sums_row(hipStream_t st, const double *v, long n, int P, double *part); // one row of n values: part[k] = sum of piece k
int gmmk_trial_reduce(hipStream_t st, long ntrial, long nseg, const int *trial_seg, const long *trial_off, const long *seg_begin, const long *seg_off,
                      const double *part, const double *wpart, double *llr, double *client_mean, double *world_mean);
