// score_norm.h -- launchers of score_norm.hip (internal).  Device pointers only; return hipError_t values.
//
// LIA_SpkDet/ComputeNorm on device-resident score matrices: DistribNorm::computeMeanStd (ComputeNorm.cpp:121-159) for every
// distribution of a cohort matrix, and the (x - mean) / std passes of the z / t / zt / tz chains (:530-751).
//
// Scratch (slot WS_NORM of ctx.h): SNK_INFO_BYTES (the four counts a device-resident selection mask is reduced to) +
// SNK_PART_BYTES per distribution (the row-slab sums of the untrimmed column pass: 32 slabs x (sum, sum2)), whatever the
// matrix.  The select kernels keep their histograms in LDS and write nothing but `mean` and `std`.
#pragma once
#include <hip/hip_runtime.h>

#define SNK_INFO_BYTES 64 // long info[4] = { n, discardH, discardL, index of the (n / 2)-th selected score }, padded
#define SNK_PART_BYTES 512 // per distribution: [32 slabs][sum | sum2] doubles

// info <- the counts of a device-resident selection mask (computed with the reference's fp64 product and truncation)
int snk_mask_info(hipStream_t st, const unsigned char *mask, long L, double percent_h, double percent_l, long *info);
// axis 0: `rows` distributions of length `cols` (contiguous); axis 1: `cols` distributions of length `rows` (stride ld).
// mask / pre_mean / pre_std: NULL or vectors along the cohort axis.  sorted: either percentage is non-zero (the reference sorts).
// n, dH, dL, qidx: the counts when info == NULL; info: device counts (snk_mask_info) that take their place.
// part: SNK_PART_BYTES x cols of scratch for axis 1 (NULL: the select kernel serves the untrimmed mean too).
int snk_cohort_stats(hipStream_t st, int axis, long rows, long cols, const double *x, long ld, const unsigned char *mask,
                     const double *pre_mean, const double *pre_std, int mean_mode, int sorted, long n, long dH, long dL, long qidx,
                     const long *info, double *part, double *mean, double *sd);
// order 0: z (rows), 1: t (columns), 2: t then z, 3: z then t; first: NULL or [M x S], the score after the first of two
int snk_apply(hipStream_t st, long M, long S, double *X, int order, const double *row_mean, const double *row_std, const double *col_mean,
              const double *col_std, double *first);
