// score_norm_lists.h -- launchers of score_norm_lists.hip (internal).  Device pointers only; return hipError_t values.
//
// ComputeNorm on score lists: DistribNorm::computeMeanStd (ComputeNorm.cpp:121-159) for distributions of different lengths held
// as a CSR list, and the (x - mean) / std steps of the four chains on a list of trials (:542-554, :576-589, :634-658, :717-742).
// off [ndist + 1] and ids [count] are device tables: ids names the distributions of ONE length class (gmmiv_plan_score_lists), a
// launch serves exactly those; pos / pre_id are indexed by slot - pos0 / slot - pre0.
#pragma once
#include <hip/hip_runtime.h>

// untrimmed mean / std; wg 0: the class of at most 4096 scores (a wave per distribution), 1: longer ones (a workgroup each)
int snk_list_sum(hipStream_t st, int wg, const double *scores, const long *pos, const int *pre_id, long pos0, long pre0, const double *pre_mean,
                 const double *pre_std, const long *off, const int *ids, long count, double *mean, double *sd);
// trimmed / median statistics of one class: `threads` per workgroup, `lds` bytes of staged keys (0: the scores are re-read per pass)
int snk_list_select(hipStream_t st, int threads, size_t lds, const double *scores, const long *pos, const int *pre_id, long pos0, long pre0,
                    const double *pre_mean, const double *pre_std, const long *off, const int *ids, long count, int mean_mode, int sorted,
                    double percent_h, double percent_l, double *mean, double *sd);
// order 0: z (rows), 1: t (columns), 2: t then z, 3: z then t; first: NULL or [n], the score after the first of two
int snk_apply_list(hipStream_t st, long n, double *x, int order, const int *row_id, const double *row_mean, const double *row_std,
                   const int *col_id, const double *col_mean, const double *col_std, double *first);
