// iv_trials_kernels.h -- launchers of iv_trials.hip (internal).  Device pointers only; return hipError_t values.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gmmiv_iv_trials.h"

// out [n x ldr] = the columns of X [dim x n] (row stride ld) as rows, the pad column (odd dim) written as 0
int ivk_cols_to_rows(hipStream_t st, int dim, long n, const double *X, long ld, double *out, int ldr);
// the pad column of a row table the GEMM has written (odd dim only): out[r][dim] = 0
int ivk_zero_pad(hipStream_t st, int dim, long n, double *out, int ldr);
// mode 1: (dot * qm) * qs; mode 2: fma(cc, dot, fma(bm, qm, fma(bs, qs, cst))).  anchor_is_seg: Atab / qa are the segment side.
// partner[k] / pos[k]: the partner vector and the list position of sorted entry k (the tiles index them)
int ivk_score_trials(hipStream_t st, int ldr, const double *Atab, const double *Ptab, const double *qa, const double *qp, int anchor_is_seg,
                     const gmmiv_iv_trial_tile *tiles, long ntiles, const int *partner, const int *pos, int mode, double cc, double bm,
                     double bs, double cst, double *scores);
