// feat_norm_window.h -- launcher of feat_norm_window.hip (NormFeat's windowMode, include/gmmiv_feat_window.h) (internal).
#pragma once
#include <hip/hip_runtime.h>

// One workgroup per file, the whole chain of the file in one launch.  partial: nrun x 2 D doubles of scratch (written before it is
// read).  gstat / step_stat may be NULL.  All pointers are device pointers.
int gmmk_norm_window(hipStream_t st, int x_f64, void *x, long ldx, int D, const long *runs, long nrun, long nfiles, const long *step_off,
                     const long *steps, const double *alpha, int cms, int var, double *partial, double *gstat, double *step_stat);
