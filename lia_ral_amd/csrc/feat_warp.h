// feat_warp.h -- launchers of feat_warp.hip (internal; the ABI is include/ext/gmmiv_feat_warp.h).
#pragma once
#include <hip/hip_runtime.h>

// elements of a unit's column the LDS sort takes (a power of two: 128 KB of keys)
constexpr long WARP_SORT_CAP_F32 = 32768, WARP_SORT_CAP_F64 = 16384;

// max_len: the longest unit when the host knows it (sizes the LDS and the workgroup), < 0 when the run table lives on the device;
// force_select: no LDS sort, every unit through the radix select
int gmmk_warp_hist(hipStream_t st, int x_f64, const void *x, long ldx, int D, const long *runs, long nrun, long nunits, int nb, long max_len,
                   int force_select, double *bounds, double *count, int *status);
// ta [nt] | tT [nt + 1]: the target's areas and their left fold
int gmmk_warp_target(hipStream_t st, int nt, const double *tb, const double *tc, double *ta, double *tT);
// 0: no column block fits the LDS (nb too large)
int gmmk_warp_apply_cols(int D, int nb);
int gmmk_warp_apply(hipStream_t st, int x_f64, const void *x, long ldx, int o_f64, void *out, long ldo, int D, const long *runs, long nrun, long nunits,
                    int nb, const double *bounds, const double *count, const int *status, int nt, const double *tb, const double *ta, const double *tT,
                    int n_cu);
