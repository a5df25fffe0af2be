// score_norm_dev.h -- what the kernels of score_norm.hip (dense matrices) and score_norm_lists.hip (ragged lists) share: the
// constants that decide a distribution's launch shape, the order-preserving keys and a 64-bit shuffle.  Device code, internal.
#pragma once
#include <hip/hip_runtime.h>

typedef unsigned long long u64;

#define SN_HS 257       // histogram stride in words (256 bins + 1: adjacent histograms start on different banks)
#define SN_MAXT 1024    // threads per workgroup, at most
#define SN_STAGE 16384  // scores of a row staged in LDS, at most
#define SN_CAND 64      // candidates per rank the select finishes on by counting

__device__ __forceinline__ u64 sn_key(double v)
{
    if (v == 0.0) v = 0.0; // -0.0 -> +0.0
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b ^ 0x8000000000000000ull);
}
__device__ __forceinline__ double sn_val(u64 k)
{
    const u64 b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    return __longlong_as_double((long long)b);
}

__device__ __forceinline__ u64 sn_shfl_xor(u64 v, int m)
{
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}

#define SN_WAVE_ROW 4096 // untrimmed mean / std: a wave per distribution up to this many scores, a workgroup above
typedef double sn_v2 __attribute__((ext_vector_type(2)));
