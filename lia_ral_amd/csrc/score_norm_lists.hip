// score_norm_lists.hip -- LIA_SpkDet/ComputeNorm on score LISTS: the statistics of many distributions of different lengths held as
// a CSR list over one score array (DistribNorm, ComputeNorm.cpp:104-159, filled line by line by getAllScores /
// getAllScoresFirstNormed, :446-489), and the normalisation of a list of trials by per-line entity indices (:542-554, :576-589,
// :634-658, :717-742).  fp64, gfx950.
//
// Distribution d owns the slots k in [off[d], off[d + 1]); slot k holds v = scores[pos ? pos[k] : k], and with pre_id
// (v - pre_mean[pre_id[k]]) / pre_std[pre_id[k]] -- exactly these two operations, computed on the fly, never stored.
//
// CONTRACT: the (mean, std) of a distribution are the bits gmmiv_score_cohort_stats (axis 0, no mask) returns for a one-row matrix
// of the same values in the same order.  The dense launcher (snk_cohort_stats, score_norm.hip) derives everything that fixes the
// fp64 summation order from the row length L alone: k_norm_rowsum<false> (64 threads) up to SN_WAVE_ROW scores and
// k_norm_rowsum<true> (256 threads) above for the untrimmed mean; k_norm_select<1> with pow2(ceil(L / 8)) in 64 .. 1024 threads
// otherwise.  The host therefore bins the distributions by LENGTH CLASS (gmmiv_plan_score_lists, capi_score_lists.hip) and this
// file is launched once per class with the class's thread count and LDS size; a workgroup (a wave of k_norm_listsum<false>) looks
// its distribution up in the class's id table.  Inside a distribution every thread visits the slots the dense kernel's thread of
// the same index visits, in the same order, and the reductions are the same DPP / LDS sequences: a result depends on the
// distribution's own values and length, not on its neighbours, on ndist or on how the call was split into launches.
//
// k_norm_select_lists: the algorithm of k_norm_select<1> per distribution -- order-preserving 64-bit keys, MSD radix select with
// 8-bit digits and one LDS histogram per rank (integer LDS atomics only), digits on which the minimum and maximum key agree
// skipped, one collecting pass once every rank is down to at most SN_CAND candidates, a distribution of at most SN_STAGE scores
// staged in LDS as keys, the summing pass over the scores STRICTLY between the thresholds plus count x value for the kept copies
// of the threshold values.  discardH / discardL / size differ per distribution and are computed here with the reference's fp64
// product and truncation (:129-130).  The quirk is kept: meanMode 1 with both percentages zero does not sort, its "median" is the
// score at slot off[d] + n / 2.
// k_norm_listsum: the untrimmed meanMode 0, one streaming pass; the pair-wise thread assignment of k_norm_rowsum counted from the
// distribution's first slot, 16-byte loads where that slot is 16-byte aligned and the values are read in place (no pos, no
// pre_id), 8-byte loads in the same order otherwise.
// k_norm_apply_list: scores[i] <- (scores[i] - mean[id[i]]) / std[id[i]], one or two steps in the order of GMMIV_NORM_*.
// No floating-point atomic anywhere.  Resource report and timings: DESIGN.md section 3.17.
#include "score_norm_lists.h"

#include "devutil.h"
#include "lds_attr.h"
#include "score_norm_dev.h"

#pragma clang fp contract(off) // (x - mean) / std, sum / size, sum2 / size - mean * mean: the reference's IEEE operations, unfused

// the value of slot k (see the head of the file); pos0 / pre0: the slot a staged host copy of pos / pre_id starts at (off[0]), else 0
struct SnSlots {
    const double *scores;
    const long *pos;
    const int *pre_id;
    const double *pm, *ps;
    long pos0, pre0;
    __device__ __forceinline__ double at(long k) const
    {
        double v = scores[pos ? pos[k - pos0] : k];
        if (pre_id) { const int j = pre_id[k - pre0]; v = (v - pm[j]) / ps[j]; }
        return v;
    }
};

// ---- trimmed / median statistics: one workgroup per distribution of the launch's length class --------------------------------
__global__ __launch_bounds__(SN_MAXT) void k_norm_select_lists(SnSlots sl, const long *__restrict__ off, const int *__restrict__ ids, int mode,
                                                               int sorted, double pH, double pL, double *__restrict__ mean,
                                                               double *__restrict__ sd)
{
    // histograms (and the candidate lists) during the select, reduction scratch before and after: the layout of k_norm_select<1>
    constexpr int RS = 16;
    constexpr int HB = 3 * SN_HS * 4;
    __shared__ u64 sbuf[(HB + 7) / 8];
    __shared__ int s_nc[3];
    __shared__ u64 s_fk[3];
    __shared__ long s_fr[3], s_fc[3];
    __shared__ u64 s_pre[3], s_kmin, s_kmax;
    __shared__ long s_rank[3], s_cnt[3];
    __shared__ int s_alias[3];
    __shared__ unsigned s_seg[3 * 8];
    extern __shared__ u64 stage[]; // [L] keys when the class is staged

    unsigned *hist = (unsigned *)sbuf;
    double *red = (double *)sbuf, *red2 = red + RS;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const long dist = ids[blockIdx.x];
    const long k0 = off[dist], L = off[dist + 1] - k0, n = L;
    const long dH = sorted ? (long)(unsigned long)((double)n * pH) : 0, dL = sorted ? (long)(unsigned long)((double)n * pL) : 0; // :129-130
    const long size = n - dH - dL;
    if (n <= 0 || size <= 0) { // the host refuses such a list before it launches
        if (tid == 0) { mean[dist] = __longlong_as_double(0x7ff8000000000000ll); sd[dist] = __longlong_as_double(0x7ff8000000000000ll); }
        return;
    }
    const bool use_stage = sorted && L <= SN_STAGE;
    if (use_stage) {
        for (long i = tid; i < L; i += nthr) stage[i] = sn_key(sl.at(k0 + i));
        __syncthreads();
    }
    auto key_at = [&](long i) -> u64 { return use_stage ? stage[i] : sn_key(sl.at(k0 + i)); };

    // wave sums by DPP, then wave order through LDS; the result is valid in thread 0
    auto reduce2 = [&](double &a, double &b) {
        a = wave_sum_f64_dpp(a);
        b = wave_sum_f64_dpp(b);
        __syncthreads();
        if ((tid & 63) == 0) { red[tid >> 6] = a; red2[tid >> 6] = b; }
        __syncthreads();
        if (tid == 0)
            for (int w = 1; w < (nthr >> 6); ++w) { a += red[w]; b += red2[w]; }
    };

    u64 kH = 0, kL = 0, kM = 0; // keys of the largest and smallest kept score and of the median
    long keptH = 0, keptL = 0;  // copies of those two values inside the kept range
    if (sorted) {
        const int NT = mode == 1 ? 3 : 2;
        { // minimum and maximum key
            u64 lo = ~0ull, hi = 0;
            for (long i = tid; i < L; i += nthr) {
                const u64 k = key_at(i);
                lo = k < lo ? k : lo;
                hi = k > hi ? k : hi;
            }
            u64 *r0 = sbuf, *r1 = sbuf + RS;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const u64 a = sn_shfl_xor(lo, o), b = sn_shfl_xor(hi, o);
                lo = a < lo ? a : lo;
                hi = b > hi ? b : hi;
            }
            if ((tid & 63) == 0) { r0[tid >> 6] = lo; r1[tid >> 6] = hi; }
            __syncthreads();
            if (tid == 0) {
                u64 a = r0[0], b = r1[0];
                for (int w = 1; w < (nthr >> 6); ++w) {
                    if (r0[w] < a) a = r0[w];
                    if (r1[w] > b) b = r1[w];
                }
                s_kmin = a; s_kmax = b;
                s_rank[0] = dH; s_rank[1] = n - dL - 1; s_rank[2] = dH + size / 2;
                for (int t = 0; t < 3; ++t) { s_pre[t] = a == b ? a : 0; s_cnt[t] = n; s_alias[t] = 0; } // a constant distribution is done
            }
            __syncthreads();
        }
        const u64 kmin = s_kmin, kmax = s_kmax;
        if (kmin != kmax) // (uniform over the workgroup)
            for (int d = 7; d >= 0; --d) {
                const int shift = 8 * d;
                // every rank down to at most SN_CAND scores sharing its prefix: collect them and read each rank off by counting
                bool fin = true;
                for (int t = 0; t < NT; ++t) fin = fin && s_cnt[t] <= SN_CAND;
                if (fin) {
                    const u64 dmask = d == 7 ? 0ull : (~0ull << (shift + 8));
                    u64 *cand = sbuf; // [3][SN_CAND]
                    __syncthreads();
                    if (tid < 3) s_nc[tid] = 0;
                    __syncthreads();
                    {
                        const u64 p0 = s_pre[0], p1 = s_pre[1], p2 = s_pre[2];
                        const bool own1 = s_alias[1] == 1, own2 = NT == 3 && s_alias[2] == 2;
                        for (long i = tid; i < L; i += nthr) {
                            const u64 k = key_at(i), kh = k & dmask;
                            if (kh == p0) { const int at = atomicAdd(&s_nc[0], 1); if (at < SN_CAND) cand[at] = k; }
                            if (own1 && kh == p1) { const int at = atomicAdd(&s_nc[1], 1); if (at < SN_CAND) cand[SN_CAND + at] = k; }
                            if (own2 && kh == p2) { const int at = atomicAdd(&s_nc[2], 1); if (at < SN_CAND) cand[2 * SN_CAND + at] = k; }
                        }
                    }
                    __syncthreads();
                    for (int w = tid; w < 3 * SN_CAND; w += nthr) {
                        const int pt = w / SN_CAND, i = w % SN_CAND;
                        if (pt >= NT) continue;
                        const int al = s_alias[pt], nc = s_nc[al] < SN_CAND ? s_nc[al] : SN_CAND;
                        if (i >= nc) continue;
                        const u64 *cd = cand + al * SN_CAND;
                        const u64 ki = cd[i];
                        long g = 0, e = 0;
                        for (int j = 0; j < nc; ++j) { g += cd[j] > ki; e += cd[j] == ki; }
                        const long r = s_rank[pt];
                        if (g <= r && r < g + e) { s_fk[pt] = ki; s_fr[pt] = r - g; s_fc[pt] = e; } // equal keys write equal values
                    }
                    __syncthreads();
                    if (tid == 0)
                        for (int t = 0; t < NT; ++t) { s_pre[t] = s_fk[t]; s_rank[t] = s_fr[t]; s_cnt[t] = s_fc[t]; }
                    __syncthreads();
                    break;
                }
                if ((kmin >> shift) == (kmax >> shift)) { // every key has kmin's digit here: no pass
                    __syncthreads();
                    if (tid == 0)
                        for (int t = 0; t < 3; ++t) s_pre[t] |= ((kmin >> shift) & 255ull) << shift;
                    __syncthreads();
                    continue;
                }
                __syncthreads();
                for (int i = tid; i < 3 * SN_HS; i += nthr) hist[i] = 0;
                __syncthreads();
                {
                    const u64 himask = d == 7 ? 0ull : (~0ull << (shift + 8));
                    const u64 p0 = s_pre[0], p1 = s_pre[1], p2 = s_pre[2];
                    const bool own1 = s_alias[1] == 1, own2 = NT == 3 && s_alias[2] == 2;
                    for (long i = tid; i < L; i += nthr) {
                        const u64 k = key_at(i), kh = k & himask;
                        const unsigned dg = (unsigned)(k >> shift) & 255u;
                        if (kh == p0) atomicAdd(&hist[dg], 1u);
                        if (own1 && kh == p1) atomicAdd(&hist[SN_HS + dg], 1u);
                        if (own2 && kh == p2) atomicAdd(&hist[2 * SN_HS + dg], 1u);
                    }
                }
                __syncthreads();
                if (tid < 3 * 8) { // 8 threads per rank: counts of 32 bins each, highest bins first
                    const int pt = tid >> 3, sub = tid & 7;
                    const unsigned *h = hist + s_alias[pt] * SN_HS;
                    unsigned s = 0;
#pragma unroll 8
                    for (int b = 0; b < 32; ++b) s += h[255 - 32 * sub - b];
                    s_seg[tid] = s;
                }
                __syncthreads();
                if (tid == 0) {
                    for (int t = 0; t < NT; ++t) {
                        const unsigned *h = hist + s_alias[t] * SN_HS;
                        const unsigned *sg = s_seg + t * 8;
                        long r = s_rank[t], cum = 0;
                        int g = 0;
                        while (g < 7 && cum + (long)sg[g] <= r) { cum += sg[g]; ++g; }
                        int b = 255 - 32 * g;
                        const int bend = b - 31;
                        while (b > bend && cum + (long)h[b] <= r) { cum += h[b]; --b; }
                        s_rank[t] = r - cum;
                        s_cnt[t] = h[b];
                        s_pre[t] |= (u64)b << shift;
                    }
                    s_alias[0] = 0;
                    s_alias[1] = s_pre[1] == s_pre[0] ? 0 : 1;
                    s_alias[2] = s_pre[2] == s_pre[0] ? 0 : (s_pre[2] == s_pre[1] ? s_alias[1] : 2);
                }
                __syncthreads();
            }
        kH = s_pre[0]; kL = s_pre[1]; kM = s_pre[2];
        if (kH == kL) { keptH = size; keptL = 0; }
        else { keptH = s_cnt[0] - s_rank[0]; keptL = s_rank[1] + 1; }
    }
    double vM = 0.0;
    if (mode == 1) vM = sorted ? sn_val(kM) : sl.at(k0 + n / 2);

    double s1 = 0.0, s2 = 0.0;
    for (long i = tid; i < L; i += nthr) {
        double v;
        if (sorted) {
            const u64 k = key_at(i);
            if (!(k < kH && k > kL)) continue;
            v = sn_val(k);
        } else
            v = sl.at(k0 + i);
        if (mode == 0) { s1 += v; s2 += v * v; }
        else s1 += __builtin_fabs(v - vM);
    }
    reduce2(s1, s2);
    if (tid == 0) {
        const double dsize = (double)size;
        if (mode == 0) {
            double sum = s1, sum2 = s2;
            if (sorted) {
                const double vH = sn_val(kH), vL = sn_val(kL);
                sum += (double)keptH * vH;
                sum2 += (double)keptH * (vH * vH);
                if (keptL) { sum += (double)keptL * vL; sum2 += (double)keptL * (vL * vL); }
            }
            const double m = sum / dsize;
            mean[dist] = m;
            sd[dist] = __dsqrt_rn(sum2 / dsize - m * m);
        } else {
            double dev = s1;
            if (sorted) {
                const double vH = sn_val(kH), vL = sn_val(kL);
                dev += (double)keptH * __builtin_fabs(vH - vM);
                if (keptL) dev += (double)keptL * __builtin_fabs(vL - vM);
            }
            mean[dist] = vM;
            sd[dist] = dev / dsize;
        }
    }
}

// ---- untrimmed mean / std: one streaming pass ------------------------------------------------------------------------------------
// WG == false: a wave per distribution, four per workgroup (the class of at most SN_WAVE_ROW scores); WG == true: a workgroup per
// distribution.  Thread t owns the pairs t, t + T, ... counted from the distribution's first slot, thread 0 the odd last score.
template <bool WG>
__global__ __launch_bounds__(256) void k_norm_listsum(SnSlots sl, const long *__restrict__ off, const int *__restrict__ ids, long count,
                                                      double *__restrict__ mean, double *__restrict__ sd)
{
    __shared__ double red[2][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long slot = WG ? (long)blockIdx.x : (long)blockIdx.x * 4 + w;
    const int T = WG ? 256 : 64, t = WG ? (int)threadIdx.x : lane;
    const bool have = slot < count;
    long dist = 0, k0 = 0, L = 0;
    if (have) { dist = ids[slot]; k0 = off[dist]; L = off[dist + 1] - k0; }
    double s1 = 0.0, s2 = 0.0;
    if (have) {
        const double *xp = sl.scores + k0;
        const long P = L >> 1;
        if (!sl.pos && !sl.pre_id && (((uintptr_t)xp) & 15) == 0) {
            const sn_v2 *xv = (const sn_v2 *)xp;
            long i = t;
            for (; i + T < P; i += 2 * T) { // two independent 16-byte loads in flight
                const sn_v2 a = xv[i], b = xv[i + T];
                s1 += a.x; s2 += a.x * a.x;
                s1 += a.y; s2 += a.y * a.y;
                s1 += b.x; s2 += b.x * b.x;
                s1 += b.y; s2 += b.y * b.y;
            }
            for (; i < P; i += T) {
                const sn_v2 a = xv[i];
                s1 += a.x; s2 += a.x * a.x;
                s1 += a.y; s2 += a.y * a.y;
            }
            if ((L & 1) && t == 0) { const double a = xp[L - 1]; s1 += a; s2 += a * a; }
        } else { // the same assignment of scores to threads and the same order: the bits do not depend on the alignment
            for (long i = t; i < P; i += T) {
                const double a = sl.at(k0 + 2 * i), b = sl.at(k0 + 2 * i + 1);
                s1 += a; s2 += a * a;
                s1 += b; s2 += b * b;
            }
            if ((L & 1) && t == 0) { const double a = sl.at(k0 + L - 1); s1 += a; s2 += a * a; }
        }
    }
    s1 = wave_sum_f64_dpp(s1);
    s2 = wave_sum_f64_dpp(s2);
    if (WG) {
        if (lane == 0) { red[0][w] = s1; red[1][w] = s2; }
        __syncthreads();
        if (threadIdx.x == 0) {
            s1 = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
            s2 = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        }
    }
    if (have && t == 0) {
        if (L <= 0) { mean[dist] = __longlong_as_double(0x7ff8000000000000ll); sd[dist] = __longlong_as_double(0x7ff8000000000000ll); return; }
        const double m = s1 / (double)L;
        mean[dist] = m;
        sd[dist] = __dsqrt_rn(s2 / (double)L - m * m);
    }
}

// ---- apply: one pass over a list of trials ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_norm_apply_list(double *__restrict__ x, long n, int order, const int *__restrict__ rid,
                                                         const double *__restrict__ rm, const double *__restrict__ rs,
                                                         const int *__restrict__ cid, const double *__restrict__ cm,
                                                         const double *__restrict__ cs, double *__restrict__ first)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = x[i], y = 0.0;
    double a = 0.0, b = 1.0, m = 0.0, s = 1.0;
    if (order != 1) { const int r = rid[i]; a = rm[r]; b = rs[r]; }
    if (order != 0) { const int c = cid[i]; m = cm[c]; s = cs[c]; }
    switch (order) {
    case 0: v = (v - a) / b; break;
    case 1: v = (v - m) / s; break;
    case 2: y = (v - m) / s; v = (y - a) / b; break;
    default: y = (v - a) / b; v = (y - m) / s; break;
    }
    x[i] = v;
    if (order >= 2 && first) first[i] = y;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
int snk_list_sum(hipStream_t st, int wg, const double *scores, const long *pos, const int *pre_id, long pos0, long pre0, const double *pre_mean,
                 const double *pre_std, const long *off, const int *ids, long count, double *mean, double *sd)
{
    if (count <= 0) return 0;
    const SnSlots sl{scores, pos, pre_id, pre_mean, pre_std, pos0, pre0};
    if (wg) k_norm_listsum<true><<<dim3((unsigned)count), 256, 0, st>>>(sl, off, ids, count, mean, sd);
    else k_norm_listsum<false><<<dim3((unsigned)((count + 3) / 4)), 256, 0, st>>>(sl, off, ids, count, mean, sd);
    return (int)hipGetLastError();
}

int snk_list_select(hipStream_t st, int threads, size_t lds, const double *scores, const long *pos, const int *pre_id, long pos0, long pre0,
                    const double *pre_mean, const double *pre_std, const long *off, const int *ids, long count, int mean_mode, int sorted,
                    double percent_h, double percent_l, double *mean, double *sd)
{
    if (count <= 0) return 0;
    const SnSlots sl{scores, pos, pre_id, pre_mean, pre_std, pos0, pre0};
    if (lds > 48 * 1024) {
        const hipError_t e = gmmiv_lds_attr<k_norm_select_lists>(lds);
        if (e != hipSuccess) return (int)e;
    }
    k_norm_select_lists<<<dim3((unsigned)count), threads, lds, st>>>(sl, off, ids, mean_mode, sorted, percent_h, percent_l, mean, sd);
    return (int)hipGetLastError();
}

int snk_apply_list(hipStream_t st, long n, double *x, int order, const int *row_id, const double *row_mean, const double *row_std,
                   const int *col_id, const double *col_mean, const double *col_std, double *first)
{
    if (n <= 0) return 0;
    k_norm_apply_list<<<dim3((unsigned)((n + 255) / 256)), 256, 0, st>>>(x, n, order, row_id, row_mean, row_std, col_id, col_mean, col_std, first);
    return (int)hipGetLastError();
}
