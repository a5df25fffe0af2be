// score_norm.hip -- LIA_SpkDet/ComputeNorm (z / t / zt / tz-norm) on device-resident score matrices, fp64, gfx950.
//
// DistribNorm::computeMeanStd (ComputeNorm.cpp:121-159) per distribution, WITHOUT sorting:
//   * every score is mapped to an order-preserving 64-bit key (sign bit flipped for non-negatives, all bits for negatives;
//     -0.0 is read as +0.0, the two compare equal in the reference's sort);
//   * the order statistics the trimmed / median modes need -- descending ranks discardH, n - discardL - 1 and, for meanMode 1,
//     discardH + size / 2 -- are located together by a most-significant-digit-first radix select: 8-bit digits, one LDS
//     histogram of 256 bins per (distribution, rank), integer LDS atomics only.  Digits on which the minimum and maximum key
//     of a distribution agree are skipped (a constant distribution needs no pass, scores of one sign and exponent skip two);
//     ranks that still share their prefix share one histogram; once every rank is down to at most 64 candidates the remaining
//     digits are replaced by one collecting pass and a count (typically after two or three digits);
//   * one summing pass over the scores STRICTLY between the two thresholds, plus count x value for the copies of a threshold
//     value the sort would have kept (the select leaves the rank of each statistic inside its run of equal keys, so ties
//     come out as a sort would leave them, upper threshold == lower threshold included).
// No floating-point atomic anywhere: every sum is reduced in a fixed order (DPP inside the wave, LDS across waves / an LDS tree
// across the row lanes of a column strip), so results do not depend on scheduling.
//
// Quirk of the reference, kept: with meanMode 1 and BOTH percentages zero it never sorts, and its "median" is the score at
// position n / 2 in input order (one load here).  NaN scores are outside the contract (the reference's qsort comparator is
// inconsistent on them).
//
// k_norm_select<CW>: one workgroup owns CW adjacent distributions.  CW = 1 (axis 0, one distribution per row, contiguous):
// all threads walk the row; a row of at most 16 K scores is staged once in LDS as keys (128 KB) and selected there, a longer
// one is re-read per digit pass (L2 / Infinity Cache).  CW = 16 (axis 1, one distribution per column): thread t owns column
// t % 16 and every wave load covers four 128-byte row segments; the strip is re-read per pass.
// The untrimmed meanMode 0 needs no select: k_norm_rowsum (16-byte loads, a wave or a workgroup per row) and k_norm_colsum
// + k_norm_colfin (64-column strips split over row slabs, slab sums in the scratch) stream the matrix once.
// k_norm_apply: the (x - mean) / std passes of the four chains, in place, column parameters in registers.
// Resource report (-Rpass-analysis=kernel-resource-usage: no scratch, no spills) and timings: DESIGN.md section 3.11.
#include "score_norm.h"

#include "devutil.h"
#include "lds_attr.h"
#include "score_norm_dev.h" // keys, constants and shuffles shared with score_norm_lists.hip

#pragma clang fp contract(off) // (x - mean) / std, sum / size, sum2 / size - mean * mean: the reference's IEEE operations, unfused

// ---- counts of a device-resident mask: n, discardH, discardL, position of the (n / 2)-th set byte ----------------------
__global__ __launch_bounds__(1024) void k_norm_mask_info(const unsigned char *mask, long L, double pH, double pL, long *info)
{
    __shared__ long cnt[1024];
    __shared__ long tot;
    const int tid = threadIdx.x;
    const long chunk = (L + 1023) / 1024, i0 = tid * chunk, i1 = i0 + chunk < L ? i0 + chunk : L;
    long c = 0;
    for (long i = i0; i < i1; ++i) c += mask[i] != 0;
    cnt[tid] = c;
    __syncthreads();
    if (tid == 0) {
        long s = 0;
        for (int t = 0; t < 1024; ++t) { const long v = cnt[t]; cnt[t] = s; s += v; }
        tot = s;
        info[0] = s;
        info[1] = (long)(unsigned long)((double)s * pH);
        info[2] = (long)(unsigned long)((double)s * pL);
        if (s == 0) info[3] = 0;
    }
    __syncthreads();
    const long want = tot / 2, before = cnt[tid];
    if (c > 0 && before <= want && want < before + c) {
        long k = before;
        for (long i = i0; i < i1; ++i)
            if (mask[i]) {
                if (k == want) { info[3] = i; break; }
                ++k;
            }
    }
}

// ---- statistics of CW adjacent distributions per workgroup --------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(SN_MAXT) void k_norm_select(const double *__restrict__ x, long ndist, long L, long dstride, long estride,
                                                         const unsigned char *__restrict__ mask, const double *__restrict__ pm,
                                                         const double *__restrict__ ps, int mode, int sorted, long n, long dH, long dL,
                                                         long qidx, const long *__restrict__ info, int staged,
                                                         double *__restrict__ mean, double *__restrict__ sd)
{
    // histograms (and the candidate lists) during the select, reduction scratch before and after.  CW == 1 reduces inside the
    // waves first and needs 16 slots per array: 3 KB per workgroup, so a 1000-score row (8 KB staged) runs 14 workgroups per CU
    constexpr int RS = CW == 1 ? 16 : SN_MAXT;
    constexpr int HB = CW * 3 * SN_HS * 4, RB = 2 * RS * 8;
    __shared__ u64 sbuf[((HB > RB ? HB : RB) + 7) / 8];
    __shared__ int s_nc[CW * 3];
    __shared__ u64 s_fk[CW * 3];
    __shared__ long s_fr[CW * 3], s_fc[CW * 3];
    __shared__ u64 s_pre[CW][3], s_kmin[CW], s_kmax[CW];
    __shared__ long s_rank[CW][3], s_cnt[CW][3];
    __shared__ int s_alias[CW][3];
    __shared__ unsigned s_seg[CW * 3 * 8];
    extern __shared__ u64 stage[]; // [L][CW] keys when `staged`

    unsigned *hist = (unsigned *)sbuf;
    double *red = (double *)sbuf, *red2 = red + RS;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int c = tid % CW, rl = tid / CW, RL = nthr / CW;
    const long dist = (long)blockIdx.x * CW + c;
    const bool live = dist < ndist;
    if (info) { n = info[0]; dH = info[1]; dL = info[2]; qidx = info[3]; }
    const long size = n - dH - dL;
    if (n <= 0 || size <= 0) { // only reachable with a device-resident mask (the host refuses it otherwise)
        if (live && rl == 0) { mean[dist] = __longlong_as_double(0x7ff8000000000000ll); sd[dist] = __longlong_as_double(0x7ff8000000000000ll); }
        return;
    }
    const double *xp = x + (live ? dist : 0) * dstride;
    auto load = [&](long i) -> double {
        double v = xp[i * estride];
        if (pm) v = (v - pm[i]) / ps[i];
        return v;
    };
    const bool use_stage = staged && sorted;
    if (use_stage) {
        for (long i = rl; i < L; i += RL) stage[i * CW + c] = sn_key(load(i));
        __syncthreads();
    }
    auto key_at = [&](long i) -> u64 { return use_stage ? stage[i * CW + c] : sn_key(load(i)); };

    // per-column reduction over the row lanes, fixed order; the result is valid in the thread with rl == 0
    auto reduce2 = [&](double &a, double &b) {
        if constexpr (CW == 1) {
            a = wave_sum_f64_dpp(a);
            b = wave_sum_f64_dpp(b);
            __syncthreads();
            if ((tid & 63) == 0) { red[tid >> 6] = a; red2[tid >> 6] = b; }
            __syncthreads();
            if (tid == 0)
                for (int w = 1; w < (nthr >> 6); ++w) { a += red[w]; b += red2[w]; }
        } else {
            __syncthreads();
            red[tid] = a; red2[tid] = b;
            __syncthreads();
            for (int s = RL >> 1; s > 0; s >>= 1) {
                if (rl < s) { red[tid] += red[tid + s * CW]; red2[tid] += red2[tid + s * CW]; }
                __syncthreads();
            }
            a = red[tid]; b = red2[tid];
        }
    };

    u64 kH = 0, kL = 0, kM = 0; // keys of the largest and smallest kept score and of the median
    long keptH = 0, keptL = 0;  // copies of those two values inside the kept range
    if (sorted) {
        const int NT = mode == 1 ? 3 : 2;
        // minimum and maximum key of each distribution
        {
            u64 lo = ~0ull, hi = 0;
            if (live)
                for (long i = rl; i < L; i += RL) {
                    if (mask && !mask[i]) continue;
                    const u64 k = key_at(i);
                    lo = k < lo ? k : lo;
                    hi = k > hi ? k : hi;
                }
            u64 *r0 = sbuf, *r1 = sbuf + RS;
            if constexpr (CW == 1) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const u64 a = sn_shfl_xor(lo, o), b = sn_shfl_xor(hi, o);
                    lo = a < lo ? a : lo;
                    hi = b > hi ? b : hi;
                }
                if ((tid & 63) == 0) { r0[tid >> 6] = lo; r1[tid >> 6] = hi; }
                __syncthreads();
                if (tid == 0)
                    for (int w = 1; w < (nthr >> 6); ++w) {
                        if (r0[w] < r0[0]) r0[0] = r0[w];
                        if (r1[w] > r1[0]) r1[0] = r1[w];
                    }
            } else {
                r0[tid] = lo; r1[tid] = hi;
                __syncthreads();
                for (int s = RL >> 1; s > 0; s >>= 1) {
                    if (rl < s) {
                        const u64 a = r0[tid + s * CW], b = r1[tid + s * CW];
                        if (a < r0[tid]) r0[tid] = a;
                        if (b > r1[tid]) r1[tid] = b;
                    }
                    __syncthreads();
                }
            }
            if (rl == 0) {
                const u64 a = r0[tid], b = r1[tid];
                s_kmin[c] = a; s_kmax[c] = b;
                s_rank[c][0] = dH; s_rank[c][1] = n - dL - 1; s_rank[c][2] = dH + size / 2;
                for (int t = 0; t < 3; ++t) { s_pre[c][t] = a == b ? a : 0; s_cnt[c][t] = n; s_alias[c][t] = 0; } // a constant distribution is done
            }
            __syncthreads();
        }
        const u64 kmin = s_kmin[c], kmax = s_kmax[c];
        for (int d = 7; d >= 0; --d) {
            const int shift = 8 * d;
            // Once every rank of every distribution of the strip is down to at most SN_CAND scores sharing its prefix, the
            // remaining digits are not worth a pass each: the candidates are collected (their order does not matter) and each
            // rank is read off by counting -- the same key, the same position inside its run of equal keys, the same run length.
            bool fin = !live || kmin == kmax;
            if (!fin) {
                fin = true;
                for (int t = 0; t < NT; ++t) fin = fin && s_cnt[c][t] <= SN_CAND;
            }
            if (__syncthreads_and(fin)) {
                const u64 dmask = d == 7 ? 0ull : (~0ull << (shift + 8));
                u64 *cand = sbuf; // [CW * 3][SN_CAND]
                if (tid < CW * 3) s_nc[tid] = 0;
                __syncthreads();
                if (live && kmin != kmax) {
                    const u64 p0 = s_pre[c][0], p1 = s_pre[c][1], p2 = s_pre[c][2];
                    const bool own1 = s_alias[c][1] == 1, own2 = NT == 3 && s_alias[c][2] == 2;
                    for (long i = rl; i < L; i += RL) {
                        if (mask && !mask[i]) continue;
                        const u64 k = key_at(i), kh = k & dmask;
                        if (kh == p0) { const int pos = atomicAdd(&s_nc[c * 3], 1); if (pos < SN_CAND) cand[(c * 3) * SN_CAND + pos] = k; }
                        if (own1 && kh == p1) { const int pos = atomicAdd(&s_nc[c * 3 + 1], 1); if (pos < SN_CAND) cand[(c * 3 + 1) * SN_CAND + pos] = k; }
                        if (own2 && kh == p2) { const int pos = atomicAdd(&s_nc[c * 3 + 2], 1); if (pos < SN_CAND) cand[(c * 3 + 2) * SN_CAND + pos] = k; }
                    }
                }
                __syncthreads();
                for (int w = tid; w < CW * 3 * SN_CAND; w += nthr) {
                    const int p = w / SN_CAND, i = w % SN_CAND, pc = p / 3, pt = p % 3;
                    if (pt >= NT || (long)blockIdx.x * CW + pc >= ndist || s_kmin[pc] == s_kmax[pc]) continue;
                    const int al = s_alias[pc][pt], nc = s_nc[pc * 3 + al] < SN_CAND ? s_nc[pc * 3 + al] : SN_CAND;
                    if (i >= nc) continue;
                    const u64 *cd = cand + (pc * 3 + al) * SN_CAND;
                    const u64 ki = cd[i];
                    long g = 0, e = 0;
                    for (int j = 0; j < nc; ++j) { g += cd[j] > ki; e += cd[j] == ki; }
                    const long r = s_rank[pc][pt];
                    if (g <= r && r < g + e) { s_fk[p] = ki; s_fr[p] = r - g; s_fc[p] = e; } // equal keys write equal values
                }
                __syncthreads();
                if (rl == 0 && live && kmin != kmax)
                    for (int t = 0; t < NT; ++t) { s_pre[c][t] = s_fk[c * 3 + t]; s_rank[c][t] = s_fr[c * 3 + t]; s_cnt[c][t] = s_fc[c * 3 + t]; }
                __syncthreads();
                break;
            }
            const bool skip = !live || (kmin >> shift) == (kmax >> shift); // every key of this distribution has kmin's digit
            if (!__syncthreads_or(!skip)) { // no distribution of the strip needs this pass
                if (live && rl == 0)
                    for (int t = 0; t < 3; ++t) s_pre[c][t] |= ((kmin >> shift) & 255ull) << shift;
                continue;
            }
            for (int i = tid; i < CW * 3 * SN_HS; i += nthr) hist[i] = 0;
            __syncthreads();
            if (!skip) {
                const u64 himask = d == 7 ? 0ull : (~0ull << (shift + 8));
                const u64 p0 = s_pre[c][0], p1 = s_pre[c][1], p2 = s_pre[c][2];
                const bool own1 = s_alias[c][1] == 1, own2 = NT == 3 && s_alias[c][2] == 2;
                const int hb = c * 3 * SN_HS;
                for (long i = rl; i < L; i += RL) {
                    if (mask && !mask[i]) continue;
                    const u64 k = key_at(i), kh = k & himask;
                    const unsigned dg = (unsigned)(k >> shift) & 255u;
                    if (kh == p0) atomicAdd(&hist[hb + dg], 1u);
                    if (own1 && kh == p1) atomicAdd(&hist[hb + SN_HS + dg], 1u);
                    if (own2 && kh == p2) atomicAdd(&hist[hb + 2 * SN_HS + dg], 1u);
                }
            }
            __syncthreads();
            // 8 threads per (distribution, rank): counts of 32 bins each, highest bins first
            if (tid < CW * 3 * 8) {
                const int p = tid >> 3, sub = tid & 7, pc = p / 3, pt = p % 3;
                const unsigned *h = hist + (pc * 3 + s_alias[pc][pt]) * SN_HS;
                unsigned s = 0;
#pragma unroll 8
                for (int b = 0; b < 32; ++b) s += h[255 - 32 * sub - b];
                s_seg[tid] = s;
            }
            __syncthreads();
            if (rl == 0) {
                if (skip) {
                    if (live)
                        for (int t = 0; t < 3; ++t) s_pre[c][t] |= ((kmin >> shift) & 255ull) << shift;
                } else {
                    for (int t = 0; t < NT; ++t) {
                        const int al = s_alias[c][t];
                        const unsigned *h = hist + (c * 3 + al) * SN_HS;
                        const unsigned *sg = s_seg + (c * 3 + t) * 8;
                        long r = s_rank[c][t], cum = 0;
                        int g = 0;
                        while (g < 7 && cum + (long)sg[g] <= r) { cum += sg[g]; ++g; }
                        int b = 255 - 32 * g;
                        const int bend = b - 31;
                        while (b > bend && cum + (long)h[b] <= r) { cum += h[b]; --b; }
                        s_rank[c][t] = r - cum;
                        s_cnt[c][t] = h[b];
                        s_pre[c][t] |= (u64)b << shift;
                    }
                    s_alias[c][0] = 0;
                    s_alias[c][1] = s_pre[c][1] == s_pre[c][0] ? 0 : 1;
                    s_alias[c][2] = s_pre[c][2] == s_pre[c][0] ? 0 : (s_pre[c][2] == s_pre[c][1] ? s_alias[c][1] : 2);
                }
            }
            __syncthreads();
        }
        kH = s_pre[c][0]; kL = s_pre[c][1]; kM = s_pre[c][2];
        if (kH == kL) { keptH = size; keptL = 0; }
        else { keptH = s_cnt[c][0] - s_rank[c][0]; keptL = s_rank[c][1] + 1; }
    }
    double vM = 0.0;
    if (mode == 1) vM = sorted ? sn_val(kM) : (live ? load(qidx) : 0.0);

    double s1 = 0.0, s2 = 0.0;
    if (live)
        for (long i = rl; i < L; i += RL) {
            if (mask && !mask[i]) continue;
            double v;
            if (sorted) {
                const u64 k = key_at(i);
                if (!(k < kH && k > kL)) continue;
                v = sn_val(k);
            } else
                v = load(i);
            if (mode == 0) { s1 += v; s2 += v * v; }
            else s1 += __builtin_fabs(v - vM);
        }
    reduce2(s1, s2);
    if (live && rl == 0) {
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

// ---- untrimmed mean / std along columns: a streaming pass split over row slabs ------------------------------------------------
// k_norm_select<16> keeps 24 waves per CU busy with one 512-byte load each: enough for the re-read passes of the select, a
// fraction of HBM for the one pass the untrimmed meanMode 0 needs.  Here a workgroup owns 64 adjacent columns (every wave load is
// one 512-byte row segment, four in flight per wave) and one of up to SN_SLABS row slabs; the slab sums go to the scratch
// ([slab][sum | sum2][column], 512 bytes per distribution) and k_norm_colfin adds them in slab order: fixed order, no atomics.
#define SN_SLABS 32

__global__ __launch_bounds__(256) void k_norm_colsum(const double *__restrict__ x, long rows, long cols, long ld,
                                                     const unsigned char *__restrict__ mask, const double *__restrict__ pm,
                                                     const double *__restrict__ ps, long rows_per_slab, double *__restrict__ part)
{
    __shared__ double red[2][4][64];
    const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * 64 + lane;
    const long r0 = (long)blockIdx.y * rows_per_slab, r1 = r0 + rows_per_slab < rows ? r0 + rows_per_slab : rows;
    double s1 = 0.0, s2 = 0.0;
    if (c < cols) {
        const double *xp = x + c;
        if (!mask && !pm) {
            long r = r0 + rl;
            for (; r + 12 < r1; r += 16) { // four independent loads in flight
                const double a = xp[r * ld], b = xp[(r + 4) * ld], cc = xp[(r + 8) * ld], d = xp[(r + 12) * ld];
                s1 += a; s2 += a * a;
                s1 += b; s2 += b * b;
                s1 += cc; s2 += cc * cc;
                s1 += d; s2 += d * d;
            }
            for (; r < r1; r += 4) { const double a = xp[r * ld]; s1 += a; s2 += a * a; }
        } else {
            for (long r = r0 + rl; r < r1; r += 4) {
                if (mask && !mask[r]) continue;
                double a = xp[r * ld];
                if (pm) a = (a - pm[r]) / ps[r];
                s1 += a; s2 += a * a;
            }
        }
    }
    red[0][rl][lane] = s1; red[1][rl][lane] = s2;
    __syncthreads();
    if (rl == 0 && c < cols) {
        for (int k = 1; k < 4; ++k) { s1 += red[0][k][lane]; s2 += red[1][k][lane]; }
        part[((long)blockIdx.y * 2 + 0) * cols + c] = s1;
        part[((long)blockIdx.y * 2 + 1) * cols + c] = s2;
    }
}

__global__ __launch_bounds__(256) void k_norm_colfin(const double *__restrict__ part, long cols, int slabs, long n, const long *__restrict__ info,
                                                     double *__restrict__ mean, double *__restrict__ sd)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    if (info) n = info[0];
    if (n <= 0) { mean[c] = __longlong_as_double(0x7ff8000000000000ll); sd[c] = __longlong_as_double(0x7ff8000000000000ll); return; }
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < slabs; ++k) { s1 += part[((long)k * 2 + 0) * cols + c]; s2 += part[((long)k * 2 + 1) * cols + c]; }
    const double m = s1 / (double)n;
    mean[c] = m;
    sd[c] = __dsqrt_rn(s2 / (double)n - m * m);
}

// ---- untrimmed mean / std along rows: one streaming pass, 16-byte loads -----------------------------------------------------
// Rows of at most SN_WAVE_ROW scores: one wave per row, four rows per workgroup; longer rows: one workgroup per row.  Sums are
// reduced by DPP inside the wave and in wave order through LDS.  vec: every row starts on 16 bytes (base aligned, even ld);
// a row that does not is read with 8-byte loads in the same order.

template <bool WG>
__global__ __launch_bounds__(256) void k_norm_rowsum(const double *__restrict__ x, long rows, long L, long ld,
                                                     const unsigned char *__restrict__ mask, const double *__restrict__ pm,
                                                     const double *__restrict__ ps, long n, const long *__restrict__ info, int vec,
                                                     double *__restrict__ mean, double *__restrict__ sd)
{
    __shared__ double red[2][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long row = WG ? (long)blockIdx.x : (long)blockIdx.x * 4 + w;
    const int T = WG ? 256 : 64, t = WG ? (int)threadIdx.x : lane;
    double s1 = 0.0, s2 = 0.0;
    if (row < rows) {
        const double *xp = x + row * ld;
        if (vec && !mask && !pm) {
            const sn_v2 *xv = (const sn_v2 *)xp;
            const long P = L >> 1;
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
            auto add = [&](long j) {
                if (mask && !mask[j]) return;
                double a = xp[j];
                if (pm) a = (a - pm[j]) / ps[j];
                s1 += a; s2 += a * a;
            };
            const long P = L >> 1;
            for (long i = t; i < P; i += T) { add(2 * i); add(2 * i + 1); }
            if ((L & 1) && t == 0) add(L - 1);
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
    if (row < rows && t == 0) {
        if (info) n = info[0];
        if (n <= 0) { mean[row] = __longlong_as_double(0x7ff8000000000000ll); sd[row] = __longlong_as_double(0x7ff8000000000000ll); return; }
        const double m = s1 / (double)n;
        mean[row] = m;
        sd[row] = __dsqrt_rn(s2 / (double)n - m * m);
    }
}

// ---- apply: one in-place pass over X[M x S] -------------------------------------------------------------------------------
#define SN_ROWS 8 // rows per workgroup (the column parameters stay in registers across them)

typedef double sn_d2 __attribute__((ext_vector_type(2)));
template <bool NT, typename T> __device__ __forceinline__ void sn_store(T *p, T v)
{
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

template <int W, bool NT>
__global__ __launch_bounds__(256) void k_norm_apply(double *__restrict__ X, long M, long S, int order, const double *__restrict__ rm,
                                                    const double *__restrict__ rs, const double *__restrict__ cm,
                                                    const double *__restrict__ cs, double *__restrict__ first)
{
    const long col = ((long)blockIdx.y * 256 + threadIdx.x) * W;
    if (col >= S) return;
    const long r0 = (long)blockIdx.x * SN_ROWS, r1 = r0 + SN_ROWS < M ? r0 + SN_ROWS : M;
    double m[W], s[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { m[j] = 0.0; s[j] = 1.0; }
    if (order != 0) {
#pragma unroll
        for (int j = 0; j < W; ++j) { m[j] = cm[col + j]; s[j] = cs[col + j]; }
    }
    for (long r = r0; r < r1; ++r) {
        double *p = X + r * S + col;
        double v[W], y[W];
        if (W == 2) { const sn_d2 t = *(const sn_d2 *)p; v[0] = t.x; v[W - 1] = t.y; }
        else v[0] = *p;
        double a = 0.0, b = 1.0;
        if (order != 1) { a = rm[r]; b = rs[r]; }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            switch (order) {
            case 0: v[j] = (v[j] - a) / b; break;
            case 1: v[j] = (v[j] - m[j]) / s[j]; break;
            case 2: y[j] = (v[j] - m[j]) / s[j]; v[j] = (y[j] - a) / b; break;
            default: y[j] = (v[j] - a) / b; v[j] = (y[j] - m[j]) / s[j]; break;
            }
        }
        if (W == 2) sn_store<NT>((sn_d2 *)p, sn_d2{v[0], v[W - 1]});
        else sn_store<NT>(p, v[0]);
        if (order >= 2 && first) {
            double *q = first + r * S + col;
            if (W == 2) sn_store<NT>((sn_d2 *)q, sn_d2{y[0], y[W - 1]});
            else sn_store<NT>(q, y[0]);
        }
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
int snk_mask_info(hipStream_t st, const unsigned char *mask, long L, double percent_h, double percent_l, long *info)
{
    k_norm_mask_info<<<1, 1024, 0, st>>>(mask, L, percent_h, percent_l, info);
    return (int)hipGetLastError();
}

static int pow2_at_least(long v)
{
    int p = 64;
    while (p < v && p < SN_MAXT) p <<= 1;
    return p;
}

int snk_cohort_stats(hipStream_t st, int axis, long rows, long cols, const double *x, long ld, const unsigned char *mask,
                     const double *pre_mean, const double *pre_std, int mean_mode, int sorted, long n, long dH, long dL, long qidx,
                     const long *info, double *part, double *mean, double *sd)
{
    if (axis == 0 && mean_mode == 0 && !sorted) {
        const int vec = (((uintptr_t)x) & 15) == 0 && (ld & 1) == 0;
        if (cols <= SN_WAVE_ROW)
            k_norm_rowsum<false><<<dim3((unsigned)((rows + 3) / 4)), 256, 0, st>>>(x, rows, cols, ld, mask, pre_mean, pre_std, n, info, vec, mean, sd);
        else
            k_norm_rowsum<true><<<dim3((unsigned)rows), 256, 0, st>>>(x, rows, cols, ld, mask, pre_mean, pre_std, n, info, vec, mean, sd);
    } else if (axis == 0) {
        const long L = cols;
        const int staged = sorted && L <= SN_STAGE;
        const size_t lds = staged ? (size_t)L * 8 : 0;
        // 8 scores per thread and pass: a 1000-score cohort runs two waves per row, several rows per CU
        const int threads = pow2_at_least((L + 7) / 8);
        if (lds > 48 * 1024) {
            const hipError_t e = gmmiv_lds_attr<k_norm_select<1>>(lds);
            if (e != hipSuccess) return (int)e;
        }
        k_norm_select<1><<<dim3((unsigned)rows), threads, lds, st>>>(x, rows, L, ld, 1, mask, pre_mean, pre_std, mean_mode, sorted, n, dH, dL,
                                                                    qidx, info, staged, mean, sd);
    } else if (mean_mode == 0 && !sorted && part) {
        const long L = rows;
        long slabs = (L + 255) / 256;
        slabs = slabs < 1 ? 1 : (slabs > SN_SLABS ? SN_SLABS : slabs);
        const long per = (((L + slabs - 1) / slabs) + 3) & ~3l;
        slabs = (L + per - 1) / per;
        k_norm_colsum<<<dim3((unsigned)((cols + 63) / 64), (unsigned)slabs), 256, 0, st>>>(x, rows, cols, ld, mask, pre_mean, pre_std, per, part);
        k_norm_colfin<<<dim3((unsigned)((cols + 255) / 256)), 256, 0, st>>>(part, cols, (int)slabs, n, info, mean, sd);
    } else {
        const long L = rows;
        k_norm_select<16><<<dim3((unsigned)((cols + 15) / 16)), 512, 0, st>>>(x, cols, L, 1, ld, mask, pre_mean, pre_std, mean_mode, sorted, n,
                                                                              dH, dL, qidx, info, 0, mean, sd);
    }
    return (int)hipGetLastError();
}

int snk_apply(hipStream_t st, long M, long S, double *X, int order, const double *row_mean, const double *row_std, const double *col_mean,
              const double *col_std, double *first)
{
    const bool vec = (S & 1) == 0 && (((uintptr_t)X | (uintptr_t)first) & 15) == 0;
    const bool nt = (size_t)M * (size_t)S * 8 > ((size_t)256 << 20); // beyond the Infinity Cache: do not keep the output there
    const int W = vec ? 2 : 1;
    const dim3 grid((unsigned)((M + SN_ROWS - 1) / SN_ROWS), (unsigned)((S + 256 * W - 1) / (256 * W)));
    if (vec && nt) k_norm_apply<2, true><<<grid, 256, 0, st>>>(X, M, S, order, row_mean, row_std, col_mean, col_std, first);
    else if (vec) k_norm_apply<2, false><<<grid, 256, 0, st>>>(X, M, S, order, row_mean, row_std, col_mean, col_std, first);
    else if (nt) k_norm_apply<1, true><<<grid, 256, 0, st>>>(X, M, S, order, row_mean, row_std, col_mean, col_std, first);
    else k_norm_apply<1, false><<<grid, 256, 0, st>>>(X, M, S, order, row_mean, row_std, col_mean, col_std, first);
    return (int)hipGetLastError();
}
