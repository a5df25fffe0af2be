// energy_det.hip -- EnergyDetector (LIA_SpkDet/EnergyDetector/src/EnergyDetector.cpp:118-279) for a whole list of files (include/gmmiv.h,
// "EnergyDetector on resident frames"): k_energy_em keeps ONE FILE'S whole chain -- FrameAccGD variance, energyMixtureInit, nb_train_it x
// (full-posterior EM statistics, getEM, varianceControl), the meanStd threshold -- inside one workgroup of one launch; k_energy_select is
// selectFrames as a parallel pass.  Both are latency kernels: a model of <= 8 one-dimensional Gaussians and a few thousand scalars per
// file, the list spread over the CUs.  No kernel here adds into memory another workgroup adds into and there is no atomic: every sum has
// one owner and one fixed order (per-lane strided partials, a DPP wave reduction, the waves added in order), a function of the file's
// selection and of the launch shape EN_THREADS alone -- a file's bits never depend on its neighbours or on its place in the list.
#include "devutil.h"
#include "gmm_kernels.h"
#include "lds_attr.h"
#include "../../include/gmmiv.h"

constexpr int EN_THREADS = 512, EN_WAVES = EN_THREADS / 64, EN_CMAX = 8, EN_NSUM = 3 * EN_CMAX + 1;
constexpr long EN_STAGE_BYTES = 128 << 10; // of the CU's 160 KB: the staged selection; the reduction scratch is static
constexpr int SEL_THREADS = 256, SEL_WAVES = SEL_THREADS / 64;

long gmmk_energy_stage_frames(int x_f64) { return EN_STAGE_BYTES / (x_f64 ? 8 : 4); }

// the runs of file f in a table whose file ids are non-decreasing: [lo, hi)
static __device__ __forceinline__ void en_file_runs(const long *__restrict__ runs, long nrun, long f, long &lo, long &hi)
{
    long a = 0, b = nrun;
    while (a < b) {
        const long mid = (a + b) >> 1;
        if (runs[3 * mid + 2] < f) a = mid + 1; else b = mid;
    }
    lo = a;
    b = nrun;
    while (a < b) {
        const long mid = (a + b) >> 1;
        if (runs[3 * mid + 2] <= f) a = mid + 1; else b = mid;
    }
    hi = a;
}

// Block sum of NS values per thread -> every thread reads tot[0 .. NS).  Order: DPP wave sum, then waves 0 .. EN_WAVES-1 added in order.
template <int NS>
static __device__ __forceinline__ void en_block_sum(const double *v, double (*part)[EN_NSUM], double *tot, int tid)
{
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < NS; ++k)
    {
        const double s = wave_sum_f64_dpp(v[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (tid < NS) {
        double a = part[0][tid];
#pragma unroll
        for (int w = 1; w < EN_WAVES; ++w) a += part[w][tid];
        tot[tid] = a;
    }
    __syncthreads();
}

// One instantiation per Gaussian count C (1 .. EN_CMAX): the model and the 3 C + 1 partial sums of a lane live in registers.
// model [nfiles x 3 C] = (w | mean | cov), threshold [nfiles], status [nfiles]; order (nullable): the file each workgroup takes
template <typename XT, int C>
__global__ __launch_bounds__(EN_THREADS) void k_energy_em(const XT *__restrict__ x, long ldx, const long *__restrict__ runs, long nrun, long nfiles,
                                                          const long *__restrict__ order, int nb_it, double flooring, double ceiling, double alpha,
                                                          long stage_frames, double *__restrict__ model, double *__restrict__ threshold,
                                                          int *__restrict__ status)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char en_lds[];
    __shared__ double part[EN_WAVES][EN_NSUM], tot[EN_NSUM];
    __shared__ double s_w[EN_CMAX], s_m[EN_CMAX], s_v[EN_CMAX], s_k[EN_CMAX], s_iv[EN_CMAX];
    __shared__ int s_fl[EN_CMAX];
    XT *stage = (XT *)en_lds;
    const int tid = threadIdx.x;
    const long f = order ? order[blockIdx.x] : (long)blockIdx.x;
    if ((unsigned long)f >= (unsigned long)nfiles) return;
    long r0, r1;
    en_file_runs(runs, nrun, f, r0, r1);
    long n = 0;
    for (long r = r0; r < r1; ++r) { const long len = runs[3 * r + 1]; n += len > 0 ? len : 0; }
    const bool staged = n <= stage_frames;

    // ---- the selection into LDS (raw values) and FrameAccGD's sums of the raw values, lane tid owns frames tid, tid + EN_THREADS, ...
    double acc[3 * C + 1];
    acc[0] = 0.0; acc[1] = 0.0;
    {
        long off = 0;
        for (long r = r0; r < r1; ++r) {
            const long first = runs[3 * r], len = runs[3 * r + 1];
            if (len <= 0) continue;
            const XT *p = x + first * ldx;
            long t = (long)tid - off % EN_THREADS; // the first frame of the run with (off + t) % EN_THREADS == tid
            if (t < 0) t += EN_THREADS;
            for (; t < len; t += EN_THREADS) {
                const XT raw = p[t * ldx];
                if (staged) stage[off + t] = raw;
                const double v = (double)raw, vv = v * v;
                acc[0] += v;
                acc[1] += vv;
            }
            off += len;
        }
    }
    en_block_sum<2>(acc, part, tot, tid); // (the barrier inside also publishes the staged frames)
    const double dn = (double)n;
    const double gmean = tot[0] / dn, gq = tot[1] / dn, gmm = gmean * gmean, gcov = gq - gmm;

    // ---- energyMixtureInit
    if (tid < C) {
        s_w[tid] = 1.0 / (double)C;
        s_m[tid] = C > 1 ? -2.0 + (double)tid * (4.0 / (double)(C - 1)) : -2.0;
        s_v[tid] = 1.0;
    }
    if (tid < EN_CMAX) s_fl[tid] = 0;
    __syncthreads();

    for (int it = 0; it < nb_it && n > 0; ++it) {
        // log(w_c / sqrt(2 pi cov_c)) and 1 / cov_c
        if (tid < C) {
            s_k[tid] = log(s_w[tid]) - 0.5 * log(6.283185307179586477 * s_v[tid]);
            s_iv[tid] = 1.0 / s_v[tid];
        }
        __syncthreads();
        double mk[C], mm[C], mi[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { mk[c] = s_k[c]; mm[c] = s_m[c]; mi[c] = s_iv[c]; }
#pragma unroll
        for (int k = 0; k < 3 * C + 1; ++k) acc[k] = 0.0;
        auto frame = [&](double xv) {
            double l[C], L = -__builtin_inf();
            bool bad = false;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                    const double d = xv - mm[c];
                    const double q = d * d * mi[c];
                    l[c] = mk[c] - 0.5 * q;
                    bad |= l[c] != l[c];
                    if (l[c] > L) L = l[c];
                }
            // the zero-likelihood rule: the largest logit below GMMIV_ZERO_LLK, or a log-sum that is not finite -> the frame adds nothing
            if (bad || !(L >= GMMIV_ZERO_LLK) || L == __builtin_inf()) return;
            double e[C], S = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) { e[c] = gexp(l[c] - L); S += e[c]; }
            const double inv = 1.0 / S, x2 = xv * xv;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                    const double g = e[c] * inv;
                    acc[1 + 3 * c] += g;
                    acc[2 + 3 * c] += g * xv;
                    acc[3 + 3 * c] += g * x2;
                }
            acc[0] += 1.0;
        };
        if (staged) {
            for (long i = tid; i < n; i += EN_THREADS) frame((double)feat_sane(stage[i]));
        } else {
            long off = 0;
            for (long r = r0; r < r1; ++r) {
                const long first = runs[3 * r], len = runs[3 * r + 1];
                if (len <= 0) continue;
                const XT *p = x + first * ldx;
                long t = (long)tid - off % EN_THREADS;
                if (t < 0) t += EN_THREADS;
                for (; t < len; t += EN_THREADS) frame((double)feat_sane(p[t * ldx]));
                off += len;
            }
        }
        en_block_sum<3 * C + 1>(acc, part, tot, tid); // count | (occ, sum g x, sum g x^2) per Gaussian
        // getEM + varianceControl, one lane per Gaussian
        if (tid < C) {
            const double occ = tot[1 + 3 * tid], count = tot[0];
            s_w[tid] = occ / count;
            double cv = s_v[tid];
            if (occ > 0.0) {
                const double m = tot[2 + 3 * tid] / occ, mq = m * m;
                s_m[tid] = m;
                cv = tot[3 + 3 * tid] / occ - mq;
            }
            int fl = 0;
            const double lo = flooring * gcov, hi = ceiling * gcov;
            if (cv <= lo) { cv = lo; fl |= GMMIV_ENERGY_FLOORED; }
            if (cv >= hi) { cv = hi; fl |= GMMIV_ENERGY_CEILED; }
            s_v[tid] = cv;
            if (it == nb_it - 1) s_fl[tid] = fl;
        }
        __syncthreads();
    }

    if (tid == 0) {
        int higher = 0, st = n > 0 ? 0 : GMMIV_ENERGY_EMPTY;
        for (int c = 1; c < C; ++c)
            if (s_m[c] > s_m[higher]) higher = c;
        for (int c = 0; c < C; ++c) st |= s_fl[c];
        const double sd = __builtin_sqrt(s_v[higher]), th = n > 0 ? s_m[higher] - alpha * sd : __builtin_nan("");
        bool fin = __builtin_isfinite(th);
        for (int c = 0; c < C; ++c) {
            model[f * 3 * C + c] = s_w[c];
            model[f * 3 * C + C + c] = s_m[c];
            model[f * 3 * C + 2 * C + c] = s_v[c];
            fin = fin && __builtin_isfinite(s_w[c]) && __builtin_isfinite(s_m[c]) && __builtin_isfinite(s_v[c]);
        }
        if (n > 0 && !fin) st |= GMMIV_ENERGY_NONFINITE;
        threshold[f] = th;
        status[f] = st;
    }
}

template <typename XT, int C>
static hipError_t en_launch(hipStream_t st, size_t lds, const void *x, long ldx, const long *runs, long nrun, long nfiles, const long *order, int nb_it,
                            double flooring, double ceiling, double alpha, long frames, double *model, double *threshold, int *status)
{
    hipError_t e;
    if (lds > (48 << 10) && (e = gmmiv_lds_attr<k_energy_em<XT, C>>(lds)) != hipSuccess) return e;
    k_energy_em<XT, C><<<(unsigned)nfiles, EN_THREADS, lds, st>>>((const XT *)x, ldx, runs, nrun, nfiles, order, nb_it, flooring, ceiling, alpha, frames, model,
                                                                 threshold, status);
    return hipGetLastError();
}

template <typename XT>
static hipError_t en_launch_c(int C, hipStream_t st, size_t lds, const void *x, long ldx, const long *runs, long nrun, long nfiles, const long *order, int nb_it,
                              double flooring, double ceiling, double alpha, long frames, double *model, double *threshold, int *status)
{
#define EN_CASE(K) case K: return en_launch<XT, K>(st, lds, x, ldx, runs, nrun, nfiles, order, nb_it, flooring, ceiling, alpha, frames, model, threshold, status);
    switch (C) {
        EN_CASE(1) EN_CASE(2) EN_CASE(3) EN_CASE(4) EN_CASE(5) EN_CASE(6) EN_CASE(7) EN_CASE(8)
    default: return hipErrorInvalidValue;
    }
#undef EN_CASE
}

int gmmk_energy_em(hipStream_t st, int x_f64, const void *x, long ldx, const long *runs, long nrun, long nfiles, const long *order, long max_frames,
                   int C, int nb_it, double flooring, double ceiling, double alpha, double *model, double *threshold, int *status)
{
    if (nfiles <= 0) return 0;
    // dynamic LDS: the longest selection when the host knows it (max_frames >= 0), else the whole staging budget; a file is staged
    // when it fits the budget -- and, the launch sized like this, then fits the launch
    const long cap = gmmk_energy_stage_frames(x_f64), es = x_f64 ? 8 : 4;
    const long frames = max_frames < 0 || max_frames > cap ? cap : max_frames;
    const size_t lds = (size_t)((frames * es + 15) / 16 * 16);
    return (int)(x_f64 ? en_launch_c<double>(C, st, lds, x, ldx, runs, nrun, nfiles, order, nb_it, flooring, ceiling, alpha, frames, model, threshold, status)
                       : en_launch_c<float>(C, st, lds, x, ldx, runs, nrun, nfiles, order, nb_it, flooring, ceiling, alpha, frames, model, threshold, status));
}

// ---- k_energy_select: selectFrames (EnergyDetector.cpp:128-166) as written, one workgroup per file ----------------------------------
// Frame i of the selection is IN when x > threshold (strict: NaN is out, +Inf is in; a NaN threshold selects nothing).  A run STARTS at
// i when i is in and (i is the first frame of its input segment or i - 1 is out), and ENDS at i when i is in and (i is the last frame of
// its input segment or i + 1 is out): the k-th start and the k-th end belong to the k-th output segment, so both are numbered by the
// same block scan and written independently.  length = frames of the run, + 1 when the run reaches its input segment's end (:151).
// seg_begin == NULL: counts only.  seg_off[f] = where file f's segments start in seg_begin / seg_len.
template <typename XT>
__global__ __launch_bounds__(SEL_THREADS) void k_energy_select(const XT *__restrict__ x, long ldx, const long *__restrict__ runs, long nrun, long nfiles,
                                                              const double *__restrict__ threshold, long *__restrict__ n_above,
                                                              long *__restrict__ seg_count, const long *__restrict__ seg_off,
                                                              long *__restrict__ seg_begin, long *__restrict__ seg_len)
{
    __shared__ int wtot[SEL_WAVES][3];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long f = blockIdx.x;
    long r0, r1;
    en_file_runs(runs, nrun, f, r0, r1);
    const double th = threshold[f];
    const long base = seg_begin ? seg_off[f] : 0, cap = seg_begin ? seg_off[f + 1] - base : 0;
    long off = 0, nseg = 0, nend = 0, above = 0; // block-uniform running totals
    for (long r = r0; r < r1; ++r) {
        const long first = runs[3 * r], len = runs[3 * r + 1];
        if (len <= 0) continue;
        const XT *p = x + first * ldx;
        for (long t0 = 0; t0 < len; t0 += SEL_THREADS) {
            const long t = t0 + tid;
            bool in = false, start = false, end = false;
            if (t < len) {
                in = (double)p[t * ldx] > th;
                if (in) {
                    start = t == 0 || !((double)p[(t - 1) * ldx] > th);
                    end = t == len - 1 || !((double)p[(t + 1) * ldx] > th);
                }
            }
            const unsigned long long bi = __ballot(in), bs = __ballot(start), be = __ballot(end);
            if (lane == 0) { wtot[wave][0] = __popcll(bi); wtot[wave][1] = __popcll(bs); wtot[wave][2] = __popcll(be); }
            __syncthreads();
            const unsigned long long below = lane ? (~0ULL >> (64 - lane)) : 0ULL;
            long ps = __popcll(bs & below), pe = __popcll(be & below), ti = 0, ts = 0, te = 0;
#pragma unroll
            for (int w = 0; w < SEL_WAVES; ++w) {
                if (w < wave) { ps += wtot[w][1]; pe += wtot[w][2]; }
                ti += wtot[w][0]; ts += wtot[w][1]; te += wtot[w][2];
            }
            if (seg_begin) {
                if (start && nseg + ps < cap) seg_begin[base + nseg + ps] = off + t;
                // the END MARK: one past the run's last frame, one more when that frame is its input segment's last; turned into a length below
                if (end && nend + pe < cap) seg_len[base + nend + pe] = off + t + 1 + (t == len - 1 ? 1 : 0);
            }
            nseg += ts; nend += te; above += ti;
            __syncthreads();
        }
        off += len;
    }
    if (seg_begin) {
        __syncthreads(); // every mark and begin of this file is written by this workgroup
        const long m = nseg < cap ? nseg : cap;
        for (long k = tid; k < m; k += SEL_THREADS) seg_len[base + k] -= seg_begin[base + k];
    }
    if (tid == 0) {
        if (n_above) n_above[f] = above;
        if (seg_count) seg_count[f] = nseg;
    }
}

int gmmk_energy_select(hipStream_t st, int x_f64, const void *x, long ldx, const long *runs, long nrun, long nfiles, const double *threshold,
                       long *n_above, long *seg_count, const long *seg_off, long *seg_begin, long *seg_len)
{
    if (nfiles <= 0) return 0;
    if (x_f64) k_energy_select<double><<<(unsigned)nfiles, SEL_THREADS, 0, st>>>((const double *)x, ldx, runs, nrun, nfiles, threshold, n_above, seg_count, seg_off, seg_begin, seg_len);
    else k_energy_select<float><<<(unsigned)nfiles, SEL_THREADS, 0, st>>>((const float *)x, ldx, runs, nrun, nfiles, threshold, n_above, seg_count, seg_off, seg_begin, seg_len);
    return (int)hipGetLastError();
}
