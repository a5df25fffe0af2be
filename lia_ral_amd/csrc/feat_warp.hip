// feat_warp.hip -- NormFeat's `warp true` on the resident frames (include/ext/gmmiv_feat_warp.h): per (unit, column) the equal-
// population histogram of the unit's values, then warping() (ScoreWarp.cpp:168-206) of every value through it onto a target table.
//
// k_warp_hist    one workgroup per (unit, column).  The values become unsigned keys whose integer order is the order of the sort
//                (sign-magnitude bits flipped: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN), f32 keys stay 32 bits.  A unit that
//                fits the LDS is sorted there (bitonic, padded to a power of two with the largest key); a longer one takes each of
//                the nbBin + 1 ranks through a most-significant-digit-first radix select on the buffer itself (8-bit digits, one
//                256-bin LDS histogram, integer LDS atomics only -- counts, so the order of the adds is immaterial).  Both give the
//                key at a rank of the sorted column, so the bounds do not depend on the path.  count and status follow from the
//                bounds alone.  Nothing is added into memory another workgroup touches.
// k_warp_target  the target's areas and their left fold, once per call (one thread folds: the reference's loop order).
// k_warp_apply   workgroup (unit, block of columns, slice of rows): the unit's bounds, areas and the left fold of the areas in LDS
//                (one thread per column folds), then per value two binary searches and the arithmetic of warping() with contraction off.
#include "devutil.h"
#include "feat_warp.h"
#include "lds_attr.h"

namespace {

template <typename XT> struct WarpKey;
template <> struct WarpKey<float> {
    typedef unsigned int K;
    static constexpr int BITS = 32;
    static __device__ __forceinline__ K to(float v) { const K u = __float_as_uint(v); return (u >> 31) ? ~u : (u | 0x80000000u); }
    static __device__ __forceinline__ double from(K k) { const K u = (k >> 31) ? (k & 0x7fffffffu) : ~k; return (double)__uint_as_float(u); }
};
template <> struct WarpKey<double> {
    typedef unsigned long long K;
    static constexpr int BITS = 64;
    static __device__ __forceinline__ K to(double v) { const K u = (K)__double_as_longlong(v); return (u >> 63) ? ~u : (u | 0x8000000000000000ull); }
    static __device__ __forceinline__ double from(K k) { const K u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k; return __longlong_as_double((long long)u); }
};

// the first run of unit u (the unit ids are non-decreasing along the table)
__device__ __forceinline__ long warp_lower(const long *runs, long nrun, long u)
{
    long lo = 0, hi = nrun;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (runs[3 * mid + 2] < u) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ long warp_len(const long *runs, long r) { const long l = runs[3 * r + 1]; return l > 0 ? l : 0; }

// dynamic LDS: sB [nb + 1] doubles (the bounds), then `cap` keys
template <typename XT>
__global__ __launch_bounds__(1024) void k_warp_hist(const XT *__restrict__ x, long ldx, int D, const long *__restrict__ runs, long nrun, int nb, long cap,
                                                    double *__restrict__ bounds, double *__restrict__ count, int *__restrict__ status)
{
#pragma clang fp contract(off)
    typedef typename WarpKey<XT>::K K;
    extern __shared__ __align__(16) unsigned char warp_smem[];
    __shared__ unsigned long long hist[256];
    __shared__ int s_deg;
    double *sB = (double *)warp_smem;
    K *keys = (K *)(sB + (((long)nb + 2) & ~1L));
    const int tid = threadIdx.x, nthr = blockDim.x;
    const long u = blockIdx.x / D;
    const int col = (int)(blockIdx.x - u * D);
    const long rlo = warp_lower(runs, nrun, u), rhi = warp_lower(runs, nrun, u + 1);
    long n = 0;
    for (long r = rlo; r < rhi; ++r) n += warp_len(runs, r);
    double *B = bounds + (size_t)blockIdx.x * ((size_t)nb + 1), *C = count + (size_t)blockIdx.x * (size_t)nb;
    if (n == 0) { // a unit without frames: zeros, DEGENERATE
        for (int i = tid; i <= nb; i += nthr) { B[i] = 0.0; if (i < nb) C[i] = 0.0; }
        if (tid == 0) status[blockIdx.x] = 1;
        return;
    }
    const long k = n / nb;
    const XT *xc = x + col;
    if (tid == 0) s_deg = 0;
    if (n <= cap) {
        long P = 2;
        while (P < n) P <<= 1;
        long off = 0;
        for (long r = rlo; r < rhi; ++r) {
            const long first = runs[3 * r], len = warp_len(runs, r);
            for (long t = tid; t < len; t += nthr) keys[off + t] = WarpKey<XT>::to(xc[(first + t) * ldx]);
            off += len;
        }
        for (long i = n + tid; i < P; i += nthr) keys[i] = ~(K)0;
        __syncthreads();
        for (long k2 = 2; k2 <= P; k2 <<= 1)
            for (long j = k2 >> 1; j > 0; j >>= 1) {
                for (long i = tid; i < (P >> 1); i += nthr) {
                    const long lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                    const K a = keys[lo], b = keys[hi];
                    if ((a > b) == ((lo & k2) == 0)) { keys[lo] = b; keys[hi] = a; }
                }
                __syncthreads();
            }
        for (int i = tid; i <= nb; i += nthr) sB[i] = WarpKey<XT>::from(keys[i < nb ? (long)i * k : n - 1]);
    } else {
        for (int i = 0; i <= nb; ++i) {
            long rem = i < nb ? (long)i * k : n - 1; // the rank, then the rank inside the keys that share `prefix`
            K prefix = 0;
            for (int shift = WarpKey<XT>::BITS - 8; shift >= 0; shift -= 8) {
                for (int h = tid; h < 256; h += nthr) hist[h] = 0;
                __syncthreads();
                for (long r = rlo; r < rhi; ++r) {
                    const long first = runs[3 * r], len = warp_len(runs, r);
                    for (long t = tid; t < len; t += nthr) {
                        const K key = WarpKey<XT>::to(xc[(first + t) * ldx]);
                        // the digits above `shift` (none on the first pass: a shift by the full width is not defined)
                        const bool in = shift == WarpKey<XT>::BITS - 8 || (key >> (shift + 8)) == prefix;
                        if (in) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1ull);
                    }
                }
                __syncthreads();
                int dg = 0; // every thread walks the 256 counts: the same digit in every thread
                unsigned long long before = 0;
                for (; dg < 255; ++dg) {
                    const unsigned long long h = hist[dg];
                    if (before + h > (unsigned long long)rem) break;
                    before += h;
                }
                rem -= (long)before;
                prefix = (prefix << 8) | (K)dg;
                __syncthreads();
            }
            if (tid == 0) sB[i] = WarpKey<XT>::from(prefix);
        }
    }
    __syncthreads();
    for (int i = tid; i <= nb; i += nthr) {
        const double b0 = sB[i];
        B[i] = b0;
        if (i < nb) {
            const double w = sB[i + 1] - b0;
            const long m = i < nb - 1 ? k : n - (long)(nb - 1) * k;
            const double p = (double)m / (double)n;
            C[i] = p / w;
            if (!(w > 0 && w < __builtin_inf())) s_deg = 1; // no width, a NaN bound, an infinite bound
        }
    }
    __syncthreads();
    if (tid == 0) status[blockIdx.x] = s_deg;
}

__global__ __launch_bounds__(256) void k_warp_target(int nt, const double *__restrict__ tb, const double *__restrict__ tc, double *__restrict__ ta, double *__restrict__ tT)
{
#pragma clang fp contract(off)
    for (int i = threadIdx.x; i < nt; i += blockDim.x) { const double w = tb[i + 1] - tb[i]; ta[i] = tc[i] * w; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        tT[0] = t;
        for (int i = 0; i < nt; ++i) { t += ta[i]; tT[i + 1] = t; }
    }
}

// linearInterpolation (AccumulateStat.cpp:432-437)
__device__ __forceinline__ double warp_lin(double val, double lower, double higher)
{
#pragma clang fp contract(off)
    const double interval = higher - lower;
    if (interval < 0.000000000000000000001) return 1.0;
    const double d = val - lower;
    return d / interval;
}

constexpr int WARP_APPLY_COLS = 64, WARP_APPLY_LDS = 64 * 1024;

// dynamic LDS: sb [cb x (nb + 1)] | sa [cb x nb] | sP [cb x (nb + 1)] | st [cb]
template <typename XT, typename OT>
__global__ __launch_bounds__(256) void k_warp_apply(const XT *x, long ldx, OT *out, long ldo, int D, const long *__restrict__ runs, long nrun, int nb, int cb,
                                                    const double *__restrict__ bounds, const double *__restrict__ count, const int *__restrict__ status, int nt,
                                                    const double *__restrict__ tb, const double *__restrict__ ta, const double *__restrict__ tT)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char warp_smem[];
    double *sb = (double *)warp_smem, *sa = sb + (size_t)cb * (nb + 1), *sP = sa + (size_t)cb * nb;
    int *st = (int *)(sP + (size_t)cb * (nb + 1));
    const int tid = threadIdx.x, nthr = blockDim.x;
    const long u = blockIdx.x;
    const int c0 = blockIdx.y * cb, nc = D - c0 < cb ? D - c0 : cb;
    const size_t h0 = (size_t)u * D + c0;
    for (int e = tid; e < nc * (nb + 1); e += nthr) sb[e] = bounds[h0 * ((size_t)nb + 1) + e];
    if (tid < nc) st[tid] = status[h0 + tid];
    __syncthreads();
    for (int e = tid; e < nc * nb; e += nthr) {
        const int c = e / nb, i = e - c * nb;
        const double w = sb[c * (nb + 1) + i + 1] - sb[c * (nb + 1) + i];
        sa[e] = count[h0 * (size_t)nb + e] * w; // areaHisto
    }
    __syncthreads();
    if (tid < nc) { // the areas folded left to right from 0.0, as the loop at ScoreWarp.cpp:178-179 does
        double t = 0.0;
        sP[tid * (nb + 1)] = t;
        for (int i = 0; i < nb; ++i) { t += sa[tid * nb + i]; sP[tid * (nb + 1) + i + 1] = t; }
    }
    __syncthreads();
    const long rlo = warp_lower(runs, nrun, u), rhi = warp_lower(runs, nrun, u + 1);
    const long stride = (long)nthr * gridDim.z;
    for (long r = rlo; r < rhi; ++r) {
        const long first = runs[3 * r], len = warp_len(runs, r), tot = len * nc;
        for (long e = (long)blockIdx.z * nthr + tid; e < tot; e += stride) {
            const long row = e / nc;
            const int c = (int)(e - row * nc);
            const XT xv = x[(first + row) * ldx + c0 + c];
            OT *po = out + (first + row) * ldo + c0 + c;
            if (st[c]) { *po = (OT)xv; continue; } // DEGENERATE: copied through
            const double score = (double)xv;
            const double *b = sb + c * (nb + 1), *a = sa + c * nb, *P = sP + c * (nb + 1);
            int lo = 0, hi = nb; // idxW: the first bin whose upper bound is not below the value
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (b[mid + 1] < score) lo = mid + 1; else hi = mid; }
            const int iw = lo < nb ? lo : nb - 1;
            const double pw = warp_lin(score, b[iw], b[iw + 1]);
            const double t0 = a[iw] * pw;
            const double tw = P[iw] + t0;
            lo = 0; hi = nt;         // idxD: the first j with not (T[j] < totalWarp); nt when the loop runs off the table
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (tT[mid] < tw) lo = mid + 1; else hi = mid; }
            int jd = lo;
            double td = tT[jd];
            if (jd == nt) { --jd; td = td - ta[jd]; }
            else if (jd > 0) { td = td - ta[jd]; --jd; } // as written (:195-198): the area of the bin after the last one added
            const double tl = tb[jd], tw_ = tb[jd + 1] - tl;
            const double up = ta[jd] + td;
            const double ph = warp_lin(tw, td, up);
            const double inc = tw_ * ph;
            *po = (OT)(tl + inc);
        }
    }
}

} // namespace

int gmmk_warp_hist(hipStream_t st, int x_f64, const void *x, long ldx, int D, const long *runs, long nrun, long nunits, int nb, long max_len,
                   int force_select, double *bounds, double *count, int *status)
{
    if (nunits <= 0) return 0;
    const long capmax = x_f64 ? WARP_SORT_CAP_F64 : WARP_SORT_CAP_F32;
    long cap = capmax;
    unsigned threads = 1024;
    if (max_len >= 0) { // the host knows the longest unit: no more LDS and threads than it needs
        long P = 64;
        while (P < max_len && P < capmax) P <<= 1;
        cap = P;
        threads = (unsigned)(P / 2 < 64 ? 64 : P / 2 > 1024 ? 1024 : P / 2);
    }
    if (force_select) cap = 0;
    const size_t lds = (size_t)(((long)nb + 2) & ~1L) * sizeof(double) + (size_t)cap * (x_f64 ? 8 : 4);
    const unsigned grid = (unsigned)(nunits * D);
    hipError_t e;
    if (x_f64) {
        if ((e = gmmiv_lds_attr<k_warp_hist<double>>(lds)) != hipSuccess) return (int)e;
        k_warp_hist<double><<<grid, threads, lds, st>>>((const double *)x, ldx, D, runs, nrun, nb, cap, bounds, count, status);
    } else {
        if ((e = gmmiv_lds_attr<k_warp_hist<float>>(lds)) != hipSuccess) return (int)e;
        k_warp_hist<float><<<grid, threads, lds, st>>>((const float *)x, ldx, D, runs, nrun, nb, cap, bounds, count, status);
    }
    return (int)hipGetLastError();
}

int gmmk_warp_target(hipStream_t st, int nt, const double *tb, const double *tc, double *ta, double *tT)
{
    k_warp_target<<<1, 256, 0, st>>>(nt, tb, tc, ta, tT);
    return (int)hipGetLastError();
}

int gmmk_warp_apply_cols(int D, int nb)
{
    const long per = (3L * nb + 2) * 8 + 4;
    long cb = WARP_APPLY_LDS / per;
    if (cb > WARP_APPLY_COLS) cb = WARP_APPLY_COLS;
    if (cb > D) cb = D;
    return (int)cb;
}

int gmmk_warp_apply(hipStream_t st, int x_f64, const void *x, long ldx, int o_f64, void *out, long ldo, int D, const long *runs, long nrun, long nunits,
                    int nb, const double *bounds, const double *count, const int *status, int nt, const double *tb, const double *ta, const double *tT,
                    int n_cu)
{
    if (nunits <= 0) return 0;
    const int cb = gmmk_warp_apply_cols(D, nb);
    if (cb < 1) return (int)hipErrorInvalidValue;
    const int ncb = (D + cb - 1) / cb;
    // slices of rows: enough workgroups for the device when the units are few (a value's result does not depend on the slicing)
    long nz = (4L * n_cu + nunits * ncb - 1) / (nunits * ncb);
    nz = nz < 1 ? 1 : nz > 64 ? 64 : nz;
    const size_t lds = (size_t)cb * ((3 * (size_t)nb + 2) * 8 + 4);
    const dim3 grid((unsigned)nunits, (unsigned)ncb, (unsigned)nz);
#define WARP_APPLY(XT, OT) k_warp_apply<XT, OT><<<grid, 256, lds, st>>>((const XT *)x, ldx, (OT *)out, ldo, D, runs, nrun, nb, cb, bounds, count, status, nt, tb, ta, tT)
    if (x_f64 && o_f64) WARP_APPLY(double, double);
    else if (x_f64) WARP_APPLY(double, float);
    else if (o_f64) WARP_APPLY(float, double);
    else WARP_APPLY(float, float);
#undef WARP_APPLY
    return (int)hipGetLastError();
}
