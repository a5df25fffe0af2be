// feat_norm.hip -- NormFeat's default mode and NormFeatWindowMode on the resident frames (include/gmmiv.h, "cepstral mean / variance
// normalisation"): k_moments_groups (FrameAccGD over a Seg or a cluster, many groups per launch), k_moments_stats (getMeanVect /
// getStdVect), k_feat_norm_apply (computeZeroOne) and the three kernels of the online mode (updateMeanAndCovParam + computeCMVnorm as a
// chunked scan).  All of them are HBM streams: one read of x for the moments, one read and one write for the apply.  No kernel here
// adds into memory another workgroup adds into: every sum has one owner and one fixed order, so every result is bitwise reproducible.
#include "devutil.h"
#include "gmm_kernels.h"

template <typename T, int V> struct fn_vec { typedef T type __attribute__((ext_vector_type(V))); };
template <typename T> struct fn_vec<T, 1> { struct type { T v; __device__ __forceinline__ T operator[](int) const { return v; } __device__ __forceinline__ T &operator[](int) { return v; } }; };

// ---- k_moments_groups ------------------------------------------------------------------------------------------------------
// One workgroup per run (first frame, length, group).  The sum of a column over the run is DEFINED as
//     sum_{j = 0 .. 15, ascending} ( x[j] + x[j + 16] + x[j + 32] + ...  added left to right ),
// i.e. FN_ROWS = 16 row lanes that each add their rows in order, then the 16 lane sums added in order: a function of the run's length
// and values alone.  How the columns are spread over the threads (VW values per 4-, 8- or 16-byte load, blockDim.x / 16 vector columns
// per pass) follows the alignment of the call and changes no bit.  Products and sums are rounded separately (the reference's
// accumulate() is a plain loop).  The run's 2 D partial sums go to partial[run]; k_moments_combine adds them per group in table order.
constexpr int FN_ROWS = 16, FN_COLS = 64;

template <typename XT, int VW>
__global__ __launch_bounds__(1024) void k_moments_groups(const XT *__restrict__ x, long ldx, int D, const long *__restrict__ runs,
                                                         double *__restrict__ partial)
{
#pragma clang fp contract(off)
    typedef typename fn_vec<XT, VW>::type vec_t;
    __shared__ double red[FN_ROWS][2 * FN_COLS];
    const int tid = threadIdx.x, nvc = blockDim.x / FN_ROWS; // vector columns per pass (nvc * VW <= FN_COLS)
    const int j = tid / nvc, v = tid - j * nvc;
    const long r = blockIdx.x, first = runs[3 * r], len = runs[3 * r + 1];
    const XT *base = x + first * ldx;
    for (int c0 = 0; c0 < D; c0 += nvc * VW) {
        const int col = c0 + v * VW;
        double s[VW], ss[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) { s[k] = 0.0; ss[k] = 0.0; }
        if (col < D) {
            const XT *p = base + col;
#pragma unroll 4
            for (long t = j; t < len; t += FN_ROWS) {
                const vec_t a = *(const vec_t *)(p + t * ldx);
#pragma unroll
                for (int k = 0; k < VW; ++k) { const double va = (double)a[k]; s[k] += va; ss[k] += va * va; }
            }
        }
#pragma unroll
        for (int k = 0; k < VW; ++k) { red[j][v * VW + k] = s[k]; red[j][FN_COLS + v * VW + k] = ss[k]; }
        __syncthreads();
        for (int e = tid; e < 2 * FN_COLS; e += blockDim.x) {
            const int sq = e >= FN_COLS, c = c0 + (e & (FN_COLS - 1));
            if ((e & (FN_COLS - 1)) < nvc * VW && c < D) {
                double a = red[0][e];
#pragma unroll
                for (int jj = 1; jj < FN_ROWS; ++jj) a += red[jj][e];
                partial[(size_t)r * 2 * D + (size_t)sq * D + c] = a;
            }
        }
        __syncthreads();
    }
}

// acc[g][0 .. 2D) += the partials of the runs of group g, added in table order; acc[g][2D] += their frame count.  The group ids are
// non-decreasing along the table: the runs of a group are found by bisection.  A group without runs keeps its row.
__global__ __launch_bounds__(256) void k_moments_combine(const long *__restrict__ runs, long nrun, long ngroups, int D,
                                                         const double *__restrict__ partial, double *__restrict__ acc)
{
    const long W = 2L * D + 1, tot = ngroups * W;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long)gridDim.x * 256) {
        const long g = e / W;
        const int c = (int)(e - g * W);
        long lo = 0, hi = nrun;
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (runs[3 * mid + 2] < g) lo = mid + 1; else hi = mid;
        }
        if (lo >= nrun || runs[3 * lo + 2] != g) continue;
        double t = c < 2 * D ? partial[(size_t)lo * 2 * D + c] : (double)runs[3 * lo + 1];
        for (long r = lo + 1; r < nrun && runs[3 * r + 2] == g; ++r) t += c < 2 * D ? partial[(size_t)r * 2 * D + c] : (double)runs[3 * r + 1];
        acc[e] += t;
    }
}

int gmmk_moments_groups(hipStream_t st, int x_f64, const void *x, long ldx, int D, const long *runs, long nrun, long ngroups, double *partial,
                        double *acc)
{
    if (nrun <= 0 || ngroups <= 0) return 0;
    const size_t es = x_f64 ? 8 : 4;
    int vw = 1;
    for (int w = (int)(16 / es); w > 1; w >>= 1)
        if (D % w == 0 && ldx % w == 0 && ((size_t)x % (w * es)) == 0) { vw = w; break; }
    int nvc = ((D + vw - 1) / vw + 3) / 4 * 4; // a multiple of 4 vector columns: 64 k threads
    if (nvc > FN_COLS / vw) nvc = FN_COLS / vw;
    const unsigned bs = (unsigned)(FN_ROWS * nvc), grid = (unsigned)nrun;
    if (x_f64) {
        if (vw == 2) k_moments_groups<double, 2><<<grid, bs, 0, st>>>((const double *)x, ldx, D, runs, partial);
        else k_moments_groups<double, 1><<<grid, bs, 0, st>>>((const double *)x, ldx, D, runs, partial);
    } else {
        if (vw == 4) k_moments_groups<float, 4><<<grid, bs, 0, st>>>((const float *)x, ldx, D, runs, partial);
        else if (vw == 2) k_moments_groups<float, 2><<<grid, bs, 0, st>>>((const float *)x, ldx, D, runs, partial);
        else k_moments_groups<float, 1><<<grid, bs, 0, st>>>((const float *)x, ldx, D, runs, partial);
    }
    const long nb = (ngroups * (2L * D + 1) + 255) / 256;
    k_moments_combine<<<(unsigned)(nb < 65536 ? nb : 65536), 256, 0, st>>>(runs, nrun, ngroups, D, partial, acc);
    return (int)hipGetLastError();
}

// ---- k_moments_stats: FrameAccGD::getMeanVect / getStdVect (biased, the form KAT-4 pins): two divisions, a product, a difference and a
// square root, each rounded on its own.  A group without frames gives 0 / 0 = NaN in both.
__global__ __launch_bounds__(256) void k_moments_stats(long ngroups, int D, const double *__restrict__ acc, double *__restrict__ mean,
                                                       double *__restrict__ sd)
{
#pragma clang fp contract(off)
    const long W = 2L * D + 1, tot = ngroups * D;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long)gridDim.x * 256) {
        const long g = e / D;
        const int i = (int)(e - g * D);
        const double n = acc[g * W + 2 * D];
        const double m = acc[g * W + i] / n;
        const double q = acc[g * W + D + i] / n;
        const double mm = m * m;
        mean[e] = m;
        sd[e] = __builtin_sqrt(q - mm);
    }
}

int gmmk_moments_stats(hipStream_t st, long ngroups, int D, const double *acc, double *mean, double *sd)
{
    if (ngroups <= 0) return 0;
    const long nb = (ngroups * D + 255) / 256;
    k_moments_stats<<<(unsigned)(nb < 65536 ? nb : 65536), 256, 0, st>>>(ngroups, D, acc, mean, sd);
    return (int)hipGetLastError();
}

// ---- k_feat_norm_apply: computeZeroOne (GeneralTools.cpp:670-682) on the frames of the runs -------------------------------------
// out = (x - mean[g]) / std[g]: one subtraction and one correctly rounded division in fp64, rounded once more for an f32 output.
// mean == NULL subtracts 0.0 and std == NULL divides by 1.0 -- what the reference does for varOnly / cmsOnly, and exact.  One
// workgroup per run; a thread keeps VW columns (their mean and std in registers) and walks the rows, so every wave-load is a row
// segment of 4-, 8- or 16-byte pieces.  A thread writes exactly the elements it read: out may be x.
template <typename XT, typename OT, int VW>
__global__ __launch_bounds__(256) void k_feat_norm_apply(const XT *x, long ldx, int D, const long *__restrict__ runs, long ngroups,
                                                         const double *__restrict__ mean, const double *__restrict__ sd, OT *out, long ldo)
{
#pragma clang fp contract(off)
    typedef typename fn_vec<XT, VW>::type xvec_t;
    typedef typename fn_vec<OT, VW>::type ovec_t;
    const long r = blockIdx.x, first = runs[3 * r], len = runs[3 * r + 1], g = runs[3 * r + 2];
    if ((unsigned long)g >= (unsigned long)ngroups) return;
    const int tid = threadIdx.x, nvc = D / VW;
    for (int v0 = 0; v0 < nvc; v0 += 256) {
        const int nv = nvc - v0 < 256 ? nvc - v0 : 256, rl = 256 / nv;
        const int j = tid / nv, col = (v0 + tid - j * nv) * VW;
        if (j >= rl) continue;
        double m[VW], s[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) { m[k] = mean ? mean[g * D + col + k] : 0.0; s[k] = sd ? sd[g * D + col + k] : 1.0; }
        const XT *p = x + first * ldx + col;
        OT *q = out + first * ldo + col;
        // four rows are read before the first is written (x and out may be one array: the compiler would not move a load over a store)
        long t = j;
        for (; t + 3L * rl < len; t += 4L * rl) {
            xvec_t a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = *(const xvec_t *)(p + (t + (long)u * rl) * ldx);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ovec_t o;
#pragma unroll
                for (int k = 0; k < VW; ++k) { const double d = (double)a[u][k] - m[k]; o[k] = (OT)(d / s[k]); }
                *(ovec_t *)(q + (t + (long)u * rl) * ldo) = o;
            }
        }
        for (; t < len; t += rl) {
            const xvec_t a = *(const xvec_t *)(p + t * ldx);
            ovec_t o;
#pragma unroll
            for (int k = 0; k < VW; ++k) { const double d = (double)a[k] - m[k]; o[k] = (OT)(d / s[k]); }
            *(ovec_t *)(q + t * ldo) = o;
        }
    }
}

template <typename XT, typename OT>
static void launch_norm_apply(hipStream_t st, int vw, const void *x, long ldx, int D, const long *runs, long nrun, long ngroups, const double *mean,
                              const double *sd, void *out, long ldo)
{
    const unsigned grid = (unsigned)nrun;
    if (vw == 4) k_feat_norm_apply<XT, OT, 4><<<grid, 256, 0, st>>>((const XT *)x, ldx, D, runs, ngroups, mean, sd, (OT *)out, ldo);
    else if (vw == 2) k_feat_norm_apply<XT, OT, 2><<<grid, 256, 0, st>>>((const XT *)x, ldx, D, runs, ngroups, mean, sd, (OT *)out, ldo);
    else k_feat_norm_apply<XT, OT, 1><<<grid, 256, 0, st>>>((const XT *)x, ldx, D, runs, ngroups, mean, sd, (OT *)out, ldo);
}

int gmmk_feat_norm_apply(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, int D, const long *runs, long nrun, long ngroups,
                         const double *mean, const double *sd, void *out, long ldo)
{
    if (nrun <= 0) return 0;
    const size_t xs = x_f64 ? 8 : 4, os = o_f64 ? 8 : 4;
    int vw = 1;
    for (int w = 4; w > 1; w >>= 1) // both vectors naturally aligned: the pointers and, through the strides, every row
        if (D % w == 0 && ldx % w == 0 && ldo % w == 0 && ((size_t)x % (w * xs)) == 0 && ((size_t)out % (w * os)) == 0) { vw = w; break; }
    if (x_f64 && o_f64) launch_norm_apply<double, double>(st, vw, x, ldx, D, runs, nrun, ngroups, mean, sd, out, ldo);
    else if (x_f64) launch_norm_apply<double, float>(st, vw, x, ldx, D, runs, nrun, ngroups, mean, sd, out, ldo);
    else if (o_f64) launch_norm_apply<float, double>(st, vw, x, ldx, D, runs, nrun, ngroups, mean, sd, out, ldo);
    else launch_norm_apply<float, float>(st, vw, x, ldx, D, runs, nrun, ngroups, mean, sd, out, ldo);
    return (int)hipGetLastError();
}

// ---- online mode: normFeatOnlineMode (NormFeatWindowMode.cpp:165-311) -----------------------------------------------------------
// Per file and dimension the tool runs, for frame k = 1 .. n,
//     m <- B m + (1 - B) x,   c <- sqrt(c c B + (1 - B) (x x)),   out = (x - m) / c,        B = 1 for k < L, else (W - 1) / W
// from the mean / biased std of (W - L zero vectors, the first L frames).  Both recurrences are LINEAR in (m, v = c c): a file is cut
// into chunks of FN_CHUNK frames counted from ITS first frame, and
//   k_online_sums    runs every chunk but a file's last from the zero state: S = (m, v) after the chunk, P = the product of its B;
//   k_online_carry   one thread per (file, dimension): the initial state, then state_in[chunk + 1] = P state_in[chunk] + S, in order;
//   k_online_replay  runs every chunk again from its carried-in state and writes the frames.
// A file of at most FN_CHUNK frames is read once and written once.  One lane owns a (chunk, dimension) chain; the lanes of a wave are
// adjacent dimensions, so a wave-load is a row segment.  The state kept between frames is v, not c: c = sqrt(v) is taken for the
// division only (the tool squares its rounded c again every frame -- one rounding per frame more, inside the tolerance of the test).
// Nothing depends on a neighbouring file: chunk boundaries, W' and the initial state are functions of the file alone.
constexpr long FN_CHUNK = 1024;

// chunk_off[f] = number of chunks of the files before f; chunk_off[nfiles] = all chunks.  One workgroup.
__global__ __launch_bounds__(1024) void k_online_prep(const long *__restrict__ file_begin, long nfiles, long *__restrict__ chunk_off)
{
    __shared__ long part[1024];
    const int tid = threadIdx.x;
    const long per = (nfiles + 1023) / 1024, lo = tid * per < nfiles ? tid * per : nfiles, hi = lo + per < nfiles ? lo + per : nfiles;
    long s = 0;
    for (long f = lo; f < hi; ++f) { const long n = file_begin[f + 1] - file_begin[f]; s += n > 0 ? (n + FN_CHUNK - 1) / FN_CHUNK : 0; }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long run = 0;
        for (int i = 0; i < 1024; ++i) { const long t = part[i]; part[i] = run; run += t; }
        chunk_off[nfiles] = run;
    }
    __syncthreads();
    long run = part[tid];
    for (long f = lo; f < hi; ++f) { const long n = file_begin[f + 1] - file_begin[f]; chunk_off[f] = run; run += n > 0 ? (n + FN_CHUNK - 1) / FN_CHUNK : 0; }
}

// the file that owns chunk u: the last f with chunk_off[f] <= u (files without frames own no chunk and are stepped over)
static __device__ __forceinline__ long online_file_of(const long *__restrict__ chunk_off, long nfiles, long u)
{
    long lo = 0, hi = nfiles; // invariant: chunk_off[lo] <= u < chunk_off[hi]
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (chunk_off[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename XT>
__global__ __launch_bounds__(256) void k_online_sums(const XT *__restrict__ x, long ldx, int D, const long *__restrict__ file_begin,
                                                     const long *__restrict__ chunk_off, long nfiles, long max_units, long W, long L,
                                                     double *__restrict__ state, double *__restrict__ decay)
{
#pragma clang fp contract(off)
    long U = chunk_off[nfiles];
    if (U > max_units) U = max_units;
    const long tot = U * D;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long)gridDim.x * 256) {
        const long u = e / D;
        const int d = (int)(e - u * D);
        const long f = online_file_of(chunk_off, nfiles, u), k = u - chunk_off[f];
        if (k + 1 >= chunk_off[f + 1] - chunk_off[f]) continue; // a file's last chunk carries nothing forward
        const long n = file_begin[f + 1] - file_begin[f], Wp = n < L ? W - L + n : W;
        const double bw = ((double)Wp - 1) / (double)Wp, ow = 1 - bw;
        const XT *p = x + (file_begin[f] + k * FN_CHUNK) * ldx + d;
        const long k0 = k * FN_CHUNK + 1; // frame count of the chunk's first frame
        double m = 0.0, v = 0.0, P = 1.0;
#pragma unroll 4
        for (long i = 0; i < FN_CHUNK; ++i) {
            const double xv = (double)p[i * ldx];
            const bool seen = k0 + i < L;
            const double b = seen ? 1.0 : bw, o = seen ? 0.0 : ow;
            const double t0 = b * m, t1 = o * xv, t2 = v * b, t3 = o * (xv * xv);
            m = t0 + t1;
            v = t2 + t3;
            P *= b;
        }
        state[2 * e] = m;
        state[2 * e + 1] = v;
        if (d == 0) decay[u] = P;
    }
}

template <typename XT>
__global__ __launch_bounds__(256) void k_online_carry(const XT *__restrict__ x, long ldx, int D, const long *__restrict__ file_begin,
                                                      const long *__restrict__ chunk_off, long nfiles, long max_units, long W, long L,
                                                      double *__restrict__ state, const double *__restrict__ decay)
{
#pragma clang fp contract(off)
    const long tot = nfiles * D;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long)gridDim.x * 256) {
        const long f = e / D;
        const int d = (int)(e - f * D);
        const long b = file_begin[f], n = file_begin[f + 1] - b;
        if (n <= 0) continue;
        // loadMeanAndCovParam over (W - L zeros, the first L frames); a file shorter than L: W' = W - L + n, the whole file
        const long nl = n < L ? n : L, Wp = n < L ? W - L + n : W;
        const XT *p = x + b * ldx + d;
        double s = 0.0, ss = 0.0;
        for (long i = 0; i < nl; ++i) { const double xv = (double)p[i * ldx]; s += xv; ss += xv * xv; }
        double m = s / (double)Wp;
        const double q = ss / (double)Wp, mm = m * m, c0 = __builtin_sqrt(q - mm);
        double v = c0 * c0;
        const long u0 = chunk_off[f];
        long nch = chunk_off[f + 1] - u0;
        if (u0 + nch > max_units) nch = max_units - u0;
        for (long k = 0; k < nch; ++k) {
            const size_t a = (size_t)((u0 + k) * D + d) * 2;
            const double sm = state[a], sv = state[a + 1]; // the chunk's own sums (unused for the last chunk) make room for its state
            state[a] = m;
            state[a + 1] = v;
            if (k + 1 < nch) {
                const double P = decay[u0 + k];
                const double t0 = P * m, t1 = P * v;
                m = t0 + sm;
                v = t1 + sv;
            }
        }
    }
}

template <typename XT, typename OT>
__global__ __launch_bounds__(256) void k_online_replay(const XT *x, long ldx, int D, const long *__restrict__ file_begin,
                                                       const long *__restrict__ chunk_off, long nfiles, long max_units, long W, long L,
                                                       const double *__restrict__ state, OT *out, long ldo)
{
#pragma clang fp contract(off)
    long U = chunk_off[nfiles];
    if (U > max_units) U = max_units;
    const long tot = U * D;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long)gridDim.x * 256) {
        const long u = e / D;
        const int d = (int)(e - u * D);
        const long f = online_file_of(chunk_off, nfiles, u), k = u - chunk_off[f];
        const long fb = file_begin[f], n = file_begin[f + 1] - fb;
        const long Wp = n < L ? W - L + n : W;
        const double bw = ((double)Wp - 1) / (double)Wp, ow = 1 - bw;
        const long k0 = k * FN_CHUNK + 1, len = n - k * FN_CHUNK < FN_CHUNK ? n - k * FN_CHUNK : FN_CHUNK;
        const XT *p = x + (fb + k * FN_CHUNK) * ldx + d;
        OT *q = out + (fb + k * FN_CHUNK) * ldo + d;
        double m = state[2 * e], v = state[2 * e + 1];
        // four frames are read before the first is written (x and out may be one array)
        for (long i0 = 0; i0 < len; i0 += 4) {
            double xs[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) xs[u] = i0 + u < len ? (double)p[(i0 + u) * ldx] : 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i0 + u >= len) break;
                const double xv = xs[u];
                const bool seen = k0 + i0 + u < L;
                const double b = seen ? 1.0 : bw, o = seen ? 0.0 : ow;
                const double t0 = b * m, t1 = o * xv, t2 = v * b, t3 = o * (xv * xv);
                m = t0 + t1;
                v = t2 + t3;
                const double df = xv - m;
                q[(i0 + u) * ldo] = (OT)(df / __builtin_sqrt(v));
            }
        }
    }
}

size_t gmmk_online_units(long nfiles, long frames) { return (size_t)(nfiles + frames / FN_CHUNK + 1); }
long gmmk_online_chunk(void) { return FN_CHUNK; }

int gmmk_feat_norm_online(hipStream_t st, int n_cu, int x_f64, int o_f64, const void *x, long ldx, int D, const long *file_begin, long nfiles,
                          long W, long L, long max_units, long *chunk_off, double *state, double *decay, void *out, long ldo)
{
    if (nfiles <= 0) return 0;
    k_online_prep<<<1, 1024, 0, st>>>(file_begin, nfiles, chunk_off);
    long nb = (max_units * D + 255) / 256;
    const long cap = (long)(n_cu > 0 ? n_cu : 256) * 8;
    if (nb > cap) nb = cap;
    const unsigned grid = (unsigned)(nb < 1 ? 1 : nb);
    long nbc = (nfiles * D + 255) / 256;
    const unsigned gridc = (unsigned)(nbc < 65536 ? nbc : 65536);
    if (x_f64) {
        k_online_sums<double><<<grid, 256, 0, st>>>((const double *)x, ldx, D, file_begin, chunk_off, nfiles, max_units, W, L, state, decay);
        k_online_carry<double><<<gridc, 256, 0, st>>>((const double *)x, ldx, D, file_begin, chunk_off, nfiles, max_units, W, L, state, decay);
        if (o_f64) k_online_replay<double, double><<<grid, 256, 0, st>>>((const double *)x, ldx, D, file_begin, chunk_off, nfiles, max_units, W, L, state, (double *)out, ldo);
        else k_online_replay<double, float><<<grid, 256, 0, st>>>((const double *)x, ldx, D, file_begin, chunk_off, nfiles, max_units, W, L, state, (float *)out, ldo);
    } else {
        k_online_sums<float><<<grid, 256, 0, st>>>((const float *)x, ldx, D, file_begin, chunk_off, nfiles, max_units, W, L, state, decay);
        k_online_carry<float><<<gridc, 256, 0, st>>>((const float *)x, ldx, D, file_begin, chunk_off, nfiles, max_units, W, L, state, decay);
        if (o_f64) k_online_replay<float, double><<<grid, 256, 0, st>>>((const float *)x, ldx, D, file_begin, chunk_off, nfiles, max_units, W, L, state, (double *)out, ldo);
        else k_online_replay<float, float><<<grid, 256, 0, st>>>((const float *)x, ldx, D, file_begin, chunk_off, nfiles, max_units, W, L, state, (float *)out, ldo);
    }
    return (int)hipGetLastError();
}
