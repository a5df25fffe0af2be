// turn_detect.hip -- LIA_SpkSeg/TurnDetection on the resident frames (include/gmmiv_turn.h): the criterion curve of every window position
// of every run in one launch (k_turn_curve), the smoothing and the decisions per run (k_turn_pick), the output segments (k_turn_segments).
//
// k_turn_curve.  A workgroup takes a tile of at most P consecutive positions of ONE run.  Its 2 W + (Pt - 1) S frames are staged in LDS
// once, as fp64, rows padded to an odd length (a wave that reads one column of 32 consecutive rows, or one row, touches 32 distinct
// bank pairs).  Then, barriers between the phases, LDS only:
//   1  block sums: thread (block start, column) adds the S frames of its block left to right and keeps (sum, sum of squares) at the
//      lengths that occur -- S, W % S, 2 W % S.  Block starts are j S from the tile's first row, and W + j S when W % S != 0.
//   2  models: thread (position, window, column) adds its window's blocks in order, mean = s / n, cov = ss / n - mean^2 (each operation
//      rounded on its own); then log cov goes where the block sums stood, 1 / cov where cov stood, and one thread per (position,
//      window) adds the D logarithms in column order.
//   3  log-likelihoods: thread (position, window, block) evaluates the frames of its block under the window's model, q = sum_d
//      fma((x - mean)^2, 1 / cov, q) in column order, llk = log cst - 0.5 q, the clamp and the zero-likelihood rule, and adds them left to right.
//   4  thread (position) adds each window's block partials in order and writes the criterion and the status.
// Every sum is a function of the position's own 2 W frames: the tile only decides which workgroup computes it.  No atomics: the two flags
// of a position are plain stores of the same value.
#include "devutil.h"
#include "lds_attr.h"
#include "turn_detect.h"

// ---- tile_off [nrun + 1]: the exclusive prefix of ceil(n_r / P), one workgroup, chunks of 1024 runs
__global__ __launch_bounds__(1024) void k_turn_tiles(const long *runs, long nrun, const long *pos_off, long W, long S, int P, long *tile_off)
{
    __shared__ long sc[1024];
    __shared__ long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (long r0 = 0; r0 < nrun; r0 += 1024) {
        const long r = r0 + tid;
        long nt = 0;
        if (r < nrun) {
            long n = pos_off[r + 1] - pos_off[r];
            const long cap = turn_run_positions(runs[3 * r + 1], W, S); // never more positions than the run holds frames for
            n = n > cap ? cap : n;
            nt = n > 0 ? (n + P - 1) / P : 0;
        }
        sc[tid] = nt;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const long a = tid >= o ? sc[tid - o] : 0;
            __syncthreads();
            sc[tid] += a;
            __syncthreads();
        }
        const long base = carry;
        if (r < nrun) tile_off[r] = base + sc[tid] - nt;
        __syncthreads();
        if (tid == 1023) carry = base + sc[1023];
        __syncthreads();
    }
    if (tid == 0) tile_off[nrun] = carry;
}

template <typename XT>
__global__ __launch_bounds__(TURN_THREADS) void k_turn_curve(const XT *x, long ldx, int D, const long *runs, long nrun, const long *pos_off, long npos, long W, long S,
                                                             int P, const long *tile_off, int crit, double penalty, double min_llk, double max_llk,
                                                             double *value, int *status)
{
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    if (b >= tile_off[nrun]) return;
    // the run of tile b: the last r with tile_off[r] <= b (runs without positions share their successor's offset)
    long lo = 0, hi = nrun;
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (tile_off[mid] <= b) lo = mid; else hi = mid;
    }
    const long r = lo;
    const long first = runs[3 * r], len = runs[3 * r + 1];
    long n = pos_off[r + 1] - pos_off[r];
    const long cap = turn_run_positions(len, W, S);
    n = n > cap ? cap : n;
    const long k0 = (b - tile_off[r]) * P; // first position of the tile inside the run
    if (k0 >= n) return;
    const int Pt = (int)(n - k0 < P ? n - k0 : P);
    TurnShape sh;
    turn_shape(D, W, S, P, sh);
    const int Dp = sh.Dp;
    const long Rt = 2 * W + (long)(Pt - 1) * S;
    double *X = lds + sh.o_x, *BS = lds + sh.o_bs, *MOD = lds + sh.o_mod, *LC = lds + sh.o_lc, *LP = lds + sh.o_lp;
    int *FL = (int *)(lds + sh.o_flag);
    // ---- 0: the frames, raw (the moments are not screened)
    {
        const XT *src = x + (first + k0 * S) * ldx;
        const long tot = Rt * D;
        for (long e = tid; e < tot; e += TURN_THREADS) {
            const long row = e / D;
            const int d = (int)(e - row * D);
            X[row * Dp + d] = (double)src[row * ldx + d];
        }
        for (int i = tid; i < 2 * P; i += TURN_THREADS) FL[i] = 0;
    }
    __syncthreads();
    // ---- 1: block sums.  BS[((start * ncap + cap) * 2 + (0: sum, 1: squares)) * Dp + d]
    {
        const long nst = sh.nA + sh.nB, tot = nst * D;
        for (long e = tid; e < tot; e += TURN_THREADS) {
            const long si = e / D;
            const int d = (int)(e - si * D);
            const long row0 = si < sh.nA ? si * S : W + (si - sh.nA) * S;
            double s = 0.0, q = 0.0;
            double *o = BS + si * sh.ncap * 2 * Dp + d;
            for (long f = 0; f < S; ++f) {
                const long row = row0 + f;
                if (row >= Rt) break;
                const double v = X[row * Dp + d];
                s += v;
                q += v * v;
                if (f + 1 == sh.r1) { o[sh.cap_r1 * 2 * Dp] = s; o[(sh.cap_r1 * 2 + 1) * Dp] = q; }
                if (f + 1 == sh.r12) { o[sh.cap_r12 * 2 * Dp] = s; o[(sh.cap_r12 * 2 + 1) * Dp] = q; }
                if (f + 1 == S) { o[0] = s; o[Dp] = q; }
            }
        }
    }
    __syncthreads();
    // ---- 2a: mean and covariance.  MOD[((pos * 3 + win) * 2 + (0: mean, 1: cov, later 1 / cov)) * Dp + d]
    {
        const long tot = (long)Pt * 3 * D;
        for (long e = tid; e < tot; e += TURN_THREADS) {
            const int d = (int)(e % D);
            const long pw = e / D;
            const int win = (int)(pw % 3), pos = (int)(pw / 3);
            long si = pos, nblk = sh.nb, shortcap = sh.cap_r1;
            if (win == 1) si = sh.r1 ? sh.nA + pos : pos + sh.nb;
            if (win == 2) { nblk = sh.nb12; shortcap = sh.cap_r12; }
            double s = 0.0, q = 0.0;
            for (long j = 0; j < nblk; ++j) {
                const long c = j == nblk - 1 ? shortcap : 0;
                const double *o = BS + ((si + j) * sh.ncap + c) * 2 * Dp + d;
                if (j == 0) { s = o[0]; q = o[Dp]; } else { s += o[0]; q += o[Dp]; }
            }
            const double nn = win == 2 ? (double)(2 * W) : (double)W;
            const double mean = s / nn, m2 = q / nn, mm = mean * mean, cov = m2 - mm;
            MOD[(pw * 2) * Dp + d] = mean;
            MOD[(pw * 2 + 1) * Dp + d] = cov;
            if (!(cov > 0.0) || !(cov <= 1.79769313486231570815e308)) FL[pos] = 1;
        }
    }
    __syncthreads();
    // ---- 2b: log cov over the block sums, 1 / cov in place
    {
        const long tot = (long)Pt * 3 * D;
        for (long e = tid; e < tot; e += TURN_THREADS) {
            const int d = (int)(e % D);
            const long pw = e / D;
            const double cov = MOD[(pw * 2 + 1) * Dp + d];
            BS[pw * Dp + d] = log(cov);
            MOD[(pw * 2 + 1) * Dp + d] = 1.0 / cov;
        }
    }
    __syncthreads();
    // ---- 2c: log cst = -0.5 (D log 2 pi + sum_d log cov_d), the logarithms added in column order
    for (int pw = tid; pw < Pt * 3; pw += TURN_THREADS) {
        double ld = 0.0;
        for (int d = 0; d < D; ++d) ld += BS[(long)pw * Dp + d];
        const double t = (double)D * 1.8378770664093454835606594728112;
        LC[pw] = -0.5 * (t + ld);
    }
    __syncthreads();
    // ---- 3: the log-likelihood of every block of every window
    {
        const long NB = sh.nblk(), tot = (long)Pt * NB;
        for (long e = tid; e < tot; e += TURN_THREADS) {
            const int pos = (int)(e / NB);
            if (FL[pos]) continue; // a window without a usable covariance: the value is NaN whatever the frames say
            long j = e - (long)pos * NB;
            int win = 0;
            long row0 = (long)pos * S, nblk = sh.nb, rs = sh.r1;
            if (j >= 2 * sh.nb) { win = 2; j -= 2 * sh.nb; nblk = sh.nb12; rs = sh.r12; }
            else if (j >= sh.nb) { win = 1; j -= sh.nb; row0 += W; }
            row0 += j * S;
            const long cnt = (j == nblk - 1 && rs) ? rs : S;
            const double *mean = MOD + ((long)(pos * 3 + win) * 2) * Dp, *iv = mean + Dp;
            const double lc = LC[pos * 3 + win];
            double acc = 0.0;
            int acted = 0;
            for (long f = 0; f < cnt; ++f) {
                const double *xr = X + (row0 + f) * Dp;
                double q = 0.0;
                for (int d = 0; d < D; ++d) {
                    const double t = xr[d] - mean[d];
                    q = __builtin_fma(t * t, iv[d], q);
                }
                double l = lc - 0.5 * q;
                if (!(l >= GMMIV_ZERO_LLK) || !(l <= 1.79769313486231570815e308)) { l = min_llk; acted = 1; } // likelihood 0 in fp64, or not finite
                else if (l < min_llk) { l = min_llk; acted = 1; }
                else if (l > max_llk) { l = max_llk; acted = 1; }
                acc += l;
            }
            LP[e] = acc;
            if (acted) FL[P + pos] = 1;
        }
    }
    __syncthreads();
    // ---- 4: the criterion
    for (int pos = tid; pos < Pt; pos += TURN_THREADS) {
        const long p = pos_off[r] + k0 + pos;
        if (p < 0 || p >= npos) continue;
        const double *lp = LP + (long)pos * sh.nblk();
        double v;
        int st = 0;
        if (FL[pos]) { v = __builtin_nan(""); st = 1; }
        else {
            double l1 = lp[0], l2 = lp[sh.nb], l12 = lp[2 * sh.nb];
            for (long j = 1; j < sh.nb; ++j) { l1 += lp[j]; l2 += lp[sh.nb + j]; }
            for (long j = 1; j < sh.nb12; ++j) l12 += lp[2 * sh.nb + j];
            const double s12 = l1 + l2, g = l12 - s12;
            v = crit == 0 ? g : (crit == 1 ? -g : -g - penalty);
            if (FL[P + pos]) st = 2;
        }
        value[p] = v;
        if (status) status[p] = st;
    }
}

// ---- k_turn_pick: one workgroup per run (TurnDetection.cpp:184-263)
__global__ __launch_bounds__(TURN_THREADS) void k_turn_pick(const double *value, const long *pos_off, long npos, double alpha, double *sm, unsigned char *dec,
                                                            double *run_stats, long *n_turns)
{
#pragma clang fp contract(off)
    __shared__ double red[2][TURN_THREADS];
    __shared__ long cnt[TURN_THREADS];
    __shared__ double s_thr;
    const int tid = threadIdx.x;
    const long r = blockIdx.x;
    long p0 = pos_off[r], n = pos_off[r + 1] - p0;
    if (p0 < 0 || p0 > npos) n = 0;
    if (n > npos - p0) n = npos - p0;
    if (n <= 0) {
        if (tid == 0) {
            if (run_stats) { run_stats[2 * r] = __builtin_nan(""); run_stats[2 * r + 1] = __builtin_nan(""); }
            if (n_turns) n_turns[r] = 0;
        }
        return;
    }
    const double *v = value + p0;
    double *w = sm + p0;
    for (long i = tid; i < n; i += TURN_THREADS) {
        double o = v[i];
        if (i >= 1 && i + 1 < n) {
            const double a = 0.25 * v[i - 1], c = 0.25 * v[i + 1], m = 0.5 * v[i], ac = a + c;
            o = ac + m;
        }
        w[i] = o;
    }
    __syncthreads();
    double s = 0.0, q = 0.0;
    for (long i = tid; i < n; i += TURN_THREADS) { const double t = w[i]; s += t; q += t * t; }
    red[0][tid] = s;
    red[1][tid] = q;
    __syncthreads();
    if (tid == 0) {
        double S = red[0][0], Q = red[1][0];
        const int m = n < TURN_THREADS ? (int)n : TURN_THREADS;
        for (int j = 1; j < m; ++j) { S += red[0][j]; Q += red[1][j]; }
        const double nn = (double)n, mean = S / nn, m2 = Q / nn, mm = mean * mean;
        const double sd = __builtin_sqrt(m2 - mm);
        s_thr = alpha * sd;
        if (run_stats) { run_stats[2 * r] = mean; run_stats[2 * r + 1] = sd; }
    }
    __syncthreads();
    const double thr = s_thr;
    long c = 0;
    for (long i = tid; i < n; i += TURN_THREADS) {
        unsigned char dd = 0;
        if (i >= 1 && i + 1 < n) {
            const double cur = w[i];
            double mn = cur;
            for (long j = i - 1; j > 0; --j) { // never looks at index 0
                const double t = w[j];
                if (t < mn) mn = t; else break;
            }
            if (__builtin_fabs(cur - mn) > thr) {
                mn = cur;
                for (long j = i + 1; j < n; ++j) { // may reach the last index
                    const double t = w[j];
                    if (t < mn) mn = t; else break;
                }
                if (__builtin_fabs(cur - mn) > thr) dd = 1;
            }
        }
        dec[p0 + i] = dd;
        c += dd;
    }
    cnt[tid] = c;
    __syncthreads();
    if (tid == 0 && n_turns) {
        long t = 0;
        for (int j = 0; j < TURN_THREADS; ++j) t += cnt[j];
        n_turns[r] = t;
    }
}

// ---- k_turn_segments: one workgroup per file, one thread per run (TurnDetection.cpp:142-145, 265-279)
static __device__ __forceinline__ long turn_lower(const long *runs, long nrun, long f)
{
    long lo = 0, hi = nrun;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (runs[3 * mid + 2] < f) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// emit(begin, length) per output segment of run r, in order
template <typename Emit>
static __device__ __forceinline__ void turn_run_segments(const long *runs, const long *pos_off, long npos, const unsigned char *dec, long W, long S, long r, Emit emit)
{
    const long b = runs[3 * r], L = runs[3 * r + 1];
    long p0 = pos_off[r], n = pos_off[r + 1] - p0;
    const long cap = turn_run_positions(L, W, S);
    n = n > cap ? cap : n;
    if (p0 < 0 || p0 > npos) n = 0;
    if (n > npos - p0) n = npos - p0;
    if (n <= 0) { emit(b, L); return; }
    const long end = b + L - 1; // endSeg
    long start = b;
    for (long i = 0; i < n; ++i)
        if (dec[p0 + i]) {
            const long fr = b + W - 1 + i * S;
            emit(start, fr - start + 1);
            start = fr + 1;
        }
    if (start < end) emit(start, end - start + 1);
}

__global__ __launch_bounds__(TURN_THREADS) void k_turn_segments(const long *runs, long nrun, const long *pos_off, long npos, const unsigned char *dec, long W, long S,
                                                                long *run_base, long *seg_count, const long *seg_off, long *seg_begin, long *seg_len)
{
    const int tid = threadIdx.x;
    const long f = blockIdx.x;
    const long rlo = turn_lower(runs, nrun, f), rhi = turn_lower(runs, nrun, f + 1);
    for (long r = rlo + tid; r < rhi; r += TURN_THREADS) {
        long c = 0;
        turn_run_segments(runs, pos_off, npos, dec, W, S, r, [&](long, long) { ++c; });
        run_base[r] = c;
    }
    __syncthreads();
    if (tid == 0) {
        long t = 0;
        for (long r = rlo; r < rhi; ++r) { const long c = run_base[r]; run_base[r] = t; t += c; }
        if (seg_count) seg_count[f] = t;
    }
    __syncthreads();
    if (!seg_begin) return;
    const long o0 = seg_off[f], room = seg_off[f + 1] - o0;
    if (o0 < 0) return;
    for (long r = rlo + tid; r < rhi; r += TURN_THREADS) {
        long k = run_base[r];
        turn_run_segments(runs, pos_off, npos, dec, W, S, r, [&](long sb, long sl) {
            if (k < room) { seg_begin[o0 + k] = sb; seg_len[o0 + k] = sl; }
            ++k;
        });
    }
}

int gmmk_turn_tiles(hipStream_t st, const long *runs, long nrun, const long *pos_off, long W, long S, int P, long *tile_off)
{
    k_turn_tiles<<<1, 1024, 0, st>>>(runs, nrun, pos_off, W, S, P, tile_off);
    return (int)hipGetLastError();
}

int gmmk_turn_curve(hipStream_t st, int x_f64, const void *x, long ldx, int D, const long *runs, long nrun, const long *pos_off, long npos, long W, long S,
                    int P, long grid, const long *tile_off, int crit, double penalty, double min_llk, double max_llk, double *value, int *status)
{
    if (grid <= 0) return 0;
    TurnShape sh;
    if (!turn_shape(D, W, S, P, sh) || sh.bytes > TURN_LDS_BUDGET) return (int)hipErrorInvalidValue;
    hipError_t e = x_f64 ? gmmiv_lds_attr<k_turn_curve<double>>((size_t)sh.bytes) : gmmiv_lds_attr<k_turn_curve<float>>((size_t)sh.bytes);
    if (e != hipSuccess) return (int)e;
    if (x_f64) k_turn_curve<double><<<(unsigned)grid, TURN_THREADS, (size_t)sh.bytes, st>>>((const double *)x, ldx, D, runs, nrun, pos_off, npos, W, S, P, tile_off, crit, penalty, min_llk, max_llk, value, status);
    else k_turn_curve<float><<<(unsigned)grid, TURN_THREADS, (size_t)sh.bytes, st>>>((const float *)x, ldx, D, runs, nrun, pos_off, npos, W, S, P, tile_off, crit, penalty, min_llk, max_llk, value, status);
    return (int)hipGetLastError();
}

int gmmk_turn_pick(hipStream_t st, const double *value, const long *pos_off, long nrun, long npos, double alpha, double *smoothed, unsigned char *dec,
                   double *run_stats, long *n_turns)
{
    if (nrun <= 0) return 0;
    k_turn_pick<<<(unsigned)nrun, TURN_THREADS, 0, st>>>(value, pos_off, npos, alpha, smoothed, dec, run_stats, n_turns);
    return (int)hipGetLastError();
}

int gmmk_turn_segments(hipStream_t st, const long *runs, long nrun, long nfiles, const long *pos_off, long npos, const unsigned char *dec, long W, long S,
                       long *run_base, long *seg_count, const long *seg_off, long *seg_begin, long *seg_len)
{
    if (nfiles <= 0) return 0;
    k_turn_segments<<<(unsigned)nfiles, TURN_THREADS, 0, st>>>(runs, nrun, pos_off, npos, dec, W, S, run_base, seg_count, seg_off, seg_begin, seg_len);
    return (int)hipGetLastError();
}
