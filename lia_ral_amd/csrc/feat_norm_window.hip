// feat_norm_window.hip -- NormFeat's windowMode on the resident frames (include/gmmiv_feat_window.h): k_norm_window, one workgroup per
// file, the file's whole chain of steps in one launch.
//
// A step's statistics are sums over the runs of its window, and the definition of those sums (feat_norm.hip, k_moments_groups +
// k_moments_combine) is per run: 2 D partial sums of a run, then the runs' partials added in table order.  A run's partials change
// only when the run is rewritten, and the schedule rewrites every run exactly once.  So the kernel keeps partial[run][2 D]:
//   pass 0   the partials of every run of the file from the frames as they came; their sum gives gm / gs;
//   a step   the window's sums are the partials of its runs added in table order (no frame is read), then the blend; the step's runs
//            are rewritten, and the thread that stores a frame adds the STORED value (an f32 store rounds first) into the new
//            partials of that run -- the bits a later read of the buffer would give.
// Every frame is read twice and written once whatever the window length; nothing of a window is staged.  x is written and never read
// again inside the launch.  Nothing here adds into memory another workgroup touches: a file's bits are a function of its own runs
// and steps.  The columns are independent of each other, so D > NW_COLS runs the whole chain once per block of NW_COLS columns.
//
// Thread (j, v) of 16 x nc: row lane j of the definition, column c0 + v.  A wave's load is a row segment of nc consecutive values.
// The 16 lane sums of a run go through LDS (two buffers in turn: one barrier per run); thread (0, v) adds them in order, owns
// partial[.][c0 + v] and partial[.][D + c0 + v] for the whole chain (it re-reads only what it wrote itself) and computes the blend.
#include "devutil.h"
#include "feat_norm_window.h"

constexpr int NW_ROWS = 16, NW_COLS = 64;

// the first run of file f (the file ids are non-decreasing along the table)
static __device__ __forceinline__ long nw_lower(const long *runs, long nrun, long f)
{
    long lo = 0, hi = nrun;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (runs[3 * mid + 2] < f) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <typename XT>
__global__ __launch_bounds__(1024) void k_norm_window(XT *x, long ldx, int D, const long *runs, long nrun, const long *step_off, const long *steps,
                                                      const double *alpha, int cms, int var, double *partial, double *gstat, double *step_stat)
{
#pragma clang fp contract(off)
    __shared__ double red[2][NW_ROWS][2 * NW_COLS];
    __shared__ double ms[2][NW_COLS];
    const int tid = threadIdx.x, nc = blockDim.x / NW_ROWS;
    const int j = tid / nc, v = tid - j * nc;
    const long f = blockIdx.x;
    const long rlo = nw_lower(runs, nrun, f), rhi = nw_lower(runs, nrun, f + 1);
    const long s0 = step_off[f], s1 = step_off[f + 1];
    int b = 0;
    for (int c0 = 0; c0 < D; c0 += nc) {
        const int col = c0 + v;
        const bool on = col < D, owner = on && j == 0;
        // ---- pass 0: the partials of every run, as the frames came
        for (long r = rlo; r < rhi; ++r) {
            const long first = runs[3 * r], len = runs[3 * r + 1];
            double s = 0.0, ss = 0.0;
            if (on) {
                const XT *p = x + first * ldx + col;
                long t = j;
                for (; t + 3L * NW_ROWS < len; t += 4L * NW_ROWS) {
                    double a[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) a[u] = (double)p[(t + (long)u * NW_ROWS) * ldx];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { s += a[u]; ss += a[u] * a[u]; }
                }
                for (; t < len; t += NW_ROWS) { const double va = (double)p[t * ldx]; s += va; ss += va * va; }
            }
            red[b][j][v] = s;
            red[b][j][NW_COLS + v] = ss;
            __syncthreads();
            if (owner) {
                double a = red[b][0][v], q = red[b][0][NW_COLS + v];
#pragma unroll
                for (int jj = 1; jj < NW_ROWS; ++jj) { a += red[b][jj][v]; q += red[b][jj][NW_COLS + v]; }
                partial[(size_t)r * 2 * D + col] = a;
                partial[(size_t)r * 2 * D + D + col] = q;
            }
            b ^= 1;
        }
        // ---- the file's global statistics (a zeroed accumulator plus the runs' partials in table order, then k_moments_stats)
        double gm = 0.0, gs = 0.0;
        if (owner) {
            double S = 0.0, Q = 0.0, n = 0.0;
            if (rhi > rlo) {
                double ts = partial[(size_t)rlo * 2 * D + col], tq = partial[(size_t)rlo * 2 * D + D + col], tn = (double)runs[3 * rlo + 1];
                for (long r = rlo + 1; r < rhi; ++r) { ts += partial[(size_t)r * 2 * D + col]; tq += partial[(size_t)r * 2 * D + D + col]; tn += (double)runs[3 * r + 1]; }
                S += ts; Q += tq; n += tn;
            }
            gm = S / n;
            const double q = Q / n, mm = gm * gm;
            gs = __builtin_sqrt(q - mm);
            if (gstat) { gstat[(size_t)f * 2 * D + col] = gm; gstat[(size_t)f * 2 * D + D + col] = gs; }
        }
        // ---- the steps, in order
        for (long st = s0; st < s1; ++st) {
            long wlo = steps[4 * st], whi = steps[4 * st + 1], alo = steps[4 * st + 2], ahi = steps[4 * st + 3];
            // nothing outside the file's own runs is read or written, whatever the table says
            wlo = wlo < rlo ? rlo : wlo; whi = whi > rhi ? rhi : whi;
            alo = alo < rlo ? rlo : alo; ahi = ahi > rhi ? rhi : ahi;
            if (owner) {
                double S = 0.0, Q = 0.0, n = 0.0;
                if (whi > wlo) {
                    double ts = partial[(size_t)wlo * 2 * D + col], tq = partial[(size_t)wlo * 2 * D + D + col], tn = (double)runs[3 * wlo + 1];
                    for (long r = wlo + 1; r < whi; ++r) { ts += partial[(size_t)r * 2 * D + col]; tq += partial[(size_t)r * 2 * D + D + col]; tn += (double)runs[3 * r + 1]; }
                    S += ts; Q += tq; n += tn;
                }
                const double m = S / n, q = Q / n, mm = m * m, sd = __builtin_sqrt(q - mm);
                // computeWindowParam (NormFeat.cpp:166-171): every product and sum rounded on its own
                const double a = alpha[st], na = 1 - a;
                const double t0 = a * m, t1 = na * gm;
                double mp = t0 + t1;
                const double u0 = (a * sd) * sd, u1 = (na * gs) * gs, dm = mp - gm, u2 = (na * a) * (dm * dm);
                const double u01 = u0 + u1;
                double sp = __builtin_sqrt(u01 + u2);
                if (cms) sp = 1.0;
                if (var) mp = 0.0;
                ms[0][v] = mp;
                ms[1][v] = sp;
                if (step_stat) { step_stat[(size_t)st * 2 * D + col] = mp; step_stat[(size_t)st * 2 * D + D + col] = sp; }
            }
            __syncthreads();
            const double mp = ms[0][v], sp = ms[1][v];
            // computeZeroOne on the step's runs; the stored values give the runs' new partials
            for (long r = alo; r < ahi; ++r) {
                const long first = runs[3 * r], len = runs[3 * r + 1];
                double s = 0.0, ss = 0.0;
                if (on) {
                    XT *p = x + first * ldx + col;
                    long t = j;
                    for (; t + 3L * NW_ROWS < len; t += 4L * NW_ROWS) {
                        double a[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) a[u] = (double)p[(t + (long)u * NW_ROWS) * ldx];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const double d = a[u] - mp;
                            const XT o = (XT)(d / sp);
                            p[(t + (long)u * NW_ROWS) * ldx] = o;
                            const double w = (double)o;
                            s += w; ss += w * w;
                        }
                    }
                    for (; t < len; t += NW_ROWS) {
                        const double d = (double)p[t * ldx] - mp;
                        const XT o = (XT)(d / sp);
                        p[t * ldx] = o;
                        const double w = (double)o;
                        s += w; ss += w * w;
                    }
                }
                red[b][j][v] = s;
                red[b][j][NW_COLS + v] = ss;
                __syncthreads();
                if (owner) {
                    double a = red[b][0][v], q = red[b][0][NW_COLS + v];
#pragma unroll
                    for (int jj = 1; jj < NW_ROWS; ++jj) { a += red[b][jj][v]; q += red[b][jj][NW_COLS + v]; }
                    partial[(size_t)r * 2 * D + col] = a;
                    partial[(size_t)r * 2 * D + D + col] = q;
                }
                b ^= 1;
            }
            __syncthreads(); // ms is rewritten by the next step
        }
    }
}

int gmmk_norm_window(hipStream_t st, int x_f64, void *x, long ldx, int D, const long *runs, long nrun, long nfiles, const long *step_off,
                     const long *steps, const double *alpha, int cms, int var, double *partial, double *gstat, double *step_stat)
{
    if (nfiles <= 0) return 0;
    int nc = (D + 3) / 4 * 4; // a multiple of 4 columns: 64 k threads
    if (nc > NW_COLS) nc = NW_COLS;
    const unsigned bs = (unsigned)(NW_ROWS * nc), grid = (unsigned)nfiles;
    if (x_f64) k_norm_window<double><<<grid, bs, 0, st>>>((double *)x, ldx, D, runs, nrun, step_off, steps, alpha, cms, var, partial, gstat, step_stat);
    else k_norm_window<float><<<grid, bs, 0, st>>>((float *)x, ldx, D, runs, nrun, step_off, steps, alpha, cms, var, partial, gstat, step_stat);
    return (int)hipGetLastError();
}
