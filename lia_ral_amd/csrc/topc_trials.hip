// topc_trials.hip -- kernels of gmmiv_llr_trials (capi_trials.hip): USE_TOP_DISTRIBS for a whole list of (segment, model) trials, the
// per-frame values summed inside the kernel.  DESIGN.md section 3.16.
//
// ComputeTest (LIA_SpkDet/ComputeTest/src/ComputeTest.cpp:129-215) needs one number per (test segment, client): the mean of the client's
// clamped log-likelihoods over the segment's frames.  k_topc_use4_multi (topc_z.hip) writes every per-frame value to HBM, a second pass
// averages them, and every ndx line is a call of its own.  Here a work item is (trial, piece): a piece is P frames counted from the
// segment's first frame; the workgroup picks its model from a device tile table (the idea of k_llk_mfma<.., MM>), walks the piece's
// frames and leaves ONE double, the sum of the piece's clamped values, in a scratch array.  k_trial_reduce adds a trial's partials in
// piece order.  No atomics, no per-frame client value in HBM; every sum has a fixed order that depends on the segment's frames alone.
#include "devutil.h"
#include "gmm_kernels.h"
#include "trials_kernels.h"

typedef double d2 __attribute__((ext_vector_type(2)));

// One workgroup per tile, four waves: wave w takes the frames lo + w, lo + w + 4, ... of the piece, one frame at a time.  The per-frame
// arithmetic is k_topc_use4's, statement for statement (four lanes per candidate, the quad exchanges, wave_max / wave_sum, gexp, the
// remainder term, the clamp): a frame's value has the bits gmmiv_llk_use_top gives.  Lane 0 of a wave adds its frames' values in frame
// order; the four wave sums are combined in wave order.
// Tiles are sorted by (segment, piece, position of the trial): the workgroups that run next to each other read the same rows of x and
// idx (from L2) and differ in the model rows they gather.
template <typename XT>
__global__ __launch_bounds__(256) void k_topc_use4_trials(const void *__restrict__ x, long xbase, long ldx, int D, const double *__restrict__ mean, long sm,
                                                          const double *__restrict__ iv, long si, const double *__restrict__ lwc, long sl, int C,
                                                          int ctop, const gmmiv_trial_tile *__restrict__ tiles, const long *__restrict__ trial_off,
                                                          long base, const int *__restrict__ idx, const double *__restrict__ nontop_llk,
                                                          int complete, double lo, double hi, double *__restrict__ part)
{
    __shared__ double wsum[4];
    const gmmiv_trial_tile tl = tiles[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slot = lane >> 2, sub = lane & 3;
    const double *mean_g = mean + (size_t)tl.model * sm, *iv_g = iv + (size_t)tl.model * si, *lwc_g = lwc + (size_t)tl.model * sl;
    const double NINF = -__builtin_inf();
    const int np = D >> 1; // dimension pairs
    double sum = 0.0;
    for (long t = tl.lo + wave; t < tl.hi; t += 4) { // wave-uniform
        const long tr = t - base, tx = t - xbase;
        const int c = slot < ctop ? idx[tr * ctop + slot] : -1;
        const bool live = (unsigned)c < (unsigned)C; // an index outside the model is skipped, never dereferenced
        const int cc = live ? c : 0;
        const d2 *mu = (const d2 *)(mean_g + (size_t)cc * D), *vi = (const d2 *)(iv_g + (size_t)cc * D);
        double acc = 0.0;
        for (int p0 = 0; p0 < np; p0 += 16) {
            d2 m[4], v[4];
            double x0[4], x1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { // all loads of the batch first
                const int p = p0 + sub + 4 * u, pc = p < np ? p : np - 1;
                m[u] = mu[pc];
                v[u] = vi[pc];
                x0[u] = feat_load<XT>::get(x, tx * ldx + 2 * pc);
                x1[u] = feat_load<XT>::get(x, tx * ldx + 2 * pc + 1);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool ok = p0 + sub + 4 * u < np;
                const double dx0 = x0[u] - m[u][0], dx1 = x1[u] - m[u][1];
                const double a1 = __builtin_fma(dx1 * dx1, v[u][1], __builtin_fma(dx0 * dx0, v[u][0], acc));
                acc = ok ? a1 : acc;
            }
        }
        acc += __hiloint2double(dpp_i32<0xB1>(__double2hiint(acc)), dpp_i32<0xB1>(__double2loint(acc))); // quad_perm [1 0 3 2]
        acc += __hiloint2double(dpp_i32<0x4E>(__double2hiint(acc)), dpp_i32<0x4E>(__double2loint(acc))); // quad_perm [2 3 0 1]
        const double z = live ? __builtin_fma(-0.5, acc, lwc_g[cc]) : NINF;
        const double r = (complete && nontop_llk) ? nontop_llk[tr] : NINF;
        const double M = wave_max_f64_dpp(fmax(z, r));
        const double s0 = wave_sum_f64_dpp((live && sub == 0) ? gexp(z - M) : 0.0);
        if (lane == 0) {
            const double s = r > NINF ? s0 + gexp(r - M) : s0;
            sum += fmin(fmax(M + log(s), lo), hi);
        }
    }
    if (lane == 0) wsum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) part[trial_off[tl.trial] + tl.piece] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// The same piece scheme on per-frame values that already sit in memory (the world's log-likelihoods; a trial's row on the any-shape
// path): frame lo + j of a piece goes to partial j & 3 in frame order, the four partials are combined in that order -- the sums the
// four waves of k_topc_use4_trials form.
__device__ __forceinline__ double piece_sum(const double *__restrict__ v, long lo, long hi)
{
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    long t = lo;
    for (; t + 4 <= hi; t += 4) {
        p[0] += v[t]; p[1] += v[t + 1]; p[2] += v[t + 2]; p[3] += v[t + 3];
    }
    if (t < hi) p[0] += v[t];
    if (t + 1 < hi) p[1] += v[t + 1];
    if (t + 2 < hi) p[2] += v[t + 2];
    return ((p[0] + p[1]) + p[2]) + p[3];
}

// one thread per piece of the segments [0, nseg): v is indexed by frame - base, the piece k of segment s goes to part[seg_off[s] + k]
__global__ void k_piece_sums_segs(const double *__restrict__ v, long base, const long *__restrict__ seg_begin, const long *__restrict__ seg_off,
                                  long s0, long s1, int P, double *__restrict__ part)
{
    const long j = seg_off[s0] + (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= seg_off[s1]) return;
    long a = s0, b = s1; // the segment whose slots hold j: seg_off[a] <= j < seg_off[a + 1]
    while (b - a > 1) {
        const long m = (a + b) >> 1;
        if (seg_off[m] <= j) a = m; else b = m;
    }
    const long k = j - seg_off[a], lo = seg_begin[a] + k * P, e = seg_begin[a + 1], hi = lo + P < e ? lo + P : e;
    part[j] = piece_sum(v - base, lo, hi);
}

// one thread per piece of ONE row of n values
__global__ void k_piece_sums_row(const double *__restrict__ v, long n, int P, double *__restrict__ part)
{
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long lo = k * P;
    if (lo >= n) return;
    part[k] = piece_sum(v, lo, lo + P < n ? lo + P : n);
}

// Thread i < ntrial: the trial's partials in piece order, / n_s, minus the world mean of its segment (recomputed from the world's
// partials in the same order as by the thread that writes world_mean: the same bits).  Thread ntrial + s: world_mean[s].
__global__ void k_trial_reduce(long ntrial, long nseg, const int *__restrict__ trial_seg, const long *__restrict__ trial_off,
                               const long *__restrict__ seg_begin, const long *__restrict__ seg_off, const double *__restrict__ part,
                               const double *__restrict__ wpart, double *__restrict__ llr, double *__restrict__ client_mean,
                               double *__restrict__ world_mean)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntrial + nseg) return;
    const long s = i < ntrial ? trial_seg[i] : i - ntrial;
    const long n = seg_begin[s + 1] - seg_begin[s];
    double ws = 0.0;
    for (long k = seg_off[s]; k < seg_off[s + 1]; ++k) ws += wpart[k];
    const double wm = n > 0 ? ws / (double)n : 0.0;
    if (i >= ntrial) {
        if (world_mean) world_mean[s] = wm;
        return;
    }
    double cs = 0.0;
    for (long k = trial_off[i]; k < trial_off[i + 1]; ++k) cs += part[k];
    const double cm = n > 0 ? cs / (double)n : 0.0;
    if (client_mean) client_mean[i] = cm;
    llr[i] = cm - wm;
}

int gmmk_topc_use4_trials(hipStream_t st, int x_f64, const void *x, long xbase, long ldx, int D, const double *mean, long sm, const double *iv,
                          long si, const double *lwc, long sl, int C, int ctop, const gmmiv_trial_tile *tiles, long ntiles, const long *trial_off,
                          long base, const int *idx, const double *nllk, int complete, double lo, double hi, double *part)
{
    if (ntiles <= 0) return 0;
    if (ctop > 16 || D % 2 != 0 || ntiles > 0x7fffffffL) return -1;
    if (x_f64)
        k_topc_use4_trials<double><<<(unsigned)ntiles, 256, 0, st>>>(x, xbase, ldx, D, mean, sm, iv, si, lwc, sl, C, ctop, tiles, trial_off, base, idx,
                                                                     nllk, complete, lo, hi, part);
    else
        k_topc_use4_trials<float><<<(unsigned)ntiles, 256, 0, st>>>(x, xbase, ldx, D, mean, sm, iv, si, lwc, sl, C, ctop, tiles, trial_off, base, idx,
                                                                    nllk, complete, lo, hi, part);
    return (int)hipGetLastError();
}

int gmmk_piece_sums_segs(hipStream_t st, const double *v, long base, const long *seg_begin, const long *seg_off, long s0, long s1, long npiece, int P,
                         double *part)
{
    if (npiece <= 0) return 0;
    k_piece_sums_segs<<<(unsigned)((npiece + 127) / 128), 128, 0, st>>>(v, base, seg_begin, seg_off, s0, s1, P, part);
    return (int)hipGetLastError();
}

int gmmk_piece_sums_row(hipStream_t st, const double *v, long n, int P, double *part)
{
    if (n <= 0) return 0;
    const long np = (n + P - 1) / P;
    k_piece_sums_row<<<(unsigned)((np + 127) / 128), 128, 0, st>>>(v, n, P, part);
    return (int)hipGetLastError();
}

int gmmk_trial_reduce(hipStream_t st, long ntrial, long nseg, const int *trial_seg, const long *trial_off, const long *seg_begin, const long *seg_off,
                      const double *part, const double *wpart, double *llr, double *client_mean, double *world_mean)
{
    if (ntrial + nseg <= 0) return 0;
    k_trial_reduce<<<(unsigned)((ntrial + nseg + 127) / 128), 128, 0, st>>>(ntrial, nseg, trial_seg, trial_off, seg_begin, seg_off, part, wpart, llr,
                                                                           client_mean, world_mean);
    return (int)hipGetLastError();
}
