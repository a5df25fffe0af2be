// iv_trials.hip -- kernels behind include/gmmiv_iv_trials.h: k_score_trials, the gather kernel that scores a list of (model, segment)
// trials from two row tables, and the transpose that builds those tables.  gfx950 (wave64).  DESIGN.md section 3.21.
//
// k_score_trials: one WAVE per work item {anchor, [lo, hi)}: the anchor row goes into registers once (lane j holds the 16-byte pairs
// j, j + 64, ...), then the partner rows of its trials are gathered IVT_ROWS at a time with one 16-byte load per lane and pass (one
// wave instruction reads 1 KiB of a row), multiplied out, reduced by a fixed xor butterfly and stored, 8 bytes per trial.  No LDS and
// no read-modify-write of memory: every trial is written once, by one lane.
//
// The summation order is a function of the row length alone (include/gmmiv_iv_trials.h): lane j adds its pairs in increasing p from +0,
// element 2p before 2p + 1, one fma each.  A pass past the end of the row contributes fma(0, 0, acc) = acc (acc is never -0: it
// starts at +0), so the instantiations below, which differ in the number of passes they unroll, give the same bits.
#include "iv_trials_kernels.h"

#define IVT_WAVES 4 // waves (work items) per workgroup

template <int NP, int ROWS>
__global__ __launch_bounds__(64 * IVT_WAVES) void k_score_trials(int ldr, const double *__restrict__ Atab, const double *__restrict__ Ptab,
                                                                 const double *__restrict__ qa, const double *__restrict__ qp, int anchor_is_seg,
                                                                 const gmmiv_iv_trial_tile *__restrict__ tiles, long ntiles,
                                                                 const int *__restrict__ partner, const int *__restrict__ pos, int mode, double cc,
                                                                 double bm, double bs, double cst, double *__restrict__ scores)
{
    const int lane = threadIdx.x & 63;
    const long t = (long)blockIdx.x * IVT_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (t >= ntiles) return;
    const int anchor = tiles[t].anchor;
    const long lo = tiles[t].lo, hi = tiles[t].hi;
    const int npairs = ldr >> 1;
    const double2 *__restrict__ arow = (const double2 *)(Atab + (size_t)anchor * ldr);
    const double2 zero = make_double2(0.0, 0.0);
    double2 a[NP > 0 ? NP : 1];
    if (NP > 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) a[i] = lane + 64 * i < npairs ? arow[lane + 64 * i] : zero;
    }
    const double q_anchor = qa[anchor];
    for (long k = lo; k < hi; k += ROWS) {
        const long left = hi - k;
        const double2 *brow[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) // past the end of the piece: its last trial again (read, never stored)
            brow[r] = (const double2 *)(Ptab + (size_t)partner[r < left ? k + r : hi - 1] * ldr);
        double acc[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[r] = 0.0;
        if (NP > 0) {
            double2 b[ROWS][NP > 0 ? NP : 1];
#pragma unroll
            for (int i = 0; i < NP; ++i)
#pragma unroll
                for (int r = 0; r < ROWS; ++r) b[r][i] = lane + 64 * i < npairs ? brow[r][lane + 64 * i] : zero;
#pragma unroll
            for (int i = 0; i < NP; ++i)
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    acc[r] = __builtin_fma(a[i].x, b[r][i].x, acc[r]);
                    acc[r] = __builtin_fma(a[i].y, b[r][i].y, acc[r]);
                }
        } else { // a row too long for the registers: the anchor is read again with every group of rows (it stays in L2)
            for (int p = lane; p < npairs; p += 64) {
                const double2 av = arow[p];
                double2 b[ROWS];
#pragma unroll
                for (int r = 0; r < ROWS; ++r) b[r] = brow[r][p];
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    acc[r] = __builtin_fma(av.x, b[r].x, acc[r]);
                    acc[r] = __builtin_fma(av.y, b[r].y, acc[r]);
                }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) acc[r] += __shfl_xor(acc[r], d, 64);
        if (lane < ROWS && lane < left) { // lane r finishes trial k + r
            double dot = acc[0];
#pragma unroll
            for (int r = 1; r < ROWS; ++r) dot = lane == r ? acc[r] : dot;
            const double q_partner = qp[partner[k + lane]];
            const double qm = anchor_is_seg ? q_partner : q_anchor, qs = anchor_is_seg ? q_anchor : q_partner;
            scores[pos[k + lane]] = mode == 1 ? (dot * qm) * qs : __builtin_fma(cc, dot, __builtin_fma(bm, qm, __builtin_fma(bs, qs, cst)));
        }
    }
}

int ivk_score_trials(hipStream_t st, int ldr, const double *Atab, const double *Ptab, const double *qa, const double *qp, int anchor_is_seg,
                     const gmmiv_iv_trial_tile *tiles, long ntiles, const int *partner, const int *pos, int mode, double cc, double bm,
                     double bs, double cst, double *scores)
{
    if (ntiles <= 0) return 0;
    const dim3 grid((unsigned)((ntiles + IVT_WAVES - 1) / IVT_WAVES)), block(64 * IVT_WAVES);
    const int passes = (ldr / 2 + 63) / 64;
#define IVT_LAUNCH(NP, ROWS) \
    k_score_trials<NP, ROWS><<<grid, block, 0, st>>>(ldr, Atab, Ptab, qa, qp, anchor_is_seg, tiles, ntiles, partner, pos, mode, cc, bm, bs, cst, scores)
    // four rows in flight while anchor and rows fit 128 registers (16 waves per CU); two rows up to dim 1024; then the re-reading form
    if (passes <= 1) IVT_LAUNCH(1, 4);
    else if (passes <= 2) IVT_LAUNCH(2, 4);
    else if (passes <= 4) IVT_LAUNCH(4, 4);
    else if (passes <= 8) IVT_LAUNCH(8, 2);
    else IVT_LAUNCH(0, 4);
#undef IVT_LAUNCH
    return (int)hipGetLastError();
}

// ---- column layout -> row tables ----------------------------------------------------------------------------------------------------
// out[j][i] = X[i][j] for i < dim, 0 for dim <= i < ldr: 32 x 32 tiles through LDS so that both sides move whole lines
__global__ __launch_bounds__(256) void k_cols_to_rows(int dim, long n, const double *__restrict__ X, long ld, double *__restrict__ out, int ldr)
{
    __shared__ double tile[32][33];
    const long j0 = (long)blockIdx.x * 32;
    const int i0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int i = i0 + r;
        const long j = j0 + tx;
        tile[r][tx] = (i < dim && j < n) ? X[(size_t)i * ld + j] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const long j = j0 + r;
        const int i = i0 + tx;
        if (j < n && i < ldr) out[(size_t)j * ldr + i] = tile[tx][r];
    }
}

int ivk_cols_to_rows(hipStream_t st, int dim, long n, const double *X, long ld, double *out, int ldr)
{
    if (n <= 0 || dim <= 0) return 0;
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)((ldr + 31) / 32));
    k_cols_to_rows<<<grid, 256, 0, st>>>(dim, n, X, ld, out, ldr);
    return (int)hipGetLastError();
}

__global__ void k_zero_pad(int dim, long n, double *__restrict__ out, int ldr)
{
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long)gridDim.x * blockDim.x) out[(size_t)r * ldr + dim] = 0.0;
}

int ivk_zero_pad(hipStream_t st, int dim, long n, double *out, int ldr)
{
    if (n <= 0 || ldr <= dim) return 0;
    const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    k_zero_pad<<<blocks, 256, 0, st>>>(dim, n, out, ldr);
    return (int)hipGetLastError();
}
