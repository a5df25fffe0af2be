// mllr.hip -- MLLR mean adaptation (computeMLLR, TrainTools.cpp:788-866) for a batch of clients: kernels and the C ABI entry
// gmmiv_mllr_adapt_models (include/gmmiv.h).  DESIGN.md section 3.15.
//
// Per (client g, dimension p) one workgroup of k_mllr_solve:
//   accumulate   S = Xa^T diag(a) Xa on v_mfma_f64_16x16x4_f64, Xa = [1 | mean0 | m_.p] (C x (D + 2), padded to 16 NT columns),
//                a_j = N_gj / cov0_jp, m_jp = F_gjp / N_gj.  The leading (D+1)^2 block of S is G_p, row D + 1 is z_p.  Only the
//                lower-triangular 16 x 16 tiles are computed (10 of 16 at D = 60); the k range (the Gaussians) is dealt to the four
//                waves, whose partial tiles are summed in LDS in wave order -- no atomics, the same bits on every run.
//   factor       square-root-free Cholesky (G = L diag(d) L^T) on the leading D + 1 columns in LDS with row D + 1 carried along:
//                that row ends up as L^-1 z (the forward substitution).  One barrier per column.
//   solve        back substitution by one wave, one lane per unknown.
// A pivot that is not positive and finite marks the system failed; k_mllr_status then turns the client's transform into [0 | I].
#include <math.h>

#include "ctx.h"
#include "devutil.h"
#include "tv_kernels.h"

#define MLLR_MAX_DIM 62  // D + 2 columns of Xa fit four 16-column tiles
#define MLLR_LD 64       // row length of the padded tables Xp and Wp
#define MLLR_PLD 65      // row stride of the LDS panel (64 x 65 doubles = 33 280 bytes, static)
#define MLLR_STAGE 2048  // Gaussians whose (a, m) are staged in LDS at a time: 2 x 2048 doubles share the panel's storage
#define MLLR_CHUNK 8192  // clients per launch (grid.y)

// Xp [Cp x 64]: row j < C = [1, mean0_j, 0 ...]; rows C .. Cp - 1 (Cp = C rounded up to 16) are zero -- the k-steps of the accumulation
// read whole rows without a bound check
__global__ void k_mllr_pack(int C, int D, long Cp, const double *__restrict__ mean0, double *__restrict__ Xp)
{
    const long tot = Cp * MLLR_LD;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
        const long j = e / MLLR_LD;
        const int q = (int)(e - j * MLLR_LD);
        double v = 0.0;
        if (j < C) {
            if (q == 0) v = 1.0;
            else if (q <= D) v = mean0[j * D + (q - 1)];
        }
        Xp[e] = v;
    }
}

template <int NT>
__global__ __launch_bounds__(256, 2) void k_mllr_solve(int C, int D, const double *__restrict__ N, const double *__restrict__ F,
                                                       const double *__restrict__ cov0, const double *__restrict__ Xp, double *__restrict__ W,
                                                       double *__restrict__ Wp, int *__restrict__ flag)
{
    __shared__ double sh[MLLR_LD * MLLR_PLD]; // first the staged (a, m) of up to MLLR_STAGE Gaussians, then the panel
    const int p = blockIdx.x, g = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
    const double *Ng = N + (size_t)g * C, *Fg = F + (size_t)g * C * D + p, *cv = cov0 + p;
    constexpr int NACC = NT * (NT + 1) / 2;
    d4 acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
    bool ism[NT]; // this lane's column of tile t is column D + 1 of Xa: the ML mean of dimension p
#pragma unroll
    for (int t = 0; t < NT; ++t) ism[t] = 16 * t + lr == D + 1;

    for (int c0 = 0; c0 < C; c0 += MLLR_STAGE) {
        const int nc = C - c0 < MLLR_STAGE ? C - c0 : MLLR_STAGE;
        __syncthreads();
        for (int j = tid; j < MLLR_STAGE; j += 256) {
            double a = 0.0, m = 0.0;
            if (j < nc) {
                const double n = Ng[c0 + j];
                if (n != 0.0) { // an unoccupied Gaussian is skipped: its F row (0 / 0 as an ML mean) never enters
                    a = n / cv[(size_t)(c0 + j) * D];
                    m = Fg[(size_t)(c0 + j) * D] / n;
                }
            }
            sh[j] = a;
            sh[MLLR_STAGE + j] = m;
        }
        __syncthreads();
        const int nks = (nc + 3) / 4; // rows beyond C: a = 0, and Xp has zero rows up to the next multiple of 16
        for (int ks = wave; ks < nks; ks += 4) {
            const int jl = 4 * ks + lk;
            const double a = sh[jl], m = sh[MLLR_STAGE + jl];
            const double *xr = Xp + (size_t)(c0 + jl) * MLLR_LD + lr;
            double x[NT], b[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double v = xr[16 * t];
                x[t] = ism[t] ? m : v;
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) b[t] = a * x[t]; // one operand carries the weight
            int q = 0;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj <= ti; ++tj, ++q) acc[q] = MFMA_F64(x[ti], b[tj], acc[q]);
        }
    }
    // the four waves' partial sums, added in wave order
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
            int q = 0;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj <= ti; ++tj, ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int idx = (16 * ti + lk + 4 * r) * MLLR_PLD + 16 * tj + lr;
                        sh[idx] = w == 0 ? acc[q][r] : sh[idx] + acc[q][r];
                    }
        }
        __syncthreads();
    }
    // G = L diag(d) L^T, right-looking; column k keeps l_ik d_k, row n = D + 1 (z) is carried along and ends as L^-1 z
    const int n = D + 1;
    bool bad = false;
    for (int k = 0; k < n; ++k) {
        const double d = sh[k * MLLR_PLD + k];
        const bool ok = d > 0.0 && d < __builtin_inf();
        bad |= !ok;
        const double inv = ok ? 1.0 / d : 0.0;
        for (int i = k + 1 + (tid >> 4); i <= n; i += 16) {
            const double lik = sh[i * MLLR_PLD + k] * inv;
            for (int j = k + 1 + (tid & 15); j <= i && j < n; j += 16) sh[i * MLLR_PLD + j] -= lik * sh[j * MLLR_PLD + k];
        }
        __syncthreads();
    }
    // L^T w = diag(d)^-1 y: w_k = (y_k - sum_{i > k} (l_ik d_k) w_i) / d_k, lane k holds the running y_k
    if (wave == 0) {
        double r = lane < n ? sh[n * MLLR_PLD + lane] : 0.0, w = 0.0;
        for (int k = n - 1; k >= 0; --k) {
            const double wk = readlane_f64u(r, k) / sh[k * MLLR_PLD + k];
            if (lane == k) w = wk;
            if (lane < k) r -= sh[k * MLLR_PLD + lane] * wk;
        }
        const size_t row = (size_t)g * D + p;
        if (lane < n) W[row * n + lane] = w;
        Wp[row * MLLR_LD + lane] = lane < n ? w : 0.0;
        if (lane == 0) flag[row] = bad ? 1 : 0;
    }
}

// one workgroup per client: status = 1 + the first failed dimension (0: none); a failed client gets the identity transform [0 | I]
__global__ void k_mllr_status(int D, const int *__restrict__ flag, double *__restrict__ W, double *__restrict__ Wp, int *__restrict__ status)
{
    __shared__ int first;
    const int g = blockIdx.x, n = D + 1;
    if (threadIdx.x == 0) {
        int f = 0;
        for (int p = D - 1; p >= 0; --p)
            if (flag[(size_t)g * D + p]) f = p + 1;
        first = f;
        status[g] = f;
    }
    __syncthreads();
    if (!first) return;
    for (int e = threadIdx.x; e < D * MLLR_LD; e += blockDim.x) {
        const int p = e / MLLR_LD, q = e - p * MLLR_LD;
        const double v = q == p + 1 ? 1.0 : 0.0;
        Wp[(size_t)g * D * MLLR_LD + e] = v;
        if (q < n) W[((size_t)g * D + p) * n + q] = v;
    }
}

// a failed client keeps the a-priori means, bit for bit
__global__ void k_mllr_keep_means(long CD, const int *__restrict__ status, const double *__restrict__ mean0, double *__restrict__ mean_out)
{
    const int g = blockIdx.y;
    if (!status[g]) return;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < CD; e += (long)gridDim.x * blockDim.x) mean_out[(size_t)g * CD + e] = mean0[e];
}

static hipError_t launch_solve(hipStream_t st, int G, int C, int D, const double *N, const double *F, const double *cov0, const double *Xp, double *W,
                               double *Wp, int *flag)
{
    const dim3 grid((unsigned)D, (unsigned)G);
    switch ((D + 2 + 15) / 16) {
    case 1: k_mllr_solve<1><<<grid, 256, 0, st>>>(C, D, N, F, cov0, Xp, W, Wp, flag); break;
    case 2: k_mllr_solve<2><<<grid, 256, 0, st>>>(C, D, N, F, cov0, Xp, W, Wp, flag); break;
    case 3: k_mllr_solve<3><<<grid, 256, 0, st>>>(C, D, N, F, cov0, Xp, W, Wp, flag); break;
    default: k_mllr_solve<4><<<grid, 256, 0, st>>>(C, D, N, F, cov0, Xp, W, Wp, flag); break;
    }
    return hipGetLastError();
}

extern "C" int gmmiv_mllr_adapt_models(gmmiv_ctx *c, int G, int C, int D, const double *N, const double *F, const double *mean0, const double *cov0,
                                       double *W_out, double *mean_out, int32_t *status)
{
    if (!c || G < 0 || C <= 0 || D <= 0 || !N || !F || !mean0 || !cov0 || (!W_out && !mean_out)) {
        gmmiv_set_error("mllr_adapt_models: bad argument");
        return GMMIV_ERR_ARG;
    }
    if (D > MLLR_MAX_DIM) {
        gmmiv_set_error("mllr_adapt_models: vectSize %d not supported (max %d: the augmented system must fit one 64 x 64 panel)", D, MLLR_MAX_DIM);
        return GMMIV_ERR_UNSUPPORTED;
    }
    if (G == 0) return GMMIV_OK;
    GBIND(c);
    int rc;
    const size_t CD = (size_t)C * D, WN = (size_t)D * (D + 1);
    const long Cp = ((long)C + 15) / 16 * 16;
    const int GC = G < MLLR_CHUNK ? G : MLLR_CHUNK; // clients per launch
    DevIn<double> i_n, i_f, i_m0, i_c0;
    DevOut<double> o_w, o_m;
    DevOut<int32_t> o_s;
    if ((rc = i_n.init(c, WS_T2, N, (size_t)G * C)) || (rc = i_f.init(c, WS_T3, F, (size_t)G * CD)) || (rc = i_m0.init(c, WS_T6, mean0, CD)) ||
        (rc = i_c0.init(c, WS_T5, cov0, CD)) || (rc = o_w.init(c, WS_T8, W_out, (size_t)G * WN, false)) ||
        (rc = o_m.init(c, WS_T9, mean_out, (size_t)G * CD, false)) || (rc = o_s.init(c, WS_T4, status, (size_t)G, false)))
        return rc;
    void *xp, *wp, *fl, *wtmp = nullptr;
    if ((rc = c->scratch(WS_PART, (size_t)Cp * MLLR_LD * sizeof(double), &xp))) return rc;
    if ((rc = c->scratch(WS_AUX, (size_t)GC * D * MLLR_LD * sizeof(double), &wp))) return rc;
    if ((rc = c->scratch(WS_FLAGS, ((size_t)GC * D + (size_t)GC) * sizeof(int), &fl))) return rc;
    if (!W_out && (rc = c->scratch(WS_T7, (size_t)GC * WN * sizeof(double), &wtmp))) return rc;
    int *flag = (int *)fl, *stat_tmp = flag + (size_t)GC * D;
    c->t_begin("k_mllr_pack");
    {
        const long nb = (Cp * MLLR_LD + 255) / 256;
        k_mllr_pack<<<(unsigned)(nb > 4096 ? 4096 : nb), 256, 0, c->stream>>>(C, D, Cp, i_m0.d, (double *)xp);
        GCHK(hipGetLastError());
    }
    c->t_end();
    for (int g0 = 0; g0 < G; g0 += GC) { // every client is computed by its own workgroups: the cut changes no bit
        const int ng = G - g0 < GC ? G - g0 : GC;
        double *Wg = W_out ? o_w.d + (size_t)g0 * WN : (double *)wtmp;
        int *sg = status ? o_s.d + g0 : stat_tmp;
        c->t_begin("k_mllr_solve", g0 == 0);
        GCHK(launch_solve(c->stream, ng, C, D, i_n.d + (size_t)g0 * C, i_f.d + (size_t)g0 * CD, i_c0.d, (const double *)xp, Wg, (double *)wp, flag));
        c->t_end();
        k_mllr_status<<<ng, 64, 0, c->stream>>>(D, flag, Wg, (double *)wp, sg);
        GCHK(hipGetLastError());
        if (mean_out) {
            // mean_out[g] (C x D) = [1 | mean0] W_g^T; the padded tables make K even and every row 16-byte aligned (columns D + 1 .. of Wp are 0)
            const int K = (D + 2) & ~1;
            GCHK(tvk_dgemm(c->stream, false, true, C, D, K, 1.0, (const double *)xp, MLLR_LD, 0, (const double *)wp, MLLR_LD, (long)D * MLLR_LD, 0.0,
                           o_m.d + (size_t)g0 * CD, D, (long)CD, ng));
            const long nb = ((long)CD + 255) / 256;
            k_mllr_keep_means<<<dim3((unsigned)(nb > 64 ? 64 : nb), (unsigned)ng), 256, 0, c->stream>>>((long)CD, sg, i_m0.d, o_m.d + (size_t)g0 * CD);
            GCHK(hipGetLastError());
        }
    }
    if ((rc = o_w.finish()) || (rc = o_m.finish()) || (rc = o_s.finish())) return rc;
    // host inputs were staged with asynchronous copies from the caller's arrays
    if (!o_w.host && !o_m.host && !o_s.host &&
        !(gmmiv_is_device_ptr(N) && gmmiv_is_device_ptr(F) && gmmiv_is_device_ptr(mean0) && gmmiv_is_device_ptr(cov0)))
        GCHK(hipStreamSynchronize(c->stream));
    return GMMIV_OK;
}
