// feat_comp.hip -- kernels that REWRITE the resident frames from a GMM's per-frame posteriors (include/gmmiv.h, "model-based feature
// compensation"): k_feat_comp (o'_t = o_t - sum_c gamma_tc offset_c from the stored scaled likelihoods of k_llk_mfma<WZ>), its generic
// tail k_feat_sub, k_feat_map (feature mapping through the best Gaussian) and k_scatter_runs (the inverse of k_gather_runs).
#include "devutil.h"
#include "gmm_kernels.h"

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i4 __attribute__((ext_vector_type(4)));

template <typename T> struct feat_store;
template <> struct feat_store<float> { static __device__ __forceinline__ void put(void *p, long i, double v) { ((float *)p)[i] = (float)v; } };
template <> struct feat_store<double> { static __device__ __forceinline__ void put(void *p, long i, double v) { ((double *)p)[i] = v; } };

// ---- the offset matrix in MFMA B-operand order ----------------------------------------------------------------------------
// offP[((ct * 4 + s) * NT + nt) * 64 + lane] = offset[16 ct + 4 s + (lane >> 4)][16 nt + (lane & 15)], 0 outside [C x D]: one
// 512-byte line per (k-step, dimension tile), read by every workgroup in the same order (C x 16 NT doubles, 1 MB at 2048 x 60: it
// stays in L2 for the whole call).  blockIdx.y = slot of a chunk of models (gmmiv_feat_compensate_models): the offsets of model
// ids[slot], `stride` doubles apart (0 = one row for all), go to the slot's own table -- one launch for all models of the chunk, like
// k_pack_models.  ids == NULL: the single table of gmmiv_feat_compensate.
__global__ __launch_bounds__(256) void k_feat_pack_offset(const double *__restrict__ off, long stride, const int *__restrict__ ids, int C, int D, int nct,
                                                          int NT, double *__restrict__ offP)
{
    const long tot = (long)nct * 4 * NT * 64;
    if (ids) off += (size_t)ids[blockIdx.y] * stride;
    offP += (size_t)blockIdx.y * tot;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long)gridDim.x * 256) {
        const int lane = (int)(e & 63), nt = (int)((e >> 6) % NT);
        const long cs = (e >> 6) / NT; // ct * 4 + s
        const int g = (int)(cs * 4) + (lane >> 4), dim = 16 * nt + (lane & 15);
        offP[e] = (g < C && dim < D) ? off[(size_t)g * D + dim] : 0.0;
    }
}

// ---- k_feat_comp -----------------------------------------------------------------------------------------------------------
// out[t][i] = x[t][i] - sum_c gamma_tc offset[c][i] (JFAAcc::normalizeFeatures, AccumulateJFAStat.cpp:4653-4675) from the likelihood
// scratch k_llk_mfma<WZ> has just written: no [T x C] posterior array exists.  A stored block holds, in lane (i16, q) register r,
// Gaussian 16 ct + i16 of frame q + 4 r -- the C/D layout of v_mfma_f64_16x16x4, whose A and B operands both carry the NON-contracted
// index in i16.  The contraction over the Gaussians therefore needs the block transposed: each wave turns the four registers into
// posteriors (the one multiply e inv_t 2^(E - Efin), bit for bit gmmiv_occ's value), writes them into its own 16 x 17 LDS tile as
// [Gaussian][frame] and reads them back as A[m = frame][k = Gaussian 4 s + q].  B[k][n] = offset[16 ct + 4 s + q][16 nt + i16]
// comes pre-ordered from k_feat_pack_offset.  One wave owns FB 16-frame blocks (the B registers of a tile are reused FB times)
// and all NT dimension tiles of them; it walks the Gaussian tiles in order ct = 0 .. nct - 1, k-steps s = 0 .. 3 inside each: ONE
// fixed summation order per frame, whatever the frame's position, chunk or neighbours; nothing is accumulated with atomics and C is
// not split across waves.  The next tile's likelihoods, exponents and offsets are fetched while the current one is multiplied.
// A frame of likelihood 0 (inv_t == 0, include/gmmiv.h "degenerate inputs") is copied through.
// LDS: 4 waves x FB x 16 x 17 doubles (17 408 bytes at FB = 2), static; no workgroup barrier (every tile is private to its wave).
#ifndef FEAT_FB // (a second build with -DFEAT_FB=4, loaded through GMMIV_LIB_PATH, prices the other tile shape: DESIGN.md 3.12)
#define FEAT_FB 2
#endif
// SEG (a model per segment, gmmiv_feat_compensate_models): a wave's work item is an entry of `tiles` (gmmiv_plan_feat_tiles,
// include/gmmiv.h; frames relative to the chunk, n = the chunk's span) instead of the next FB blocks: at most FB consecutive blocks that
// hold rows [lo, hi) of ONE segment, and the packed offset is the table of the entry's model slot (offP + model * off_stride), so the
// B registers are still reused over the item's blocks.  A block that several segments share is visited once per segment; every row
// of it is computed on whatever the scratch holds and only rows of [lo, hi) are loaded from x and written.  The arithmetic of a row is
// the one above, whatever its row in the block: the bits of the plain kernel under that model.
template <int NT, typename XT, typename OT, bool SEG = false>
__global__ __launch_bounds__(256, FEAT_FB <= 2 ? 2 : 1) void k_feat_comp(const void *x, long ldx, long n, int D, int nct,
                                                      const double *__restrict__ zbuf, long nfb, const int *__restrict__ eit,
                                                      const double *__restrict__ inv, const int *__restrict__ efin,
                                                      const double *__restrict__ offP, void *out, long ldo,
                                                      const gmmiv_feat_tile *__restrict__ tiles, long ntiles, long off_stride)
{
    constexpr int FB = FEAT_FB;
    __shared__ double tile[4][FB][16 * 17];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i16 = lane & 15, q = lane >> 4;
    long fb0 = ((long)blockIdx.x * 4 + wave) * FB;
    long wlo = 0, whi = n; // the rows written
    if constexpr (SEG) {
        if ((long)blockIdx.x * 4 + wave >= ntiles) return; // (wave-uniform)
        const gmmiv_feat_tile me = tiles[(long)blockIdx.x * 4 + wave];
        fb0 = me.block; wlo = me.lo; whi = me.hi < n ? me.hi : n;
        offP += (size_t)me.model * off_stride;
    }
    if (fb0 * 16 >= whi) return; // (wave-uniform; the kernel has no workgroup barrier)
    long fbj[FB];
    double fs[FB][4];
    int ef[FB][4];
#pragma unroll
    for (int j = 0; j < FB; ++j) {
        fbj[j] = (fb0 + j) * 16 < whi ? fb0 + j : fb0; // a block past the end repeats the first one (never written)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long t = fbj[j] * 16 + q + 4 * r, tc = t < n ? t : n - 1;
            fs[j][r] = inv[tc];
            ef[j][r] = efin[tc];
        }
    }
    d4 acc[FB][NT];
#pragma unroll
    for (int j = 0; j < FB; ++j)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[j][nt] = d4{0.0, 0.0, 0.0, 0.0};

    d2 za[FB], zb[FB];
    i4 ev[FB];
    double b[4][NT];
    auto fetch = [&](int ct, d2 (&pa)[FB], d2 (&pb)[FB], i4 (&pe)[FB], double (&pw)[4][NT]) {
#pragma unroll
        for (int j = 0; j < FB; ++j) {
            const d2 *pz = (const d2 *)(zbuf + (((size_t)ct * nfb + fbj[j]) * 64 + lane) * 4);
            pa[j] = __builtin_nontemporal_load(pz);
            pb[j] = __builtin_nontemporal_load(pz + 1);
            pe[j] = *(const i4 *)(eit + (size_t)(ct >> 1) * (nfb * 16) + fbj[j] * 16 + 4 * q); // frames q + 4 r at slots 4 q + r (eit_slot)
        }
        const double *po = offP + (size_t)ct * 4 * NT * 64 + lane;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) pw[s][nt] = po[(s * NT + nt) * 64];
    };
    fetch(0, za, zb, ev, b);
    for (int ct = 0; ct < nct; ++ct) {
        d2 na[FB], nb[FB];
        i4 ne[FB];
        double nw[4][NT];
        fetch(ct + 1 < nct ? ct + 1 : ct, na, nb, ne, nw);
        double a[FB][4];
#pragma unroll
        for (int j = 0; j < FB; ++j) {
            const double e[4] = {za[j][0], za[j][1], zb[j][0], zb[j][1]};
            double *tl = tile[wave][j];
#pragma unroll
            for (int r = 0; r < 4; ++r) tl[i16 * 17 + q + 4 * r] = __builtin_ldexp(e[r] * fs[j][r], ev[j][r] - ef[j][r]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int j = 0; j < FB; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s) a[j][s] = tile[wave][j][(4 * s + q) * 17 + i16];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int j = 0; j < FB; ++j) acc[j][nt] = MFMA_F64(a[j][s], b[s][nt], acc[j][nt]);
#pragma unroll
        for (int j = 0; j < FB; ++j) { za[j] = na[j]; zb[j] = nb[j]; ev[j] = ne[j]; }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[s][nt] = nw[s][nt];
    }
    // lane (i16, q) register r of acc[j][nt]: frame q + 4 r of block j, dimension 16 nt + i16
#pragma unroll
    for (int j = 0; j < FB; ++j) {
        if ((fb0 + j) * 16 >= whi) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long t = (fb0 + j) * 16 + q + 4 * r;
            if (t >= whi || (SEG && t < wlo)) continue;
            const bool dead = !(fs[j][r] > 0.0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int dim = 16 * nt + i16;
                if (dim < D) {
                    const double xv = feat_load<XT>::raw(x, t * ldx + dim);
                    feat_store<OT>::put(out, t * ldo + dim, dead ? xv : xv - acc[j][nt][r]);
                }
            }
        }
    }
}

template <int NT>
static int launch_feat_comp(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, long n, int D, int nct, const gmmk_zview &z,
                            const double *offP, void *out, long ldo)
{
    const double *zbuf = z.zbuf, *inv = z.inv;
    const int *eit = z.eit, *efin = z.efin;
    const long nfb = z.nfb;
    const unsigned grid = (unsigned)((n + 64 * FEAT_FB - 1) / (64 * FEAT_FB));
    if (x_f64 && o_f64) k_feat_comp<NT, double, double><<<grid, 256, 0, st>>>(x, ldx, n, D, nct, zbuf, nfb, eit, inv, efin, offP, out, ldo, nullptr, 0, 0);
    else if (x_f64) k_feat_comp<NT, double, float><<<grid, 256, 0, st>>>(x, ldx, n, D, nct, zbuf, nfb, eit, inv, efin, offP, out, ldo, nullptr, 0, 0);
    else if (o_f64) k_feat_comp<NT, float, double><<<grid, 256, 0, st>>>(x, ldx, n, D, nct, zbuf, nfb, eit, inv, efin, offP, out, ldo, nullptr, 0, 0);
    else k_feat_comp<NT, float, float><<<grid, 256, 0, st>>>(x, ldx, n, D, nct, zbuf, nfb, eit, inv, efin, offP, out, ldo, nullptr, 0, 0);
    return (int)hipGetLastError();
}

// a model per segment: one wave per entry of the tile table (device array), four entries per workgroup
template <int NT>
static int launch_feat_comp_models(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, long n, int D, int nct, const gmmk_zview &z,
                                   const double *offP, long off_stride, const gmmiv_feat_tile *tiles, long ntiles, void *out, long ldo)
{
    const double *zbuf = z.zbuf, *inv = z.inv;
    const int *eit = z.eit, *efin = z.efin;
    const long nfb = z.nfb;
    const unsigned grid = (unsigned)((ntiles + 3) / 4);
#define FEAT_MM(XT, OT) k_feat_comp<NT, XT, OT, true><<<grid, 256, 0, st>>>(x, ldx, n, D, nct, zbuf, nfb, eit, inv, efin, offP, out, ldo, tiles, ntiles, off_stride)
    if (x_f64 && o_f64) FEAT_MM(double, double);
    else if (x_f64) FEAT_MM(double, float);
    else if (o_f64) FEAT_MM(float, double);
    else FEAT_MM(float, float);
#undef FEAT_MM
    return (int)hipGetLastError();
}

#ifdef FEAT_VALU // measurement builds only: the vector-ALU form (tools/variants/feat_comp_valu.hip) serves 49 <= D <= 60
#include "../../tools/variants/feat_comp_valu.hip"
#endif

size_t gmmk_feat_offset_doubles(int nct, int D) { return (size_t)nct * 4 * ((D + 15) / 16) * 64; }

int gmmk_feat_pack_offset(hipStream_t st, const double *off, int C, int D, int nct, double *offP)
{
    const int NT = (D + 15) / 16;
    const long tot = (long)nct * 4 * NT * 64;
#ifdef FEAT_VALU
    if (NT == 4) { k_feat_pack_offset_valu<<<1024, 256, 0, st>>>(off, C, D, nct, offP); return (int)hipGetLastError(); }
#endif
    k_feat_pack_offset<<<(unsigned)((tot + 255) / 256 < 1024 ? (tot + 255) / 256 : 1024), 256, 0, st>>>(off, 0, nullptr, C, D, nct, NT, offP);
    return (int)hipGetLastError();
}

// the offsets of models ids[0 .. n) (device list), `stride` doubles apart, into n tables gmmk_feat_offset_doubles apart: one launch
int gmmk_feat_pack_offsets(hipStream_t st, int n, const int *ids, const double *off, long stride, int C, int D, int nct, double *offP)
{
    if (n <= 0) return 0;
    const int NT = (D + 15) / 16;
    const long tot = (long)nct * 4 * NT * 64, nb = (tot + 255) / 256;
    k_feat_pack_offset<<<dim3((unsigned)(nb < 256 ? nb : 256), (unsigned)n), 256, 0, st>>>(off, stride, ids, C, D, nct, NT, offP);
    return (int)hipGetLastError();
}

int gmmk_feat_comp(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, long n, int D, int nct, const gmmk_zview &z,
                   const double *offP, void *out, long ldo)
{
    if (n <= 0) return 0;
#ifdef FEAT_VALU
    if ((D + 15) / 16 == 4) return launch_feat_comp_valu(st, x_f64, o_f64, x, ldx, n, D, nct, z.zbuf, z.nfb, z.eit, z.inv, z.efin, offP, out, ldo);
#endif
    switch ((D + 15) / 16) {
    case 1: return launch_feat_comp<1>(st, x_f64, o_f64, x, ldx, n, D, nct, z, offP, out, ldo);
    case 2: return launch_feat_comp<2>(st, x_f64, o_f64, x, ldx, n, D, nct, z, offP, out, ldo);
    case 3: return launch_feat_comp<3>(st, x_f64, o_f64, x, ldx, n, D, nct, z, offP, out, ldo);
    case 4: return launch_feat_comp<4>(st, x_f64, o_f64, x, ldx, n, D, nct, z, offP, out, ldo);
    }
    return -1; // D > 64: the caller takes the generic path
}

int gmmk_feat_blocks_per_tile(void) { return FEAT_FB; }

int gmmk_feat_comp_models(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, long n, int D, int nct, const gmmk_zview &z,
                          const double *offP, long off_stride, const gmmiv_feat_tile *tiles, long ntiles, void *out, long ldo)
{
    if (n <= 0 || ntiles <= 0) return 0;
    switch ((D + 15) / 16) {
    case 1: return launch_feat_comp_models<1>(st, x_f64, o_f64, x, ldx, n, D, nct, z, offP, off_stride, tiles, ntiles, out, ldo);
    case 2: return launch_feat_comp_models<2>(st, x_f64, o_f64, x, ldx, n, D, nct, z, offP, off_stride, tiles, ntiles, out, ldo);
    case 3: return launch_feat_comp_models<3>(st, x_f64, o_f64, x, ldx, n, D, nct, z, offP, off_stride, tiles, ntiles, out, ldo);
    case 4: return launch_feat_comp_models<4>(st, x_f64, o_f64, x, ldx, n, D, nct, z, offP, off_stride, tiles, ntiles, out, ldo);
    }
    return -1;
}

// ---- generic tail: out = x - P, P [n x D] = gamma offset from the fp64 GEMM; a frame whose log-sum is not finite is copied through ----
template <typename XT, typename OT>
__global__ __launch_bounds__(256) void k_feat_sub(const void *x, long ldx, long n, int D, const double *__restrict__ P,
                                                  const double *__restrict__ lse, void *out, long ldo)
{
    const long tot = n * D;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long)gridDim.x * 256) {
        const long t = e / D;
        const int d = (int)(e - t * D);
        const double l = lse[t], xv = feat_load<XT>::raw(x, t * ldx + d);
        const bool dead = !(__builtin_fabs(l) <= 1.0e300);
        feat_store<OT>::put(out, t * ldo + d, dead ? xv : xv - P[e]);
    }
}

int gmmk_feat_sub(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, long n, int D, const double *P, const double *lse, void *out, long ldo)
{
    if (n <= 0) return 0;
    const long nb = (n * D + 255) / 256;
    const unsigned grid = (unsigned)(nb < 65536 ? nb : 65536);
    if (x_f64 && o_f64) k_feat_sub<double, double><<<grid, 256, 0, st>>>(x, ldx, n, D, P, lse, out, ldo);
    else if (x_f64) k_feat_sub<double, float><<<grid, 256, 0, st>>>(x, ldx, n, D, P, lse, out, ldo);
    else if (o_f64) k_feat_sub<float, double><<<grid, 256, 0, st>>>(x, ldx, n, D, P, lse, out, ldo);
    else k_feat_sub<float, float><<<grid, 256, 0, st>>>(x, ldx, n, D, P, lse, out, ldo);
    return (int)hipGetLastError();
}

// ---- k_feat_map: mapDataToDistrib (GeneralTools.cpp:777-780) through the best Gaussian of every frame ----------------------
// data = sqrt(covMap / covData) * (data - meanData) + meanMap: a division, a square root, a subtraction, a product and a sum, each
// rounded on its own (no fused multiply-add: the reference's compiler emits none here).  The raw feature value is used: a NaN
// goes through the map like in the reference.
template <typename XT, typename OT>
__global__ __launch_bounds__(256) void k_feat_map(const void *x, long ldx, long T, int D, int C, const int *__restrict__ best,
                                                  const double *__restrict__ cd_mean, const double *__restrict__ cd_cov,
                                                  const double *__restrict__ ci_mean, const double *__restrict__ ci_cov,
                                                  void *out, long ldo)
{
#pragma clang fp contract(off)
    const long tot = T * D;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long)gridDim.x * 256) {
        const long t = e / D;
        const int d = (int)(e - t * D);
        const int b = best[t];
        const size_t m = (size_t)((unsigned)b < (unsigned)C ? b : 0) * D + d; // (an index outside the model is never dereferenced)
        const double xv = feat_load<XT>::raw(x, t * ldx + d);
        const double sc = __builtin_sqrt(ci_cov[m] / cd_cov[m]);
        const double df = xv - cd_mean[m];
        const double pr = sc * df;
        feat_store<OT>::put(out, t * ldo + d, pr + ci_mean[m]);
    }
}

int gmmk_feat_map(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, long T, int D, int C, const int *best, const double *cd_mean,
                  const double *cd_cov, const double *ci_mean, const double *ci_cov, void *out, long ldo)
{
    if (T <= 0) return 0;
    const long nb = (T * D + 255) / 256;
    const unsigned grid = (unsigned)(nb < 65536 ? nb : 65536);
    if (x_f64 && o_f64) k_feat_map<double, double><<<grid, 256, 0, st>>>(x, ldx, T, D, C, best, cd_mean, cd_cov, ci_mean, ci_cov, out, ldo);
    else if (x_f64) k_feat_map<double, float><<<grid, 256, 0, st>>>(x, ldx, T, D, C, best, cd_mean, cd_cov, ci_mean, ci_cov, out, ldo);
    else if (o_f64) k_feat_map<float, double><<<grid, 256, 0, st>>>(x, ldx, T, D, C, best, cd_mean, cd_cov, ci_mean, ci_cov, out, ldo);
    else k_feat_map<float, float><<<grid, 256, 0, st>>>(x, ldx, T, D, C, best, cd_mean, cd_cov, ci_mean, ci_cov, out, ldo);
    return (int)hipGetLastError();
}

// ---- k_scatter_runs: the inverse of k_gather_runs -- rows [dst, dst + len) of `in` (ld = D) go back to frames [src, src + len) of x.
// One wave per run, 16 bytes per lane when both sides allow it.
template <typename XT>
__global__ __launch_bounds__(256) void k_scatter_runs(XT *__restrict__ x, long ldx, int D, const long *__restrict__ runs, long nrun,
                                                      const XT *__restrict__ in)
{
    const int lane = threadIdx.x & 63;
    const long nw = (long)gridDim.x * (blockDim.x >> 6);
    constexpr int V = 16 / (int)sizeof(XT);
    for (long r = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < nrun; r += nw) {
        const long src = runs[3 * r], dst = runs[3 * r + 1], len = runs[3 * r + 2];
        if (ldx == D) {
            XT *d = x + src * D;
            const XT *s = in + dst * D;
            const long tot = len * D;
            if ((((size_t)s | (size_t)d) & 15) == 0) {
                const long nv = tot / V;
                for (long e = lane; e < nv; e += 64) ((float4 *)d)[e] = ((const float4 *)s)[e];
                for (long e = nv * V + lane; e < tot; e += 64) d[e] = s[e];
            } else
                for (long e = lane; e < tot; e += 64) d[e] = s[e];
        } else
            for (long i = 0; i < len; ++i)
                for (int e = lane; e < D; e += 64) x[(src + i) * ldx + e] = in[(dst + i) * D + e];
    }
}

int gmmk_scatter_runs(hipStream_t st, int x_f64, void *x, long ldx, int D, const long *runs, long nrun, const void *in)
{
    if (nrun <= 0) return 0;
    const long nb = (nrun + 3) / 4;
    const unsigned blocks = (unsigned)(nb < 65536 ? nb : 65536);
    if (x_f64) k_scatter_runs<double><<<blocks, 256, 0, st>>>((double *)x, ldx, D, runs, nrun, (const double *)in);
    else k_scatter_runs<float><<<blocks, 256, 0, st>>>((float *)x, ldx, D, runs, nrun, (const float *)in);
    return (int)hipGetLastError();
}
