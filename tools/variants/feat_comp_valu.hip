// tools/variants/feat_comp_valu.hip -- the vector-ALU form of k_feat_comp, measured slower than the MFMA form and
// kept as a record.  NOT part of libgmmiv.so: lia_ral_amd/csrc/feat_comp.hip includes this file only when built with -DFEAT_VALU, and
// then serves 49 <= D <= 60 with it (the shape of the measurement); load that build through GMMIV_LIB_PATH.
//
// No transpose: lane (i16, q) keeps the share of ITS Gaussian 16 ct + i16 for its four frames q + 4 r.  Four waves per 16-frame block,
// wave w owns dimensions 15 w .. 15 w + 14: 60 accumulators per lane, per Gaussian tile 4 posteriors x 15 offsets = 60 fused
// multiply-adds against 15 offset loads (each offset value is used 4 times; the MFMA form uses it 16 times per instruction).  The 16
// partial sums of a (frame, dimension) meet at the end through four DPP row rotations in a fixed order.
__global__ __launch_bounds__(256) void k_feat_pack_offset_valu(const double *__restrict__ off, int C, int D, int nct, double *__restrict__ offV)
{
    const long tot = (long)nct * 4 * 15 * 16; // offV[((ct * 4 + w) * 15 + k) * 16 + i16] = offset[16 ct + i16][15 w + k]
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long)gridDim.x * 256) {
        const int i16 = (int)(e & 15), k = (int)((e >> 4) % 15);
        const long cw = (e >> 4) / 15;
        const int g = (int)(cw >> 2) * 16 + i16, dim = 15 * (int)(cw & 3) + k;
        offV[e] = (g < C && dim < D) ? off[(size_t)g * D + dim] : 0.0;
    }
}

template <typename XT, typename OT>
__global__ __launch_bounds__(256, 2) void k_feat_comp_valu(const void *x, long ldx, long n, int D, int nct, const double *__restrict__ zbuf, long nfb,
                                                           const int *__restrict__ eit, const double *__restrict__ inv,
                                                           const int *__restrict__ efin, const double *__restrict__ offV, void *out, long ldo)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i16 = lane & 15, q = lane >> 4;
    const long fb = blockIdx.x;
    double fs[4];
    int ef[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long t = fb * 16 + q + 4 * r, tc = t < n ? t : n - 1;
        fs[r] = inv[tc];
        ef[r] = efin[tc];
    }
    double acc[4][15];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 15; ++k) acc[r][k] = 0.0;
    d2 za, zb;
    i4 ev;
    double b[15];
    auto fetch = [&](int ct, d2 &pa, d2 &pb, i4 &pe, double (&pw)[15]) {
        const d2 *pz = (const d2 *)(zbuf + (((size_t)ct * nfb + fb) * 64 + lane) * 4);
        pa = pz[0];
        pb = pz[1];
        pe = *(const i4 *)(eit + (size_t)(ct >> 1) * (nfb * 16) + fb * 16 + 4 * q);
        const double *po = offV + ((size_t)ct * 4 + wave) * 15 * 16 + i16;
#pragma unroll
        for (int k = 0; k < 15; ++k) pw[k] = po[k * 16];
    };
    fetch(0, za, zb, ev, b);
    for (int ct = 0; ct < nct; ++ct) {
        d2 na, nb;
        i4 ne;
        double nw[15];
        fetch(ct + 1 < nct ? ct + 1 : ct, na, nb, ne, nw);
        const double e[4] = {za[0], za[1], zb[0], zb[1]};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double g = __builtin_ldexp(e[r] * fs[r], ev[r] - ef[r]);
#pragma unroll
            for (int k = 0; k < 15; ++k) acc[r][k] = __builtin_fma(g, b[k], acc[r][k]);
        }
        za = na; zb = nb; ev = ne;
#pragma unroll
        for (int k = 0; k < 15; ++k) b[k] = nw[k];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long t = fb * 16 + q + 4 * r;
        const bool dead = !(fs[r] > 0.0);
#pragma unroll
        for (int k = 0; k < 15; ++k) {
            double v = acc[r][k];
            v += dpp_f64_0x128(v); v += dpp_f64_0x124(v); v += dpp_f64_0x122(v); v += dpp_f64_0x121(v);
            const int dim = 15 * wave + k;
            if (i16 == k && t < n && dim < D) {
                const double xv = feat_load<XT>::raw(x, t * ldx + dim);
                feat_store<OT>::put(out, t * ldo + dim, dead ? xv : xv - v);
            }
        }
    }
}

static int launch_feat_comp_valu(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, long n, int D, int nct, const double *zbuf, long nfb,
                                 const int *eit, const double *inv, const int *efin, const double *offV, void *out, long ldo)
{
    const unsigned grid = (unsigned)((n + 15) / 16);
    if (x_f64 && o_f64) k_feat_comp_valu<double, double><<<grid, 256, 0, st>>>(x, ldx, n, D, nct, zbuf, nfb, eit, inv, efin, offV, out, ldo);
    else if (x_f64) k_feat_comp_valu<double, float><<<grid, 256, 0, st>>>(x, ldx, n, D, nct, zbuf, nfb, eit, inv, efin, offV, out, ldo);
    else if (o_f64) k_feat_comp_valu<float, double><<<grid, 256, 0, st>>>(x, ldx, n, D, nct, zbuf, nfb, eit, inv, efin, offV, out, ldo);
    else k_feat_comp_valu<float, float><<<grid, 256, 0, st>>>(x, ldx, n, D, nct, zbuf, nfb, eit, inv, efin, offV, out, ldo);
    return (int)hipGetLastError();
}
