// capi_gmm.hip -- C ABI (include/gmmiv.h): the entry points that evaluate a model on frames -- likelihood, top-C, posteriors, EM and the
// Baum-Welch N / F rows.  (Context and model handle: capi_ctx.hip; frames read or rewritten: capi_feat.hip.)
#include <math.h>
#include <stdlib.h>

#include "ctx.h"
#include "gmm_kernels.h"
#include "tv_kernels.h"
#include "capi_gmm_util.h"

// ---- helpers of the entry points below (count_unusable, run_lse, generic_gamma_gemm: declared in capi_gmm_util.h) ----
namespace {
// The outputs of DETERMINE_TOP_DISTRIBS on the device: idx / lk [T x ctop], the others [T]; every one but idx may be absent (run_lse
// asks for llk alone).  at(c0) = the outputs of the frames from c0 on: the one place that computes the offsets of a frame chunk.
struct TopOut {
    int *idx;
    double *lk, *nlk, *nllk, *nw, *llk;
    int ctop;
    template <typename V> static V *from(V *p, size_t off) { return p ? p + off : nullptr; }
    TopOut at(int64_t c0) const { return TopOut{from(idx, (size_t)c0 * ctop), from(lk, (size_t)c0 * ctop), from(nlk, c0), from(nllk, c0), from(nw, c0), from(llk, c0), ctop}; }
};
} // namespace

// ---- degenerate inputs (include/gmmiv.h) ----
// Kind (1) frames are not removed from a call: every kernel reads such a value as GMMIV_UNUSABLE_READ_AS (devutil.h, feat_sane), which makes the
// frame a zero-likelihood frame on the device.  What is left for the host side is the COUNT ("screened_frames"): one pass over x that
// flags the frames and adds their number to a device counter -- enqueued, never read back here (option "assume_finite" 1 skips it;
// results do not depend on it).
int count_unusable(gmmiv_ctx *c, const XView &xv, int dt, int64_t T, int D)
{
    if (c->assume_finite || T <= 0) return GMMIV_OK;
    void *p;
    int rc;
    const size_t fbytes = ((size_t)T + 15) / 16 * 16;
    if ((rc = c->scratch(WS_GFLAG, fbytes + 16, &p))) return rc;
    unsigned char *flag = (unsigned char *)p;
    GCHK(hipMemsetAsync(flag, 0, fbytes + 16, c->stream));
    GCHK(gmmk_flag_frames(c->stream, dt == GMMIV_F64, xv.d, T, xv.ldx, D, flag, (int *)(flag + fbytes)));
    GCHK(gmmk_count_flags(c->stream, flag, (long)T, c->d_screened));
    return GMMIV_OK;
}

// DETERMINE_TOP_DISTRIBS by the any-shape kernel (k_topc_determine_big), frames in chunks whose logit rows fit 1 GiB of scratch
static int topc_big(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t T, int complete, double lo, double hi, const TopOut &o)
{
    const int ctop = o.ctop;
    if (T <= 0) return GMMIV_OK;
    int64_t per = (int64_t)(((size_t)1 << 30) / ((size_t)g->Cp64 * sizeof(double))) / 4 * 4;
    if (per < 4) per = 4;
    if (per > T) per = (T + 3) / 4 * 4;
    void *zs;
    int rc = c->scratch(WS_Z, gmmk_topc_big_scratch_doubles((long)per, g->Cp64) * sizeof(double), &zs);
    if (rc) return rc;
    for (int64_t c0 = 0; c0 < T; c0 += per) { // one timed launch per chunk, like the other chunked paths (kernel_launches counts them)
        const int64_t n = T - c0 < per ? T - c0 : per;
        c->t_begin("k_topc_determine", c0 == 0);
        const TopOut oc = o.at(c0);
        int krc = gmmk_topc_determine_big(c->stream, dt == GMMIV_F64, gmmiv_x_at(xv, dt, c0), (long)n, xv.ldx, g->D, g->C, g->Cp64, g->meanT, g->ivT, g->lwc,
                                          g->w, ctop, complete, lo, hi, oc.idx, oc.lk, oc.nlk, oc.nllk, oc.nw, oc.llk, (double *)zs);
        c->t_end();
        if (krc == -1) { gmmiv_set_error("vectSize %d exceeds the generic kernels' bound", g->D); return GMMIV_ERR_UNSUPPORTED; }
        if (krc == -2) { gmmiv_set_error("topDistribsCount %d outside 1 .. mixtureDistribCount %d", ctop, g->C); return GMMIV_ERR_ARG; }
        GCHK(krc);
    }
    return GMMIV_OK;
}

int run_lse(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t T, double **lse_out)
{
    void *lse;
    int rc = c->scratch(WS_LSE, (size_t)(T > 0 ? T : 1) * sizeof(double), &lse);
    if (rc) return rc;
    if (g->KS == GMMK_KS_GENERIC) { // no MFMA instantiation: log sum_c w_c lk_c in the direct form (the top-1 pass of the any-shape kernel, COMPLETE)
        if ((rc = topc_big(c, g, xv, dt, T, 1, -INFINITY, INFINITY, TopOut{nullptr, nullptr, nullptr, nullptr, nullptr, (double *)lse, 1}))) return rc;
        GCHK(count_dead(c, (const double *)lse, T));
        *lse_out = (double *)lse;
        return GMMIV_OK;
    }
    c->t_begin("k_llk_mfma");
    GCHK(gmmk_llk(c->stream, g->KS, dt == GMMIV_F64, xv.d, T, xv.ldx, g->D, g->Pt, g->nct, (double *)lse, (int)(c->use_glds | (c->dbg << 8)), (int)c->wg_waves));
    c->t_end();
    GCHK(count_dead(c, (const double *)lse, T)); // every caller of run_lse is a statistics / likelihood entry point
    *lse_out = (double *)lse;
    return GMMIV_OK;
}

// ---- statistics of a model WITHOUT an MFMA instantiation (vectSize > 80): gamma[t][c] = exp(z_tc - lse_t) by the direct-form VALU
// kernel (k_posteriors), then S[C x NC] (+)= gamma^T [x | 1 | x^2 | 0] on the fp64 GEMM (k_dgemm), frames in chunks whose posterior
// block fits 512 MiB.  S: sum_t g x | sum_t g | sum_t g x^2.  The same sums as MixtureStat::computeAndAccumulateEM
// (AccumulateStat.cpp:103-152) / TVAcc::computeAndAccumulateTVStat (AccumulateTVStat.cpp:332-348), any vectSize.
int generic_gamma_gemm(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t t0, int64_t n, const double *lse, bool sq, int NC,
                       double *S)
{
    int rc;
    int64_t per = (int64_t)(((size_t)512 << 20) / ((size_t)g->C * sizeof(double)));
    if (per < 64) per = 64;
    per = per / 2 * 2; // an even K keeps the aligned GEMM instantiation
    void *gam, *xa;
    const int64_t first = n < per ? n : per;
    if ((rc = c->scratch(WS_Z, (size_t)(first > 0 ? first : 1) * g->C * sizeof(double), &gam))) return rc;
    if ((rc = c->scratch(WS_INV, (size_t)(first > 0 ? first : 1) * NC * sizeof(double), &xa))) return rc;
    if (n <= 0) { GCHK(hipMemsetAsync(S, 0, (size_t)g->C * NC * sizeof(double), c->stream)); return GMMIV_OK; }
    for (int64_t b = 0; b < n; b += per) {
        const int64_t m = n - b < per ? n - b : per;
        c->t_begin("k_posteriors", b == 0);
        GCHK(gmmk_posteriors(c->stream, dt == GMMIV_F64, gmmiv_x_at(xv, dt, t0 + b), (long)m, xv.ldx, g->D, g->C, g->Cp64, g->meanT, g->ivT, g->lwc, lse + t0 + b,
                             (double *)gam));
        c->t_end();
        GCHK(gmmk_build_xa(c->stream, dt == GMMIV_F64, gmmiv_x_at(xv, dt, t0 + b), xv.ldx, g->D, (long)m, sq ? 1 : 0, NC, (double *)xa));
        GCHK(tvk_dgemm(c->stream, true, false, g->C, NC, (int)m, 1.0, (const double *)gam, g->C, 0, (const double *)xa, NC, 0, b == 0 ? 0.0 : 1.0, S, NC, 0, 1));
    }
    return GMMIV_OK;
}

// ---- the three paths of gmmiv_llk_determine_top (which one runs: the entry point) ----
// Fused path (default): the candidates are collected in the epilogue of the MFMA log-likelihood kernel itself (k_llk_mfma<TC>: 4 KB of
// candidate records per frame instead of the 16 KB likelihood round trip) and ranked by k_topc_rank.  *done = false: a frame
// overflowed its list or failed the margin check in numbers (or the shape has no instantiation), the other paths redo the call.
static size_t fused_frame_bytes() { return (size_t)gmmk_topc_cap() * 16; }

// frames per chunk whose candidate records fit the "z_scratch_mb" budget (multiple of 256), 0 when not even one workgroup's do
static int64_t fused_chunk_frames(const gmmiv_ctx *c)
{
    size_t budget = (size_t)(c->z_scratch_mb > 0 ? c->z_scratch_mb : 0) << 20;
    if (c->total_mem && budget > c->total_mem / 4) budget = c->total_mem / 4;
    const int64_t Tf = (int64_t)(budget / fused_frame_bytes() / 1.2) / 256 * 256;
    return Tf >= 256 ? Tf : 0;
}

static int top_fused(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t T, int complete, double min_llk, double max_llk,
                     const TopOut &o, int64_t Tf, bool *done)
{
    int rc;
    const int ctop = o.ctop;
    const int64_t nalloc = T < Tf ? (T + 255) / 256 * 256 : Tf;
    const int stats = getenv("GMMIV_TOPC_STATS") != nullptr;
    void *cand, *cnt, *th, *sl, *flg, *redo;
    if ((rc = c->scratch(WS_Z, (size_t)nalloc * fused_frame_bytes(), &cand))) return rc;
    if ((rc = c->scratch(WS_EIT, (size_t)nalloc * sizeof(int), &cnt))) return rc;
    if ((rc = c->scratch(WS_INV, (size_t)nalloc * (sizeof(double) + sizeof(int)), &sl))) return rc;
    if ((rc = c->scratch(WS_LSE, (size_t)nalloc * sizeof(double), &th))) return rc;
    if ((rc = c->scratch(WS_FLAGS, 64, &flg))) return rc;
    int *efin = (int *)((double *)sl + nalloc);
    if ((rc = c->scratch(WS_SEG, (size_t)nalloc * 2 * sizeof(long), &redo))) return rc; // second half: the frames k_topc_rank2 hands to k_topc_rank
    int krc = 0;
    bool whole = false; // too many frames failed the fused path: the other paths redo the call
    // one chunk [c0, c0 + n): k_llk_mfma<TC> + k_topc_rank on the context's stream, flags read back, failed frames redone
    for (int64_t c0 = 0; c0 < T; c0 += Tf) {
        const int64_t n = (T - c0) < Tf ? (T - c0) : Tf;
        const TopOut oc = o.at(c0);
        GCHK(hipMemsetAsync(flg, 0, 64, c->stream));
        c->t_begin("k_llk_mfma", c0 == 0);
        krc = gmmk_llk_topc(c->stream, g->KS, dt == GMMIV_F64, gmmiv_x_at(xv, dt, c0), n, xv.ldx, g->D, g->Pt, g->nct, (int)c->use_glds,
                            ctop, (double *)cand, (int *)cnt, (double *)th, (double *)sl, efin);
        c->t_end();
        if (krc) break;
        c->t_begin("k_topc_rank", c0 == 0);
        krc = gmmk_topc_rank(c->stream, dt == GMMIV_F64, gmmiv_x_at(xv, dt, c0), n, xv.ldx, g->D, g->C, (const double *)cand, (const int *)cnt,
                             (const double *)th, (const double *)sl, efin, g->mean, g->iv, g->lwc, g->w, ctop, complete,
                             min_llk, max_llk, oc.idx, oc.lk, oc.nlk, oc.nllk, oc.nw, oc.llk, (int *)flg, (long *)redo,
                             stats | (c->topc_rank_direct ? 2 : 0) | (c->topc_rank2 ? 0 : 4), (long *)redo + nalloc);
        c->t_end();
        if (krc) break;
        int hf[16] = {0};
        GCHK(hipMemcpyAsync(hf, flg, 64, hipMemcpyDeviceToHost, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
        if (stats)
            fprintf(stderr, "topc fused: %ld frames, redone %d | overflow %d, survivors > 64: %d, < ctop: %d, margin %d | list max %d mean %.1f | survivors max %d mean %.1f\n",
                    (long)n, hf[0], hf[1], hf[2], hf[3], hf[4], hf[5], (double)*(unsigned long long *)&hf[6] / (double)n, hf[8],
                    (double)*(unsigned long long *)&hf[10] / (double)n);
        const int64_t nr = hf[0];
        c->topc_fallbacks += nr;
        if (nr == 0) continue;
        if (nr > n / 8 + 64) { whole = true; break; }
        // the few frames whose list overflowed / piled up / failed the margin: direct form for every Gaussian
        // (k_topc_determine) on a gathered copy, results scattered back
        void *gx, *t_idx, *t_d;
        if ((rc = c->scratch(WS_PART, (size_t)nr * g->D * gmmiv_esize(dt), &gx))) return rc;
        if ((rc = c->scratch(WS_T6, (size_t)nr * ctop * sizeof(int), &t_idx))) return rc;
        if ((rc = c->scratch(WS_T7, (size_t)nr * (ctop + 4) * sizeof(double), &t_d))) return rc;
        double *t_lk = (double *)t_d, *t_nlk = t_lk + (size_t)nr * ctop, *t_nllk = t_nlk + nr, *t_nw = t_nllk + nr, *t_llk = t_nw + nr;
        GCHK(gmmk_gather_frames(c->stream, dt == GMMIV_F64, gmmiv_x_at(xv, dt, c0), xv.ldx, g->D, (const long *)redo, nr, gx));
        c->t_begin("k_topc_determine", c0 == 0);
        GCHK(gmmk_topc_determine(c->stream, dt == GMMIV_F64, gx, nr, g->D, g->D, g->C, g->Cp64, g->meanT, g->ivT, g->lwc, g->w, ctop,
                                 complete, min_llk, max_llk, (int *)t_idx, t_lk, t_nlk, t_nllk, t_nw, t_llk));
        c->t_end();
        GCHK(gmmk_topc_scatter(c->stream, nr, ctop, (const long *)redo, (const int *)t_idx, t_lk, t_nlk, t_nllk, t_nw, t_llk, oc.idx, oc.lk, oc.nlk,
                               oc.nllk, oc.nw, oc.llk));
    }
    if (krc > 0) GCHK(krc);
    *done = krc == 0 && !whole;
    return GMMIV_OK;
}

// Stored-likelihood path: all logits on the matrix cores (k_llk_mfma<WZ>, the EM path's kernel), selection on the stored likelihoods,
// the direct form only for the candidates (topc_z.hip).  *done = false in the (never observed) case that a non-candidate comes within
// 1e-6 of the selected set: the direct path redoes the call.
static int top_from_z(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t T, int complete, double min_llk, double max_llk,
                      const TopOut &o, int64_t Tc, bool *done)
{
    int rc;
    gmmk_zview z;
    double *lse;
    void *flg;
    if ((rc = gmmiv_z_reserve(c, g->nct, T < Tc ? T : Tc, true, &z, &lse))) return rc;
    if ((rc = c->scratch(WS_FLAGS, 64, &flg))) return rc;
    GCHK(hipMemsetAsync(flg, 0, sizeof(int), c->stream));
    for (int64_t c0 = 0; c0 < T; c0 += Tc) {
        const int64_t n = (T - c0) < Tc ? (T - c0) : Tc;
        const TopOut oc = o.at(c0);
        if ((rc = llk_z_run(c, g, xv, dt, c0, n, lse, z, c0 == 0))) return rc; // (this entry point does not count zero-likelihood frames)
        c->t_begin("k_topc_from_z", c0 == 0);
        GCHK(gmmk_topc_from_z(c->stream, dt == GMMIV_F64, gmmiv_x_at(xv, dt, c0), n, xv.ldx, g->D, g->C, g->nct, z, g->mean, g->iv, g->lwc, g->w,
                              o.ctop, complete, min_llk, max_llk, oc.idx, oc.lk, oc.nlk, oc.nllk, oc.nw, oc.llk, (int *)flg));
        c->t_end();
    }
    int hflag = 0;
    GCHK(hipMemcpyAsync(&hflag, flg, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    GCHK(hipStreamSynchronize(c->stream));
    *done = hflag == 0;
    return GMMIV_OK;
}

// Direct path: every logit in the reference's direct form on the vector ALUs -- the LDS selection kernel, or the any-shape kernel for
// topDistribsCount > 64 and for a model whose logit rows do not fit LDS (about 4 700 Gaussians)
static int top_direct(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t T, int complete, double min_llk, double max_llk,
                      const TopOut &o)
{
    if (o.ctop > 64 || !gmmk_topc_frames_per_block(g->Cp64, g->D)) return topc_big(c, g, xv, dt, T, complete, min_llk, max_llk, o);
    c->t_begin("k_topc_determine");
    GCHK(gmmk_topc_determine(c->stream, dt == GMMIV_F64, xv.d, T, xv.ldx, g->D, g->C, g->Cp64, g->meanT, g->ivT, g->lwc,
                             g->w, o.ctop, complete, min_llk, max_llk, o.idx, o.lk, o.nlk, o.nllk, o.nw, o.llk));
    c->t_end();
    return GMMIV_OK;
}

extern "C" {

// ---- LLK ---------------------------------------------------------------------------------
int gmmiv_llk(gmmiv_ctx *c, const gmmiv_gmm *g, const void *x, int dt, int64_t T, int64_t ldx, double min_llk,
              double max_llk, double *llk_out, double *sums)
{
    int rc = check_model(c, g);
    if (rc) return rc;
    if (T < 0) { gmmiv_set_error("llk: T < 0"); return GMMIV_ERR_ARG; }
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, g->D))) return rc;
    if ((rc = count_unusable(c, xv, dt, T, g->D))) return rc;
    double *lse;
    if ((rc = run_lse(c, g, xv, dt, T, &lse))) return rc;
    DevOut<double> o_llk, o_sum;
    if ((rc = o_llk.init(c, WS_T0, llk_out, (size_t)T, false))) return rc;
    if ((rc = o_sum.init(c, WS_T1, sums, 2, true))) return rc;
    void *part;
    if ((rc = c->scratch(WS_SMALL, 3 * 256 * sizeof(double), &part))) return rc;
    GCHK(gmmk_llk_finalize(c->stream, lse, T, min_llk, max_llk, o_llk.d, (double *)part, 1.0, 0.0,
                           sums ? o_sum.d : nullptr, nullptr));
    if (sums) GCHK(gmmk_add_scalar(c->stream, o_sum.d + 1, (double)T));
    if ((rc = o_llk.finish())) return rc;
    return o_sum.finish();
}

int gmmiv_llk_determine_top(gmmiv_ctx *c, const gmmiv_gmm *g, const void *x, int dt, int64_t T, int64_t ldx, int ctop,
                            int mode, double min_llk, double max_llk, int32_t *idx, double *lk, double *nontop_lk,
                            double *nontop_llk, double *nontop_w, double *llk_out)
{
    int rc = check_model(c, g);
    if (rc) return rc;
    if (T < 0 || !idx || ctop <= 0) { gmmiv_set_error("determine_top: bad argument"); return GMMIV_ERR_ARG; }
    // no silent clamp: the stride of idx / lk is the caller's ctop, so a caller that asks for more than the model has must
    // clamp on its side (liagpu::computeTestLLR and the Python binding do) -- otherwise its buffers and use_top disagree
    if (ctop > g->C) { gmmiv_set_error("determine_top: topDistribsCount %d exceeds mixtureDistribCount %d (clamp it at the call site)", ctop, g->C); return GMMIV_ERR_ARG; }
    // (topDistribsCount > 64, or a model whose logit rows do not fit LDS -- about 4 700 Gaussians --, go through the any-shape kernel of
    //  top_direct: mixtureDistribCount / vectSize / topDistribsCount are free keys of the reference, ComputeTest.cpp:129-215)
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, g->D))) return rc;
    if ((rc = count_unusable(c, xv, dt, T, g->D))) return rc;
    DevOut<int32_t> o_idx;
    DevOut<double> o_lk, o_nlk, o_nllk, o_nw, o_llk;
    if ((rc = o_idx.init(c, WS_T0, idx, (size_t)T * ctop, false))) return rc;
    if ((rc = o_lk.init(c, WS_T1, lk, (size_t)T * ctop, false))) return rc;
    if ((rc = o_nlk.init(c, WS_T2, nontop_lk, (size_t)T, false))) return rc;
    if ((rc = o_nllk.init(c, WS_T3, nontop_llk, (size_t)T, false))) return rc;
    if ((rc = o_nw.init(c, WS_T4, nontop_w, (size_t)T, false))) return rc;
    if ((rc = o_llk.init(c, WS_T5, llk_out, (size_t)T, false))) return rc;
    const TopOut o{o_idx.d, o_lk.d, o_nlk.d, o_nllk.d, o_nw.d, o_llk.d, ctop};
    const int complete = mode == GMMIV_TOP_COMPLETE;
    bool done = false;
    // fused (default) -> stored likelihoods -> direct: each path hands a call it cannot finish to the next one
    const int64_t Tf = (c->topc_fused && T > 0 && ctop <= 16 && g->C <= 2048 && g->D <= 64 && g->KS <= 15 && c->wg_waves == 8) ? fused_chunk_frames(c) : 0;
    if (Tf > 0 && (rc = top_fused(c, g, xv, dt, T, complete, min_llk, max_llk, o, Tf, &done))) return rc;
    const int64_t Tc = (!done && c->topc_z) ? z_chunk_frames(c, g) : 0;
    if (Tc > 0 && T > 0 && ctop + 4 <= 64 && gmmk_topc_z_lds(g->nct, g->D) && (rc = top_from_z(c, g, xv, dt, T, complete, min_llk, max_llk, o, Tc, &done))) return rc;
    if (!done && (rc = top_direct(c, g, xv, dt, T, complete, min_llk, max_llk, o))) return rc;
    if ((rc = o_idx.finish())) return rc;
    if ((rc = o_lk.finish())) return rc;
    if ((rc = o_nlk.finish())) return rc;
    if ((rc = o_nllk.finish())) return rc;
    if ((rc = o_nw.finish())) return rc;
    return o_llk.finish();
}

int gmmiv_topgauss_compute(gmmiv_ctx *c, const gmmiv_gmm *g, const void *x, int dt, int64_t T, int64_t ldx, int cap, double top_gauss,
                           int mode, double min_llk, double max_llk, int32_t *idx, int32_t *count, double *snsw, double *snsl,
                           double *llk_out, int64_t *n_capped)
{
    int rc = check_model(c, g);
    if (rc) return rc;
    if (T < 0 || !idx || !count || !snsw || !snsl || cap <= 0 || !(top_gauss > 0.0)) { gmmiv_set_error("topgauss_compute: bad argument"); return GMMIV_ERR_ARG; }
    if (n_capped && gmmiv_is_device_ptr(n_capped)) { gmmiv_set_error("topgauss_compute: n_capped must be a host variable"); return GMMIV_ERR_ARG; }
    const int fixed = top_gauss >= 1.0 ? (int)top_gauss : 0; // _nbg[t] = (unsigned long)topD, TopGauss.cpp:170
    if (fixed > cap) { gmmiv_set_error("topgauss_compute: topGauss %d exceeds the list length %d", fixed, cap); return GMMIV_ERR_ARG; }
    if (n_capped) *n_capped = 0;
    if (T == 0) return GMMIV_OK;
    // the sorted top list of every frame (DETERMINE_TOP_DISTRIBS with topDistribsCount = cap), kept on the device
    void *p;
    const bool idx_dev = gmmiv_is_device_ptr(idx);
    int32_t *d_idx = idx;
    // (slots the DETERMINE pass does not touch: its redo path uses WS_T6 / WS_T7)
    if (!idx_dev) { if ((rc = c->scratch(WS_LP, (size_t)T * cap * sizeof(int32_t), &p))) return rc; d_idx = (int32_t *)p; }
    if ((rc = c->scratch(WS_AUX, (size_t)T * cap * sizeof(double), &p))) return rc;
    double *d_lk = (double *)p;
    const bool llk_dev = llk_out && gmmiv_is_device_ptr(llk_out);
    double *d_llk = llk_out;
    if (!llk_dev) { if ((rc = c->scratch(WS_SLAB, (size_t)T * sizeof(double), &p))) return rc; d_llk = (double *)p; }
    if ((rc = gmmiv_llk_determine_top(c, g, x, dt, T, ldx, cap, mode, min_llk, max_llk, d_idx, d_lk, nullptr, nullptr, nullptr, d_llk))) return rc;
    DevOut<int32_t> o_cnt;
    DevOut<double> o_w, o_l;
    if ((rc = o_cnt.init(c, WS_T0, count, (size_t)T, false))) return rc;
    if ((rc = o_w.init(c, WS_T1, snsw, (size_t)T, false))) return rc;
    if ((rc = o_l.init(c, WS_T2, snsl, (size_t)T, false))) return rc;
    if ((rc = c->scratch(WS_SMALL, 3 * 256 * sizeof(double), &p))) return rc;
    unsigned long long *d_cap = (unsigned long long *)p;
    GCHK(hipMemsetAsync(d_cap, 0, sizeof(unsigned long long), c->stream));
    GCHK(gmmk_topgauss_select(c->stream, T, cap, top_gauss, fixed, g->w, d_idx, d_lk, d_llk, o_cnt.d, o_w.d, o_l.d, d_cap));
    if (!idx_dev) GCHK(hipMemcpyAsync(idx, d_idx, (size_t)T * cap * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (llk_out && !llk_dev) GCHK(hipMemcpyAsync(llk_out, d_llk, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n_capped) {
        unsigned long long h = 0;
        GCHK(hipMemcpyAsync(&h, d_cap, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
        *n_capped = (int64_t)h;
    } else if (!idx_dev || (llk_out && !llk_dev))
        GCHK(hipStreamSynchronize(c->stream));
    if ((rc = o_cnt.finish())) return rc;
    if ((rc = o_w.finish())) return rc;
    return o_l.finish();
}

int gmmiv_llk_use_top(gmmiv_ctx *c, const gmmiv_gmm *g, const void *x, int dt, int64_t T, int64_t ldx, int ctop,
                      const int32_t *idx, const double *nontop_llk, int mode, double min_llk, double max_llk,
                      double *llk_out)
{
    int rc = check_model(c, g);
    if (rc) return rc;
    if (T < 0 || !idx || !llk_out || ctop <= 0) { gmmiv_set_error("use_top: bad argument"); return GMMIV_ERR_ARG; }
    if (ctop > g->C) { gmmiv_set_error("use_top: topDistribsCount %d exceeds mixtureDistribCount %d", ctop, g->C); return GMMIV_ERR_ARG; }
    if (mode == GMMIV_TOP_COMPLETE && !nontop_llk) { gmmiv_set_error("use_top: COMPLETE mode needs nontop_llk"); return GMMIV_ERR_ARG; }
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, g->D))) return rc;
    DevIn<int32_t> i_idx;
    DevIn<double> i_n;
    DevOut<double> o_llk;
    if ((rc = i_idx.init(c, WS_T0, idx, (size_t)T * ctop))) return rc;
    if ((rc = i_n.init(c, WS_T1, nontop_llk, (size_t)T))) return rc;
    if ((rc = o_llk.init(c, WS_T2, llk_out, (size_t)T, false))) return rc;
    if ((rc = count_unusable(c, xv, dt, T, g->D))) return rc;
    c->t_begin("k_topc_use");
    // four lanes per candidate, one frame per wave ("topc_use_lanes" 1: one lane per candidate, four frames per wave) when the
    // selection has at most 16 entries (topc_z.hip); else one wave per frame
    int krc = ctop > 64 ? gmmk_topc_use_big(c->stream, dt == GMMIV_F64, xv.d, T, xv.ldx, g->D, g->mean, g->iv, g->lwc, g->C, ctop, i_idx.d, i_n.d,
                                            mode == GMMIV_TOP_COMPLETE, min_llk, max_llk, o_llk.d)
              : c->topc_z ? gmmk_topc_use16(c->stream, dt == GMMIV_F64, xv.d, T, xv.ldx, g->D, g->mean, g->iv, g->lwc, g->C, ctop, i_idx.d, i_n.d,
                                          mode == GMMIV_TOP_COMPLETE, min_llk, max_llk, o_llk.d, (int)c->topc_use_lanes)
                        : -1;
    if (krc == -1 && ctop <= 64)
        krc = gmmk_topc_use(c->stream, dt == GMMIV_F64, xv.d, T, xv.ldx, g->D, g->mean, g->iv, g->lwc, g->C, ctop, i_idx.d, i_n.d,
                            mode == GMMIV_TOP_COMPLETE, min_llk, max_llk, o_llk.d);
    GCHK(krc);
    c->t_end();
    return o_llk.finish();
}

int gmmiv_llk_use_top_multi(gmmiv_ctx *c, int n_clients, const gmmiv_gmm *const *clients, const void *x, int dt, int64_t T, int64_t ldx,
                            int ctop, const int32_t *idx, const double *nontop_llk, int mode, double min_llk, double max_llk,
                            double *llk_out)
{
    if (!c) { gmmiv_set_error("use_top_multi: null context"); return GMMIV_ERR_ARG; }
    if (n_clients < 0 || (n_clients > 0 && !clients)) { gmmiv_set_error("use_top_multi: bad client list"); return GMMIV_ERR_ARG; }
    if (n_clients == 0) return GMMIV_OK;
    int rc;
    for (int i = 0; i < n_clients; ++i) {
        if ((rc = check_model(c, clients[i]))) return rc;
        if (clients[i]->D != clients[0]->D) { gmmiv_set_error("use_top_multi: client %d has %d dimensions, client 0 has %d", i, clients[i]->D, clients[0]->D); return GMMIV_ERR_ARG; }
        if (ctop > clients[i]->C) { gmmiv_set_error("use_top_multi: topDistribsCount %d exceeds mixtureDistribCount %d of client %d", ctop, clients[i]->C, i); return GMMIV_ERR_ARG; }
    }
    if (T < 0 || !idx || !llk_out || ctop <= 0) { gmmiv_set_error("use_top_multi: bad argument"); return GMMIV_ERR_ARG; }
    if (mode == GMMIV_TOP_COMPLETE && !nontop_llk) { gmmiv_set_error("use_top_multi: COMPLETE mode needs nontop_llk"); return GMMIV_ERR_ARG; }
    const gmmiv_gmm *g0 = clients[0];
    // a HOST output of [n_clients x T] is staged on the device: bound the staging to 1 GiB by going through the clients in groups
    // (a long segment scored against thousands of models would otherwise grow the workspace without limit)
    {
        const size_t cap = (size_t)1 << 30, row = (size_t)(T > 0 ? T : 1) * sizeof(double);
        if (n_clients > 1 && !gmmiv_is_device_ptr(llk_out) && (size_t)n_clients * row > cap) {
            const int per = (int)(cap / row > 0 ? cap / row : 1);
            for (int i0 = 0; i0 < n_clients; i0 += per) {
                const int n = n_clients - i0 < per ? n_clients - i0 : per;
                if ((rc = gmmiv_llk_use_top_multi(c, n, clients + i0, x, dt, T, ldx, ctop, idx, nontop_llk, mode, min_llk, max_llk, llk_out + (size_t)i0 * T))) return rc;
            }
            return GMMIV_OK;
        }
    }
    // one launch for all clients when the four-lanes-per-candidate kernel applies; otherwise client by client (same results either way)
    const bool batched = c->topc_z && c->topc_use_lanes == 4 && ctop <= 16 && g0->D % 2 == 0 && n_clients <= 65535 && T > 0;
    if (!batched) {
        for (int i = 0; i < n_clients; ++i)
            if ((rc = gmmiv_llk_use_top(c, clients[i], x, dt, T, ldx, ctop, idx, nontop_llk, mode, min_llk, max_llk, llk_out + (size_t)i * T))) return rc;
        return GMMIV_OK;
    }
    GBIND(c);
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, g0->D))) return rc;
    if ((rc = count_unusable(c, xv, dt, T, g0->D))) return rc;
    DevIn<int32_t> i_idx;
    DevIn<double> i_n;
    DevOut<double> o_llk;
    if ((rc = i_idx.init(c, WS_T0, idx, (size_t)T * ctop))) return rc;
    if ((rc = i_n.init(c, WS_T1, nontop_llk, (size_t)T))) return rc;
    if ((rc = o_llk.init(c, WS_T2, llk_out, (size_t)T * n_clients, false))) return rc;
    struct Rec { const double *mean, *iv, *lwc; long C; };
    std::vector<Rec> recs((size_t)n_clients);
    for (int i = 0; i < n_clients; ++i) recs[i] = Rec{clients[i]->mean, clients[i]->iv, clients[i]->lwc, (long)clients[i]->C};
    void *drec;
    if ((rc = c->scratch(WS_T3, recs.size() * sizeof(Rec), &drec))) return rc;
    GCHK(hipMemcpyAsync(drec, recs.data(), recs.size() * sizeof(Rec), hipMemcpyHostToDevice, c->stream));
    GCHK(hipStreamSynchronize(c->stream)); // recs lives on this stack frame
    c->t_begin("k_topc_use");
    GCHK(gmmk_topc_use4_multi(c->stream, dt == GMMIV_F64, xv.d, T, xv.ldx, g0->D, drec, n_clients, ctop, i_idx.d, i_n.d, mode == GMMIV_TOP_COMPLETE,
                              min_llk, max_llk, o_llk.d));
    c->t_end();
    return o_llk.finish();
}

int gmmiv_occ(gmmiv_ctx *c, const gmmiv_gmm *g, const void *x, int dt, int64_t T, int64_t ldx, double *gamma)
{
    int rc = check_model(c, g);
    if (rc) return rc;
    if (T < 0 || !gamma) { gmmiv_set_error("occ: bad argument"); return GMMIV_ERR_ARG; }
    if (T > 0x7fffffff) { gmmiv_set_error("occ: too many frames in one call"); return GMMIV_ERR_UNSUPPORTED; }
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, g->D))) return rc;
    DevOut<double> o;
    if ((rc = o.init(c, WS_T0, gamma, (size_t)T * g->C, false))) return rc;
    if ((rc = count_unusable(c, xv, dt, T, g->D))) return rc;
    // Fast path: logits on the matrix cores (k_llk_mfma<WZ>), posteriors = the stored scaled likelihoods rescaled and transposed
    const int64_t Tcz = c->topc_z ? z_chunk_frames(c, g) : 0;
    if (Tcz > 0 && T > 0) {
        gmmk_zview z;
        double *lz;
        if ((rc = gmmiv_z_reserve(c, g->nct, T < Tcz ? T : Tcz, true, &z, &lz))) return rc;
        for (int64_t c0 = 0; c0 < T; c0 += Tcz) {
            const int64_t n = (T - c0) < Tcz ? (T - c0) : Tcz;
            if ((rc = llk_z_run(c, g, xv, dt, c0, n, lz, z, c0 == 0))) return rc;
            GCHK(count_dead(c, lz, n));
            c->t_begin("k_post_from_z", c0 == 0);
            GCHK(gmmk_post_from_z(c->stream, n, g->C, g->nct, z, o.d + (size_t)c0 * g->C));
            c->t_end();
        }
        return o.finish();
    }
    double *lse;
    if ((rc = run_lse(c, g, xv, dt, T, &lse))) return rc;
    c->t_begin("k_posteriors");
    GCHK(gmmk_posteriors(c->stream, dt == GMMIV_F64, xv.d, T, xv.ldx, g->D, g->C, g->Cp64, g->meanT, g->ivT, g->lwc, lse, o.d));
    c->t_end();
    return o.finish();
}

// ---- EM ----------------------------------------------------------------------------------
size_t gmmiv_em_acc_len(int C, int D) { return (size_t)C * (1 + 2 * (size_t)D) + 2; }

// frame segments [0,T) -> nseg pieces aligned to the 64-frame tile; device array in WS_SEG
static int make_chunks(gmmiv_ctx *c, int64_t T, int nseg, long **dev)
{
    const int64_t per = ((T + nseg - 1) / nseg + 63) / 64 * 64;
    void *buf;
    int rc = c->scratch(WS_SEG, (nseg + 1) * sizeof(long), &buf);
    if (rc) return rc;
    GCHK(gmmk_fill_chunks(c->stream, (long *)buf, nseg, (long)per, (long)T)); // seg[i] = min(i per, T), on the device: nothing to wait for
    *dev = (long *)buf;
    return GMMIV_OK;
}

// EM statistics of frames [0, T) into the partial blocks part[nseg] (summed by the caller)
static int em_stats_z(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t T, int64_t Tc, double weight,
                      double *lse, int *nseg_out, void **part_out)
{
    int rc;
    const int ngrp = gmmk_stats_z_groups(g->nct);
    int nseg = c->em_chunks > 0 ? (int)c->em_chunks : (c->n_cu * gmmk_stats_z_wg_per_cu() + ngrp - 1) / ngrp;
    nseg = (nseg + 7) / 8 * 8;
    const int64_t first = T < Tc ? T : Tc;
    // at least 256 frames (four tiles) per segment: with 2048 a pass over 12 000 frames (a TrainTarget client) ran 64 workgroups of
    // 24 tiles each -- 0.39 ms where 256 workgroups of 6 tiles take 0.12
    const int64_t cap = (first + 255) / 256;
    if (nseg > cap) nseg = (int)((cap + 7) / 8 * 8);
    const int64_t nchunk = (T + Tc - 1) / Tc;
    // segment bounds relative to the chunk start: one table for full chunks, one for the last chunk
    const int64_t lastn = T - (nchunk - 1) * Tc;
    void *seg, *part;
    if ((rc = c->scratch(WS_SEG, 2 * (size_t)(nseg + 1) * sizeof(long), &seg))) return rc;
    auto fill = [&](long *dst, int64_t n) { // dst[i] = min(i per, n): written on the device, the call does not wait for the stream
        const int64_t per = ((n + nseg - 1) / nseg + 63) / 64 * 64;
        return gmmk_fill_chunks(c->stream, dst, nseg, (long)per, (long)n);
    };
    GCHK(fill((long *)seg, first));
    GCHK(fill((long *)seg + nseg + 1, lastn));
    gmmk_zview z;
    if ((rc = gmmiv_z_reserve(c, g->nct, first, !(c->dbg & 64), &z, nullptr))) return rc; // lse: the caller's, T frames
    const int RL = gmmk_rl_for_ks(g->KS);
    const size_t Cp = (size_t)g->nct * 16;
    if ((rc = c->scratch(WS_PART, (size_t)nseg * Cp * 2 * RL * sizeof(double), &part))) return rc;
    for (int64_t k = 0; k < nchunk; ++k) {
        const int64_t c0 = k * Tc, n = (k == nchunk - 1) ? lastn : Tc;
        if ((rc = llk_z_run(c, g, xv, dt, c0, n, lse + c0, z, k == 0))) return rc;
        GCHK(count_dead(c, lse + c0, n));
        c->t_begin("k_stats_z", k == 0);
        GCHK(gmmk_stats_z(c->stream, g->KS, 1, dt == GMMIV_F64, gmmiv_x_at(xv, dt, c0), xv.ldx, g->D, g->C, g->nct, z, weight,
                          (const long *)seg + (k == nchunk - 1 ? nseg + 1 : 0), nseg, (double *)part, nullptr, 0, k > 0, c->prune_thr()));
        c->t_end();
    }
    *nseg_out = nseg;
    *part_out = part;
    return GMMIV_OK;
}

int gmmiv_em_accumulate(gmmiv_ctx *c, const gmmiv_gmm *g, const void *x, int dt, int64_t T, int64_t ldx, double weight,
                        double *acc)
{
    int rc = check_model(c, g);
    if (rc) return rc;
    if (T < 0 || !acc || !(weight > 0.0)) { gmmiv_set_error("em_accumulate: bad argument (T >= 0, weight > 0, acc != NULL)"); return GMMIV_ERR_ARG; }
    const size_t nacc = gmmiv_em_acc_len(g->C, g->D);
    DevOut<double> o;
    if ((rc = o.init(c, WS_T0, acc, nacc, true))) return rc;
    if (T == 0) return o.finish();
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, g->D))) return rc;
    if ((rc = count_unusable(c, xv, dt, T, g->D))) return rc;
    const int64_t Tc = z_chunk_frames(c, g);
    if (Tc > 0) { // logits written once, statistics from the stored logits
        void *lsew, *small, *part;
        int nseg = 0;
        if ((rc = c->scratch(WS_LSE, (size_t)T * sizeof(double), &lsew))) return rc;
        if ((rc = c->scratch(WS_SMALL, 3 * 256 * sizeof(double), &small))) return rc;
        if ((rc = em_stats_z(c, g, xv, dt, T, Tc, weight, (double *)lsew, &nseg, &part))) return rc;
        GCHK(gmmk_llk_finalize(c->stream, (const double *)lsew, T, -INFINITY, INFINITY, nullptr, (double *)small, 0.0, weight, nullptr,
                               o.d + nacc - 2, weight, o.d + nacc - 1));
        GCHK(gmmk_em_reduce(c->stream, (const double *)part, nseg, g->C, g->nct * 16, g->D, g->KS, o.d));
        return o.finish();
    }
    double *lse;
    if ((rc = run_lse(c, g, xv, dt, T, &lse))) return rc;
    void *small;
    if ((rc = c->scratch(WS_SMALL, 3 * 256 * sizeof(double), &small))) return rc;
    // sum_t weight * log lk_t  and  sum_t weight
    GCHK(gmmk_llk_finalize(c->stream, lse, T, -INFINITY, INFINITY, nullptr, (double *)small, 0.0, weight, nullptr,
                           o.d + nacc - 2, weight, o.d + nacc - 1));
    if (g->KS == GMMK_KS_GENERIC) { // no MFMA instantiation for this vectSize: gamma^T [x | 1 | x^2] on the fp64 GEMM
        const int NC = 2 * g->D + 2;
        void *S;
        if ((rc = c->scratch(WS_PART, (size_t)g->C * NC * sizeof(double), &S))) return rc;
        if ((rc = generic_gamma_gemm(c, g, xv, dt, 0, T, lse, true, NC, (double *)S))) return rc;
        GCHK(gmmk_scatter_em(c->stream, g->C, g->D, NC, (const double *)S, weight, o.d));
        return o.finish();
    }
    // frame chunks: enough workgroups to fill the chip about twice, each >= 4096 frames
    const int nw = c->wg_waves == 8 ? 8 : 4;
    const int ngrp = (g->nct + nw - 1) / nw;
    int nseg = c->em_chunks > 0 ? (int)c->em_chunks : ((nw == 8 ? 2 : 4) * c->n_cu + ngrp - 1) / ngrp;
    nseg = (nseg + 7) / 8 * 8;
    const int64_t cap = (T + 4095) / 4096;
    if (nseg > cap) nseg = (int)cap;
    if (nseg < 1) nseg = 1;
    long *seg;
    if ((rc = make_chunks(c, T, nseg, &seg))) return rc;
    const int RL = gmmk_rl_for_ks(g->KS);
    const size_t Cp = (size_t)g->nct * 16;
    void *part;
    if ((rc = c->scratch(WS_PART, (size_t)nseg * Cp * 2 * RL * sizeof(double), &part))) return rc;
    c->t_begin("k_stats_mfma");
    GCHK(gmmk_stats(c->stream, g->KS, 1, dt == GMMIV_F64, xv.d, xv.ldx, g->D, g->C, g->Pt, g->nct, lse, -log(weight), seg,
                    nseg, (double *)part, nullptr, 0, (int)c->wg_waves, c->prune_arg()));
    c->t_end();
    GCHK(gmmk_em_reduce(c->stream, (const double *)part, nseg, g->C, (int)Cp, g->D, g->KS, o.d));
    return o.finish();
}

int gmmiv_em_get(gmmiv_ctx *c, int C, int D, const double *acc, const double *prev_mean, const double *prev_cov,
                 double *w, double *mean, double *cov)
{
    if (!c || !acc || !prev_mean || !prev_cov || !w || !mean || !cov || C <= 0 || D <= 0) { gmmiv_set_error("em_get: bad argument"); return GMMIV_ERR_ARG; }
    GBIND(c);
    const size_t CD = (size_t)C * D;
    DevIn<double> i_acc, i_pm, i_pc;
    DevOut<double> o_w, o_m, o_c;
    int rc;
    if ((rc = i_acc.init(c, WS_T0, acc, gmmiv_em_acc_len(C, D)))) return rc;
    if ((rc = i_pm.init(c, WS_T1, prev_mean, CD))) return rc;
    if ((rc = i_pc.init(c, WS_T2, prev_cov, CD))) return rc;
    if ((rc = o_w.init(c, WS_T3, w, C, false))) return rc;
    if ((rc = o_m.init(c, WS_T4, mean, CD, false))) return rc;
    if ((rc = o_c.init(c, WS_T5, cov, CD, false))) return rc;
    GCHK(gmmk_em_get(c->stream, C, D, i_acc.d, i_pm.d, i_pc.d, o_w.d, o_m.d, o_c.d));
    if ((rc = o_w.finish())) return rc;
    if ((rc = o_m.finish())) return rc;
    return o_c.finish();
}

int gmmiv_variance_control(gmmiv_ctx *c, int C, int D, double *cov, double flooring, double ceiling,
                           const double *cov_signal, int64_t *counts)
{
    if (!c || C <= 0 || D <= 0 || !cov || !cov_signal) { gmmiv_set_error("variance_control: bad argument"); return GMMIV_ERR_ARG; }
    if (counts && gmmiv_is_device_ptr(counts)) { gmmiv_set_error("variance_control: counts must be a host array"); return GMMIV_ERR_ARG; }
    GBIND(c);
    DevOut<double> o;
    DevIn<double> i_cs;
    int rc;
    if ((rc = o.init(c, WS_T0, cov, (size_t)C * D, true))) return rc;
    if ((rc = i_cs.init(c, WS_T1, cov_signal, D))) return rc;
    unsigned long long *dc = nullptr;
    if (counts) {
        void *p;
        if ((rc = c->scratch(WS_SMALL, 3 * 256 * sizeof(double), &p))) return rc;
        dc = (unsigned long long *)p;
        GCHK(hipMemsetAsync(dc, 0, 2 * sizeof(unsigned long long), c->stream));
    }
    GCHK(gmmk_variance_control(c->stream, C, D, o.d, flooring, ceiling, i_cs.d, dc));
    if (counts) {
        unsigned long long h[2];
        GCHK(hipMemcpyAsync(h, dc, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
        counts[0] = (int64_t)h[0];
        counts[1] = (int64_t)h[1];
    }
    return o.finish();
}

// ---- Baum-Welch N / F ----------------------------------------------------------------------
// Chunks of whole utterances whose frames fit the logit scratch (Tcz frames): chunk k = utterances [cu[k], cu[k+1]).  rel = the segment
// bounds relative to each chunk's first frame, chunk after chunk (chunk k occupies cu[k] + k .. cu[k+1] + k); maxn = the frames of the
// longest chunk.  false: an utterance is longer than the scratch.
static bool plan_utt_chunks(const int64_t *utt_begin, int64_t U, int64_t Tcz, std::vector<int64_t> &cu, std::vector<long> &rel, int64_t *maxn)
{
    cu.assign(1, 0);
    // chunks of about EQUAL length (the last one of a greedy fill is a fraction of the others and runs the chip half empty:
    // 512 utterances x 3000 frames on a 0.79 M-frame scratch went 283 + 229, 3 % slower than 256 + 256)
    const int64_t Ttot = utt_begin[U] - utt_begin[0], nch = (Ttot + Tcz - 1) / Tcz;
    const int64_t target = nch > 0 ? (Ttot + nch - 1) / nch : Tcz;
    for (int64_t u = 0; u < U;) {
        int64_t v = u;
        while (v < U && utt_begin[v + 1] - utt_begin[u] <= Tcz && (v == u || utt_begin[v] - utt_begin[u] < target)) ++v;
        // whole rounds of the statistics kernel: it runs one workgroup per (utterance, Gaussian group), 64 utterances fill the chip
        // an integer number of times in every shape -- 262 utterances of 3000 frames took 9 rounds where 256 take 8
        if (v < U && v - u > 64) v = u + (v - u) / 64 * 64;
        if (v == u) return false;
        if (utt_begin[v] - utt_begin[u] > *maxn) *maxn = utt_begin[v] - utt_begin[u];
        cu.push_back(v);
        u = v;
    }
    for (size_t k = 0; k + 1 < cu.size(); ++k)
        for (int64_t u = cu[k]; u <= cu[k + 1]; ++u) rel.push_back((long)(utt_begin[u] - utt_begin[cu[k]]));
    return true;
}

// A few utterances (on-line extraction: ONE) give the statistics kernel a few workgroups -- 8 per utterance, each walking all its
// frames: 0.39 ms for 3000 frames.  Up to 16 utterances in one chunk are cut into about 32 pieces of whole 64-frame tiles: pb = the
// piece bounds relative to the first frame, rbh[u] .. rbh[u + 1] = the pieces of utterance u.  false: no utterance was cut.
static bool plan_utt_pieces(const int64_t *utt_begin, int64_t U, std::vector<long> &pb, std::vector<int> &rbh)
{
    rbh.assign((size_t)U + 1, 0);
    const int64_t per_utt = 32 / U > 1 ? 32 / U : 1;
    for (int64_t u = 0; u < U; ++u) {
        const int64_t b = utt_begin[u] - utt_begin[0], e = utt_begin[u + 1] - utt_begin[0], len = e - b;
        int64_t S = (len + 255) / 256;
        S = S < 1 ? 1 : (S > per_utt ? per_utt : S);
        const int64_t per = ((len + S - 1) / S + 63) / 64 * 64;
        int64_t pos = b;
        int cntp = 0;
        do { pb.push_back((long)pos); pos = per > 0 && pos + per < e ? pos + per : e; ++cntp; } while (pos < e);
        rbh[u + 1] = rbh[u] + cntp;
    }
    pb.push_back((long)(utt_begin[U] - utt_begin[0]));
    return rbh[U] > U;
}

int gmmiv_tv_stats(gmmiv_ctx *c, const gmmiv_gmm *g, const void *x, int dt, int64_t T, int64_t ldx,
                   const int64_t *utt_begin, int64_t U, double *N, double *F)
{
    int rc = check_model(c, g);
    if (rc) return rc;
    if (T < 0 || U < 0 || !utt_begin || !N || !F) { gmmiv_set_error("tv_stats: bad argument"); return GMMIV_ERR_ARG; }
    if (gmmiv_is_device_ptr(utt_begin)) { gmmiv_set_error("tv_stats: utt_begin must be a host array"); return GMMIV_ERR_ARG; }
    if (U == 0) return GMMIV_OK;
    if (utt_begin[0] < 0 || utt_begin[U] > T) { gmmiv_set_error("tv_stats: utt_begin out of range"); return GMMIV_ERR_ARG; }
    for (int64_t u = 0; u < U; ++u)
        if (utt_begin[u + 1] < utt_begin[u]) { gmmiv_set_error("tv_stats: utt_begin must be non-decreasing"); return GMMIV_ERR_ARG; }
    if (U > 0x7fffffff / 64) { gmmiv_set_error("tv_stats: too many utterances in one call"); return GMMIV_ERR_UNSUPPORTED; }
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, g->D))) return rc;
    if ((rc = count_unusable(c, xv, dt, T, g->D))) return rc;
    std::vector<long> h(utt_begin, utt_begin + U + 1);
    void *seg;
    if ((rc = c->scratch(WS_SEG, (U + 1) * sizeof(long), &seg))) return rc;
    GCHK(hipMemcpyAsync(seg, h.data(), (U + 1) * sizeof(long), hipMemcpyHostToDevice, c->stream));
    GCHK(hipStreamSynchronize(c->stream));
    const size_t SV = (size_t)g->C * g->D;
    DevOut<double> o_n, o_f;
    if ((rc = o_n.init(c, WS_T0, N, (size_t)U * g->C, false))) return rc;
    if ((rc = o_f.init(c, WS_T1, F, (size_t)U * SV, false))) return rc;
    const int64_t Tcz = z_chunk_frames(c, g);
    std::vector<int64_t> cu;
    std::vector<long> rel;
    int64_t maxn = 0;
    if (Tcz > 0 && plan_utt_chunks(utt_begin, U, Tcz, cu, rel, &maxn)) { // (an utterance longer than a chunk: the recomputing kernel below)
        if ((rc = c->scratch(WS_SEG, rel.size() * sizeof(long), &seg))) return rc;
        GCHK(hipMemcpyAsync(seg, rel.data(), rel.size() * sizeof(long), hipMemcpyHostToDevice, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
        gmmk_zview z;
        double *lsew;
        if ((rc = gmmiv_z_reserve(c, g->nct, maxn, true, &z, &lsew))) return rc;
        // one chunk of a few utterances: the pieces are "utterances" of the kernel, written to scratch rows and summed back in piece order
        std::vector<long> pb;
        std::vector<int> rbh;
        const bool split = cu.size() == 2 && U <= 16 && c->tv_stats_split && plan_utt_pieces(utt_begin, U, pb, rbh);
        const int np = split ? rbh[U] : 0;
        void *pseg = nullptr, *prb = nullptr, *tn = o_n.d, *tf = o_f.d;
        if (split) {
            if ((rc = c->scratch(WS_SEG, pb.size() * sizeof(long), &pseg))) return rc;
            if ((rc = c->scratch(WS_SMALL, rbh.size() * sizeof(int) + 64, &prb))) return rc;
            if ((rc = c->scratch(WS_T2, (size_t)np * g->C * sizeof(double), &tn))) return rc;
            if ((rc = c->scratch(WS_T3, (size_t)np * SV * sizeof(double), &tf))) return rc;
            GCHK(hipMemcpyAsync(pseg, pb.data(), pb.size() * sizeof(long), hipMemcpyHostToDevice, c->stream));
            GCHK(hipMemcpyAsync(prb, rbh.data(), rbh.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
            GCHK(hipStreamSynchronize(c->stream)); // pb / rbh live on this stack frame
        }
        for (size_t k = 0; k + 1 < cu.size(); ++k) {
            const int64_t u0 = cu[k], u1 = cu[k + 1], c0 = utt_begin[u0], n = utt_begin[u1] - c0;
            if ((rc = llk_z_run(c, g, xv, dt, c0, n, lsew, z, k == 0))) return rc;
            GCHK(count_dead(c, lsew, n));
            c->t_begin("k_stats_z", k == 0);
            GCHK(gmmk_stats_z(c->stream, g->KS, 0, dt == GMMIV_F64, gmmiv_x_at(xv, dt, c0), xv.ldx, g->D, g->C, g->nct, z, 1.0,
                              split ? (const long *)pseg : (const long *)seg + u0 + k, split ? np : (int)(u1 - u0), (double *)tn + (size_t)u0 * g->C,
                              (double *)tf + (size_t)u0 * SV, 1, 0, c->prune_thr()));
            if (split) {
                GCHK(gmmk_rows_sum_groups(c->stream, g->C, (int)U, (const int *)prb, (const double *)tn, o_n.d));
                GCHK(gmmk_rows_sum_groups(c->stream, (long)SV, (int)U, (const int *)prb, (const double *)tf, o_f.d));
            }
            c->t_end();
        }
        if ((rc = o_n.finish())) return rc;
        return o_f.finish();
    }
    double *lse;
    if ((rc = run_lse(c, g, xv, dt, T, &lse))) return rc;
    if (g->KS == GMMK_KS_GENERIC) { // utterance by utterance: S_u = gamma_u^T [x | 1], N row = its last column, F row = the rest
        const int NC = g->D + 2 - (g->D & 1); // [x | 1] padded to an even width
        void *S;
        if ((rc = c->scratch(WS_PART, (size_t)g->C * NC * sizeof(double), &S))) return rc;
        for (int64_t u = 0; u < U; ++u) {
            if ((rc = generic_gamma_gemm(c, g, xv, dt, utt_begin[u], utt_begin[u + 1] - utt_begin[u], lse, false, NC, (double *)S))) return rc;
            GCHK(gmmk_scatter_nf(c->stream, g->C, g->D, NC, (const double *)S, o_n.d + (size_t)u * g->C, o_f.d + (size_t)u * SV));
        }
        if ((rc = o_n.finish())) return rc;
        return o_f.finish();
    }
    // every (u, c < C) row is written by exactly one wave (zeros for an empty utterance)
    c->t_begin("k_stats_mfma");
    GCHK(gmmk_stats(c->stream, g->KS, 0, dt == GMMIV_F64, xv.d, xv.ldx, g->D, g->C, g->Pt, g->nct, lse, 0.0,
                    (const long *)seg, (int)U, o_n.d, o_f.d, 1, (int)c->wg_waves, c->prune_arg()));
    c->t_end();
    if ((rc = o_n.finish())) return rc;
    return o_f.finish();
}

// TVAcc::computeAndAccumulateTVStat with the reference's file -> ndx-line map (AccumulateTVStat.cpp:318-346: the statistics of a
// feature file are added to EVERY line `locidcs` that lists it, and a line sums all of its files): the Baum-Welch pass runs
// ONCE per file, the line rows are sums of file rows.
int gmmiv_tv_stats_lines(gmmiv_ctx *c, const gmmiv_gmm *g, const void *x, int dt, int64_t T, int64_t ldx, const int64_t *file_begin,
                         int64_t nfiles, int64_t nlines, const int64_t *line_off, const int64_t *line_files, double *N, double *F)
{
    int rc = check_model(c, g);
    if (rc) return rc;
    if (nfiles < 0 || nlines < 0 || !file_begin || !line_off || (!line_files && nlines && line_off[nlines]) || !N || !F) { gmmiv_set_error("tv_stats_lines: bad argument"); return GMMIV_ERR_ARG; }
    if (gmmiv_is_device_ptr(line_off) || gmmiv_is_device_ptr(line_files)) { gmmiv_set_error("tv_stats_lines: the line map must be host arrays"); return GMMIV_ERR_ARG; }
    if (nlines == 0) return GMMIV_OK;
    if (line_off[0] != 0) { gmmiv_set_error("tv_stats_lines: line_off must start at 0"); return GMMIV_ERR_ARG; }
    for (int64_t l = 0; l < nlines; ++l)
        if (line_off[l + 1] < line_off[l]) { gmmiv_set_error("tv_stats_lines: line_off must be non-decreasing"); return GMMIV_ERR_ARG; }
    const int64_t npairs = line_off[nlines];
    for (int64_t p = 0; p < npairs; ++p)
        if (line_files[p] < 0 || line_files[p] >= nfiles) { gmmiv_set_error("tv_stats_lines: file index %lld out of range", (long long)line_files[p]); return GMMIV_ERR_ARG; }
    const size_t SV = (size_t)g->C * g->D;
    void *pn, *pf, *pm;
    if ((rc = c->scratch(WS_T6, (size_t)(nfiles ? nfiles : 1) * g->C * sizeof(double), &pn))) return rc;
    if ((rc = c->scratch(WS_T7, (size_t)(nfiles ? nfiles : 1) * SV * sizeof(double), &pf))) return rc;
    if ((rc = gmmiv_tv_stats(c, g, x, dt, T, ldx, file_begin, nfiles, (double *)pn, (double *)pf))) return rc;   // once per file, on the device
    if ((rc = c->scratch(WS_T8, (size_t)(nlines + 1 + npairs + 1) * sizeof(long), &pm))) return rc;
    std::vector<long> h((size_t)nlines + 1 + npairs);
    for (int64_t l = 0; l <= nlines; ++l) h[l] = (long)line_off[l];
    for (int64_t p = 0; p < npairs; ++p) h[nlines + 1 + p] = (long)line_files[p];
    GCHK(hipMemcpyAsync(pm, h.data(), h.size() * sizeof(long), hipMemcpyHostToDevice, c->stream));
    DevOut<double> o_n, o_f;
    if ((rc = o_n.init(c, WS_T4, N, (size_t)nlines * g->C, false))) return rc;
    if ((rc = o_f.init(c, WS_T5, F, (size_t)nlines * SV, false))) return rc;
    const long *off = (const long *)pm, *rows = off + nlines + 1;
    GCHK(tvk_merge_rows(c->stream, (long)nlines, g->C, off, rows, (const double *)pn, o_n.d));
    GCHK(tvk_merge_rows(c->stream, (long)nlines, (long)SV, off, rows, (const double *)pf, o_f.d));
    GCHK(hipStreamSynchronize(c->stream)); // h is a stack-lifetime vector
    if ((rc = o_n.finish())) return rc;
    return o_f.finish();
}

} // extern "C"
