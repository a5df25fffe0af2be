// capi_gmm_util.h -- helpers that more than one of capi_gmm.hip, capi_feat.hip, capi_models.hip and capi_trials.hip use (internal).
#pragma once
#include "ctx.h"
#include "gmm_kernels.h"

static inline int check_model(gmmiv_ctx *c, const gmmiv_gmm *g)
{
    if (!c || !g) { gmmiv_set_error("NULL context or model"); return GMMIV_ERR_ARG; }
    if (g->ctx != c) { gmmiv_set_error("model belongs to a different context"); return GMMIV_ERR_ARG; }
    GBIND(c);
    return GMMIV_OK;
}

static inline size_t gmmiv_esize(int dt) { return dt == GMMIV_F64 ? 8 : 4; }

// Device view of the feature block [T x ldx]; host input is copied (compacted to ldx = D).
struct XView {
    const void *d = nullptr;
    int64_t ldx = 0;
    int init(gmmiv_ctx *c, const void *x, int dt, int64_t T, int64_t ld, int D)
    {
        if (dt != GMMIV_F32 && dt != GMMIV_F64) { gmmiv_set_error("feature dtype must be GMMIV_F32 or GMMIV_F64"); return GMMIV_ERR_ARG; }
        if (ld < D) { gmmiv_set_error("ldx (%ld) < D (%d)", (long)ld, D); return GMMIV_ERR_ARG; }
        if (T == 0) { d = x; ldx = ld; return GMMIV_OK; }
        if (!x) { gmmiv_set_error("x == NULL"); return GMMIV_ERR_ARG; }
        if (gmmiv_is_device_ptr(x)) { d = x; ldx = ld; return GMMIV_OK; }
        void *buf;
        int rc = c->scratch(WS_X, (size_t)T * D * gmmiv_esize(dt), &buf);
        if (rc) return rc;
        GCHK(hipMemcpy2DAsync(buf, D * gmmiv_esize(dt), x, ld * gmmiv_esize(dt), D * gmmiv_esize(dt), T, hipMemcpyHostToDevice, c->stream));
        d = buf; ldx = D;
        return GMMIV_OK;
    }
};

static inline const void *gmmiv_x_at(const XView &xv, int dt, int64_t frame) { return (const char *)xv.d + (size_t)frame * xv.ldx * gmmiv_esize(dt); }

// Device view of the output frames [F0, F1) of a matrix of row stride ldo, indexed like the input: at(frame) is valid inside the range.
// A host output is produced compact (ld = D) in WS_FEAT_OUT for the frames of the range alone and copied back to those rows by
// finish(), so that frames outside it and padding columns keep what the caller has there.
struct FeatOut {
    void *d = nullptr, *host = nullptr; // d: the (virtual) address of frame 0
    int64_t ld = 0, hld = 0, F0 = 0, F1 = 0;
    int D = 0, dt = 0;
    gmmiv_ctx *c = nullptr;
    int init(gmmiv_ctx *ctx, void *out, int odt, int64_t F0_, int64_t F1_, int64_t ldo, int D_)
    {
        c = ctx; F0 = F0_; F1 = F1_; D = D_; dt = odt;
        if (F1 == F0 || gmmiv_is_device_ptr(out)) { d = out; ld = ldo; return GMMIV_OK; }
        void *stage;
        int rc = c->scratch(WS_FEAT_OUT, (size_t)(F1 - F0) * D * gmmiv_esize(odt), &stage);
        if (rc) return rc;
        host = out; hld = ldo; ld = D;
        d = (char *)stage - (ptrdiff_t)F0 * ld * (ptrdiff_t)gmmiv_esize(dt); // (only frames of [F0, F1) are ever addressed)
        return GMMIV_OK;
    }
    void *at(int64_t frame) const { return (char *)d + (ptrdiff_t)frame * ld * (ptrdiff_t)gmmiv_esize(dt); }
    int finish()
    {
        if (host) {
            GCHK(hipMemcpy2DAsync((char *)host + (size_t)F0 * hld * gmmiv_esize(dt), hld * gmmiv_esize(dt), at(F0), D * gmmiv_esize(dt), D * gmmiv_esize(dt),
                                  (size_t)(F1 - F0), hipMemcpyDeviceToHost, c->stream));
            GCHK(hipStreamSynchronize(c->stream));
        }
        return GMMIV_OK;
    }
};

// ---- the stored-likelihood scratch (k_llk_mfma<WZ> writes it, k_stats_z / k_topc_from_z / k_post_from_z / k_feat_comp read it) ----
// Blocks (2 KB) per Gaussian tile of the likelihood scratch for n frames: whole workgroups of the log-likelihood kernel (256 frames),
// then padded so that the tile stride is an ODD number of 4 KB granules.  A statistics workgroup reads 16 tiles at the same frame
// position at once; with a stride that is a multiple of the HBM channel interleave (a large power of two) all 16 streams -- and those
// of every other workgroup of the segment -- would sit on the same channel.
static inline long gmmiv_z_tile_blocks(int64_t n, bool pad)
{
    long nfb = 16 * ((n + 255) / 256);
    if (pad && (nfb / 2) % 2 == 0) nfb += 2;
    return nfb;
}

// The scratch of `frames` frames (0 counts as 1) under a model of nct Gaussian tiles: the only place that knows its layout.  lse
// (nullable: the caller keeps its own array) = one log-sum per frame in WS_LSE.  pad = false (the "dbg" bit 64 of the EM pass,
// tools/z_stride_ab.py) leaves the tile stride unpadded.
static inline int gmmiv_z_reserve(gmmiv_ctx *c, int nct, int64_t frames, bool pad, gmmk_zview *z, double **lse)
{
    const size_t n = (size_t)(frames > 0 ? frames : 1);
    void *zb, *eit, *inv, *l;
    int rc;
    z->nfb = gmmiv_z_tile_blocks(frames, pad);
    if ((rc = c->scratch(WS_Z, (size_t)nct * z->nfb * 2048, &zb))) return rc;
    if ((rc = c->scratch(WS_EIT, (size_t)(nct / 2) * z->nfb * 16 * sizeof(int), &eit))) return rc;
    if ((rc = c->scratch(WS_INV, n * (sizeof(double) + sizeof(int)), &inv))) return rc;
    if (lse && (rc = c->scratch(WS_LSE, n * sizeof(double), &l))) return rc;
    z->zbuf = (double *)zb; z->eit = (int *)eit; z->inv = (double *)inv;
    z->efin = (int *)(z->inv + n); // Efin behind 1 / S_t in the same slot
    if (lse) *lse = (double *)l;
    return GMMIV_OK;
}

// Frames whose scratch fits the "z_scratch_mb" budget; `extra` = the bytes per frame beyond the likelihoods and exponents.  A chunk
// length fixes the segment bounds and with them the fp64 summation order of every reduction of the path, so it depends ONLY on the
// option, the model shape and the device's TOTAL memory (the same on every rank of a node), never on what happens to be free:
// replicated M-steps stay bit-identical.  If the scratch then does not fit, scratch() fails loudly.
static inline int64_t gmmiv_z_budget_frames(const gmmiv_ctx *c, int nct, size_t extra)
{
    size_t budget = (size_t)(c->z_scratch_mb > 0 ? c->z_scratch_mb : 0) << 20;
    if (c->total_mem && budget > c->total_mem / 4) budget = c->total_mem / 4;
    const size_t per_frame = (size_t)nct * 16 * sizeof(double) + (size_t)nct * 2 + extra; // likelihoods + exponents
    return (int64_t)(budget / per_frame / 1.2); // scratch() over-allocates by 1/8
}

// frames per chunk that fit the logit scratch budget (multiple of 64), 0 when the stored-likelihood path does not apply
static inline int64_t z_chunk_frames(gmmiv_ctx *c, const gmmiv_gmm *g)
{
    if (!c->stats_z || g->KS > 15 || c->wg_waves != 8) return 0;
    int64_t tc = gmmiv_z_budget_frames(c, g->nct, 16); // 16 and the rounding below are pinned by results: they fix the summation order
    // whole rounds of the log-likelihood kernel: 2 resident workgroups per CU x 256 frames
    const int64_t round = (int64_t)c->n_cu * 2 * 256;
    tc = tc >= round ? tc / round * round : tc / 64 * 64;
    return tc >= 4096 ? tc : 0;
}

// k_llk_mfma<WZ> on frames [c0, c0 + n): their log-sums into lse[0 .. n), the stored likelihoods into z.  Counting the
// zero-likelihood frames afterwards (count_dead) is the caller's decision.
static inline int llk_z_run(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t c0, int64_t n, double *lse, const gmmk_zview &z, bool first)
{
    c->t_begin("k_llk_mfma", first);
    GCHK(gmmk_llk_z(c->stream, g->KS, dt == GMMIV_F64, gmmiv_x_at(xv, dt, c0), n, xv.ldx, g->D, g->Pt, g->nct, lse,
                    (int)(c->use_glds | ((c->dbg & 15) << 8)), z));
    c->t_end();
    return GMMIV_OK;
}

// zero-likelihood frames of kind (2) among the n frames whose log-sums K1 has just left in `lse` -> the context's device counter
static inline int count_dead(gmmiv_ctx *c, const double *lse, int64_t n) { return gmmk_count_dead(c->stream, lse, (long)n, c->d_zero_llk); }

// defined in capi_gmm.hip (the last: capi_feat.hip), used by the other units too: C++ linkage, hidden from the library's ABI
#pragma GCC visibility push(hidden)
int count_unusable(gmmiv_ctx *c, const XView &xv, int dt, int64_t T, int D); // the "screened_frames" pass over T frames
int run_lse(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t T, double **lse_out); // WS_LSE; counts zero-likelihood frames
int generic_gamma_gemm(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t t0, int64_t n, const double *lse, bool sq, int NC,
                       double *S);
// the dtype, stride and overlap rules of gmmiv_feat_compensate / gmmiv_feat_map (GMMIV_ERR_ARG with a message; nothing is enqueued)
extern "C" int gmmiv_feat_check_args(const char *who, const void *x, int xdt, int64_t T, int64_t ldx, const void *out, int odt, int64_t ldo, int D);
#pragma GCC visibility pop
