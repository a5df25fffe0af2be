// capi_gmm_util.h -- helpers of capi_gmm.hip that capi_models.hip and capi_trials.hip use too (internal).
#pragma once
#include "ctx.h"
#include "gmm_kernels.h"

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

// defined in capi_gmm.hip, used by capi_models.hip too: C++ linkage, hidden from the library's ABI
#pragma GCC visibility push(hidden)
int count_unusable(gmmiv_ctx *c, const XView &xv, int dt, int64_t T, int D); // the "screened_frames" pass over T frames
int run_lse(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t T, double **lse_out); // WS_LSE; counts zero-likelihood frames
int generic_gamma_gemm(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t t0, int64_t n, const double *lse, bool sq, int NC,
                       double *S);
// the dtype, stride and overlap rules of gmmiv_feat_compensate / gmmiv_feat_map (GMMIV_ERR_ARG with a message; nothing is enqueued)
extern "C" int gmmiv_feat_check_args(const char *who, const void *x, int xdt, int64_t T, int64_t ldx, const void *out, int odt, int64_t ldo, int D);
#pragma GCC visibility pop
