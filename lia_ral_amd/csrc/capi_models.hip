// capi_models.hip -- C ABI (include/gmmiv.h): a batch of models of one shape, log-likelihood / Baum-Welch statistics with a model per
// segment, channel compensation with a model and an offset per segment, computeMAP for the whole batch.  DESIGN.md sections 3.14, 3.19.
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "capi_gmm_util.h"
#include "gmm_kernels.h"

#define MODEL_TILE_FRAMES 256 // frames per workgroup of k_llk_mfma (8 waves x 32)

extern "C" {

// ---- the tile table (pure host) ---------------------------------------------------------------------------------------------------
int64_t gmmiv_plan_model_tiles(const int64_t *seg_begin, const int32_t *seg_model, int64_t nseg, int tile_frames, gmmiv_model_tile *tiles,
                               int64_t cap)
{
    if (!seg_begin || !seg_model || nseg < 0 || tile_frames <= 0 || tile_frames % 32 || seg_begin[0] < 0) return -1;
    int64_t first_ne = -1, last_ne = -1;
    for (int64_t s = 0; s < nseg; ++s) {
        if (seg_begin[s + 1] < seg_begin[s]) return -1;
        if (seg_begin[s + 1] > seg_begin[s]) { if (first_ne < 0) first_ne = s; last_ne = s; }
    }
    int64_t n = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t b = seg_begin[s], e = seg_begin[s + 1];
        if (e <= b) continue; // an empty segment has no tile
        for (int64_t f = b & ~(int64_t)15; f < e; f += tile_frames) {
            gmmiv_model_tile t;
            t.first = f;
            t.lo = b > f ? b : f;
            t.hi = e < f + tile_frames ? e : f + tile_frames;
            t.model = seg_model[s];
            t.seg = (int32_t)s;
            // rows of the first / last block that no segment owns: written (as the likelihoods of a zero frame) by the tile next to them
            t.pad_lo = (s == first_ne && f <= b) ? (int32_t)(b - f) : 0;
            t.pad_hi = (s == last_ne && t.hi == e) ? (int32_t)(((e + 15) & ~(int64_t)15) - e) : 0;
            if (tiles && n < cap) tiles[n] = t;
            ++n;
        }
    }
    return n;
}

// the work list of the segment-aware k_feat_comp: per segment, runs of blocks_per_tile 16-frame blocks from the block of its first frame
int64_t gmmiv_plan_feat_tiles(const int64_t *seg_begin, const int32_t *seg_model, int64_t nseg, int blocks_per_tile, gmmiv_feat_tile *tiles,
                              int64_t cap)
{
    if (!seg_begin || (nseg > 0 && !seg_model) || nseg < 0 || blocks_per_tile < 1 || seg_begin[0] < 0) return -1;
    for (int64_t s = 0; s < nseg; ++s)
        if (seg_begin[s + 1] < seg_begin[s]) return -1;
    int64_t n = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t b = seg_begin[s], e = seg_begin[s + 1];
        if (e <= b) continue; // an empty segment has no entry
        for (int64_t blk = b >> 4; blk * 16 < e; blk += blocks_per_tile) {
            gmmiv_feat_tile t;
            t.block = blk;
            t.lo = b > blk * 16 ? b : blk * 16;
            t.hi = e < (blk + blocks_per_tile) * 16 ? e : (blk + blocks_per_tile) * 16;
            t.model = seg_model[s];
            t.seg = (int32_t)s;
            if (tiles && n < cap) tiles[n] = t;
            ++n;
        }
    }
    return n;
}

// ---- the batch ----------------------------------------------------------------------------------------------------------------------
int gmmiv_gmm_batch_create(gmmiv_ctx *c, int G, int C, int D, gmmiv_gmm_batch **out)
{
    if (!c || !out || G <= 0 || C <= 0 || D <= 0) { gmmiv_set_error("gmm_batch_create: bad argument"); return GMMIV_ERR_ARG; }
    const int KS = gmmk_ks_for_dim(D);
    if (!KS) { gmmiv_set_error("gmm_batch_create: vectSize %d not supported (max %d)", D, GMMK_MAX_DIM); return GMMIV_ERR_UNSUPPORTED; }
    GBIND(c);
    gmmiv_gmm_batch *b = new gmmiv_gmm_batch();
    b->ctx = c; b->G = G; b->C = C; b->D = D; b->KS = KS;
    b->nct = ((C + 15) / 16 + 1) / 2 * 2; // as gmmiv_gmm_create
    b->Cp64 = (C + 63) / 64 * 64;
    b->Cpa = b->Cp64 > b->nct * 16 ? b->Cp64 : b->nct * 16;
    if (hipMalloc((void **)&b->a, (size_t)G * b->Cpa * sizeof(double)) != hipSuccess || hipMalloc((void **)&b->lwc, (size_t)G * b->Cpa * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        gmmiv_gmm_batch_destroy(b);
        gmmiv_set_error("gmm_batch_create: hipMalloc of the constants of %d models failed", G);
        return GMMIV_ERR_HIP;
    }
    *out = b;
    return GMMIV_OK;
}

void gmmiv_gmm_batch_destroy(gmmiv_gmm_batch *b)
{
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    (void)hipStreamSynchronize(b->ctx->stream);
    void *ptrs[] = {b->w, b->mean, b->iv, b->a, b->lwc};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete b;
}

static int batch_reserve(gmmiv_gmm_batch *b, double **dst, size_t *cap, size_t need)
{
    gmmiv_ctx *c = b->ctx;
    if (*cap < need) {
        if (*dst) { GCHK(hipStreamSynchronize(c->stream)); GCHK(hipFree(*dst)); *dst = nullptr; *cap = 0; }
        const hipError_t e = hipMalloc((void **)dst, need * sizeof(double));
        if (e != hipSuccess) { (void)hipGetLastError(); *dst = nullptr; gmmiv_set_error("gmm_batch_load: hipMalloc of %zu bytes -> %s", need * sizeof(double), hipGetErrorString(e)); return GMMIV_ERR_HIP; }
        *cap = need;
    }
    return GMMIV_OK;
}
// one table: G rows of `row` doubles `stride` apart (or one shared row) into a compact device copy
static int batch_table(gmmiv_gmm_batch *b, double **dst, size_t *cap, long *dst_stride, const double *src, int64_t stride, size_t row)
{
    gmmiv_ctx *c = b->ctx;
    const size_t rows = stride == 0 ? 1 : (size_t)b->G, need = rows * row;
    const int rc = batch_reserve(b, dst, cap, need);
    if (rc) return rc;
    const hipMemcpyKind kind = gmmiv_is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    GCHK(hipMemcpy2DAsync(*dst, row * sizeof(double), src, (stride == 0 ? row : (size_t)stride) * sizeof(double), row * sizeof(double), rows, kind, c->stream));
    *dst_stride = stride == 0 ? 0 : (long)row;
    return GMMIV_OK;
}

static int batch_load(gmmiv_gmm_batch *b, const double *w, int64_t w_stride, const double *mean, int64_t mean_stride, const double *covinv,
                      int64_t covinv_stride, bool from_cov)
{
    if (!b || !w || !mean || !covinv) { gmmiv_set_error("gmm_batch_load: bad argument"); return GMMIV_ERR_ARG; }
    const size_t CD = (size_t)b->C * b->D;
    if ((w_stride && w_stride < b->C) || (mean_stride && mean_stride < (int64_t)CD) || (covinv_stride && covinv_stride < (int64_t)CD)) {
        gmmiv_set_error("gmm_batch_load: a stride must be 0 (shared) or at least the size of one model's table");
        return GMMIV_ERR_ARG;
    }
    gmmiv_ctx *c = b->ctx;
    GBIND(c);
    int rc;
    b->loaded = false;
    if ((rc = batch_table(b, &b->w, &b->cap_w, &b->sw, w, w_stride, (size_t)b->C))) return rc;
    if ((rc = batch_table(b, &b->mean, &b->cap_mean, &b->sm, mean, mean_stride, CD))) return rc;
    if (from_cov) { // the variances compact into a scratch, covInv = 1 / cov from there into the batch's table (gmmiv_gmm_set_cov)
        const size_t rows = covinv_stride == 0 ? 1 : (size_t)b->G;
        void *tmp;
        if ((rc = c->scratch(WS_T0, rows * CD * sizeof(double), &tmp))) return rc;
        if ((rc = batch_reserve(b, &b->iv, &b->cap_iv, rows * CD))) return rc;
        GCHK(hipMemcpy2DAsync(tmp, CD * sizeof(double), covinv, (covinv_stride == 0 ? CD : (size_t)covinv_stride) * sizeof(double), CD * sizeof(double), rows,
                              gmmiv_is_device_ptr(covinv) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        GCHK(gmmk_reciprocal(c->stream, (long)(rows * CD), (const double *)tmp, b->iv));
        b->si = covinv_stride == 0 ? 0 : (long)CD;
    } else if ((rc = batch_table(b, &b->iv, &b->cap_iv, &b->si, covinv, covinv_stride, CD))) return rc;
    GCHK(gmmk_const_models(c->stream, b->G, b->C, b->Cpa, b->D, b->w, b->sw, b->mean, b->sm, b->iv, b->si, b->a, b->lwc));
    if (!gmmiv_is_device_ptr(w) || !gmmiv_is_device_ptr(mean) || !gmmiv_is_device_ptr(covinv)) GCHK(hipStreamSynchronize(c->stream)); // host sources may be freed by the caller on return
    b->loaded = true;
    return GMMIV_OK;
}

int gmmiv_gmm_batch_load(gmmiv_gmm_batch *b, const double *w, int64_t w_stride, const double *mean, int64_t mean_stride, const double *covinv,
                         int64_t covinv_stride)
{
    return batch_load(b, w, w_stride, mean, mean_stride, covinv, covinv_stride, false);
}
int gmmiv_gmm_batch_load_cov(gmmiv_gmm_batch *b, const double *w, int64_t w_stride, const double *mean, int64_t mean_stride, const double *cov,
                             int64_t cov_stride)
{
    return batch_load(b, w, w_stride, mean, mean_stride, cov, cov_stride, true);
}

static int check_batch(gmmiv_ctx *c, const gmmiv_gmm_batch *b, const char *who)
{
    if (!c || !b) { gmmiv_set_error("%s: NULL context or batch", who); return GMMIV_ERR_ARG; }
    if (b->ctx != c) { gmmiv_set_error("%s: the batch belongs to a different context", who); return GMMIV_ERR_ARG; }
    if (!b->loaded) { gmmiv_set_error("%s: the batch has no models yet (gmmiv_gmm_batch_load)", who); return GMMIV_ERR_ARG; }
    GBIND(c);
    return GMMIV_OK;
}

static int check_segments(const gmmiv_gmm_batch *b, const char *who, int64_t T, const int64_t *seg_begin, const int32_t *seg_model, int64_t nseg)
{
    if (T < 0 || nseg < 0 || !seg_begin || (nseg && !seg_model)) { gmmiv_set_error("%s: bad argument", who); return GMMIV_ERR_ARG; }
    if (gmmiv_is_device_ptr(seg_begin) || gmmiv_is_device_ptr(seg_model)) { gmmiv_set_error("%s: seg_begin and seg_model must be host arrays", who); return GMMIV_ERR_ARG; }
    if (nseg > 0x7fffffff / 64) { gmmiv_set_error("%s: too many segments in one call", who); return GMMIV_ERR_UNSUPPORTED; }
    if (seg_begin[0] < 0 || seg_begin[nseg] > T) { gmmiv_set_error("%s: seg_begin out of range", who); return GMMIV_ERR_ARG; }
    for (int64_t s = 0; s < nseg; ++s) {
        if (seg_begin[s + 1] < seg_begin[s]) { gmmiv_set_error("%s: seg_begin must be non-decreasing", who); return GMMIV_ERR_ARG; }
        if (seg_model[s] < 0 || seg_model[s] >= b->G) { gmmiv_set_error("%s: seg_model[%lld] = %d outside [0, %d)", who, (long long)s, seg_model[s], b->G); return GMMIV_ERR_ARG; }
    }
    return GMMIV_OK;
}

int gmmiv_gmm_batch_packed(const gmmiv_gmm_batch *b, int g, double *out, int64_t *len)
{
    if (!b || g < 0 || g >= b->G) { gmmiv_set_error("gmm_batch_packed: bad argument"); return GMMIV_ERR_ARG; }
    int rc = check_batch(b->ctx, b, "gmm_batch_packed");
    if (rc) return rc;
    if (b->KS == GMMK_KS_GENERIC) { gmmiv_set_error("gmm_batch_packed: vectSize %d has no packed operands", b->D); return GMMIV_ERR_UNSUPPORTED; }
    if (len) *len = (int64_t)b->packed_doubles();
    if (!out) return GMMIV_OK;
    gmmiv_ctx *c = b->ctx;
    void *pt, *ids;
    if ((rc = c->scratch(WS_MB_PT, b->packed_doubles() * sizeof(double), &pt))) return rc;
    if ((rc = c->scratch(WS_MB_IDS, sizeof(int), &ids))) return rc;
    GCHK(hipMemcpyAsync(ids, &g, sizeof(int), hipMemcpyHostToDevice, c->stream));
    GCHK(gmmk_pack_models(c->stream, 1, (const int *)ids, b->C, b->Cpa, b->D, b->KS, b->nct, b->mean, b->sm, b->iv, b->si, b->a, (double *)pt));
    GCHK(hipMemcpyAsync(out, pt, b->packed_doubles() * sizeof(double), gmmiv_is_device_ptr(out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    GCHK(hipStreamSynchronize(c->stream));
    return GMMIV_OK;
}

// ---- chunks of whole segments: frames that fit the scratch, distinct models that fit the packed-model scratch --------------------------
struct ModelChunk {
    int64_t s0, s1;      // segments [s0, s1)
    int64_t base;        // first frame of the chunk's coordinate system: the 16-frame block holding seg_begin[s0]
    size_t tile_off, ntiles, id_off, nids, seg_off;
    size_t ftile_off = 0, nftiles = 0; // gmmiv_feat_compensate_models: the chunk's entries of ModelPlan::ftiles
};
struct ModelPlan {
    std::vector<ModelChunk> chunks;
    std::vector<gmmiv_model_tile> tiles;
    std::vector<int> ids;
    std::vector<long> segrel;
    int feat_blocks = 0; // > 0: the work list of the segment-aware k_feat_comp is planned too, with this many blocks per entry
    std::vector<gmmiv_feat_tile> ftiles;
    const gmmiv_feat_tile *d_ftiles = nullptr;
    int64_t max_span = 0; // frames from a chunk's base to its end
    int max_models = 0;
    const gmmiv_model_tile *d_tiles = nullptr;
    const int *d_ids = nullptr;
    const long *d_seg = nullptr;
};

// false: a segment is longer than max_frames (the caller walks the segments one by one)
static bool plan_chunks(const gmmiv_gmm_batch *b, const int64_t *seg_begin, const int32_t *seg_model, int64_t nseg, int64_t max_frames, int max_models,
                        ModelPlan &p)
{
    std::vector<int> slot((size_t)b->G, -1);
    for (int64_t s0 = 0; s0 < nseg;) {
        ModelChunk ck;
        ck.s0 = s0;
        ck.base = seg_begin[s0] & ~(int64_t)15;
        ck.id_off = p.ids.size();
        int64_t s1 = s0;
        while (s1 < nseg) {
            const bool ne = seg_begin[s1 + 1] > seg_begin[s1];
            if (ne && seg_begin[s1 + 1] - ck.base > max_frames) break;
            if (ne && slot[seg_model[s1]] < 0) {
                if ((int)(p.ids.size() - ck.id_off) >= max_models) break;
                slot[seg_model[s1]] = (int)(p.ids.size() - ck.id_off);
                p.ids.push_back(seg_model[s1]);
            }
            ++s1;
        }
        if (s1 == s0) return false;
        ck.s1 = s1;
        ck.nids = p.ids.size() - ck.id_off;
        ck.seg_off = p.segrel.size();
        for (int64_t s = s0; s <= s1; ++s) p.segrel.push_back((long)(seg_begin[s] - ck.base));
        ck.tile_off = p.tiles.size();
        const int64_t nt = gmmiv_plan_model_tiles(seg_begin + s0, seg_model + s0, s1 - s0, MODEL_TILE_FRAMES, nullptr, 0);
        p.tiles.resize(ck.tile_off + (size_t)nt);
        gmmiv_plan_model_tiles(seg_begin + s0, seg_model + s0, s1 - s0, MODEL_TILE_FRAMES, p.tiles.data() + ck.tile_off, nt);
        for (size_t i = ck.tile_off; i < p.tiles.size(); ++i) {
            gmmiv_model_tile &t = p.tiles[i];
            t.first -= ck.base; t.lo -= ck.base; t.hi -= ck.base;
            t.model = slot[t.model];
        }
        ck.ntiles = (size_t)nt;
        if (p.feat_blocks > 0) { // the same coordinates and model slots for the consumer of the chunk's likelihoods
            ck.ftile_off = p.ftiles.size();
            const int64_t nf = gmmiv_plan_feat_tiles(seg_begin + s0, seg_model + s0, s1 - s0, p.feat_blocks, nullptr, 0);
            p.ftiles.resize(ck.ftile_off + (size_t)nf);
            gmmiv_plan_feat_tiles(seg_begin + s0, seg_model + s0, s1 - s0, p.feat_blocks, p.ftiles.data() + ck.ftile_off, nf);
            for (size_t i = ck.ftile_off; i < p.ftiles.size(); ++i) {
                gmmiv_feat_tile &t = p.ftiles[i];
                t.block -= ck.base / 16; t.lo -= ck.base; t.hi -= ck.base;
                t.model = slot[t.model];
            }
            ck.nftiles = (size_t)nf;
        }
        for (size_t i = ck.id_off; i < p.ids.size(); ++i) slot[p.ids[i]] = -1;
        const int64_t span = seg_begin[s1] - ck.base;
        if (span > p.max_span) p.max_span = span;
        if ((int)ck.nids > p.max_models) p.max_models = (int)ck.nids;
        p.chunks.push_back(ck);
        s0 = s1;
    }
    return true;
}

static int upload_plan(gmmiv_ctx *c, ModelPlan &p)
{
    void *dt, *di, *ds;
    int rc;
    if ((rc = c->scratch(WS_MB_TILES, p.tiles.size() * sizeof(gmmiv_model_tile), &dt))) return rc;
    if ((rc = c->scratch(WS_MB_IDS, p.ids.size() * sizeof(int), &di))) return rc;
    if ((rc = c->scratch(WS_MB_SEG, p.segrel.size() * sizeof(long), &ds))) return rc;
    if (!p.tiles.empty()) GCHK(hipMemcpyAsync(dt, p.tiles.data(), p.tiles.size() * sizeof(gmmiv_model_tile), hipMemcpyHostToDevice, c->stream));
    if (!p.ids.empty()) GCHK(hipMemcpyAsync(di, p.ids.data(), p.ids.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    GCHK(hipMemcpyAsync(ds, p.segrel.data(), p.segrel.size() * sizeof(long), hipMemcpyHostToDevice, c->stream));
    if (!p.ftiles.empty()) {
        void *df;
        if ((rc = c->scratch(WS_MB_FTILES, p.ftiles.size() * sizeof(gmmiv_feat_tile), &df))) return rc;
        GCHK(hipMemcpyAsync(df, p.ftiles.data(), p.ftiles.size() * sizeof(gmmiv_feat_tile), hipMemcpyHostToDevice, c->stream));
        p.d_ftiles = (const gmmiv_feat_tile *)df;
    }
    GCHK(hipStreamSynchronize(c->stream)); // the tables live in host vectors
    p.d_tiles = (const gmmiv_model_tile *)dt; p.d_ids = (const int *)di; p.d_seg = (const long *)ds;
    return GMMIV_OK;
}

static int models_per_chunk(const gmmiv_ctx *c, const gmmiv_gmm_batch *b)
{
    const size_t budget = (size_t)(c->models_scratch_mb > 0 ? c->models_scratch_mb : 0) << 20;
    const size_t n = budget / (b->packed_doubles() * sizeof(double));
    return n < 1 ? 1 : (n > 0x7fff ? 0x7fff : (int)n);
}

// frames per chunk of the stored-likelihood path (multiple of 256), 0 when it does not apply.  The budget of z_chunk_frames
// (capi_gmm_util.h); unlike it, it goes down to one tile: a call of short segments is served with any scratch that holds its longest
// segment.  24 (lse, 1 / S, Efin) and the rounding are pinned by results: they fix the summation order.
static int64_t models_chunk_frames(const gmmiv_ctx *c, const gmmiv_gmm_batch *b)
{
    if (!c->stats_z || b->KS > 15) return 0;
    return gmmiv_z_budget_frames(c, b->nct, 24) / 256 * 256;
}

static int pack_chunk(gmmiv_ctx *c, const gmmiv_gmm_batch *b, const ModelPlan &p, const ModelChunk &ck, double *pt, bool first)
{
    c->t_begin("k_gmm_pack", first);
    GCHK(gmmk_pack_models(c->stream, (int)ck.nids, p.d_ids + ck.id_off, b->C, b->Cpa, b->D, b->KS, b->nct, b->mean, b->sm, b->iv, b->si, b->a, pt));
    c->t_end();
    return GMMIV_OK;
}

// the packed models of the largest chunk of a plan
static int reserve_packed(gmmiv_ctx *c, const gmmiv_gmm_batch *b, const ModelPlan &p, double **pt)
{
    void *q;
    const int rc = c->scratch(WS_MB_PT, (size_t)(p.max_models ? p.max_models : 1) * b->packed_doubles() * sizeof(double), &q);
    *pt = (double *)q;
    return rc;
}

// The likelihood stage of one (non-empty) chunk, the same for every batched entry point: the unusable frames of its segments counted, its
// models packed into pt, k_llk_mfma over its tiles -- the log-sums into lse, indexed from ck.base; with a scratch view z the stored
// likelihoods too -- and the zero-likelihood frames of its segments counted.  first: this is the first chunk the call launches (the
// kernel timers restart); the flag is the caller's, which clears it after its own first launch.
static int llk_chunk(gmmiv_ctx *c, const gmmiv_gmm_batch *b, const XView &xv, int dt, const int64_t *seg_begin, const ModelPlan &p, const ModelChunk &ck,
                     double *pt, double *lse, const gmmk_zview *z, bool first)
{
    const int64_t f0 = seg_begin[ck.s0], n = seg_begin[ck.s1] - f0;
    int rc;
    XView sub;
    sub.d = gmmiv_x_at(xv, dt, f0); sub.ldx = xv.ldx;
    if ((rc = count_unusable(c, sub, dt, n, b->D))) return rc;
    if ((rc = pack_chunk(c, b, p, ck, pt, first))) return rc;
    const void *xb = gmmiv_x_at(xv, dt, ck.base);
    c->t_begin("k_llk_mfma", first);
    if (z)
        GCHK(gmmk_llk_z_models(c->stream, b->KS, dt == GMMIV_F64, xb, xv.ldx, b->D, pt, (long)b->packed_doubles(), b->nct, p.d_tiles + ck.tile_off,
                               (long)ck.ntiles, lse, (int)(c->use_glds & 1), *z));
    else
        GCHK(gmmk_llk_models(c->stream, b->KS, dt == GMMIV_F64, xb, xv.ldx, b->D, pt, (long)b->packed_doubles(), b->nct, p.d_tiles + ck.tile_off,
                             (long)ck.ntiles, lse, (int)(c->use_glds & 1)));
    c->t_end();
    GCHK(gmmk_count_dead(c->stream, lse + (f0 - ck.base), (long)n, c->d_zero_llk));
    return GMMIV_OK;
}

// ---- the walk for shapes / calls the batched kernel does not serve: one segment at a time on a single-model handle -----------------
struct OneModel {
    gmmiv_gmm *g = nullptr;
    int cur = -1;
    ~OneModel() { if (g) gmmiv_gmm_destroy(g); }
    int set(gmmiv_ctx *c, const gmmiv_gmm_batch *b, int m)
    {
        if (m == cur) return GMMIV_OK;
        const double *w = b->w + (size_t)m * b->sw, *mean = b->mean + (size_t)m * b->sm, *iv = b->iv + (size_t)m * b->si;
        const int rc = g ? gmmiv_gmm_set(g, w, mean, iv) : gmmiv_gmm_create(c, b->C, b->D, w, mean, iv, &g);
        if (!rc) cur = m;
        return rc;
    }
};

// The head of the walk for segment [f0, f0 + n) of xv under model m: the handle switched to the model, the segment as a view of its
// own with its unusable frames counted, its log-sums by the single-model kernel (run_lse: WS_LSE, zero-likelihood frames counted) and
// the one-segment table {0, n}.
static int walk_segment(gmmiv_ctx *c, const gmmiv_gmm_batch *b, OneModel &om, int m, const XView &xv, int dt, int64_t f0, int64_t n, XView *sub,
                        double **lse, long **sb)
{
    int rc;
    if ((rc = om.set(c, b, m))) return rc;
    sub->d = gmmiv_x_at(xv, dt, f0); sub->ldx = xv.ldx;
    if ((rc = count_unusable(c, *sub, dt, n, b->D))) return rc;
    if ((rc = run_lse(c, om.g, *sub, dt, n, lse))) return rc;
    void *p;
    if ((rc = c->scratch(WS_MB_SEG, 2 * sizeof(long), &p))) return rc;
    GCHK(gmmk_fill_chunks(c->stream, (long *)p, 1, (long)n, (long)n)); // {0, n}, written on the device
    *sb = (long *)p;
    return GMMIV_OK;
}

int gmmiv_llk_models(gmmiv_ctx *c, const gmmiv_gmm_batch *b, const void *x, int dt, int64_t T, int64_t ldx, const int64_t *seg_begin,
                     const int32_t *seg_model, int64_t nseg, double min_llk, double max_llk, double *llk, double *seg_sum)
{
    int rc = check_batch(c, b, "llk_models");
    if (rc) return rc;
    if ((rc = check_segments(b, "llk_models", T, seg_begin, seg_model, nseg))) return rc;
    if (nseg == 0) return GMMIV_OK;
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, b->D))) return rc;
    DevOut<double> o_llk, o_sum;
    if ((rc = o_llk.init(c, WS_T0, llk, (size_t)T, true))) return rc; // frames outside the segments keep what the caller has there
    if ((rc = o_sum.init(c, WS_T1, seg_sum, (size_t)nseg, false))) return rc;
    ModelPlan p;
    // the plain log-likelihood needs one double of scratch per frame: chunks by models, and by 16 M frames
    if (b->KS <= 15 && plan_chunks(b, seg_begin, seg_model, nseg, (int64_t)1 << 24, models_per_chunk(c, b), p)) {
        if ((rc = upload_plan(c, p))) return rc;
        double *pt;
        void *lse;
        if ((rc = reserve_packed(c, b, p, &pt))) return rc;
        if ((rc = c->scratch(WS_LSE, (size_t)(p.max_span > 0 ? p.max_span : 1) * sizeof(double), &lse))) return rc;
        bool first = true; // the first launch of the call restarts the kernel timers
        for (size_t k = 0; k < p.chunks.size(); ++k) {
            const ModelChunk &ck = p.chunks[k];
            if (seg_begin[ck.s1] > seg_begin[ck.s0]) {
                if ((rc = llk_chunk(c, b, xv, dt, seg_begin, p, ck, pt, (double *)lse, nullptr, first))) return rc;
                first = false;
            }
            GCHK(gmmk_llk_seg_finalize(c->stream, (const double *)lse, p.d_seg + ck.seg_off, (long)(ck.s1 - ck.s0), min_llk, max_llk,
                                       llk ? o_llk.d + ck.base : nullptr, seg_sum ? o_sum.d + ck.s0 : nullptr, nullptr));
        }
        if ((rc = o_llk.finish())) return rc;
        return o_sum.finish();
    }
    // launch-bound walk: per segment one model upload, the single-model log-likelihood kernel, the clamp
    OneModel om;
    if (seg_sum) GCHK(hipMemsetAsync(o_sum.d, 0, (size_t)nseg * sizeof(double), c->stream));
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t f0 = seg_begin[s], n = seg_begin[s + 1] - f0;
        if (n <= 0) continue;
        XView sub;
        double *lse;
        long *sb;
        if ((rc = walk_segment(c, b, om, seg_model[s], xv, dt, f0, n, &sub, &lse, &sb))) return rc;
        GCHK(gmmk_llk_seg_finalize(c->stream, lse, sb, 1, min_llk, max_llk, llk ? o_llk.d + f0 : nullptr, seg_sum ? o_sum.d + s : nullptr, nullptr));
    }
    if ((rc = o_llk.finish())) return rc;
    return o_sum.finish();
}

// N / F rows (second = false: gmmiv_tv_stats_models) or N / F / S rows (gmmiv_em_stats_models) of every segment under its model
static int stats_models(gmmiv_ctx *c, const gmmiv_gmm_batch *b, const void *x, int dt, int64_t T, int64_t ldx, const int64_t *seg_begin,
                        const int32_t *seg_model, int64_t nseg, double *N, double *F, double *S, double *seg_llk, bool second, const char *who)
{
    int rc = check_batch(c, b, who);
    if (rc) return rc;
    if ((rc = check_segments(b, who, T, seg_begin, seg_model, nseg))) return rc;
    if (!N || !F || (second && !S)) { gmmiv_set_error("%s: %s are required", who, second ? "N, F and S" : "N and F"); return GMMIV_ERR_ARG; }
    if (nseg == 0) return GMMIV_OK;
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, b->D))) return rc;
    const size_t SV = (size_t)b->C * b->D;
    DevOut<double> o_n, o_f, o_s, o_l;
    if ((rc = o_n.init(c, WS_T0, N, (size_t)nseg * b->C, false))) return rc;
    if ((rc = o_f.init(c, WS_T1, F, (size_t)nseg * SV, false))) return rc;
    if (second && (rc = o_s.init(c, WS_T5, S, (size_t)nseg * SV, false))) return rc;
    if ((rc = o_l.init(c, WS_T4, seg_llk, 2 * (size_t)nseg, false))) return rc;
    auto finish = [&]() { int r = o_n.finish(); if (!r) r = o_f.finish(); if (!r && second) r = o_s.finish(); if (!r) r = o_l.finish(); return r; };
    ModelPlan p;
    const int64_t Tc = models_chunk_frames(c, b);
    if (Tc > 0 && plan_chunks(b, seg_begin, seg_model, nseg, Tc, models_per_chunk(c, b), p)) {
        if ((rc = upload_plan(c, p))) return rc;
        gmmk_zview z;
        double *pt, *lse;
        if ((rc = reserve_packed(c, b, p, &pt))) return rc;
        if ((rc = gmmiv_z_reserve(c, b->nct, p.max_span, true, &z, &lse))) return rc;
        bool first = true; // the first launch of the call restarts the kernel timers
        for (size_t k = 0; k < p.chunks.size(); ++k) {
            const ModelChunk &ck = p.chunks[k];
            const void *xb = gmmiv_x_at(xv, dt, ck.base);
            if (seg_begin[ck.s1] > seg_begin[ck.s0]) {
                if ((rc = llk_chunk(c, b, xv, dt, seg_begin, p, ck, pt, lse, &z, first))) return rc;
                first = false;
            }
            // every (segment, c < C) row is written by exactly one wave (zeros for an empty segment, whose likelihood blocks are never read)
            c->t_begin("k_stats_z", k == 0);
            if (second) // the EM shape (x^2 accumulators) with the row epilogue
                GCHK(gmmk_stats_z_rows(c->stream, b->KS, dt == GMMIV_F64, xb, xv.ldx, b->D, b->C, b->nct, z, p.d_seg + ck.seg_off, (int)(ck.s1 - ck.s0),
                                       o_n.d + (size_t)ck.s0 * b->C, o_f.d + (size_t)ck.s0 * SV, o_s.d + (size_t)ck.s0 * SV, c->prune_thr()));
            else
                GCHK(gmmk_stats_z(c->stream, b->KS, 0, dt == GMMIV_F64, xb, xv.ldx, b->D, b->C, b->nct, z, 1.0, p.d_seg + ck.seg_off, (int)(ck.s1 - ck.s0),
                                  o_n.d + (size_t)ck.s0 * b->C, o_f.d + (size_t)ck.s0 * SV, 1, 0, c->prune_thr()));
            c->t_end();
            if (seg_llk)
                GCHK(gmmk_llk_seg_finalize(c->stream, lse, p.d_seg + ck.seg_off, (long)(ck.s1 - ck.s0), 0.0, 0.0, nullptr, nullptr, o_l.d + 2 * (size_t)ck.s0));
        }
        return finish();
    }
    // launch-bound walk: per segment one model upload, the single-model log-likelihood kernel and the recomputing statistics kernel
    // (k_stats_mfma; the generic posteriors + GEMM for vectSize > 80) -- what gmmiv_tv_stats runs when the stored-likelihood path
    // does not apply
    OneModel om;
    GCHK(hipMemsetAsync(o_n.d, 0, (size_t)nseg * b->C * sizeof(double), c->stream));
    GCHK(hipMemsetAsync(o_f.d, 0, (size_t)nseg * SV * sizeof(double), c->stream));
    if (second) GCHK(hipMemsetAsync(o_s.d, 0, (size_t)nseg * SV * sizeof(double), c->stream));
    if (seg_llk) GCHK(hipMemsetAsync(o_l.d, 0, 2 * (size_t)nseg * sizeof(double), c->stream));
    // second order: the single-model EM kernels fill a flat accumulator [occ | sum g x | sum g x^2] (zeroed per segment: they add),
    // unpacked into the segment's rows
    const size_t nacc = (size_t)b->C * (1 + 2 * b->D);
    void *accw = nullptr;
    if (second && (rc = c->scratch(WS_T6, nacc * sizeof(double), &accw))) return rc;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t f0 = seg_begin[s], n = seg_begin[s + 1] - f0;
        if (n <= 0) continue;
        XView sub;
        double *lse;
        long *sb;
        if ((rc = walk_segment(c, b, om, seg_model[s], xv, dt, f0, n, &sub, &lse, &sb))) return rc;
        const gmmiv_gmm *g = om.g;
        double *Nrow = o_n.d + (size_t)s * b->C, *Frow = o_f.d + (size_t)s * SV;
        if (second) {
            GCHK(hipMemsetAsync(accw, 0, nacc * sizeof(double), c->stream));
            if (g->KS == GMMK_KS_GENERIC) {
                const int NC = 2 * g->D + 2; // [x | 1 | x^2 | 0]
                void *Sg;
                if ((rc = c->scratch(WS_PART, (size_t)g->C * NC * sizeof(double), &Sg))) return rc;
                if ((rc = generic_gamma_gemm(c, g, sub, dt, 0, n, lse, true, NC, (double *)Sg))) return rc;
                GCHK(gmmk_scatter_em(c->stream, g->C, g->D, NC, (const double *)Sg, 1.0, (double *)accw));
            } else {
                void *part;
                if ((rc = c->scratch(WS_PART, (size_t)g->nct * 16 * 2 * gmmk_rl_for_ks(g->KS) * sizeof(double), &part))) return rc;
                c->t_begin("k_stats_mfma", s == 0);
                GCHK(gmmk_stats(c->stream, g->KS, 1, dt == GMMIV_F64, sub.d, sub.ldx, g->D, g->C, g->Pt, g->nct, lse, 0.0, sb, 1, (double *)part, nullptr, 0,
                                (int)c->wg_waves, c->prune_arg()));
                c->t_end();
                GCHK(gmmk_em_reduce(c->stream, (const double *)part, 1, g->C, g->nct * 16, g->D, g->KS, (double *)accw));
            }
            GCHK(gmmk_acc_to_rows(c->stream, g->C, g->D, (const double *)accw, Nrow, Frow, o_s.d + (size_t)s * SV));
        } else if (g->KS == GMMK_KS_GENERIC) {
            const int NC = g->D + 2 - (g->D & 1); // [x | 1] padded to an even width
            void *S;
            if ((rc = c->scratch(WS_PART, (size_t)g->C * NC * sizeof(double), &S))) return rc;
            if ((rc = generic_gamma_gemm(c, g, sub, dt, 0, n, lse, false, NC, (double *)S))) return rc;
            GCHK(gmmk_scatter_nf(c->stream, g->C, g->D, NC, (const double *)S, Nrow, Frow));
        } else {
            c->t_begin("k_stats_mfma", s == 0);
            GCHK(gmmk_stats(c->stream, g->KS, 0, dt == GMMIV_F64, sub.d, sub.ldx, g->D, g->C, g->Pt, g->nct, lse, 0.0, sb, 1, Nrow, Frow, 1,
                            (int)c->wg_waves, c->prune_arg()));
            c->t_end();
        }
        if (seg_llk) GCHK(gmmk_llk_seg_finalize(c->stream, lse, sb, 1, 0.0, 0.0, nullptr, nullptr, o_l.d + 2 * (size_t)s));
    }
    return finish();
}

int gmmiv_tv_stats_models(gmmiv_ctx *c, const gmmiv_gmm_batch *b, const void *x, int dt, int64_t T, int64_t ldx, const int64_t *seg_begin,
                          const int32_t *seg_model, int64_t nseg, double *N, double *F, double *seg_llk)
{
    return stats_models(c, b, x, dt, T, ldx, seg_begin, seg_model, nseg, N, F, nullptr, seg_llk, false, "tv_stats_models");
}
int gmmiv_em_stats_models(gmmiv_ctx *c, const gmmiv_gmm_batch *b, const void *x, int dt, int64_t T, int64_t ldx, const int64_t *seg_begin,
                          const int32_t *seg_model, int64_t nseg, double *N, double *F, double *S, double *seg_llk)
{
    return stats_models(c, b, x, dt, T, ldx, seg_begin, seg_model, nseg, N, F, S, seg_llk, true, "em_stats_models");
}

// ---- channel compensation with a session model and an offset per segment (include/gmmiv.h) --------------------------------------------
int gmmiv_feat_compensate_models(gmmiv_ctx *c, const gmmiv_gmm_batch *b, const void *x, int dt, int64_t T, int64_t ldx, const int64_t *seg_begin,
                                 const int32_t *seg_model, int64_t nseg, const double *offset, int64_t offset_stride, void *out, int odt, int64_t ldo)
{
    const char *who = "feat_compensate_models";
    int rc = check_batch(c, b, who);
    if (rc) return rc;
    if ((rc = check_segments(b, who, T, seg_begin, seg_model, nseg))) return rc;
    if (!offset) { gmmiv_set_error("%s: offset == NULL", who); return GMMIV_ERR_ARG; }
    const size_t CD = (size_t)b->C * b->D;
    if (offset_stride && offset_stride < (int64_t)CD) { gmmiv_set_error("%s: offset_stride must be 0 (shared) or at least C * D", who); return GMMIV_ERR_ARG; }
    if ((rc = gmmiv_feat_check_args(who, x, dt, T, ldx, out, odt, ldo, b->D))) return rc;
    const int64_t F0 = seg_begin[0], F1 = seg_begin[nseg]; // every frame of [F0, F1) belongs to a segment, no other frame does
    if (T == 0 || nseg == 0 || F1 == F0) return GMMIV_OK;
    XView xv;
    if ((rc = xv.init(c, x, dt, T, ldx, b->D))) return rc;
    // the output as a device view indexed like x: a host output is staged for the frames [F0, F1) alone, so that frames of no segment
    // and padding columns keep what the caller has there
    FeatOut o;
    if ((rc = o.init(c, out, odt, F0, F1, ldo, b->D))) return rc;
    DevIn<double> i_off;
    if ((rc = i_off.init(c, WS_MB_OFFSRC, offset, offset_stride ? (size_t)(b->G - 1) * offset_stride + CD : CD))) return rc;
    ModelPlan p;
    p.feat_blocks = gmmk_feat_blocks_per_tile();
    const int64_t Tc = models_chunk_frames(c, b); // (0 for vectSize > 60: k_feat_comp serves every shape the stored likelihoods exist for)
    if (Tc > 0 && plan_chunks(b, seg_begin, seg_model, nseg, Tc, models_per_chunk(c, b), p)) {
        if ((rc = upload_plan(c, p))) return rc;
        const size_t offd = gmmk_feat_offset_doubles(b->nct, b->D);
        void *offp;
        gmmk_zview z;
        double *pt, *lse;
        if ((rc = reserve_packed(c, b, p, &pt))) return rc;
        if ((rc = c->scratch(WS_MB_OFF, (size_t)(p.max_models ? p.max_models : 1) * offd * sizeof(double), &offp))) return rc;
        if ((rc = gmmiv_z_reserve(c, b->nct, p.max_span, true, &z, &lse))) return rc;
        bool first = true; // the first launch of the call restarts the kernel timers
        for (size_t k = 0; k < p.chunks.size(); ++k) {
            const ModelChunk &ck = p.chunks[k];
            if (seg_begin[ck.s1] <= seg_begin[ck.s0]) continue;
            // In place across a chunk boundary: the log-likelihood kernel loads the rows of its tiles outside their segments as 0, so a
            // row of a shared 16-frame block that the previous chunk has rewritten is never evaluated; k_feat_comp loads the rows it
            // writes and no others.
            if ((rc = llk_chunk(c, b, xv, dt, seg_begin, p, ck, pt, lse, &z, first))) return rc;
            c->t_begin("k_gmm_pack", false); // the offsets of the chunk's models, in the order of its model slots
            GCHK(gmmk_feat_pack_offsets(c->stream, (int)ck.nids, p.d_ids + ck.id_off, i_off.d, (long)offset_stride, b->C, b->D, b->nct, (double *)offp));
            c->t_end();
            c->t_begin("k_feat_comp", first);
            first = false;
            GCHK(gmmk_feat_comp_models(c->stream, dt == GMMIV_F64, odt == GMMIV_F64, gmmiv_x_at(xv, dt, ck.base), xv.ldx, (long)(seg_begin[ck.s1] - ck.base), b->D,
                                       b->nct, z, (const double *)offp, (long)offd, p.d_ftiles + ck.ftile_off, (long)ck.nftiles, o.at(ck.base), o.ld));
            c->t_end();
        }
        return o.finish();
    }
    // launch-bound walk: per segment one model upload and gmmiv_feat_compensate on the single-model handle (device views throughout,
    // so it stages nothing; it counts its own unusable and zero-likelihood frames)
    OneModel om;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t f0 = seg_begin[s], n = seg_begin[s + 1] - f0;
        if (n <= 0) continue;
        if ((rc = om.set(c, b, seg_model[s]))) return rc;
        if ((rc = gmmiv_feat_compensate(c, om.g, gmmiv_x_at(xv, dt, f0), dt, n, xv.ldx, i_off.d + (size_t)seg_model[s] * offset_stride, o.at(f0), odt, o.ld)))
            return rc;
    }
    return o.finish();
}

// ---- computeMAP for the batch -----------------------------------------------------------------------------------------------------------
int gmmiv_map_adapt_models(gmmiv_ctx *c, int G, int C, int D, const double *N, const double *F, const double *count, int64_t count_stride,
                           const double *w0, const double *mean0, const double *cur_mean, int64_t cur_stride, int method, int mean_adapt,
                           int weight_adapt, double mean_reg, double weight_reg, double mean_alpha, double *mean_out, double *w_out)
{
    if (!c || G < 0 || C <= 0 || D <= 0 || !N || !F || !count || count_stride < 1 || !w0 || !mean0 || !cur_mean || cur_stride < 0 || !mean_out ||
        method < GMMIV_MAP_NONE || method > GMMIV_MAP_CONST2) {
        gmmiv_set_error("map_adapt_models: bad argument");
        return GMMIV_ERR_ARG;
    }
    const size_t CD = (size_t)C * D;
    if (cur_stride && cur_stride < (int64_t)CD) { gmmiv_set_error("map_adapt_models: cur_stride must be 0 (shared) or at least C * D"); return GMMIV_ERR_ARG; }
    if (G == 0) return GMMIV_OK;
    GBIND(c);
    int rc;
    DevIn<double> i_n, i_f, i_c, i_w0, i_m0, i_cur;
    DevOut<double> o_m, o_w;
    if ((rc = i_n.init(c, WS_T2, N, (size_t)G * C)) || (rc = i_f.init(c, WS_T3, F, (size_t)G * CD)) ||
        (rc = i_c.init(c, WS_T4, count, (size_t)(G - 1) * count_stride + 1)) || (rc = i_w0.init(c, WS_T5, w0, (size_t)C)) ||
        (rc = i_m0.init(c, WS_T6, mean0, CD)) || (rc = i_cur.init(c, WS_T7, cur_mean, cur_stride ? (size_t)(G - 1) * cur_stride + CD : CD)) ||
        (rc = o_m.init(c, WS_T8, mean_out, (size_t)G * CD, false)) || (rc = o_w.init(c, WS_T9, w_out, (size_t)G * C, false)))
        return rc;
    c->t_begin("k_map_adapt");
    GCHK(gmmk_map_adapt_models(c->stream, G, C, D, i_n.d, i_f.d, i_c.d, (long)count_stride, i_w0.d, i_m0.d, i_cur.d, (long)cur_stride, method, mean_adapt,
                               weight_adapt, mean_reg, weight_reg, mean_alpha, o_m.d, w_out ? o_w.d : nullptr));
    c->t_end();
    if ((rc = o_m.finish())) return rc;
    if ((rc = o_w.finish())) return rc;
    // host inputs were staged with asynchronous copies from the caller's arrays
    if (!o_m.host && !o_w.host && !(gmmiv_is_device_ptr(N) && gmmiv_is_device_ptr(F) && gmmiv_is_device_ptr(count) && gmmiv_is_device_ptr(w0) &&
                                    gmmiv_is_device_ptr(mean0) && gmmiv_is_device_ptr(cur_mean)))
        GCHK(hipStreamSynchronize(c->stream));
    return GMMIV_OK;
}

int gmmiv_map_adapt_models_full(gmmiv_ctx *c, int G, int C, int D, const double *N, const double *F, const double *S, const double *count,
                                int64_t count_stride, const double *w0, const double *mean0, const double *cov0, const double *cur_mean,
                                int64_t cur_mean_stride, const double *cur_cov, int64_t cur_cov_stride, int method, int mean_adapt, int var_adapt,
                                int weight_adapt, double mean_reg, double var_reg, double weight_reg, double mean_alpha, double *mean_out,
                                double *cov_out, double *w_out, int32_t *status)
{
    if (!c || G < 0 || C <= 0 || D <= 0 || !N || !F || !count || count_stride < 1 || !w0 || !mean0 || !cov0 || !cur_mean || cur_mean_stride < 0 ||
        cur_cov_stride < 0 || (!mean_out && !cov_out && !w_out) || !status || method < GMMIV_MAP_NONE || method > GMMIV_MAP_CONST2) {
        gmmiv_set_error("map_adapt_models_full: bad argument");
        return GMMIV_ERR_ARG;
    }
    const size_t CD = (size_t)C * D;
    const bool ml_cov = cov_out && (method == GMMIV_MAP_NONE || (var_adapt && (method == GMMIV_MAP_OCC_DEP || method == GMMIV_MAP_MODEL_BASED)));
    if (ml_cov && (!S || !cur_cov)) { gmmiv_set_error("map_adapt_models_full: this configuration reads S and cur_cov"); return GMMIV_ERR_ARG; }
    if ((cur_mean_stride && cur_mean_stride < (int64_t)CD) || (cur_cov_stride && cur_cov_stride < (int64_t)CD)) {
        gmmiv_set_error("map_adapt_models_full: a stride must be 0 (shared) or at least C * D");
        return GMMIV_ERR_ARG;
    }
    if (G == 0) return GMMIV_OK;
    GBIND(c);
    int rc;
    auto span = [&](int64_t stride) { return stride ? (size_t)(G - 1) * stride + CD : CD; };
    DevIn<double> i_n, i_f, i_s, i_c, i_w0, i_m0, i_c0, i_cm, i_cc;
    DevOut<double> o_m, o_v, o_w;
    DevOut<int32_t> o_st;
    if ((rc = i_n.init(c, WS_T2, N, (size_t)G * C)) || (rc = i_f.init(c, WS_T3, F, (size_t)G * CD)) || (rc = i_s.init(c, WS_T0, ml_cov ? S : nullptr, (size_t)G * CD)) ||
        (rc = i_c.init(c, WS_T4, count, (size_t)(G - 1) * count_stride + 1)) || (rc = i_w0.init(c, WS_T5, w0, (size_t)C)) ||
        (rc = i_m0.init(c, WS_T6, mean0, CD)) || (rc = i_c0.init(c, WS_T1, cov0, CD)) || (rc = i_cm.init(c, WS_T7, cur_mean, span(cur_mean_stride))) ||
        (rc = i_cc.init(c, WS_TIV, ml_cov ? cur_cov : nullptr, span(cur_cov_stride))) || (rc = o_m.init(c, WS_T8, mean_out, (size_t)G * CD, false)) ||
        (rc = o_v.init(c, WS_LP, cov_out, (size_t)G * CD, false)) || (rc = o_w.init(c, WS_T9, w_out, (size_t)G * C, false)) ||
        (rc = o_st.init(c, WS_AUX, status, (size_t)G, false)))
        return rc;
    c->t_begin("k_map_adapt");
    GCHK(gmmk_map_adapt_models_full(c->stream, G, C, D, i_n.d, i_f.d, i_s.d, i_c.d, (long)count_stride, i_w0.d, i_m0.d, i_c0.d, i_cm.d, (long)cur_mean_stride,
                                    i_cc.d, (long)cur_cov_stride, method, mean_adapt, var_adapt, weight_adapt, mean_reg, var_reg, weight_reg, mean_alpha,
                                    mean_out ? o_m.d : nullptr, cov_out ? o_v.d : nullptr, w_out ? o_w.d : nullptr, o_st.d));
    c->t_end();
    if ((rc = o_m.finish()) || (rc = o_v.finish()) || (rc = o_w.finish()) || (rc = o_st.finish())) return rc;
    // host inputs were staged with asynchronous copies from the caller's arrays
    const void *ins[] = {N, F, ml_cov ? S : nullptr, count, w0, mean0, cov0, cur_mean, ml_cov ? cur_cov : nullptr};
    bool host_in = false;
    for (const void *q : ins) host_in |= q && !gmmiv_is_device_ptr(q);
    if (host_in && !o_m.host && !o_v.host && !o_w.host && !o_st.host) GCHK(hipStreamSynchronize(c->stream));
    return GMMIV_OK;
}

int gmmiv_normalize_models(gmmiv_ctx *c, int G, int C, int D, const double *w, int64_t w_stride, double *mean, double *cov, int nb_it, int mean_only)
{
    if (!c || G < 0 || C <= 0 || D <= 0 || !w || !mean || !cov || nb_it < 0 || (w_stride && w_stride < C)) {
        gmmiv_set_error("normalize_models: bad argument (cov is read in either mode: the fusion needs the variances)");
        return GMMIV_ERR_ARG;
    }
    if (!gmmiv_is_device_ptr(mean) || !gmmiv_is_device_ptr(cov)) { gmmiv_set_error("normalize_models: mean and cov are device arrays (updated in place)"); return GMMIV_ERR_ARG; }
    if (G == 0 || nb_it == 0) return GMMIV_OK;
    GBIND(c);
    DevIn<double> i_w;
    int rc = i_w.init(c, WS_T0, w, w_stride ? (size_t)(G - 1) * w_stride + C : (size_t)C);
    if (rc) return rc;
    c->t_begin("k_normalize_models");
    GCHK(gmmk_normalize_models(c->stream, G, C, D, i_w.d, (long)w_stride, mean, cov, nb_it, mean_only));
    c->t_end();
    if (!gmmiv_is_device_ptr(w)) GCHK(hipStreamSynchronize(c->stream));
    return GMMIV_OK;
}

} // extern "C"
