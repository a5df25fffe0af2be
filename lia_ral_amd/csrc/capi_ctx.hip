// capi_ctx.hip -- C ABI (include/gmmiv.h): the thread-local error and kernel-option state, the context, the model handle.
#include <stdarg.h>
#include <stdlib.h>

#include "ctx.h"
#include "gmm_kernels.h"

static thread_local char g_err[512] = "";

// The bound set is a COPY (52 bytes per call): a thread that last drove a context which another thread has destroyed since holds no
// pointer into freed memory; g_kopts_src is kept for the identity test of "kopts_bound" only and never dereferenced.
static thread_local gmmiv_kopts g_kopts_val;
static thread_local const gmmiv_kopts *g_kopts_src = nullptr;
const gmmiv_kopts &gmmiv_kopts_cur() { return g_kopts_val; }
void gmmiv_kopts_bind(const gmmiv_kopts *ko) { g_kopts_val = ko ? *ko : gmmiv_kopts(); g_kopts_src = ko; }

void gmmiv_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

bool gmmiv_is_device_ptr(const void *p)
{
    if (!p) return false;
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError(); // plain malloc'ed host memory on older runtimes
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

extern "C" {

const char *gmmiv_last_error(void) { return g_err; }
const char *gmmiv_version(void) { return "gmmiv 0.1 (gfx950)"; }

int gmmiv_ctx_create(int device, void *stream, gmmiv_ctx **out)
{
    if (!out) { gmmiv_set_error("ctx_create: out == NULL"); return GMMIV_ERR_ARG; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        gmmiv_set_error("ctx_create: no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return GMMIV_ERR_HIP;
    }
    if (device < 0 || device >= ndev) { gmmiv_set_error("ctx_create: device %d out of range [0,%d)", device, ndev); return GMMIV_ERR_ARG; }
    GCHK(hipSetDevice(device));
    gmmiv_ctx *c = new gmmiv_ctx();
    c->device = device;
    if (stream == GMMIV_STREAM_DEFAULT || stream == (void *)hipStreamLegacy) { c->stream = nullptr; c->own_stream = false; } // the NULL stream itself
    else if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else { GCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) { c->n_cu = prop.multiProcessorCount; c->total_mem = prop.totalGlobalMem; }
    if (hipMalloc((void **)&c->d_zero_llk, 2 * sizeof(unsigned long long)) != hipSuccess || hipMemset(c->d_zero_llk, 0, 2 * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        if (c->own_stream) (void)hipStreamDestroy(c->stream);
        delete c;
        gmmiv_set_error("ctx_create: hipMalloc of the context's device counters failed");
        return GMMIV_ERR_HIP;
    }
    c->d_screened = c->d_zero_llk + 1;
    *out = c;
    return GMMIV_OK;
}

void gmmiv_ctx_destroy(gmmiv_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (gmmiv_comm *cm : std::vector<gmmiv_comm *>(c->comms)) gmmiv_comm_orphan(cm); // their handles stay valid for gmmiv_comm_destroy
    for (int i = 0; i < WS_COUNT; ++i)
        if (c->ws[i]) (void)hipFree(c->ws[i]);
    for (int i = 0; i < gmmiv_ctx::NSLOT; ++i) {
        for (hipEvent_t e : c->ev0[i]) (void)hipEventDestroy(e);
        for (hipEvent_t e : c->ev1[i]) (void)hipEventDestroy(e);
    }
    if (c->d_zero_llk) (void)hipFree(c->d_zero_llk);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    if (g_kopts_src == &c->ko) gmmiv_kopts_bind(nullptr); // back to the defaults on this thread
    delete c;
}

int gmmiv_ctx_sync(gmmiv_ctx *c)
{
    if (!c) return GMMIV_ERR_ARG;
    GCHK(hipStreamSynchronize(c->stream));
    return GMMIV_OK;
}

void *gmmiv_ctx_stream(gmmiv_ctx *c) { return c ? (void *)c->stream : nullptr; }

long gmmiv_ctx_set_option(gmmiv_ctx *c, const char *key, long value)
{
    if (!c || !key) return -1;
    long *slot = nullptr;
    if (!strcmp(key, "glds")) slot = &c->use_glds;
    else if (!strcmp(key, "em_chunks")) slot = &c->em_chunks;
    else if (!strcmp(key, "timing")) slot = &c->timing;
    else if (!strcmp(key, "wg_waves")) slot = &c->wg_waves;
    else if (!strcmp(key, "dbg")) slot = &c->dbg;
    else if (!strcmp(key, "prune_log2")) slot = &c->prune_log2;
    else if (!strcmp(key, "stats_z")) slot = &c->stats_z;
    else if (!strcmp(key, "z_scratch_mb")) slot = &c->z_scratch_mb;
    else if (!strcmp(key, "models_scratch_mb")) slot = &c->models_scratch_mb;
    else if (!strcmp(key, "trials_scratch_mb")) slot = &c->trials_scratch_mb;
    else if (!strcmp(key, "trials_piece")) slot = &c->trials_piece;
    else if (!strcmp(key, "iv_trials_anchor")) slot = &c->iv_trials_anchor;
    else if (!strcmp(key, "iv_trials_piece")) slot = &c->iv_trials_piece;
    else if (!strcmp(key, "tv_batch")) slot = &c->tv_batch;
    else if (!strcmp(key, "tv_tett_direct")) slot = &c->tv_tett_direct;
    else if (!strcmp(key, "tv_stats_split")) slot = &c->tv_stats_split;
    else if (!strcmp(key, "topc_z")) slot = &c->topc_z;
    else if (!strcmp(key, "tv_mstep_solve")) slot = &c->tv_mstep_solve;
    else if (!strcmp(key, "tv_md_device")) slot = &c->tv_md_device;
    else if (!strcmp(key, "tv_acc_mb")) slot = &c->tv_acc_mb;
    else if (!strcmp(key, "topc_fused")) slot = &c->topc_fused;
    else if (!strcmp(key, "topc_fallbacks")) slot = &c->topc_fallbacks;
    else if (!strcmp(key, "topc_rank_direct")) slot = &c->topc_rank_direct;
    else if (!strcmp(key, "topc_rank2")) slot = &c->topc_rank2;
    else if (!strcmp(key, "topc_use_lanes")) slot = &c->topc_use_lanes;
    else if (!strcmp(key, "assume_finite")) slot = &c->assume_finite;
    // options read by the kernel launchers: kept in the context's gmmiv_kopts, bound to the calling thread by every call (GBIND)
    int *ks = nullptr;
    if (!strcmp(key, "z_waves")) { const long prev = c->ko.z_waves; c->ko.z_waves = (value == 4 || value == 16) ? (int)value : 8; return prev; }
    if (!strcmp(key, "z_depth_em")) { const long prev = c->ko.z_depth_em; if (value == 2 || value == 4) c->ko.z_depth_em = (int)value; return prev; }
    if (!strcmp(key, "z_depth_tv")) { const long prev = c->ko.z_depth_tv; if (value == 2 || value == 4) c->ko.z_depth_tv = (int)value; return prev; }
    if (!strcmp(key, "z_tv4")) ks = &c->ko.z_tv4;                 // A/B knob: 0 = two Gaussian tiles per wave in the N / F mode of k_stats_z
    else if (!strcmp(key, "gemm_remap")) ks = &c->ko.gemm_remap;   // A/B knob: 2 = 8 x 8 tile blocks per XCD, 1 = M tiles fastest per XCD (rounds 2-4), 0 = hardware tile order in k_dgemm
    else if (!strcmp(key, "gemm_clamp")) ks = &c->ko.gemm_clamp;   // A/B knob: 0 = cut GEMM tiles on the per-element checked instantiation
    else if (!strcmp(key, "gemm_narrow")) ks = &c->ko.gemm_narrow; // A/B knob: 0 = 128 x 128 tiles on the strips cut by M / N too
    else if (!strcmp(key, "gemm_nt80")) ks = &c->ko.gemm_nt80;     // A/B knob: 0 = no 128 x 80 tiles for N = 5 x 80 (aux at rank 400)
    else if (!strcmp(key, "chol_lds")) ks = &c->ko.chol_lds;       // 0 = panel rows from memory per wave
    else if (!strcmp(key, "chol_gemm")) ks = &c->ko.chol_gemm;     // the GEMM-built batched Cholesky instead of k_chol_left
    else if (!strcmp(key, "chol_waves")) ks = &c->ko.chol_waves;   // 16 = k_trinv_left / k_uut on 1024-thread workgroups
    else if (!strcmp(key, "short_calls")) ks = &c->ko.short_calls; // 0 = calls of at most 32768 frames on the kernel shapes of long calls
    else if (!strcmp(key, "chol_flow")) ks = &c->ko.chol_flow;     // 0 = the round-2 k_chol_left (diagonal update from L2, eight partial blocks)
    if (ks) { const long prev = *ks; *ks = (int)value; return prev; }
    // the device counters of kind-(2) frames (zero likelihood under the call's model -- this INCLUDES the kind-(1) frames, which every
    // kernel evaluates as such) and of kind-(1) frames (unusable feature values, counted by the screening pass): reading one waits
    // for the stream, the counting itself never does
    if (!strcmp(key, "zero_llk_frames") || !strcmp(key, "screened_frames")) {
        unsigned long long *ctr = key[0] == 'z' ? c->d_zero_llk : c->d_screened;
        unsigned long long prev = 0, nv = value > 0 ? (unsigned long long)value : 0;
        if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(&prev, ctr, sizeof prev, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(ctr, &nv, sizeof nv, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return -1; }
        return (long)prev;
    }
    if (!strcmp(key, "kopts_bound")) return g_kopts_src == &c->ko ? 1 : 0; // read-only: is this context's set the one bound to the calling thread?
    if (!slot) return -1;
    long prev = *slot;
    *slot = value;
    return prev;
}

int gmmiv_ctx_set_hook(gmmiv_ctx *c, const char *point, gmmiv_hook_fn fn, void *user)
{
    if (!c || !point) return -1;
    gmmiv_ctx::Hook *h = !strcmp(point, "tv_a_ready") ? &c->hook_tv_a_ready : (!strcmp(point, "md_factored") ? &c->hook_md_factored : nullptr);
    if (!h) return -1;
    h->fn = fn;
    h->user = fn ? user : nullptr;
    return 0;
}

double gmmiv_ctx_last_kernel_ms(gmmiv_ctx *c, const char **name)
{
    if (!c || c->ev_last < 0) return -1.0;
    if (name) *name = c->ev_name[c->ev_last];
    return c->t_query(c->ev_last);
}

double gmmiv_ctx_kernel_ms(gmmiv_ctx *c, const char *name)
{
    if (!c || !name) return -1.0;
    for (int i = 0; i < gmmiv_ctx::NSLOT; ++i)
        if (c->ev_name[i] && !strcmp(c->ev_name[i], name)) return c->t_query(i);
    return -1.0;
}

long gmmiv_ctx_kernel_launches(gmmiv_ctx *c, const char *name)
{
    if (!c || !name) return -1;
    for (int i = 0; i < gmmiv_ctx::NSLOT; ++i)
        if (c->ev_name[i] && !strcmp(c->ev_name[i], name)) return c->ev_used[i];
    return -1;
}

// ---- model -------------------------------------------------------------------------------
static int gmm_upload(gmmiv_gmm *g, const double *w, const double *mean, const double *covinv)
{
    gmmiv_ctx *c = g->ctx;
    GBIND(c);
    const size_t CD = (size_t)g->C * g->D;
    auto kind = [](const void *p) { return gmmiv_is_device_ptr(p) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice; };
    GCHK(hipMemcpyAsync(g->w, w, g->C * sizeof(double), kind(w), c->stream));
    GCHK(hipMemcpyAsync(g->mean, mean, CD * sizeof(double), kind(mean), c->stream));
    GCHK(hipMemcpyAsync(g->iv, covinv, CD * sizeof(double), kind(covinv), c->stream));
    GCHK(gmmk_pack_model(c->stream, g->C, g->D, g->KS, g->nct, g->Cp64, g->w, g->mean, g->iv, g->a, g->lwc, g->Pt,
                         g->meanT, g->ivT));
    GCHK(hipStreamSynchronize(c->stream)); // host sources may be freed by the caller on return
    return GMMIV_OK;
}

int gmmiv_gmm_create(gmmiv_ctx *c, int C, int D, const double *w, const double *mean, const double *covinv,
                     gmmiv_gmm **out)
{
    if (!c || !out || !w || !mean || !covinv || C <= 0 || D <= 0) { gmmiv_set_error("gmm_create: bad argument"); return GMMIV_ERR_ARG; }
    const int KS = gmmk_ks_for_dim(D);
    if (!KS) { gmmiv_set_error("gmm_create: vectSize %d not supported (max %d)", D, GMMK_MAX_DIM); return GMMIV_ERR_UNSUPPORTED; }
    // KS == GMMK_KS_GENERIC (vectSize > 80): no packed MFMA model; every entry point takes its generic path (VALU logits in the
    // reference's direct form, statistics as gamma^T [x | 1 | x^2] on the fp64 GEMM) -- slower, same results, nothing refused
    GBIND(c);
    gmmiv_gmm *g = new gmmiv_gmm();
    g->ctx = c; g->C = C; g->D = D; g->KS = KS;
    g->nct = ((C + 15) / 16 + 1) / 2 * 2; // c-tiles of 16, padded to the LLK kernel's stage of 2
    g->Cp64 = (C + 63) / 64 * 64;
    const size_t CD = (size_t)C * D;
    const int Cpa = g->Cp64 > g->nct * 16 ? g->Cp64 : g->nct * 16;
    struct { void **p; size_t n; } need[] = {{(void **)&g->w, (size_t)C}, {(void **)&g->mean, CD}, {(void **)&g->iv, CD}, {(void **)&g->a, (size_t)Cpa},
                                           {(void **)&g->lwc, (size_t)Cpa}, {(void **)&g->Pt, KS == GMMK_KS_GENERIC ? (size_t)64 : (size_t)g->nct * (2 * KS + 2) * 64},
                                           {(void **)&g->meanT, (size_t)D * g->Cp64}, {(void **)&g->ivT, (size_t)D * g->Cp64}};
    for (auto &a : need) {
        const hipError_t e = hipMalloc(a.p, a.n * sizeof(double));
        if (e != hipSuccess) { // nothing allocated so far may leak
            gmmiv_set_error("gmm_create: hipMalloc of %zu bytes -> %s", a.n * sizeof(double), hipGetErrorString(e));
            gmmiv_gmm_destroy(g);
            return GMMIV_ERR_HIP;
        }
    }
    int rc = gmm_upload(g, w, mean, covinv);
    if (rc) { gmmiv_gmm_destroy(g); return rc; }
    *out = g;
    return GMMIV_OK;
}

int gmmiv_gmm_set(gmmiv_gmm *g, const double *w, const double *mean, const double *covinv)
{
    if (!g || !w || !mean || !covinv) { gmmiv_set_error("gmm_set: bad argument"); return GMMIV_ERR_ARG; }
    return gmm_upload(g, w, mean, covinv);
}

int gmmiv_gmm_set_cov(gmmiv_gmm *g, const double *w, const double *mean, const double *cov)
{
    if (!g || !w || !mean || !cov) { gmmiv_set_error("gmm_set_cov: bad argument"); return GMMIV_ERR_ARG; }
    gmmiv_ctx *c = g->ctx;
    GBIND(c);
    const size_t CD = (size_t)g->C * g->D;
    DevIn<double> i_cov;
    int rc = i_cov.init(c, WS_T0, cov, CD);
    if (rc) return rc;
    void *p;
    if ((rc = c->scratch(WS_T1, CD * sizeof(double), &p))) return rc;
    GCHK(gmmk_reciprocal(c->stream, (long)CD, i_cov.d, (double *)p));   // covInv = 1 / cov (DistribGD::computeAll)
    return gmm_upload(g, w, mean, (const double *)p);
}

void gmmiv_gmm_destroy(gmmiv_gmm *g)
{
    if (!g) return;
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);
    void *ptrs[] = {g->w, g->mean, g->iv, g->a, g->lwc, g->Pt, g->meanT, g->ivT};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete g;
}

} // extern "C"
