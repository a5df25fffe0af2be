// capi_gmm_util.h -- helpers of capi_gmm.hip that capi_models.hip uses too (internal).
#pragma once
#include "ctx.h"

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

extern "C" {
int gmmiv_i_count_unusable(gmmiv_ctx *c, const XView &xv, int dt, int64_t T, int D);  // the "screened_frames" pass over T frames
int gmmiv_i_run_lse(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t T, double **lse_out); // WS_LSE; counts zero-likelihood frames
int gmmiv_i_generic_gamma_gemm(gmmiv_ctx *c, const gmmiv_gmm *g, const XView &xv, int dt, int64_t t0, int64_t n, const double *lse, bool sq, int NC,
                               double *S);
}
