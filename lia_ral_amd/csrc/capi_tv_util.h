// capi_tv_util.h -- helpers shared by the i-vector units of the C API: capi_tv.hip, capi_iv_score.hip, capi_backend.hip (internal).
#pragma once
#include "ctx.h"
#include "tv_kernels.h"

// host copy of a host-or-device array / store of a host vector into a host-or-device array (defined in capi_tv.hip)
#pragma GCC visibility push(hidden)
int fetch_host(gmmiv_ctx *c, const double *p, size_t n, std::vector<double> &out);
int store_out(gmmiv_ctx *c, double *p, const std::vector<double> &v);
#pragma GCC visibility pop

// Utterances (rows) per batch of a call over n of them: the "tv_batch" option (unset: 256), at most n.  floor = 1 where the caller
// sizes scratch from the result and n may be 0; tv_estep (n >= 1) passes 0.
static inline int tv_batch_size(const gmmiv_ctx *c, int64_t n, int floor = 1)
{
    const int tvb = c->tv_batch > 0 ? (int)c->tv_batch : 256;
    return n < tvb ? (int)(n > floor ? n : floor) : tvb;
}

// C[M x N] = alpha op(A) op(B) + beta C for few output tiles and a long K: K split over nz workgroup layers whose partial products
// go to WS_SLAB and are summed in a fixed order.  nz -- and with it the summation order -- comes from Mz x N x K: a caller that
// runs batches of up to Mz rows passes the batch size there, so that a short last batch sums like the full ones.
static inline int splitk_gemm(gmmiv_ctx *c, int Mz, bool ta, bool tb, int M, int N, int K, double alpha, const double *A, long lda,
                              const double *B, long ldb, double beta, double *C, long ldc)
{
    const int nz = tvk_splitk_count(Mz, N, K, c->n_cu);
    void *slabs;
    int rc;
    if ((rc = c->scratch(WS_SLAB, (size_t)nz * Mz * N * 8, &slabs))) return rc;
    GCHK(tvk_dgemm_splitk(c->stream, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, nz, (double *)slabs));
    return GMMIV_OK;
}

namespace {

// The scratch slot of each buffer of an SpdBatch; -1: the caller never runs the operation that needs it
struct SpdSlots { int full = WS_T4, inv = WS_T5, X = WS_T6, invd = WS_T7, panel = WS_T8, status = WS_SMALL; };

// A batch of nb SPD matrices of one order on the device: the ONLY place that knows how such a batch is factored, solved and
// inverted.  Orders the left-looking kernels of chol_fused.hip serve (even, option "chol_gemm" off: left()) are factored by one
// workgroup per matrix, straight from packed lower rows when that is how the matrices arrive; every other order goes through a
// full copy and the GEMM-built factorisation of tv_kernels.hip.  Use: reserve once; per batch begin, then -- where the matrices are
// packed -- from_packed, then ONE of factor (+ solve / solve_multi), inverse, inverse_e, then check (inverse_e checks itself).
struct SpdBatch {
    gmmiv_ctx *c = nullptr;
    double *full = nullptr, *inv = nullptr, *X = nullptr, *invd = nullptr, *panel = nullptr; // factor | inverse | scratch | 32 x 32 diagonal-block inverses | scratch
    int *status = nullptr; // one word per matrix, non-zero: not positive definite
    int n = 0, nb = 0;
    const double *P = nullptr; // the batch as packed lower rows (stride sp) + diag I, when left() reads it directly
    long sp = 0;
    double diag = 0.0;

    int reserve(gmmiv_ctx *ctx, int order, int nbmax, const SpdSlots &s = SpdSlots())
    {
        c = ctx; n = order;
        const size_t nn = (size_t)n * n;
        const int nblk = (n + 31) / 32;
        void *p;
        int rc;
        if (s.full >= 0) { if ((rc = c->scratch(s.full, nbmax * nn * 8, &p))) return rc; full = (double *)p; }
        if (s.inv >= 0) { if ((rc = c->scratch(s.inv, nbmax * nn * 8, &p))) return rc; inv = (double *)p; }
        if (s.X >= 0) { if ((rc = c->scratch(s.X, nbmax * nn * 8, &p))) return rc; X = (double *)p; }
        if (s.invd >= 0) { if ((rc = c->scratch(s.invd, (size_t)nbmax * nblk * 1024 * 8, &p))) return rc; invd = (double *)p; }
        if (s.panel >= 0) { if ((rc = c->scratch(s.panel, (size_t)nbmax * n * 32 * 8, &p))) return rc; panel = (double *)p; }
        if (s.status >= 0) { if ((rc = c->scratch(s.status, (size_t)nbmax * sizeof(int) + 64, &p))) return rc; status = (int *)p; }
        return GMMIV_OK;
    }
    // whether orders like this one take the left-looking kernels (under the options bound to this thread)
    static bool left(int order) { return tvk_chol_accepts_packed(order) != 0; }
    bool left() const { return left(n); }

    // a new batch of count matrices (in `full` unless from_packed follows); order: a smaller one than reserved, in the same buffers
    int begin(int count, int order = 0)
    {
        nb = count; P = nullptr; sp = 0; diag = 0.0;
        if (order > 0) n = order;
        GCHK(hipMemsetAsync(status, 0, nb * sizeof(int), c->stream));
        return GMMIV_OK;
    }
    // the batch is packed + diag_add I (stride spk): read in place by the left-looking kernels, unpacked into `full` otherwise
    int from_packed(const double *packed, long spk, double diag_add)
    {
        if (left()) { P = packed; sp = spk; diag = diag_add; }
        else GCHK(tvk_unpack_sym(c->stream, n, nb, packed, spk, full, diag_add));
        return GMMIV_OK;
    }
    int factor() // full <- the lower Cholesky factor
    {
        GCHK(left() ? tvk_chol_left_batched(c->stream, n, nb, full, invd, status, P, sp, diag) : tvk_chol_batched(c->stream, n, nb, full, invd, panel, status));
        return GMMIV_OK;
    }
    // after factor: w[i] = A[i]^-1 b[i]; X[i] = A[i]^-1 B[i] for nrhs <= 64 right-hand sides (left() orders only)
    int solve(const double *b, double *w) { GCHK(tvk_chol_solve_batched(c->stream, n, nb, full, invd, b, w)); return GMMIV_OK; }
    int solve_multi(int nrhs, const double *B, long ldb, long sB, double *Xo, long ldx, long sX)
    {
        GCHK(tvk_chol_solve_multi_batched(c->stream, n, nb, nrhs, full, invd, B, ldb, sB, Xo, ldx, sX));
        return GMMIV_OK;
    }
    int inverse(double *dst) // dst[i] = A[i]^-1 (full); `full` ends up holding the factor
    {
        GCHK(left() ? tvk_spd_inverse_left_batched(c->stream, n, nb, full, dst, X, invd, status, P, sp, diag)
                    : tvk_spd_inverse_batched(c->stream, n, nb, full, dst, X, invd, panel, status));
        return GMMIV_OK;
    }
    // T-matrix E-step form, after from_packed(E, ..): W[i] = A[i]^-1 aux[i] and E[i] <- A[i]^-1 + w w^T, packed, over the input
    int inverse_e(const double *aux, double *W, double *E, long spk, const char *what)
    {
        if (left()) {
            GCHK(tvk_inverse_e_packed_batched(c->stream, n, nb, full, X, invd, status, E, spk, diag, aux, W));
            return check(what);
        }
        int rc = inverse(inv); // explicit inverse like the reference
        if (rc) return rc;
        GCHK(tvk_batched_matvec(c->stream, n, nb, inv, aux, W));
        if ((rc = check(what))) return rc;
        GCHK(tvk_pack_sym(c->stream, n, nb, inv, (long)n * n, W, E, spk));
        return GMMIV_OK;
    }
    // one matrix given in full at src: copy, begin, inverse, check
    int inverse_of(int order, const double *src, double *dst, const char *what)
    {
        GCHK(hipMemcpyAsync(full, src, (size_t)order * order * 8, hipMemcpyDeviceToDevice, c->stream));
        int rc;
        return (rc = begin(1, order)) || (rc = inverse(dst)) ? rc : check(what);
    }
    // reads the status words back (synchronises the stream)
    int check(const char *what)
    {
        std::vector<int> h(nb);
        GCHK(hipMemcpyAsync(h.data(), status, nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < nb; ++i)
            if (h[i]) { gmmiv_set_error("%s: matrix %d of the batch is not positive definite", what, i); return GMMIV_ERR_NUMERIC; }
        return GMMIV_OK;
    }
};

} // namespace
