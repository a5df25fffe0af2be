/* gmmiv_iv_trials.h -- C ABI: the i-vector scoring rules of gmmiv.h on a LIST of (model, segment) trials.
 *
 * IvTest / PldaTest are driven by an ndx ("segment model model ...", PldaTools.cpp:3437-3622): cosineDistance and mahalanobisDistance
 * score only where _trials(m, s) holds (:3871, :3889) and IvTest.cpp:415-439 writes only those lines.  The dense rules of gmmiv.h
 * (gmmiv_score_cosine / _mahalanobis / _twocov / _plda) fill the whole M x S matrix: 2 dim flop per cell on all M S cells, and a matrix
 * that cannot be formed at 10^5 models x 10^6 segments.  The calls below read two rows of dim doubles per trial instead.
 *
 * Arguments.  models [dim x M] and segs [dim x S] hold one vector per column, host or device, exactly as the dense rules take them; the
 * rule matrices (Mah, G, H, FTJF, nsess) are those of the dense rules.  trial_model / trial_seg are HOST arrays of length ntrial: trial i
 * is (trial_model[i], trial_seg[i]).  They may come in any order, a pair may repeat, a vector may have no trial; they are copied before
 * return.  scores [ntrial] is a host or device array in LIST ORDER.  ntrial == 0 is valid, and so is M == 0 or S == 0 with ntrial == 0.
 *
 * Errors.  GMMIV_ERR_ARG, before anything is enqueued and with a message that names the FIRST offending trial, for an index outside
 * [0, M) / [0, S); also for a trial table on the device, for nsess on the device and for nsess[m] < 1 on a model that occurs in a trial
 * (a model without a trial is not looked at).  These checks come before the context is looked at (a NULL context is the last of them).
 *
 * Formulation: the expansion of the dense rules, cut differently.
 *   A [M x ldr]   the models as ROWS, ldr = dim rounded up to even, the pad 0
 *   B [S x ldr]   the rows ((Q + Q^T) s)^T, written in row form by the fp64 GEMM (segs^T (Q + Q^T)); for cosine the segments as rows.
 *                 It is always the SEGMENT side that is projected, for all S columns: what is projected never depends on the list.
 *   qm [M], qs [S]  m^T Qm m and s^T Qs s as the dense rules compute them (a GEMM and a column dot); for cosine 1 / |m| and 1 / |s|
 *   score_i = fma(ccross, dot(A[m_i], B[s_i]), fma(bm, qm[m_i], fma(bs, qs[s_i], cst)));   cosine: (dot * qm[m_i]) * qs[s_i]
 *   Mahalanobis: Q = Qm = Qs = Mah, ccross 1/2, bm = bs = -1/2.   Two-covariance: Q = G, Qm = Qs = G - H, all factors 1.
 *   PLDA: the trials are grouped by the DISTINCT value L of nsess[m] (not by runs), classes in increasing L.  A class has
 *   Q = K_{L+1}, Qm = K_{L+1} - K_L, Qs = K_{L+1} - K_1, factors 1/2, cst = (a_{L+1} - a_L - a_1) / 2 with K_n = (n FTJF + I)^-1 and
 *   a_n = log det K_n from the context's cache (the one gmmiv_score_plda fills): one B table, one qs and one constant per class.
 *
 * Summation order of dot(): a function of dim alone.  The row is ldr / 2 pairs of elements (2p, 2p + 1).  Lane j of 64 owns the pairs
 * p = j, j + 64, j + 128, ... and adds them in increasing p, one fused multiply-add per element, element 2p before 2p + 1, starting
 * from +0; the 64 partials are combined by the xor butterfly v_j <- v_j + v_(j xor d), d = 32, 16, 8, 4, 2, 1.  A product does not care
 * which factor was the anchor.  A trial's score therefore depends on its two vectors, the rule's matrices (and nsess of its model), M
 * and S (the shapes of the GEMMs behind B, qm and qs) -- NOT on the rest of the list, its order, repeated pairs, the anchor side or the
 * piece.
 *
 * Work items (k_score_trials, iv_trials.hip).  One wave takes an ANCHOR vector and a piece of at most P of its trials: the anchor row is
 * loaded once into registers (16-byte pairs over the 64 lanes; beyond dim 1024 it is re-read, from L2), the partner rows are gathered
 * with 16-byte loads, four rows in flight.  No LDS, no atomics, one 8-byte store per trial.  No dim is refused.  The anchor side is the
 * side with FEWER distinct vectors in the list (gmmiv_iv_trial_anchor; a tie goes to the model; PLDA decides per class); the option
 * "iv_trials_anchor" (0 auto, 1 model, 2 segment) forces it.  P = GMMIV_IV_TRIAL_PIECE unless the option "iv_trials_piece" names another
 * positive value (gmmiv_iv_trial_piece(ctx) returns the P in effect).  Neither option changes a bit of any score.
 *
 * Workspace (grow-only slots of their own, so no other call's scratch is touched and a repeated call allocates nothing):
 *   A  8 M ldr      B  8 S ldr      Y (the GEMM behind qm / qs)  8 dim max(M, S)      qm, qs  8 (M + S)
 *   rule matrices  32 dim^2      tables  GMMIV_IV_TRIAL_TABLE_BYTES(ntrial, ntiles)
 *   staging of HOST arguments only:  8 dim M,  8 dim S,  8 ntrial
 * each rounded up by an eighth as every workspace slot is.
 *
 * Synchronisation.  Like gmmiv_llr_trials the call is NOT enqueue-only: it waits for the context's stream once after uploading its
 * tables (they live in host memory of the call), and PLDA waits once more per class for its K_n; a rule matrix (Mah, G, H) given in
 * HOST memory adds one wait for its copy.  With device vectors and device `scores` everything after that is only enqueued: the scores
 * are valid in stream order.  Host `scores` are complete on return.
 * Host work.  The work list is built on the host for every call: two counting passes over the list, on up to 16 host threads from 2^18
 * trials on.  At 10^7 trials that is an order of magnitude more time than the kernel takes (DESIGN.md section 3.21 has the figures).
 * Kernel timers: "k_score_trials" (summed over the classes of a PLDA call), "k_dgemm(score)" (the projection behind B). */
#ifndef GMMIV_IV_TRIALS_H
#define GMMIV_IV_TRIALS_H

#include "gmmiv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GMMIV_IV_TRIAL_PIECE 512 /* default trials per work item */
#define GMMIV_IV_ANCHOR_AUTO 0
#define GMMIV_IV_ANCHOR_MODEL 1
#define GMMIV_IV_ANCHOR_SEG 2

typedef struct gmmiv_iv_trial_tile {
    int32_t anchor, reserved; /* index of the anchor vector (a model or a segment) */
    int64_t lo, hi;           /* entries [lo, hi) of the order array: trials of this anchor, hi - lo <= piece */
} gmmiv_iv_trial_tile;
#define GMMIV_IV_TRIAL_TABLE_BYTES(ntrial, ntiles) ((size_t)(ntiles) * sizeof(gmmiv_iv_trial_tile) + (size_t)(ntrial) * 8)

int gmmiv_iv_trial_piece(const gmmiv_ctx *ctx); /* "iv_trials_piece" if positive, else (and for NULL) GMMIV_IV_TRIAL_PIECE */
/* The auto rule (pure host): GMMIV_IV_ANCHOR_SEG when the list names fewer distinct segments than distinct models, else
 * GMMIV_IV_ANCHOR_MODEL (a tie and the empty list included); -1 for a bad argument (an index out of range, a negative count). */
int gmmiv_iv_trial_anchor(int64_t M, int64_t S, const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial);
/* The work list (pure host): the trials sorted by (anchor, partner, position in the list) and cut into pieces of at most `piece`
 * trials of ONE anchor, so the tiles of one anchor are adjacent and neighbouring waves share rows in cache.  anchor: GMMIV_IV_ANCHOR_MODEL,
 * _SEG or _AUTO (the rule above).  order [ntrial] (nullable) receives the list positions in sorted order, tiles (nullable) the table.
 * Returns the number of tiles (entries beyond `cap` are counted, not written), or -1 for a bad argument (a negative count, piece < 1,
 * an unknown anchor, a missing table with ntrial > 0, an index outside [0, M) / [0, S)). */
int64_t gmmiv_plan_iv_trial_tiles(int64_t M, int64_t S, const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial, int anchor,
                                  int piece, int64_t *order, gmmiv_iv_trial_tile *tiles, int64_t cap);

int gmmiv_score_cosine_trials(gmmiv_ctx *ctx, int dim, int64_t M, int64_t S, const double *models, const double *segs,
                              const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial, double *scores);
int gmmiv_score_mahalanobis_trials(gmmiv_ctx *ctx, int dim, int64_t M, int64_t S, const double *models, const double *segs,
                                   const double *Mah, const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial, double *scores);
int gmmiv_score_twocov_trials(gmmiv_ctx *ctx, int dim, int64_t M, int64_t S, const double *models, const double *segs, const double *G,
                              const double *H, const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial, double *scores);
int gmmiv_score_plda_trials(gmmiv_ctx *ctx, int rf, int64_t M, int64_t S, const double *models_sum, const int64_t *nsess,
                            const double *segs, const double *FTJF, const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial,
                            double *scores);

#ifdef __cplusplus
}
#endif
#endif
