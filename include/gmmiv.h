/*
 * gmmiv.h -- C ABI of libgmmiv, the MI355X (gfx950) GMM / i-vector compute engine.
 *
 * Drop-in boundary for ONE hot path of LIA_RAL: per-frame diagonal-GMM log-likelihood, top-C
 * selection, full-posterior (Baum-Welch / EM) sufficient statistics, the i-vector solve and the
 * i-vector scoring rules.  The reference has no FFI layer: these loops call C++ objects of the
 * external alize-core library once per frame.  Each entry point below therefore
 * replaces one *batched* reference loop; the comment on it cites the loop (paths relative to the
 * LIA_RAL tree).  INTEGRATION.md shows the branch a maintainer adds at each of those call sites.
 *
 * Conventions
 *  - plain C, opaque handles, int status (0 = ok, <0 = error; gmmiv_last_error() has the text);
 *  - every array argument may be a HOST pointer or a DEVICE (HIP) pointer -- detected with
 *    hipPointerGetAttributes.  Host arrays are staged through the context's device workspace;
 *    device arrays are used in place (no copy), which is what bench.py times;
 *  - matrices are row-major, arithmetic is fp64 like the reference (features may be given as
 *    float32, the on-disk SPro type, or as double, the type Feature::getDataVector() returns);
 *  - one context per GPU / per host thread; a context is not thread-safe, different contexts are;
 *  - no hidden state: the per-frame top-C vector that ALIZE keeps inside StatServer is an
 *    explicit output / input here.
 */
#ifndef GMMIV_H
#define GMMIV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gmmiv_ctx gmmiv_ctx; /* device + stream + workspace                       */
typedef struct gmmiv_gmm gmmiv_gmm; /* device-resident diagonal GMM in kernel-ready layout */

enum { GMMIV_F32 = 0, GMMIV_F64 = 1 };           /* feature element type               */
enum { GMMIV_TOP_PARTIAL = 0, GMMIV_TOP_COMPLETE = 1 }; /* computeLLKWithTopDistribs */

#define GMMIV_OK 0
#define GMMIV_ERR_ARG (-1)
#define GMMIV_ERR_HIP (-2)
#define GMMIV_ERR_UNSUPPORTED (-3)
#define GMMIV_ERR_NUMERIC (-4)

/* ---- context --------------------------------------------------------------------------- */
/* stream: a hipStream_t to launch on (e.g. torch's current stream), or NULL for a private non-blocking one.  A caller whose
 * other work runs on the NULL (legacy default) stream -- torch's default stream is that one -- passes GMMIV_STREAM_DEFAULT to
 * have the context launch there too (hipStreamLegacy, (hipStream_t)1, is taken to mean the same): a private stream is NOT
 * ordered with the NULL stream, so buffers written by NULL-stream work would have to be complete before each call. */
#define GMMIV_STREAM_DEFAULT ((void *)(intptr_t)-1)
int gmmiv_ctx_create(int device, void *stream, gmmiv_ctx **out);
void gmmiv_ctx_destroy(gmmiv_ctx *ctx);
int gmmiv_ctx_sync(gmmiv_ctx *ctx);
/* The hipStream_t every call of this context is enqueued on (the one given to gmmiv_ctx_create, or the private one): a host
 * layer that keeps its own device buffers orders its copies / memsets on it instead of synchronising around every call. */
void *gmmiv_ctx_stream(gmmiv_ctx *ctx);
/* STREAM ORDER.  A device array handed to a call is read and written in the order of the context's stream: the call behaves like a
 * kernel launched on that stream.  The library never reads such an array from another stream, and never on the host before the
 * stream has reached the call -- so an input need not be complete when the call is MADE, only when the stream gets to it: the
 * output of gmmiv_plda_precompute, of gmmiv_dgemm or of the caller's own kernel on this stream can go straight into the next call,
 * with no synchronisation in between.  Conversely it is NOT enough for an array written on ANOTHER stream to be complete at the time
 * of the call unless that stream has been joined with the context's (an event, or gmmiv_ctx_sync after a host wait).  A call that has
 * to look at device data on the host (the PLDA rules read FTJF for their K_n cache, the host factorisations of the T-matrix M-step
 * their small matrices) copies it on the context's stream and waits for that stream.  Outputs in device memory are valid in stream order; which calls return with the
 * stream still busy ("only enqueue") is said per entry point, and DESIGN.md section 4 has the observed table. */
/* ADDRESSING.  Every offset from a pointer handed to a call is computed in 64 bits: a frame t of (x, T, ldx) is read at x + t * ldx, a
 * row of (out, ldo), of a matrix with ld / lda / ldb / ldc, a matrix of a batch with sA / sB / sC and a model of a table with *_stride
 * likewise, wherever the product lies -- beyond 2^32 bytes, 2^31 elements or 2^32 elements from the pointer.  Frame numbers and row
 * numbers in tables (runs, frame_idx, file_begin, utt_begin, seg_begin and the segment / trial tables) are int64_t and are used as such:
 * a resident corpus of 60 float32 per frame passes 2^32 bytes at 18 M frames and 2^31 elements at 36 M frames, and nothing changes
 * there.  Results depend on the frames addressed, not on how far from the pointer they lie.
 * COUNTS are narrower than offsets.  Model and matrix dimensions (C, D, M, N, K, batch, nrows, G, ctop) are int.  The int64_t counts --
 * frames per call (T), entries per table (n, nrun, nseg, nfiles, ntrial, U, nlines, npos, ngroups) -- go up to 2^31 - 1 at the most, and
 * some stop earlier.  The limits that are CHECKED and refused with a message:
 *   nseg of gmmiv_llk_models, gmmiv_tv_stats_models, gmmiv_em_stats_models, gmmiv_feat_compensate_models; nseg and ntrial of
 *   gmmiv_llr_trials; U of gmmiv_tv_stats          more than (2^31 - 1) / 64 = 33 554 431: GMMIV_ERR_UNSUPPORTED ("too many ..")
 *   T of gmmiv_occ; the distributions (rows for axis 0, columns for axis 1) of gmmiv_score_cohort_stats and of gmmiv_score_list_stats;
 *   M of gmmiv_score_normalize; n of gmmiv_iv_normalize; M and S of the scoring rules, M, S and ntrial of the *_trials scoring rules
 *                                                  more than 2^31 - 1: GMMIV_ERR_UNSUPPORTED
 *   n of gmmiv_score_normalize_list                more than 256 (2^31 - 1): GMMIV_ERR_UNSUPPORTED
 *   gmmiv_turn_curve                               npos / gmmiv_turn_tile_positions + min(nrun, npos) tiles beyond 2^31 - 1: GMMIV_ERR_ARG
 * Every other count (T of the other frame-consuming calls, n, nrun, nfiles, nlines, ngroups) is NOT checked against 2^31 - 1: several
 * launch grids and work lists are sized by them in 32 bits, and beyond it the behaviour is undefined.  A caller with more frames or
 * table entries than that cuts the call -- the frames stay where they are: the pointer or the frame numbers move, which is what the
 * paragraph above is for. */
const char *gmmiv_last_error(void);
const char *gmmiv_version(void);
/* Runtime knobs; returns the previous value (-1: unknown key).  EVERY option is state of the context it is set on -- two
 * contexts driven from one host thread keep their own settings, a context keeps its settings whichever thread drives it.
 *   "stats_z" 1        EM / Baum-Welch statistics from stored scaled likelihoods (k_llk_mfma<WZ> + k_stats_z);
 *                      0: the recomputing k_stats_mfma (also used for D > 60 or when the scratch does not fit)
 *   "z_scratch_mb"     likelihood scratch budget in MiB (default 16384, at most a quarter of the device's TOTAL memory):
 *                      frames are processed in chunks that fit.  The chunk length -- and with it the fp64 summation
 *                      order -- depends only on this option, the model shape and the device model, not on the memory
 *                      free at call time: results are bitwise reproducible across runs and ranks.  (The order differs
 *                      from the reference's frame-by-frame accumulation: parity is to a tolerance, see DESIGN.md.)
 *   "trials_scratch_mb" 2048  gmmiv_llr_trials: MiB of per-frame world results (4 ctop + 16 bytes per frame) kept per chunk of whole segments
 *   "trials_piece" 0   A/B knob of gmmiv_llr_trials: frames per work item, a multiple of 4 that is >= 4; 0 (default) or any other value =
 *                      GMMIV_TRIAL_PIECE.  It moves the boundaries of the summation pieces and with them the LAST BITS of every result
 *                      (the definition and the independence properties hold for any value); not meant for production use
 *   "models_scratch_mb" 2048  gmmiv_*_models: MiB of packed models (nct (2 KS + 2) 512 bytes each, 2 MiB at 2048 x 60) built per chunk
 *                      of segments; a chunk holds at least one model whatever the value
 *   "z_waves" 8        workgroup shape of k_stats_z (8, 16 or 4 waves)
 *   "z_depth_tv" 4     register sets of k_stats_z's likelihood stream (prefetch distance + 1; 2 or 4) in the N / F mode,
 *   "z_depth_em" 2     and in the EM mode; bit-identical results
 *   "prune_log2" 0     n > 0: skip groups of posteriors that are all below 2^-n (NOT the reference's arithmetic
 *                      for dead Gaussians; off by default)
 *   "tv_stats_split" 1 gmmiv_tv_stats on at most 16 utterances: every utterance in pieces of whole 64-frame tiles (more workgroups for the
 *                      N / F kernel), summed back in piece order; 0 = one segment per utterance.  The fp64 summation ORDER of an
 *                      utterance's row therefore depends on how many utterances share the call (pieces for <= 16, one segment above):
 *                      the same utterance extracted alone and inside a large batch gives N / F -- and i-vectors -- that agree to about
 *                      1e-13 relative, not bitwise (both within the 1e-9 of the parity tests); set the option to 0 when a row must not
 *                      depend on its neighbours
 *   "assume_finite" 0  1: skip the pass that COUNTS the frames with unusable feature values ("DEGENERATE INPUTS" below; results never depend on it)
 *   "screened_frames", "zero_llk_frames"   counters of the frames of kind (1) / kind (2) of "DEGENERATE INPUTS" (read: returns the
 *                      count so far and stores `value`)
 *   "tv_tett_direct" 1 estimateTETt as one kernel that computes the lower triangles only and writes them packed (D <= 64); 0 = batched
 *                      GEMM into full matrices + pack
 *   "tv_batch" 1024    utterances per batch of the i-vector solve / T-matrix E-step (one workgroup factors one
 *                      system L_u; workspace 4 x tv_batch x R^2 doubles)
 *   "tv_acc_mb" 8192   T-matrix E-step: MiB of packed E_u = L_u^-1 + w_u w_u^T kept in HBM before A += N^T E and Cmx += W^T F run
 *                      (one GEMM per super-batch, K = its utterances, instead of one per tv_batch)
 *   "chol_gemm" 0      1: the GEMM-built right-looking batched Cholesky / inverse instead of chol_fused.hip (always
 *                      used for odd orders); A/B switch (like "gemm_remap", "gemm_clamp", "gemm_narrow", "z_tv4")
 *   "gemm_nt80" 1      split-K NT products whose N is a multiple of 80 but not of 128 (aux = F (T Sigma^-1)^T at rank 400) on 128 x 80
 *                      tiles instead of 128 x 128 tiles + a 16-column strip; 0: the latter (A/B switch)
 *   "chol_lds" 1       chol_fused.hip stages the panel rows once per workgroup in LDS; 0: every wave fetches them itself (A/B switch)
 *   "chol_flow" 1      batched Cholesky k_chol_left2 (panel staged first, diagonal update from LDS on all waves); 0: round 2's k_chol_left
 *   "kopts_bound"      read-only: 1 when this context's kernel-launcher options are the set bound to the calling thread (they are
 *                      bound by each call of the context on entry)
 *   "tv_mstep_solve" 1 updateTestimate by blocked substitution through the Cholesky factor of A_c (k_chol_solve_multi);
 *                      0: explicit inverse + GEMM like the reference
 *   "tv_md_device" 1   minDivergence: R normalised and factored on the device (even R); 0: on the host
 *   "topc_fused" 1     DETERMINE_TOP_DISTRIBS with the candidates collected in the epilogue of the MFMA log-likelihood kernel
 *                      (k_llk_mfma<TC> + k_topc_rank; C' <= 16, C <= 2048, D <= 64); 0 or not applicable: "topc_z".
 *                      "topc_fallbacks" counts the calls the fused path handed on (candidate list overflow / margin check)
 *   "short_calls" 1    log-likelihood kernels: a call of at most 32 768 frames runs 4-wave workgroups (one round, one wave per SIMD: 0.3 ms
 *                      instead of 0.55 for the walk through a 2048-Gaussian model); 0 = the 8-wave workgroups of long calls.  Per-frame
 *                      results are the same either way.
 *   "topc_rank2" 1     fused path: the ranking kernel handles two frames per wave (k_topc_rank2; frames with more than 128 candidate
 *                      records or more than 32 survivors go through the one-frame kernel right behind it); 0 = one frame per wave
 *   "topc_use_lanes" 4  USE_TOP_DISTRIBS with at most 16 candidates: four lanes per candidate read 64 contiguous bytes of its model row per
 *                      instruction (k_topc_use4, one frame per wave); 1 = one lane per candidate (k_topc_use16, four frames per wave)
 *   "topc_rank_direct" 0  fused path: k_topc_rank ranks the survivors of the final threshold on their MFMA logits and re-evaluates them in
 *                      the reference's direct form only when another survivor lies within 1e-6 of a selected one (same selection and
 *                      order; selected likelihoods differ by < 1e-11 relative); 1 = direct form for every frame (the round-2 behaviour)
 *   "topc_z" 1         DETERMINE_TOP_DISTRIBS from the stored MFMA likelihoods (k_llk_mfma<WZ> + k_topc_from_z, direct form only
 *                      for the candidates); 0: the direct-form VALU kernel for every Gaussian
 *   "timing" 0         1: record HIP events around the kernels (gmmiv_ctx_kernel_ms)
 *   "glds", "wg_waves", "em_chunks", "dbg": A/B switches of the measurement tools */
long gmmiv_ctx_set_option(gmmiv_ctx *ctx, const char *key, long value);
/* Host callbacks at the two points of a TotalVariability iteration where an exchange can start before the call that produces its
 * payload has returned (the reference's threaded estimateAandC merges A, Cmx, R, r under one mutex AFTER all workers are done,
 * AccumulateTVStat.cpp:1920-1937; with one rank per GPU the 1.31 GB reduce-scatter of A can run under the Cmx GEMM instead):
 *   "tv_a_ready"    inside gmmiv_tv_estimate_a_and_c, right after the LAST `A += N^T E` GEMM has been enqueued on the context's
 *                   stream and before `Cmx += W^T F` is (device accumulators only) -- the callback typically calls
 *                   gmmiv_reduce_scatter_f64_begin on A;
 *   "md_factored"   inside gmmiv_tv_min_divergence, after R has been normalised and factored and before T is read -- the
 *                   callback joins an all-gather of T that was begun before the call (gmmiv_comm_join) and may finish T's layout.
 * The callback runs on the calling host thread; anything it enqueues on the context's stream is ordered like the library's own
 * work.  fn == NULL removes the hook.  Returns 0, or -1 for an unknown point. */
typedef void (*gmmiv_hook_fn)(void *user);
int gmmiv_ctx_set_hook(gmmiv_ctx *ctx, const char *point, gmmiv_hook_fn fn, void *user);
/* Duration (ms, HIP events on the context's stream) of the last call's dominant kernel. */
double gmmiv_ctx_last_kernel_ms(gmmiv_ctx *ctx, const char **kernel_name);
/* Same for a named kernel ("k_llk_mfma", "k_stats_z", "k_stats_mfma", ...): TOTAL over its launches
 * inside the most recent call that used it (a call may process its frames in several chunks);
 * -1 if none.  gmmiv_ctx_kernel_launches gives that number of launches. */
double gmmiv_ctx_kernel_ms(gmmiv_ctx *ctx, const char *kernel_name);
long gmmiv_ctx_kernel_launches(gmmiv_ctx *ctx, const char *kernel_name);

/* ---- model: MixtureGD / DistribGD ----------------------------------------------------------
 * w[C], mean[C*D], covinv[C*D] (DistribGD::getMeanVect / getCovInvVect, MixtureGD::weight(c);
 * LIA_SpkTools/src/AccumulateTVStat.cpp:154-162).  cst/det are derived like computeAll().
 * SHAPES.  mixtureDistribCount, vectSize and topDistribsCount are free configuration keys of the reference
 * (LIA_SpkDet/TrainWorld/cfg/TrainWorld.cfg, ComputeTest.cpp:129-215) and none of them is refused here: vectSize <= 80 runs the fp64
 * MFMA kernels (compiled for D <= 16 / 32 / 60 / 80; the stored-likelihood statistics path for D <= 60); a larger vectSize (<= 4096)
 * runs generic paths with the same results -- logits in the reference's direct form on the vector ALUs, statistics as
 * gamma^T [x | 1 | x^2] on the fp64 GEMM -- at about a tenth of the rate; gmmiv_tv_stats walks the UTTERANCES one by one there (per
 * utterance: posteriors, one C x (vectSize + 2) x length GEMM, a scatter -- five launches), so a call of many short utterances is
 * launch-bound on that path, not merely slower (vectSize 1 .. 80 never takes it).  The fused / stored-likelihood top-C selection serves
 * topDistribsCount <= 16 / <= 60, the LDS selection kernel <= 64 with up to ~4 700 Gaussians; anything beyond (8192 Gaussians,
 * topDistribsCount 100, ...) goes through an any-shape selection kernel whose logit rows live in device scratch. */
int gmmiv_gmm_create(gmmiv_ctx *ctx, int C, int D, const double *w, const double *mean,
                     const double *covinv, gmmiv_gmm **out);
int gmmiv_gmm_set(gmmiv_gmm *g, const double *w, const double *mean, const double *covinv);
/* Same from covariances (DistribGD::setCov + computeAll, TrainTools.cpp:577-582): covInv = 1/cov. */
int gmmiv_gmm_set_cov(gmmiv_gmm *g, const double *w, const double *mean, const double *cov);
void gmmiv_gmm_destroy(gmmiv_gmm *g);

/* ---- DEGENERATE INPUTS: what every frame-consuming entry point does with them ------------------------------------------
 * The reference has no defined behaviour here (a NaN feature poisons every accumulator it touches; ALIZE's handling of a frame of
 * likelihood 0 is not visible from LIA_RAL -- SURVEY.md U1; the one in-tree guard, TopGauss.cpp:247, maps a NaN likelihood to
 * exp(minLLK)).  This library defines it, and tests/test_gpu_degenerate.py holds every path to it -- tests/test_gpu_gmm_dead_frames.py
 * per frame, per posterior and per accumulator element, counters included, on every shape and option path of the core entry points:
 *
 * A frame is a ZERO-LIKELIHOOD FRAME when (1) one of its feature values is NaN, infinite or larger than 1e18 in magnitude, or
 * (2) its likelihood is 0 in fp64: the LARGEST term w_c lk_c(x_t) lies below 2^-1075 = exp(-745.13) (so every term of the
 * reference's linear-domain sum rounds to 0 and log of it is -inf), or the log-sum is not finite.  The decision is made on the
 * largest logit, threshold log 2^-1075 = -745.1332 (GMMIV_ZERO_LLK in csrc/devutil.h), on every path; a frame whose best Gaussian
 * is at -744 is an ordinary frame, one at -746 is a zero-likelihood frame (tests/test_gpu_degenerate.py pins both sides).  Then
 *   gmmiv_llk                     llk_t = min_llk (the clamp of log 0); counted in sums like any frame
 *   gmmiv_llk_determine_top       idx = 0 .. ctop-1 (the tie rule -- lowest index first -- on equal, zero, likelihoods), lk = 0,
 *                                 nontop_lk = 0, nontop_llk = -inf, nontop_w = 1 - sum of those weights, llk = min_llk
 *   gmmiv_topgauss_compute        as determine_top; count = cap for a mass threshold (the reference's loop runs to the end), idx as above
 *   gmmiv_llk_use_top(_multi)     llk_t = min_llk on a kind-(1) frame; a kind-(2) frame is seen through the client's logits of the selected
 *                                 Gaussians (0 .. ctop-1) and the world's remainder (-inf) only: llk_t = the clamp of their log-sum, which
 *                                 is min_llk wherever the client's own value lies below min_llk
 *   gmmiv_occ                     a row of zeros
 *   gmmiv_em_accumulate           the frame adds NOTHING: no occupancy, no first / second order statistics, nothing to the sum of
 *                                 log-likelihoods and nothing to the frame count (the M-step weights still sum to 1)
 *   gmmiv_tv_stats(_lines), gmmiv_jfa statistics    nothing added to N / F
 *   gmmiv_frame_moments           NOT screened: sums of the raw values, a NaN goes into the sums like in the reference
 *   gmmiv_feat_compensate         the frame is COPIED THROUGH unchanged (converted to out_dtype), either kind, and counted in
 *                                 "zero_llk_frames" (the reference divides 0 by 0 there); kind (1) also in "screened_frames"
 *   gmmiv_feat_compensate_models  as gmmiv_feat_compensate, under the segment's model; each frame counted once
 *   gmmiv_feat_map                NOT screened: best = 0 on a frame whose every term is 0 (the reference's loop leaves idx = 0), the
 *                                 raw values go through the map of that Gaussian -- a NaN stays a NaN
 *   gmmiv_frame_moments_groups    NOT screened: like gmmiv_frame_moments, a NaN goes into the sums of its group
 *   gmmiv_feat_norm_apply         NOT screened: (x - mean) / std of the raw value; std = 0 gives Inf / NaN like computeZeroOne
 *   gmmiv_feat_norm_online        NOT screened: a NaN / Inf frame poisons the running mean and std of its file from there on, like
 *                                 the tool's (1 - B) * f[i]; a running std of 0 gives Inf / NaN
 *   gmmiv_energy_train            globalCov NOT screened (FrameAccGD: a NaN / Inf energy makes it NaN, and a comparison with NaN is false: no
 *                                 floor, no ceiling); the EM statistics read the column through feat_sane: a frame of either kind adds nothing
 *                                 and is not counted; when EVERY frame is one, count = 0: weights 0 / 0 = NaN, means and covariances kept,
 *                                 status GMMIV_ENERGY_NONFINITE.  Neither counter ("screened_frames", "zero_llk_frames") is bumped.
 *   gmmiv_energy_select           NOT screened: a frame is in when x > threshold (strict): NaN is out, +Inf and 1e30 are in; a NaN threshold
 *                                 (an empty file) selects nothing
 * Frames of kind (1) are handled ON THE DEVICE, inside the kernels: every kernel that reads features reads an unusable value as 1e10
 * (csrc/devutil.h, feat_sane: one compare + select where the value is loaded -- in the MFMA log-likelihood kernel once per frame and
 * workgroup, outside its loop).  The value is finite, so no 0 x NaN reaches a statistic, and it puts every logit of the frame near
 * -0.5e20 / variance: the frame then IS a frame of kind (2) for every kernel (holds for variances in 1e-17 .. 1e17) and follows the
 * table above with no host decision -- no flags read back, no compaction, NO SYNCHRONISATION: a call whose arrays are all device
 * pointers only enqueues on the context's stream (rounds 1-5 screened on the host and waited for the stream once per call).
 * That holds for gmmiv_llk, gmmiv_occ, gmmiv_em_accumulate, gmmiv_llk_use_top(_multi) and gmmiv_frame_moments.  It does NOT hold for
 * gmmiv_llk_determine_top and gmmiv_topgauss_compute (the fallback flags are read back once per chunk), gmmiv_tv_stats(_lines) (the call
 * waits once for its utterance table), gmmiv_feat_map (its top-1 selection) and the *_models / gmmiv_llr_trials calls (their table
 * uploads): these wait for the stream for reasons of their own, whatever the screening does.
 * What remains of the screening is a COUNT: at the start of a frame-consuming call one pass over x (0.3 % of an EM pass) adds the number
 * of kind-(1) frames to a device counter, option "screened_frames" (read / reset like "zero_llk_frames" below).  The option
 * "assume_finite" 1 skips that pass; RESULTS do not depend on it (the C++ host layer checks a FeatureBuffer once, at upload, and
 * sets it per call from the buffer the call reads).  Kind (2) is decided per frame where the log-likelihood kernel finishes a
 * frame -- no per-element work in the hot loops -- and COUNTED on the device by the entry points that drop such a frame from a sum:
 * gmmiv_llk, gmmiv_em_accumulate, gmmiv_tv_stats(_lines) (and the JFA statistics built on it), gmmiv_occ; a kind-(1) frame is
 * evaluated as a kind-(2) frame and therefore counted here TOO.  gmmiv_ctx_set_option(ctx, "zero_llk_frames", v) returns the count so
 * far and stores v (0 to reset); the read waits for the context's stream, the counting never does.  Not counted: the top-C entry
 * points (a zero-likelihood frame is visible there as llk = min_llk with lk = 0).
 * Other edges: T = 0 is valid everywhere (outputs untouched, accumulators unchanged); a Gaussian of weight 0 has likelihood 0
 * (never selected before a Gaussian of positive likelihood, occupancy 0); gmmiv_em_get keeps the previous mean / covariance of a
 * Gaussian whose occupancy is 0 and gives it weight 0; identical Gaussians tie and the lower index wins.
 *
 * gmmiv_count_unusable_frames: the counting pass on its own, read back -- *count = frames of kind (1) (this call waits for the stream). */
int gmmiv_count_unusable_frames(gmmiv_ctx *ctx, const void *x, int x_dtype, int64_t T, int64_t ldx, int D,
                                int64_t *count);

/* ---- FrameAccGD::accumulate loop (LIA_SpkTools/src/AccumulateStat.cpp:387-396) ---------------
 * acc[0..D) += sum x, acc[D..2D) += sum x^2, acc[2D] += T.  mean/cov: sum/n, sumsq/n - mean^2. */
int gmmiv_frame_moments(gmmiv_ctx *ctx, const void *x, int x_dtype, int64_t T, int64_t ldx, int D,
                        double *acc);

/* ---- frame selection on the device: out[i][0..D) = x[frame_idx[i]][0..D) ----------------------
 * Replaces the seekFeature/readFeature walk over a SegCluster (label selection, bagging:
 * LIA_SpkTools/src/AccumulateStat.cpp:121-128, GeneralTools.cpp:455-510) for features that stay
 * resident in HBM.  x, out: DEVICE arrays (out has ld = D); frame_idx: host or device. */
int gmmiv_gather_frames(gmmiv_ctx *ctx, const void *x, int x_dtype, int64_t ldx, int D,
                        const int64_t *frame_idx, int64_t n, void *out);
/* The same selection given as RUNS of adjacent frames -- what a SegCluster is (a bagged chunk of
 * baggedSegments is 3..7 frames, GeneralTools.cpp:455-510; a label segment thousands):
 * runs[3 r + 0 .. 2] = (first source frame, first output row, length); run r copies frames
 * [src, src + len) to rows [dst, dst + len) of out.  24 bytes per run cross PCIe instead of 8 per
 * frame.  Runs must not overlap in `out`; long runs should be cut into pieces of <= 64 frames by
 * the caller (one wavefront moves one run).  x, out: DEVICE arrays; runs: host or device -- with a
 * device table the call only enqueues on the context's stream (no synchronisation). */
int gmmiv_gather_runs(gmmiv_ctx *ctx, const void *x, int x_dtype, int64_t ldx, int D,
                      const int64_t *runs, int64_t nrun, void *out);

/* The inverse of gmmiv_gather_runs: rows [dst, dst + len) of `in` (ld = D, the matrix gmmiv_gather_runs filled and a frame-rewriting
 * call has worked on) go back to frames [src, src + len) of x -- FeatureServer::writeFeature over a SegCluster
 * (AccumulateJFAStat.cpp:4675, GeneralTools.cpp:800) for features that stay resident.  Same run table, same rules: x, in DEVICE
 * arrays, runs host or device (a device table only enqueues), pieces of <= 64 frames, runs must not overlap in x.  Frames outside
 * the runs are not touched. */
int gmmiv_scatter_runs(gmmiv_ctx *ctx, void *x, int x_dtype, int64_t ldx, int D, const int64_t *runs, int64_t nrun, const void *in);

/* ---- cepstral mean / variance normalisation on resident frames: NormFeat's default mode (normFeat(), NormFeat.cpp:231-518) and the
 * online mode of NormFeatWindowMode (normFeatOnlineMode, NormFeatWindowMode.cpp:165-311) -------------------------------------------
 * x and out are DEVICE arrays (like gmmiv_gather_runs); every other array is host or device, and with device pointers throughout
 * every call only enqueues on the context's stream.  x_dtype / out_dtype: GMMIV_F32 or GMMIV_F64 independently; arithmetic is fp64,
 * an f32 output is rounded once.  No result is accumulated with atomics: every value is bitwise reproducible and does not depend on
 * what else shares the call.  nrun = 0, nfiles = 0 and files / runs without frames are valid.
 *
 * RUN TABLE: runs[3 r + 0 .. 2] = (first frame, length, group).  Group ids are non-decreasing along the table and lie in
 * [0, ngroups); a group may have no run.  A HOST table that breaks this is GMMIV_ERR_ARG before anything is enqueued; a DEVICE
 * table is not checked.  A run may have any length, but one run is one unit of work (one workgroup): the caller cuts long runs
 * (the host layer cuts at 4096 frames), as with gmmiv_gather_runs.
 *
 * gmmiv_frame_moments_groups: acc[g * (2 D + 1) + ...] += (sum x [D], sum x^2 [D], n) over the frames of group g's runs -- the layout of
 * gmmiv_frame_moments per group, accumulateStatFrame over a Seg (segmental mode, NormFeat.cpp:352-356) or over a cluster (file mode,
 * :455-459).  Order: the partial sums of a run depend on its LENGTH alone (16 interleaved row sums, each left to right, added in
 * order), a group's total is its runs' partials added in table order, and that total is added to acc once.  n is exact.
 * gmmiv_frame_moments_stats: mean = s / n, std = sqrt(ss / n - mean mean), [ngroups x D] each: FrameAccGD::getMeanVect / getStdVect,
 * biased, every operation rounded on its own (the form KAT-4 pins).  n = 0 gives NaN in both.
 * gmmiv_feat_norm_apply: out[t][i] = (x[t][i] - mean[g][i]) / std[g][i] on the frames of the runs -- computeZeroOne
 * (GeneralTools.cpp:670-682), one subtraction and one true division.  mean == NULL: nothing is subtracted (varOnly; the reference
 * subtracts 0.0), std == NULL: nothing is divided (cmsOnly; the reference divides by 1.0).  out may be exactly x (same pointer, dtype
 * and stride); any other overlap of the two frame ranges is GMMIV_ERR_ARG (the rule of gmmiv_feat_compensate; with a device table only
 * out == x with another dtype or stride can be seen and is refused).  Frames outside the runs and columns >= D of a row are not
 * touched; a column slice is a pointer offset (x + 16, D = 1, ldx = 34: the energy pass of the recipe).
 *
 * gmmiv_feat_norm_online: per file f = frames [file_begin[f], file_begin[f + 1]) of n frames, with W = window >= 1 and
 * L = min(look_ahead, W) >= 0: the state (m, c) starts as the FrameAccGD mean / biased std of W - L zero vectors followed by the first L
 * frames (:243-270; n < L: the window shrinks to W' = W - L + n -- zeros and the whole file -- and W' replaces W below, :256-262; L = 0
 * is the tool without initWithDelay, state 0).  Then for frame k = 1 .. n:  B = 1 if k < L else (W - 1) / W;  m <- B m + (1 - B) x;
 * c <- sqrt(c c B + (1 - B) (x x));  out = (x - m) / c with the UPDATED m, c (:114-137, :285-296).  Two quirks of the tool are kept:
 * frame k = L is folded in a second time, and c blends raw second moments, not variances.  One is NOT: in the tool a shrunken
 * window length stays in force for the following files of the list; here every file starts from the caller's W, so a file's result
 * never depends on its neighbours.  The recurrences are linear in m and c c and run as a chunked scan (chunks of 1024 frames counted
 * from the file's first frame; one chain per chunk and dimension), within W' 2^-53 (max|x| / c + |out|) of the sequential loop.
 * With a device file_begin the scratch of the scan is sized from the allocation that holds x.  Same overlap rule as above.
 * Kernel timers: "k_moments_groups", "k_moments_stats", "k_feat_norm_apply", "k_feat_norm_online". */
int gmmiv_frame_moments_groups(gmmiv_ctx *ctx, const void *x, int x_dtype, int64_t ldx, int D, const int64_t *runs, int64_t nrun,
                               int64_t ngroups, double *acc);
int gmmiv_frame_moments_stats(gmmiv_ctx *ctx, int64_t ngroups, int D, const double *acc, double *mean, double *std);
int gmmiv_feat_norm_apply(gmmiv_ctx *ctx, const void *x, int x_dtype, int64_t ldx, int D, const int64_t *runs, int64_t nrun, int64_t ngroups,
                          const double *mean /* nullable */, const double *std /* nullable */, void *out, int out_dtype, int64_t ldo);
int gmmiv_feat_norm_online(gmmiv_ctx *ctx, const void *x, int x_dtype, int64_t ldx, int D, const int64_t *file_begin, int64_t nfiles,
                           int64_t window, int64_t look_ahead, void *out, int out_dtype, int64_t ldo);

/* ---- EnergyDetector on resident frames (LIA_SpkDet/EnergyDetector/src/EnergyDetector.cpp:118-279, thresholdMode meanStd) for a whole
 * list of files: gmmiv_energy_train keeps every file's EM chain inside one workgroup of ONE launch, gmmiv_energy_select is selectFrames
 * as a parallel pass.  x is a DEVICE array and points at the ENERGY COLUMN (a column slice is a pointer offset, as with
 * gmmiv_feat_norm_apply: x + 16 with ldx = 34); frame t is x[t * ldx], GMMIV_F32 or GMMIV_F64.  Every other array is host or device,
 * and with device pointers throughout both calls only enqueue on the context's stream.  nfiles = 0, nrun = 0 and files without frames
 * are valid.
 *
 * RUN TABLE: that of the NormFeat calls, runs[3 r + 0 .. 2] = (first frame, length, file); file ids non-decreasing and in [0, nfiles),
 * a file may have no run; a HOST table that breaks this is GMMIV_ERR_ARG before anything is enqueued, a DEVICE table is not checked.  A
 * run here is ONE INPUT LABEL SEGMENT of any length -- never cut it: selectFrames' end-of-segment rule depends on where it ends.  A
 * file's selection is its runs' frames in table order (wherever they lie in the buffer), x_0 .. x_(n-1).
 *
 * gmmiv_energy_train, per file, fp64 throughout, a model of C in 1 .. 8 one-dimensional Gaussians:
 *   globalCov = ss / n - (s / n)^2  (FrameAccGD's biased covariance, the rule of gmmiv_frame_moments; not screened);
 *   init (:173-193): mean_c = -2 + c 4 / (C - 1) (-2 for C = 1), cov 1, weights 1 / C;
 *   nb_train_it x ( full-posterior EM statistics occ, sum g x, sum g x^2, count under the zero-likelihood rule of "DEGENERATE INPUTS";
 *                   gmmiv_em_get's formula: w = occ / count, mean = sum g x / occ, cov = sum g x^2 / occ - mean^2, occ == 0 keeps the previous
 *                   mean and covariance with weight 0;  gmmiv_variance_control against globalCov: floor test first, then ceiling );
 *   threshold = mean[higher] - alpha sqrt(cov[higher]), higher = the first index of the largest mean (strict >, findMaxEnergyDistrib).
 * nb_train_it = 0 is valid (the threshold of the init model).  Outputs: model [nfiles x 3 C] = (w | mean | cov) per file, threshold
 * [nfiles], status [nfiles] (int32 bit set): GMMIV_ENERGY_EMPTY -- no frame: the model as initialised, threshold NaN, no other bit;
 * GMMIV_ENERGY_NONFINITE -- the threshold or a model value is not finite; GMMIV_ENERGY_FLOORED / _CEILED -- an entry was floored /
 * ceiled in the LAST iteration.  No atomics: every sum is 512 strided per-lane partials (lane j adds frames j, j + 512, ... in order),
 * a wave reduction, the 8 waves added in order -- a function of the file's selection alone, so a file's bits never depend on its
 * neighbours, its place in the list or the rest of the call.  A selection of at most gmmiv_energy_stage_frames(x_dtype) frames is
 * staged in LDS once, a longer one is streamed per iteration (same order, same bits).  C outside 1 .. 8 is GMMIV_ERR_ARG.
 *
 * gmmiv_energy_select, per file: frame i of the selection is IN when x_i > threshold[f] (strict).  Output segments never cross an input
 * run; begin and length count frames of the SELECTION (the reference's `ind`); a run of frames that ends inside its input segment has
 * length = its frame count, one that reaches the input segment's end is one frame longer (:144 against :151, as written).
 * n_above [nfiles] (nullable) = frames in; seg_count [nfiles] (nullable) = output segments; seg_begin / seg_len (both or neither) =
 * the segments of file f at [seg_off[f], seg_off[f + 1]) -- CSR, seg_off [nfiles + 1] from a first call with seg_begin = seg_len = NULL
 * (counts only; seg_off is then not read).  Segments beyond a file's CSR room are not written.  Worst case of a file: one segment per
 * two frames plus one per input run.
 * Kernel timers: "k_energy_em", "k_energy_select". */
#define GMMIV_ENERGY_EMPTY 1
#define GMMIV_ENERGY_NONFINITE 2
#define GMMIV_ENERGY_FLOORED 4
#define GMMIV_ENERGY_CEILED 8
#define GMMIV_ENERGY_MAX_C 8
int64_t gmmiv_energy_stage_frames(int x_dtype); /* the longest selection gmmiv_energy_train stages in LDS (0 for an unknown dtype) */
int gmmiv_energy_train(gmmiv_ctx *ctx, const void *x, int x_dtype, int64_t ldx, const int64_t *runs, int64_t nrun, int64_t nfiles, int C,
                       int nb_train_it, double variance_flooring, double variance_ceiling, double alpha, double *model, double *threshold,
                       int32_t *status);
int gmmiv_energy_select(gmmiv_ctx *ctx, const void *x, int x_dtype, int64_t ldx, const int64_t *runs, int64_t nrun, int64_t nfiles,
                        const double *threshold, int64_t *n_above /* nullable */, int64_t *seg_count /* nullable */,
                        const int64_t *seg_off /* with seg_begin */, int64_t *seg_begin /* nullable */, int64_t *seg_len /* nullable */);

/* ---- segment means of per-frame values (ComputeTest's score per segment, ComputeTest.cpp:181-199) ------
 * out[r * nseg + s] = mean of v[r * ld + t], t in [seg_begin[s], seg_begin[s+1])  (0 for an empty segment).
 * v: DEVICE array of nrows rows (the world's and the clients' per-frame log-likelihoods as the llk_* entry points
 * leave them); seg_begin: nseg + 1 HOST offsets; out: host or device.  The summation order is fixed by the
 * segment bounds alone (pieces of 8192 frames, added in order). */
int gmmiv_segment_means(gmmiv_ctx *ctx, const double *v, int64_t ld, int nrows, const int64_t *seg_begin,
                        int64_t nseg, double *out);

/* ---- MixtureStat::computeAndAccumulateLLK(f,1.0,TOP_DISTRIBS_NO_ACTION) loop -------------------
 * (LIA_SpkTools/src/AccumulateStat.cpp:69-94, :344-379; AccumulateTVStat.cpp:1644-1648)
 * llk_out[T] (nullable) = clamp(log sum_c w_c lk_c(x_t), min_llk, max_llk);
 * sums[0] += sum_t llk_out[t] (clamped), sums[1] += T  -> getMeanLLK() = sums[0]/sums[1]. */
int gmmiv_llk(gmmiv_ctx *ctx, const gmmiv_gmm *g, const void *x, int x_dtype, int64_t T, int64_t ldx,
              double min_llk, double max_llk, double *llk_out, double *sums);

/* ---- computeAndAccumulateLLK(f,1.0,DETERMINE_TOP_DISTRIBS) + StatServer::getTopDistribIndexVector
 * (LIA_SpkDet/ComputeTest/src/ComputeTest.cpp:163; LIA_SpkTools/src/TopGauss.cpp:167-193)
 * Per frame: idx[t*ctop+j] / lk[t*ctop+j] = the ctop largest w_c lk_c, descending (ties: lower
 * index first); nontop_lk = sum of the others (linear, may underflow), nontop_llk = its log
 * (-inf when empty), nontop_w = 1 - sum of the selected weights; llk = clamp(log(top [+ rest])).
 * lk, nontop_lk, nontop_w, llk_out may be NULL.  1 <= ctop <= min(64, C): a request for more Gaussians than the
 * model has is GMMIV_ERR_ARG, not clamped -- the row stride of idx / lk is the caller's ctop, so the caller clamps. */
int gmmiv_llk_determine_top(gmmiv_ctx *ctx, const gmmiv_gmm *world, const void *x, int x_dtype,
                            int64_t T, int64_t ldx, int ctop, int mode, double min_llk, double max_llk,
                            int32_t *idx, double *lk, double *nontop_lk, double *nontop_llk,
                            double *nontop_w, double *llk_out);

/* ---- TopGauss::compute (LIA_SpkTools/src/TopGauss.cpp:136-198): the per-frame Gaussian selection that the factor-analysis
 * tools store per feature file.  The sorted top list of every frame comes from DETERMINE_TOP_DISTRIBS with topDistribsCount =
 * cap (1 <= cap <= min(64, C); the reference's "this should be high enough"), then
 *   top_gauss >= 1 : count[t] = (int)top_gauss                                            (:170)
 *   top_gauss <  1 : Gaussians are taken, heaviest first, until their cumulative likelihood exceeds top_gauss * exp(llk_t)
 *                    (the test precedes each addition, :163-167) -- a VARIABLE count per frame, at most cap; *n_capped
 *                    (HOST, nullable) = frames whose mass was not reached within cap entries;
 *   snsw[t] = 1 - sum of the selected weights, snsl[t] = max(exp(llk_t) - sum of the selected likelihoods, EPS_LK = 1e-200).
 * idx [T x cap]: the selected indices of frame t first, -1 behind them -- gmmiv_llk_use_top(ctop = cap, idx, log(snsl)) then
 * evaluates exactly the stored selection (TopGauss::get, :275-316).  llk_out (nullable) = the clamped per-frame llk of the
 * DETERMINE pass (its mean is what compute() returns).  All arrays host or device. */
int gmmiv_topgauss_compute(gmmiv_ctx *ctx, const gmmiv_gmm *ubm, const void *x, int x_dtype, int64_t T, int64_t ldx,
                           int cap, double top_gauss, int mode, double min_llk, double max_llk, int32_t *idx,
                           int32_t *count, double *snsw, double *snsl, double *llk_out, int64_t *n_capped);

/* ---- computeAndAccumulateLLK(f,1.0,USE_TOP_DISTRIBS) on a client model ------------------------
 * (ComputeTest.cpp:166-167; StatServer::setTopDistribIndexVector, TopGauss.cpp:297-308)
 * llk_out[t] = clamp(log(sum_j w_c lk_c(client) over c = idx[t][j]  [+ exp(nontop_llk[t])])).
 * ctop as above; an entry of idx outside [0, C) contributes nothing (it is never dereferenced). */
int gmmiv_llk_use_top(gmmiv_ctx *ctx, const gmmiv_gmm *client, const void *x, int x_dtype, int64_t T,
                      int64_t ldx, int ctop, const int32_t *idx, const double *nontop_llk, int mode,
                      double min_llk, double max_llk, double *llk_out);

/* The same for SEVERAL client models on one test segment -- the client loop of ComputeTest.cpp:170-207 (every model of an ndx line
 * is scored on the same frames with the same world indices) as ONE call: llk_out is [n_clients][T] (host or device), row i what
 * gmmiv_llk_use_top returns for clients[i].  All clients must have the dimension count of clients[0]; one launch when the
 * four-lanes-per-candidate kernel applies (ctop <= 16, even dimension count), client by client otherwise. */
int gmmiv_llk_use_top_multi(gmmiv_ctx *ctx, int n_clients, const gmmiv_gmm *const *clients, const void *x, int x_dtype, int64_t T,
                            int64_t ldx, int ctop, const int32_t *idx, const double *nontop_llk, int mode,
                            double min_llk, double max_llk, double *llk_out);

/* ---- MixtureGDStat::computeAndAccumulateOcc + getOccVect (AccumulateTVStat.cpp:302,334-335;
 * FactorAnalysis.cpp:204-205): the full posterior vector of every frame,
 * gamma[t*C + c] = w_c lk_c(x_t) / sum_c' w_c' lk_c'(x_t)   (row-major [T x C]). */
int gmmiv_occ(gmmiv_ctx *ctx, const gmmiv_gmm *gmm, const void *x, int x_dtype, int64_t T, int64_t ldx,
              double *gamma);

/* ---- model-based feature compensation: the two reference loops that REWRITE the frames from a GMM's per-frame posteriors ----------
 * gmmiv_feat_compensate: channel compensation in the feature domain, JFAAcc::normalizeFeatures (AccumulateJFAStat.cpp:4623-4686,
 * substractUXfromFeatures :4689-4697) and its LFA twin FactorAnalysisStat::normalizeFeatures (FactorAnalysis.cpp:979-1024); callers
 * NormFeat.cpp:825, TrainTarget.cpp:347, SimpleSpkDetSystem.cpp:392:
 *   out[t][i] = x[t][i] - sum_c gamma_tc offset[c * D + i],   gamma = the full posterior of g (what gmmiv_occ returns),
 * g = the session model m + Vy + Dz + Ux, offset [C x D] = U x_h of the session (getUX, :1788-1800).
 * gmmiv_feat_map: featureMapping / getBestGaussian / mapDataToDistrib (GeneralTools.cpp:762-811, caller NormFeat.cpp:619):
 *   best[t] = argmax_c w_c lk_c(x_t) of the channel-dependent model cd (lowest index on ties, 0 when every term is 0: the strict
 *   `>` from 0 of getBestGaussian); out[t][i] = sqrt(ci_cov / cd_cov) * (x - cd_mean) + ci_mean of that Gaussian, these operations in
 *   this order, each rounded on its own.  cd_mean, cd_cov, ci_mean, ci_cov: [C x D] (getMean / getCov of both mixtures); best
 *   (nullable): int32 [T].
 * Both: x_dtype and out_dtype are GMMIV_F32 or GMMIV_F64 independently; arithmetic is fp64, an f32 output is rounded once.  out may
 * be exactly x (same pointer, dtype and stride: in place, like the reference's writeFeature); any other overlap of the two frame
 * ranges is GMMIV_ERR_ARG, checked -- like the dtypes -- before anything is enqueued.  T = 0 is valid.  All arrays host or device;
 * with device pointers throughout gmmiv_feat_compensate only enqueues (gmmiv_feat_map waits once for its top-1 selection, like
 * gmmiv_llk_determine_top).  No shape is refused: vectSize <= 60 with "stats_z" 1 runs k_llk_mfma<WZ> + k_feat_comp per frame chunk
 * of the likelihood scratch ("z_scratch_mb") -- the stored likelihoods are streamed once, turned into posteriors with one multiply
 * and contracted against the offsets on the matrix cores; no [T x C] posterior array exists --, anything else (vectSize > 60,
 * "stats_z" 0, a scratch budget too small for a chunk) takes posteriors in frame chunks of 512 MiB, the fp64 GEMM and a subtraction.
 * A frame's result does not depend on its position or its neighbours: the Gaussians are summed in one fixed order (tile by tile,
 * ascending), nothing is accumulated with atomics.  The order differs from the reference's sequential loop: parity is within
 * 2 (C + 1) 2^-53 (|x| + sum_c gamma |offset|) plus the posterior tolerance (tests/test_gpu_feat_comp.py).
 * Kernel timers: "k_llk_mfma" and "k_feat_comp" ("k_posteriors", "k_feat_sub" on the generic path); "k_feat_map". */
int gmmiv_feat_compensate(gmmiv_ctx *ctx, const gmmiv_gmm *g, const void *x, int x_dtype, int64_t T, int64_t ldx,
                          const double *offset, void *out, int out_dtype, int64_t ldo);
int gmmiv_feat_map(gmmiv_ctx *ctx, const gmmiv_gmm *cd, const double *cd_mean, const double *cd_cov, const double *ci_mean,
                   const double *ci_cov, const void *x, int x_dtype, int64_t T, int64_t ldx, void *out, int out_dtype,
                   int64_t ldo, int32_t *best /* nullable */);

/* ---- MixtureStat::computeAndAccumulateEM loop (accumulateStatEM, AccumulateStat.cpp:103-152) ---
 * acc is the flat EM accumulator, length gmmiv_em_acc_len(C,D) = C*(1+2D)+2 doubles:
 *   [ occ[C] | sum g x [C*D] | sum g x^2 [C*D] | sum_t weight*log lk_t | sum_t weight ].
 * ACCUMULATES (resetEM = zero the array; addAccEM = add two arrays; one RCCL all-reduce of this
 * array merges ranks).  gamma_tc = full posterior (all C). */
size_t gmmiv_em_acc_len(int C, int D);
int gmmiv_em_accumulate(gmmiv_ctx *ctx, const gmmiv_gmm *g, const void *x, int x_dtype, int64_t T,
                        int64_t ldx, double weight, double *acc);
/* MixtureStat::getEM(): w = occ/count, mean = sx/occ, cov = sxx/occ - mean^2 (host formula run on
 * the device copy; components with occ == 0 keep prev_mean / prev_cov).  Outputs [C],[C*D],[C*D]. */
int gmmiv_em_get(gmmiv_ctx *ctx, int C, int D, const double *acc, const double *prev_mean,
                 const double *prev_cov, double *w, double *mean, double *cov);

/* varianceControl (LIA_SpkTools/src/TrainTools.cpp:567-587): cov[c,d] clamped to
 * [flooring*cov_signal[d], ceiling*cov_signal[d]] in place (floor test first, then ceiling);
 * counts (HOST, nullable): [0] += floored entries, [1] += ceiled entries. */
int gmmiv_variance_control(gmmiv_ctx *ctx, int C, int D, double *cov, double flooring, double ceiling,
                           const double *cov_signal, int64_t *counts);

/* ---- TVAcc::computeAndAccumulateTVStat (LIA_SpkTools/src/AccumulateTVStat.cpp:281-351) ---------
 * Frames of statistics row u are x[utt_begin[u] .. utt_begin[u+1]) (utt_begin: U+1 HOST offsets).
 * N[u*C+c] = sum_t g_tc ; F[u*C*D + c*D + i] = sum_t g_tc x_ti   (rows are overwritten). */
int gmmiv_tv_stats(gmmiv_ctx *ctx, const gmmiv_gmm *g, const void *x, int x_dtype, int64_t T,
                   int64_t ldx, const int64_t *utt_begin, int64_t U, double *N, double *F);
/* The same with the reference's file -> ndx-line map (AccumulateTVStat.cpp:318-346, TVTranslate::locIndices): the frames of
 * feature file f are x[file_begin[f] .. file_begin[f+1]); statistics row l (an ndx line) is the SUM over the files
 * line_files[line_off[l] .. line_off[l+1]) -- a file listed on several lines is evaluated once and added to each of them
 * (file_begin, line_off, line_files: HOST arrays; rows are overwritten). */
int gmmiv_tv_stats_lines(gmmiv_ctx *ctx, const gmmiv_gmm *g, const void *x, int x_dtype, int64_t T, int64_t ldx,
                         const int64_t *file_begin, int64_t nfiles, int64_t nlines, const int64_t *line_off,
                         const int64_t *line_files, double *N, double *F);

/* ---- MANY MODELS OF ONE SHAPE, ONE MODEL PER SEGMENT: batched enrolment ----------------------------------------------------------
 * TrainTarget adapts thousands of clients with a few thousand frames each (adaptModel, TrainTools.cpp:850-905: per client and
 * iteration one statistics pass under the client's CURRENT model, then computeMAP); verifyEMLK / getLLK score many short files, each
 * under its own model.  The single-model entry points above run one small launch per client between host round trips.  A
 * gmmiv_gmm_batch holds G models of a common (C, D); the *_models entry points evaluate every SEGMENT of one frame matrix under the
 * model the caller names for it, in one log-likelihood pass per chunk.
 *
 * gmmiv_gmm_batch_load: w [G x C], mean [G x C*D], covinv [G x C*D], host or device, model g at p + g * stride (strides in doubles);
 * stride 0 = the array is shared by all G models (the usual case: shared weights and variances, means per client).  The batch keeps
 * device copies and the constants a_c of every model; the packed MFMA operands (what gmmiv_gmm_create keeps per model -- the same
 * bits) are built per call, one launch for all models of a chunk, into a scratch of "models_scratch_mb" MiB (context option, default
 * 2048 = 1024 models of 2048 x 60; never fewer than one model per chunk).
 *
 * Segments: s = frames [seg_begin[s], seg_begin[s+1]) under model seg_model[s]; seg_begin (nseg + 1, non-decreasing) and seg_model
 * are HOST arrays.  A model may serve many segments or none; an empty segment gives zeros.  Frames before seg_begin[0] and from
 * seg_begin[nseg] on belong to no segment: they are not read and their outputs are not touched.  Zero-likelihood frames follow
 * "DEGENERATE INPUTS" exactly like gmmiv_llk / gmmiv_tv_stats, counters included.
 *   gmmiv_llk_models       llk[t] (nullable, indexed like x) = clamp(log sum_c w_c lk_c(x_t)) under the segment's model;
 *                          seg_sum[s] (nullable) = the sum of those over the segment (OVERWRITTEN; 0 for an empty segment)
 *   gmmiv_tv_stats_models  N [nseg x C], F [nseg x C*D] as gmmiv_tv_stats; seg_llk (nullable) [2 s] = sum of the log-likelihoods of the
 *                          segment's frames (unclamped, zero-likelihood frames left out), [2 s + 1] = the number of frames in that sum
 * Work is cut into chunks of whole segments whose frames fit the likelihood scratch ("z_scratch_mb") and whose distinct models fit
 * the model scratch.  A per-frame value does not depend on the chunking; a statistics row depends only on its own segment.
 * Shapes without a stored-likelihood kernel (vectSize > 60) and calls with a segment longer than the scratch walk the segments one
 * by one through the single-model kernels: same results, launch-bound (one model upload and ~5 launches per segment).
 * Kernel timers: "k_llk_mfma", "k_stats_z", "k_gmm_pack". */
typedef struct gmmiv_gmm_batch gmmiv_gmm_batch;
int gmmiv_gmm_batch_create(gmmiv_ctx *ctx, int G, int C, int D, gmmiv_gmm_batch **out);
int gmmiv_gmm_batch_load(gmmiv_gmm_batch *b, const double *w, int64_t w_stride, const double *mean, int64_t mean_stride,
                         const double *covinv, int64_t covinv_stride);
void gmmiv_gmm_batch_destroy(gmmiv_gmm_batch *b);
int gmmiv_llk_models(gmmiv_ctx *ctx, const gmmiv_gmm_batch *b, const void *x, int x_dtype, int64_t T, int64_t ldx,
                     const int64_t *seg_begin, const int32_t *seg_model, int64_t nseg, double min_llk, double max_llk,
                     double *llk /* [T], nullable */, double *seg_sum /* [nseg], nullable */);
int gmmiv_tv_stats_models(gmmiv_ctx *ctx, const gmmiv_gmm_batch *b, const void *x, int x_dtype, int64_t T, int64_t ldx,
                          const int64_t *seg_begin, const int32_t *seg_model, int64_t nseg, double *N, double *F,
                          double *seg_llk /* [2 nseg], nullable */);
/* Debug / test access: the packed block of model g as a call would build it, nct * (2 KS + 2) * 64 doubles (*len, also returned when
 * out == NULL); GMMIV_ERR_UNSUPPORTED for a shape without packed operands. */
int gmmiv_gmm_batch_packed(const gmmiv_gmm_batch *b, int g, double *out, int64_t *len);

/* The work list of the batched log-likelihood kernel, exported so that it can be checked without a GPU (pure host function).  One
 * entry per workgroup: a tile of tile_frames frames (a multiple of 32; the kernel uses 256) that starts at `first`, a multiple of 16 --
 * the 16-frame block holding the segment's first frame, then every tile_frames from there (the stored likelihoods are laid out in
 * blocks of 16 frames, frame = 16 block + row, so a segment cannot be shifted inside its blocks).  The workgroup evaluates the
 * frames [lo, hi) of its tile -- the part that belongs to segment `seg` -- under model `model`; the other rows of its tile are loaded
 * as 0 and none of their outputs is written, so a block that straddles two segments is visited by two workgroups that write
 * disjoint rows.  Rows of the first / last 16-frame block that lie before seg_begin[0] / from seg_begin[nseg] on belong to nobody; the
 * first and the last tile of the list also write those rows of the LIKELIHOOD scratch (pad_lo / pad_hi rows, evaluated on zeros), so
 * that the statistics kernel, which reads whole blocks and masks by multiplying with 0, never meets uninitialised memory.
 * Returns the number of tiles (entries beyond `cap` are counted, not written), or -1 for a bad argument. */
typedef struct gmmiv_model_tile {
    int64_t first;           /* first frame of the tile (multiple of 16) */
    int64_t lo, hi;          /* frames of the segment inside the tile: first <= lo < hi <= first + tile_frames */
    int32_t model, seg;
    int32_t pad_lo, pad_hi;  /* rows [lo - pad_lo, lo) and [hi, hi + pad_hi) are written to the likelihood scratch too (< 16 each) */
} gmmiv_model_tile;
int64_t gmmiv_plan_model_tiles(const int64_t *seg_begin, const int32_t *seg_model, int64_t nseg, int tile_frames,
                               gmmiv_model_tile *tiles, int64_t cap);

/* ---- batched channel compensation: a session model and an offset per segment ------------------------------------------------------
 * gmmiv_feat_compensate for MANY sessions at once (JFAAcc::normalizeFeatures loops over the sessions, ComputeTestJFA over the ndx
 * lines, each with its own model m + Vy + Dz + Ux_h and its own offset U x_h).  Segment s = frames [seg_begin[s], seg_begin[s+1]) is
 * rewritten with the full posterior of model seg_model[s] of the batch and the offset row offset + seg_model[s] * offset_stride
 * ([C x D] doubles, host or device; offset_stride 0 = one row shared by all models, else >= C * D):
 *   out[t][i] = x[t][i] - sum_c gamma_tc offset_row[c * D + i].
 * seg_begin / seg_model are HOST arrays as in gmmiv_llk_models (a device table is GMMIV_ERR_ARG); the call waits once for its table
 * upload, like the other *_models calls, and otherwise only enqueues when x, offset and out are device arrays.  Frames before
 * seg_begin[0] and from seg_begin[nseg] on belong to no segment: they are neither read from x nor written to out (a host out is staged
 * and copied back for the frames of the segments only; padding columns are never written).  Everything gmmiv_feat_compensate promises
 * carries over: x_dtype / out_dtype independent with fp64 arithmetic; out may be exactly x (same pointer, dtype and stride), any other
 * overlap is GMMIV_ERR_ARG; every argument error (a batch of another context, seg_model outside [0, G), a decreasing table,
 * offset == NULL, a bad dtype or stride) is reported before anything is enqueued; T = 0 and nseg = 0 are valid; unusable and
 * zero-likelihood frames are copied through and counted once in "zero_llk_frames" / "screened_frames".
 * Work is cut into chunks of whole segments like gmmiv_tv_stats_models (frames that fit "z_scratch_mb", distinct models that fit
 * "models_scratch_mb"; the packed offsets of a chunk's models take 16 C ceil(D / 16) doubles each on top).  Per chunk: one model
 * pack, one offset pack, k_llk_mfma<WZ> with a model per tile, k_feat_comp with a segment per wave.  A frame has the bits
 * gmmiv_feat_compensate gives it on a single-model handle, whatever its row in a 16-frame block, its chunk or its neighbours.  In
 * place across a chunk boundary is right by construction: the log-likelihood kernel loads the rows outside its chunk's segments as
 * 0, so a row the previous chunk has rewritten is never evaluated.  Shapes without the stored-likelihood path (vectSize > 60,
 * "stats_z" 0) and calls with a segment longer than the scratch walk the segments one by one through gmmiv_feat_compensate on a
 * single-model handle: the same definition, launch-bound.
 * Kernel timers: "k_gmm_pack", "k_llk_mfma", "k_feat_comp". */
int gmmiv_feat_compensate_models(gmmiv_ctx *ctx, const gmmiv_gmm_batch *b, const void *x, int x_dtype, int64_t T, int64_t ldx,
                                 const int64_t *seg_begin, const int32_t *seg_model, int64_t nseg, const double *offset,
                                 int64_t offset_stride, void *out, int out_dtype, int64_t ldo);

/* The work list of the segment-aware k_feat_comp (pure host function, the conventions of gmmiv_plan_model_tiles).  One entry per
 * wave: the 16-frame blocks [block, block + blocks_per_tile) (block b = frames [16 b, 16 b + 16)) and the frames [lo, hi) of segment
 * `seg` inside them, 16 block <= lo < hi <= 16 (block + blocks_per_tile), under model `model` = seg_model[seg].  The entries of a
 * segment start at the block holding its first frame and step by blocks_per_tile; entries are sorted by (seg, block), so the items of
 * one segment -- which read the same packed offset -- are adjacent; an empty segment has none.  Returns the number of entries
 * (entries beyond `cap` are counted, not written; tiles may be NULL), or -1 for a decreasing seg_begin, blocks_per_tile < 1 or
 * nseg < 0. */
typedef struct gmmiv_feat_tile {
    int64_t block;
    int64_t lo, hi;
    int32_t model, seg;
} gmmiv_feat_tile;
int64_t gmmiv_plan_feat_tiles(const int64_t *seg_begin, const int32_t *seg_model, int64_t nseg, int blocks_per_tile,
                              gmmiv_feat_tile *tiles, int64_t cap);

/* ---- A WHOLE LIST OF TRIALS: batched ComputeTest ---------------------------------------------------------------------------------------
 * ComputeTest (ComputeTest.cpp:129-215) scores every line of an ndx -- a test file against its handful of clients out of thousands --
 * with DETERMINE_TOP_DISTRIBS on the world model, USE_TOP_DISTRIBS per client and a mean over the selected frames.  Line by line that is
 * three launches, a table upload, a stream drain and a read-back around a few tens of microseconds of kernel time.  gmmiv_llr_trials takes
 * the frames of ALL lines as segments of one matrix (as gmmiv_llk_models), the clients as a gmmiv_gmm_batch of the world's (C, D), and a
 * list of trials i = (trial_seg[i], trial_model[i]) in any order; a pair may repeat and a segment may have no trial.
 *   per segment s, n_s frames:  the world's top set, remainder and clamped llk_w(t) are exactly those of gmmiv_llk_determine_top(world,
 *                               ctop, mode, min_llk, max_llk); world_mean[s] = sum_t llk_w(t) / n_s
 *   per trial i = (s, g):       llk_c(t) is exactly what gmmiv_llk_use_top returns for model g on the world's indices and remainder of
 *                               frame t; client_mean[i] = sum_t llk_c(t) / n_s; llr[i] = client_mean[i] - world_mean[s]
 * Zero-likelihood and NaN frames follow "DEGENERATE INPUTS": both passes give min_llk and the frame counts in n_s (the frames are
 * screened and counted once, by the world pass).  An empty segment gives 0 for all three.  Frames outside [seg_begin[0],
 * seg_begin[nseg]) are not read.  seg_begin (nseg + 1, non-decreasing), trial_seg and trial_model are HOST arrays, copied before return;
 * llr, client_mean (nullable), world_mean (nullable; written for every segment, also with ntrial = 0) are host or device arrays.  T = 0,
 * nseg = 0 and ntrial = 0 are valid.  GMMIV_ERR_ARG: a batch of another (C, D) than the world, ctop outside 1 .. min(64, C), a trial
 * index out of range, a table on the device.
 * Sums: a work item of the kernel is (trial, piece), a piece being P frames counted from the segment's first frame, P = GMMIV_TRIAL_PIECE
 * unless the A/B option "trials_piece" names another multiple of 4 (gmmiv_trial_piece(ctx) returns the P in effect); frame
 * j of a piece is added, in frame order, to partial j mod 4, a piece is ((p0 + p1) + p2) + p3, a segment the sum of its pieces in order.
 * A result therefore depends on its segment's frames and its model only -- not on the rest of the list, its order, or the chunking
 * (per-frame world results, 4 ctop + 16 bytes per frame, are kept for chunks of whole segments of "trials_scratch_mb" MiB, default 2048).
 * ctop <= 16 with an even vectSize runs k_topc_use4_trials (no per-frame client value in memory); any other shape walks the trials
 * through the kernels of gmmiv_llk_use_top into a scratch row that the same piece scheme sums: same definition, launch-bound.
 * Synchronisation: the call is NOT enqueue-only.  It waits for the context's stream once after uploading its tables (they live in host
 * memory of the call) and once per chunk inside the world pass (gmmiv_llk_determine_top reads its fallback flags back); with x and the
 * outputs on the device everything else -- the trial kernel, the reductions, the writes of llr / client_mean / world_mean -- is only
 * enqueued, so the outputs are valid in stream order (gmmiv_ctx_sync before reading them from another stream).  Host outputs are
 * complete on return.
 * Kernel timers: "k_topc_use" (the trial kernel), "k_trial_reduce", and the world pass's own ("k_llk_mfma", "k_topc_rank", ...). */
#define GMMIV_TRIAL_PIECE 128 /* default frames per work item; a multiple of 4 (DESIGN.md section 3.16 has the A/B) */
int gmmiv_trial_piece(const gmmiv_ctx *ctx); /* the piece gmmiv_llr_trials uses on ctx: "trials_piece" if set and valid, else (and for NULL) GMMIV_TRIAL_PIECE */
int gmmiv_llr_trials(gmmiv_ctx *ctx, const gmmiv_gmm *world, const gmmiv_gmm_batch *clients, const void *x, int x_dtype, int64_t T,
                     int64_t ldx, const int64_t *seg_begin, int64_t nseg, const int32_t *trial_seg, const int32_t *trial_model,
                     int64_t ntrial, int ctop, int mode, double min_llk, double max_llk, double *llr /* [ntrial] */,
                     double *client_mean /* [ntrial], nullable */, double *world_mean /* [nseg], nullable */);
/* The work list of the trial kernel (pure host function): the pieces [b + k P, min(b + (k + 1) P, e)) of every trial's segment [b, e),
 * P = piece_frames (a positive multiple of 4), sorted by (segment, piece, position of the trial in the list) -- the trials of one
 * segment and piece run next to each other and share the rows of x and of the world's indices in cache.  An empty segment and a segment
 * without a trial have no tile.  Returns the number of tiles (entries beyond `cap` are counted, not written; tiles may be NULL), or -1
 * for a bad argument (a decreasing seg_begin, a bad piece_frames, a trial_seg outside [0, nseg)). */
typedef struct gmmiv_trial_tile {
    int64_t lo, hi;                    /* frames [lo, hi) of the segment */
    int32_t trial, seg, model, piece;  /* position in the trial list, trial_seg / trial_model of it, piece number inside the segment */
} gmmiv_trial_tile;
int64_t gmmiv_plan_trial_tiles(const int64_t *seg_begin, int64_t nseg, const int32_t *trial_seg, const int32_t *trial_model,
                               int64_t ntrial, int piece_frames, gmmiv_trial_tile *tiles, int64_t cap);

/* computeMAP (TrainTools.cpp:445-556) for G models at once, from the statistics rows of gmmiv_tv_stats_models: element-wise over
 * [G x C x D], nothing leaves the device.  Per model g: count_g = count[g * count_stride] (seg_llk + 1 with stride 2 fits), the ML
 * estimate w_c = N_c / count_g (0 when count_g = 0), mean_c = F_c / N_c, a Gaussian with N_c = 0 keeps cur_mean (model g at
 * cur_mean + g * cur_stride, stride 0 = shared) and gets weight 0 like gmmiv_em_get; then, with n = count_g TRUNCATED to an integer
 * (the reference passes an unsigned long) and the a-priori model (w0, mean0):
 *   GMMIV_MAP_OCC_DEP / GMMIV_MAP_MODEL_BASED   alpha = w_c n; a = alpha / (alpha + mean_reg); mean = (1 - a) mean0 + a mean_ml;
 *                          weights (weight_adapt): a = alpha / (alpha + weight_reg), a w_c + (1 - a) w0_c, renormalised to sum 1
 *   GMMIV_MAP_CONST        mean = mean_alpha mean0 + (1 - mean_alpha) mean_ml
 *   GMMIV_MAP_CONST2       mean = (mean_alpha w0 mean0 + (1 - mean_alpha) w mean_ml) / (w0 mean_alpha + w (1 - mean_alpha))
 *   GMMIV_MAP_NONE         the ML estimate itself (an unknown mapAlgo: "No adaptation will be perform")
 * mean_adapt = 0 gives mean0; without weight_adapt (and for the two constant methods) the weights are w0.  Variances are not touched
 * here: varAdapt is gmmiv_map_adapt_models_full below, on the second-order rows of gmmiv_em_stats_models.  mean_out [G x C*D],
 * w_out [G x C] (nullable): device or host; device outputs can be handed straight to gmmiv_gmm_batch_load.  Every operation is rounded
 * on its own (no contraction). */
enum { GMMIV_MAP_NONE = 0, GMMIV_MAP_OCC_DEP = 1, GMMIV_MAP_MODEL_BASED = 2, GMMIV_MAP_CONST = 3, GMMIV_MAP_CONST2 = 4 };
int gmmiv_map_adapt_models(gmmiv_ctx *ctx, int G, int C, int D, const double *N, const double *F, const double *count,
                           int64_t count_stride, const double *w0, const double *mean0, const double *cur_mean, int64_t cur_stride,
                           int method, int mean_adapt, int weight_adapt, double mean_reg, double weight_reg, double mean_alpha,
                           double *mean_out, double *w_out);

/* ---- batched enrolment WITH VARIANCES: second-order statistics per segment, the variance branch of computeMAP, normalizeMixture ------
 * gmmiv_em_stats_models: the contract of gmmiv_tv_stats_models (host segment tables, an empty segment gives zeros, frames outside the
 * segments are not read, zero-likelihood / NaN frames left out and counted once, rows OVERWRITTEN, seg_llk nullable, host or device
 * outputs; with device pointers the call only enqueues beyond what gmmiv_tv_stats_models waits for) plus
 *   S [nseg x C*D],  S[s*C*D + c*D + i] = sum_t g_tc x_ti^2.
 * vectSize <= 60: the per-model tiles of the batched log-likelihood kernel, then the stored-likelihood statistics kernel in its EM shape
 * (x^2 staged in LDS) with one segment per workgroup row and a row epilogue that writes N, F and S directly: every (segment, Gaussian)
 * row is written by one wave in the fixed order of its own segment's 16-frame blocks.  No floating-point atomics; a row depends only on
 * its own segment's frames (at their position modulo 16 in x) and model -- not on the other segments, their order, the chunking or the
 * scratch options: the same bits when the segment is the only one of the call.  Other shapes (vectSize 61-80, > 80, a segment longer than
 * the likelihood scratch) walk the segments through the single-model second-order kernels (the recomputing statistics kernel with x^2,
 * the generic gamma^T [x | 1 | x^2] GEMM): the same definition, launch-bound.  "prune_log2", "z_waves" and "z_depth_em" apply as in
 * gmmiv_em_accumulate.  Kernel timers: "k_llk_mfma", "k_stats_z", "k_gmm_pack" ("k_stats_mfma", "k_posteriors" on the walk).
 *
 * gmmiv_map_adapt_models_full: computeMAP for G models with all three branches.  N, F, count, w0, mean0, cur_mean, method, mean_adapt,
 * weight_adapt, the regulation factors and mean_alpha are those of gmmiv_map_adapt_models, and mean_out / w_out are ITS BITS (the same
 * device function) whatever var_adapt says.  The variance: the ML estimate cov_ml = S / N - mean_ml^2 as gmmiv_em_get (a Gaussian with
 * N = 0 keeps cur_cov, model g at cur_cov + g * cur_cov_stride, stride 0 = shared, like its mean); then
 *   GMMIV_MAP_OCC_DEP / GMMIV_MAP_MODEL_BASED with var_adapt   alpha = w_c n and n as for the mean, aV = alpha / (alpha + var_reg),
 *                          cov = (1 - aV) cov0 + aV cov_ml + ((1 - aV) aV) (mean0 - mean_ml)^2      (TrainTools.cpp:468-475, :518-525)
 *   ... without var_adapt, GMMIV_MAP_CONST, GMMIV_MAP_CONST2    cov0 (the reference has a TODO for the constant methods)
 *   GMMIV_MAP_NONE         cov_ml
 * S and cur_cov may be NULL when no branch reads them (var_adapt = 0 and a method other than NONE, or cov_out = NULL).  mean_out, cov_out,
 * w_out: each nullable, not all three.  status [G] (int32, required, where the outputs live: device or host) = the number of entries of
 * cov_out of model g that are not positive and finite (0 without cov_out); it is written on the device and not read by the call.
 * Every operation is rounded on its own (no contraction).
 *
 * gmmiv_normalize_models: normalizeMixture (TrainTools.cpp:287-315) towards N(0, 1), in place, for G models: nb_it times {mixtureFusion
 * (:241-284): per dimension the single Gaussian with the mixture's first two moments, a LEFT FOLD over the Gaussians c = 0 .. C-1;
 * mean = (mean - m) / sqrt(v); unless mean_only, cov = cov / v}.  One thread per (model, dimension) in the host code's order of
 * operations.  w at w + g * w_stride (0 = shared), mean / cov [G x C*D] DEVICE arrays.  cov is read in either mode (the fusion needs the
 * variances) and written unless mean_only.
 *
 * gmmiv_gmm_batch_load_cov: gmmiv_gmm_batch_load from VARIANCES, covInv = 1 / cov on the device as gmmiv_gmm_set_cov does -- the device
 * outputs of the two calls above go back into the batch without a host round trip. */
int gmmiv_em_stats_models(gmmiv_ctx *ctx, const gmmiv_gmm_batch *b, const void *x, int x_dtype, int64_t T, int64_t ldx,
                          const int64_t *seg_begin, const int32_t *seg_model, int64_t nseg, double *N, double *F, double *S,
                          double *seg_llk /* [2 nseg], nullable */);
int gmmiv_map_adapt_models_full(gmmiv_ctx *ctx, int G, int C, int D, const double *N, const double *F, const double *S /* nullable */,
                                const double *count, int64_t count_stride, const double *w0, const double *mean0, const double *cov0,
                                const double *cur_mean, int64_t cur_mean_stride, const double *cur_cov /* nullable */,
                                int64_t cur_cov_stride, int method, int mean_adapt, int var_adapt, int weight_adapt, double mean_reg,
                                double var_reg, double weight_reg, double mean_alpha, double *mean_out, double *cov_out, double *w_out,
                                int32_t *status);
int gmmiv_normalize_models(gmmiv_ctx *ctx, int G, int C, int D, const double *w, int64_t w_stride, double *mean, double *cov, int nb_it,
                           int mean_only);
int gmmiv_gmm_batch_load_cov(gmmiv_gmm_batch *b, const double *w, int64_t w_stride, const double *mean, int64_t mean_stride,
                             const double *cov, int64_t cov_stride);

/* computeMLLR (TrainTools.cpp:788-866) for G clients at once, from the statistics rows of gmmiv_tv_stats_models: one global affine
 * transform of the a-priori means per client.  With xi_j = [1, mean0_j] (D + 1 values), a_j = N_gj / cov0_jp and the ML mean
 * m_jp = F_gjp / N_gj, for every dimension p
 *   G_p = sum_j a_j xi_j xi_j^T,   z_p = sum_j a_j m_jp xi_j,   W_g[p, :] = G_p^-1 z_p        (G_p symmetric, (D+1) x (D+1))
 * and mean_out[g, j, :] = W_g[:, 0] + W_g[:, 1:] mean0_j.  The reference weights with occ_j = w_j frameCount = N_gj up to one factor
 * common to G_p and z_p, so W does not depend on the frame count, on its truncation, or on the normalisation of the ML weights.  A
 * Gaussian with N_gj = 0 is left out of both sums (its F row is never read into them).  Weights and variances of an MLLR client are
 * the a-priori model's: nothing to compute here.
 *   k_mllr_solve   one workgroup per (g, p): the augmented Gram matrix [xi | m]^T diag(a) [xi | m] on the fp64 matrix cores (lower
 *                  16 x 16 tiles only), then a square-root-free Cholesky factorisation and the two substitutions in LDS.  No atomics:
 *                  a client's result does not depend on G, on its place in the batch or on the chunking, and is the same bits on
 *                  every run.  The reference divides by cov0 inside its sums and multiplies by an explicit inverse of G_p; the device
 *                  divides once per Gaussian and substitutes through the factor -- the same result to within the rounding of a
 *                  backward-stable solve (tests/test_gpu_mllr.py states the bar), not bitwise.  Dividing by the variance, as here and
 *                  in the reference, against multiplying by a stored reciprocal 1 / cov0 is a difference of the same kind: within
 *                  that bar, not bitwise.
 *   status [G] (nullable): 0, or 1 + p for the first dimension p whose G_p met a pivot that is not positive and finite (fewer than
 *                  D + 1 occupied Gaussians in general position, a client without frames, NaN statistics).  Such a client gets the
 *                  identity transform W = [0 | I] and mean_out = mean0, bit for bit.  The call never reads the status back: with
 *                  device arrays it only enqueues.
 * W_out [G x D x (D+1)] and mean_out [G x C*D] are nullable, not both; every array may be host or device.  D <= 62
 * (GMMIV_ERR_UNSUPPORTED above).  Kernel timers: "k_mllr_solve", "k_mllr_pack" (the padded [1 | mean0] table, once per call). */
int gmmiv_mllr_adapt_models(gmmiv_ctx *ctx, int G, int C, int D, const double *N /* [G x C] */, const double *F /* [G x C*D] */,
                            const double *mean0 /* [C*D] */, const double *cov0 /* [C*D] variances */,
                            double *W_out /* [G x D x (D+1)], nullable */, double *mean_out /* [G x C*D], nullable */,
                            int32_t *status /* [G], nullable */);

/* ---- TVAcc i-vector maths (exact mode) -------------------------------------------------------
 * T: [R x C*D] row-major total-variability matrix; invvar: [C*D] UBM inverse variances.
 * substractM          AccumulateTVStat.cpp:1088-1105   F[u,c,:] -= mean[c,:] N[u,c]  (in place)
 * estimateTETt        :777-805    TETt packed lower triangle: [C x R(R+1)/2], row i>=j at i(i+1)/2+j
 * estimateW           :2114-2169  W[U x R] = (I + sum_c N[u,c] TETt_c)^-1 T Sigma^-1 F_u
 * estimateAandC       :1702-1795  + A[C x R(R+1)/2] (packed), Cmx[R x C*D], Rm[R x R], r[R], meanW[R]
 *                     (A, Cmx, Rm, r, meanW ACCUMULATE: zero them first; meanW is the SUM of w --
 *                      divide by the total utterance count after the all-reduce)
 * updateTestimate     :974-1005   T_c = A_c^-1 Cmx_c
 * minDivergence       :2056-2099  T <- chol_upper(Rm/n - r r^T / n^2) T ; mean += T^T meanW
 */
int gmmiv_tv_subtract_m(gmmiv_ctx *ctx, int64_t U, int C, int D, const double *N, double *F,
                        const double *ubm_means);
/* F_dst = F_src - N ubm_means, out of place (F_dst may be F_src): TotalVariability reloads N / F and calls substractM at the top of
 * every iteration (TotalVariability.cpp:123-124, substractM works in place); with the pristine statistics kept in HBM the restore
 * and the centring are ONE pass over F instead of a copy and a read-modify-write. */
int gmmiv_tv_subtract_m_to(gmmiv_ctx *ctx, int64_t U, int C, int D, const double *N, const double *F_src, double *F_dst,
                           const double *ubm_means);
size_t gmmiv_tv_packed_len(int R);
int gmmiv_tv_tett(gmmiv_ctx *ctx, int C, int D, int R, const double *Tm, const double *invvar,
                  double *tett_packed);
int gmmiv_tv_estimate_w(gmmiv_ctx *ctx, int64_t U, int C, int D, int R, const double *N,
                        const double *F, const double *Tm, const double *invvar,
                        const double *tett_packed, double *W);
int gmmiv_tv_estimate_a_and_c(gmmiv_ctx *ctx, int64_t U, int C, int D, int R, const double *N,
                              const double *F, const double *Tm, const double *invvar,
                              const double *tett_packed, double *W, double *A_packed, double *Cmx,
                              double *Rm, double *r, double *meanW);
int gmmiv_tv_update_t(gmmiv_ctx *ctx, int C, int D, int R, const double *A_packed, const double *Cmx,
                      double *Tm);
int gmmiv_tv_min_divergence(gmmiv_ctx *ctx, int C, int D, int R, double n_sessions, double *Rm,
                            double *r, const double *meanW, double *ubm_means, double *Tm);
/* orthonormalizeT (AccumulateTVStat.cpp:1548-1596): classical Gram-Schmidt over the rows of
 * T[R x SV], in place (coefficients taken against the ORIGINAL row, zero rows stay zero). */
int gmmiv_tv_orthonormalize_t(gmmiv_ctx *ctx, int R, int64_t SV, double *Tm);

/* ---- approximate extractors (IvExtractor modes ubmWeight / eigenDecomposition, IvExtractor.cpp:150-360) ----
 * normStatistics (AccumulateTVStat.cpp:1225-1242): F[u,c,d] = (F - mean[c,d] N[u,c]) sqrt(invvar[c,d]), in place.
 * substractMplusTW (:1379-1399, getMplusTW :964-971): F[u,c,d] -= (mean[c,d] + sum_i T[i,cD+d] W[u,i]) N[u,c].
 * normTMatrix (:1600-1609): T[j,k] *= sqrt(invvar[k]), in place.
 * getWeightedCov (:2837-2855): Wm[R x R] = sum_c weight[c] T_c T_c^T.
 * approximateTcTc (:3116-3136): Dm[c,i] += || (T_c^T Q)[:, i] ||^2, Dm [C x R], Q [R x R]; accumulates like the
 *   reference (zero Dm first for a fresh result).  Q comes from computeEigenProblem (:2997-3102, Eigen / LAPACK
 *   on the host in the reference; its column order is the solver's, so Q is an input here).
 * estimateWUbmWeight (:2348-2396): W[u] += (I + (sum_c N[u,c]) Wm)^-1 (T F[u]); T, F normalised as above.
 * estimateWEigenDecomposition (:2566-2609): W[u] += Q diag(1 / (1 + N[u] Dm)) Q^T (T F[u]).
 * W is accumulated into (the reference zeroes _W in ubmWeight mode only: pass zeros for a fresh result). */
int gmmiv_tv_norm_statistics(gmmiv_ctx *ctx, int64_t U, int C, int D, const double *N, double *F,
                             const double *ubm_means, const double *invvar);
int gmmiv_tv_subtract_m_plus_tw(gmmiv_ctx *ctx, int64_t U, int C, int D, int R, const double *N, double *F,
                                const double *ubm_means, const double *Tm, const double *W);
int gmmiv_tv_norm_t(gmmiv_ctx *ctx, int C, int D, int R, double *Tm, const double *invvar);
int gmmiv_tv_weighted_cov(gmmiv_ctx *ctx, int C, int D, int R, const double *Tm, const double *weight, double *Wm);
int gmmiv_tv_approximate_tctc(gmmiv_ctx *ctx, int C, int D, int R, const double *Tm, const double *Q, double *Dm);
int gmmiv_tv_estimate_w_ubm_weight(gmmiv_ctx *ctx, int64_t U, int C, int D, int R, const double *N, const double *F,
                                   const double *Tm, const double *Wm, double *W);
int gmmiv_tv_estimate_w_eigen(gmmiv_ctx *ctx, int64_t U, int C, int D, int R, const double *N, const double *F,
                              const double *Tm, const double *Dm, const double *Q, double *W);

/* ---- PldaTest::center / rotateLeft / lengthNorm (PldaTools.cpp:3706-3790); one iteration of
 * sphericalNuisanceNormalization (:3793-3839) = all three ------------------------------------------
 * Y[dim_out x n] = lengthNorm( M[dim_out x dim_in] * (X[dim_in x n] - mean[dim_in]) ), vectors as
 * columns.  mean == NULL: no centring; M == NULL: no rotation (dim_out == dim_in);
 * length_norm == 0: columns are not normalised.  Y may alias X when M == NULL. */
int gmmiv_iv_normalize(gmmiv_ctx *ctx, int dim_in, int dim_out, int64_t n, const double *X,
                       const double *mean, const double *M, int length_norm, double *Y);

/* ---- i-vector back-end estimation on a development set: PldaDev (LIA_SpkTools/src/PldaTools.cpp) ----------------
 * X [dim x n], one vector per column like PldaDev::_data; sessions are grouped by speaker and
 * sessions_per_speaker[nspk] (host array, PldaDev::_session_per_speaker) gives the group sizes (sum = n, all > 0).
 *   gmmiv_dev_means        computeAll                 :353-387   mean[dim], spk_means[dim x nspk]
 *   gmmiv_dev_cov_mat      computeCovMat              :527-566   Sigma, W, B [dim x dim], all divided by n
 *   gmmiv_dev_wccn_chol    computeWccnChol            :1124-1176 upperCholesky((mean_c cov_c / n_c)^-1)
 *   gmmiv_dev_mahalanobis  computeMahalanobis         :1366-1378 W^-1
 *   gmmiv_dev_scatter_mat  computeScatterMat          :1610-1644 as written in the reference (SB unweighted and
 *                          unnormalised; SW = matrix of the LAST speaker, built from the first n_c sessions of the set)
 *   gmmiv_sym_eigen        computeEigenProblem        :1490-1535 for a SYMMETRIC matrix: vect[n x rank] (columns =
 *                          eigenvectors), val[rank] descending (host Jacobi; the reference calls Eigen / LAPACK)
 *   gmmiv_dev_efr_matrix   sphericalNuisanceNormalization :1852-1902: (V diag(lambda^-1/2))^T of Sigma (EFR) or W (sphNorm)
 *   gmmiv_dev_lda          computeLDA                 :1381-1413 rank leading eigenvectors (unit norm) of W^-1 B as rows
 * Any null output pointer is skipped.  The O(dim^3) pieces (eigen problems, the WCCN Cholesky) run on the host like
 * the reference's; the O(dim^2 n) covariance GEMMs run on the device. */
int gmmiv_dev_means(gmmiv_ctx *ctx, int dim, int64_t n, const double *X, int64_t nspk, const int64_t *sessions_per_speaker,
                    double *mean, double *spk_means);
int gmmiv_dev_cov_mat(gmmiv_ctx *ctx, int dim, int64_t n, const double *X, int64_t nspk, const int64_t *sessions_per_speaker,
                      double *Sigma, double *W, double *B);
int gmmiv_dev_wccn_chol(gmmiv_ctx *ctx, int dim, int64_t n, const double *X, int64_t nspk, const int64_t *sessions_per_speaker,
                        double *WCCN);
int gmmiv_dev_mahalanobis(gmmiv_ctx *ctx, int dim, int64_t n, const double *X, int64_t nspk, const int64_t *sessions_per_speaker,
                          double *M);
int gmmiv_dev_scatter_mat(gmmiv_ctx *ctx, int dim, int64_t n, const double *X, int64_t nspk, const int64_t *sessions_per_speaker,
                          double *SB, double *SW);
int gmmiv_sym_eigen(gmmiv_ctx *ctx, int n, const double *A, int rank, double *vect, double *val);
int gmmiv_dev_efr_matrix(gmmiv_ctx *ctx, int dim, const double *Cov, double *M);
int gmmiv_dev_lda(gmmiv_ctx *ctx, int dim, const double *W, const double *B, int rank, double *ldaMat, double *eigval);

/* PldaModel::em_iteration (PldaTools.cpp:2329-2343 = center(Delta) + computeCovMatEigen :931-950 +
 * getExpectedValues :2359-2484 + mStep :2790-2815): one EM iteration of the PLDA model
 *   x = mu + F h_spk + G w_session + eps,  eps ~ N(0, Sigma)
 * on the development set X [dim x n] (sessions grouped by speaker; X is centred IN PLACE by the incoming Delta, like
 * _Dev.center(_Delta)).  F [dim x rf], G [dim x rg], Sigma [dim x dim], Delta [dim] are updated in place (M-step with
 * the minimum-divergence re-scaling of F and G).  rg may be 0 (pldaEigenChannelNumber 0, the simplified model: G is then
 * ignored and may be NULL).  The O(dim n r) products run on the device, the per-speaker r x r algebra on the host like the
 * reference's Eigen code. */
int gmmiv_plda_em_iteration(gmmiv_ctx *ctx, int dim, int64_t n, double *X, int64_t nspk, const int64_t *sessions_per_speaker,
                            int rf, int rg, double *F, double *G, double *Sigma, double *Delta);

/* PldaModel::preComputation + FTJ / FTJF of pldaNativeScoring (PldaTools.cpp:2950-2972, 4494-4496):
 *   FTJ[rf x dim] = F^T S^-1 - F^T S^-1 G (G^T S^-1 G + I)^-1 G^T S^-1,  FTJF[rf x rf] = FTJ F
 * F [dim x rf], G [dim x rg] (rg may be 0), Sigma [dim x dim] symmetric positive definite, all row-major.
 * rotateLeft(FTJ) is gmmiv_iv_normalize with FTJ as the matrix; FTJF feeds gmmiv_score_plda. */
int gmmiv_plda_precompute(gmmiv_ctx *ctx, int dim, int rf, int rg, const double *F, const double *G,
                          const double *Sigma, double *FTJ, double *FTJF);
/* The two-covariance model of PldaTest::twoCovScoring (PldaTools.cpp:4089-4125):
 *   G = W^-1 (B^-1 + 2 W^-1)^-1 W^-1,   H = W^-1 (B^-1 + W^-1)^-1 W^-1     (W, B symmetric positive definite) */
int gmmiv_twocov_model(gmmiv_ctx *ctx, int dim, const double *W, const double *B, double *G, double *H);
/* ---- PldaTest scoring (LIA_SpkTools/src/PldaTools.cpp) ------------------------------------------
 * models[dim x M], segs[dim x S]: one vector per COLUMN like PldaTest::_models/_segments;
 * scores[M x S].
 * cosineDistance :3842-3879, mahalanobisDistance :3882-3909 (-1/2 (m-s)^T Mah (m-s)),
 * twoCovScoring :4127-4171 ((m+s)^T G (m+s) - m^T H m - s^T H s),
 * pldaScoringUnThreaded :4186-4271 on vectors already projected by FTJ; models = per-speaker sums,
 * nsess[m] = enrolment sessions of model m (HOST array). */
int gmmiv_score_cosine(gmmiv_ctx *ctx, int dim, int64_t M, int64_t S, const double *models,
                       const double *segs, double *scores);
int gmmiv_score_mahalanobis(gmmiv_ctx *ctx, int dim, int64_t M, int64_t S, const double *models,
                            const double *segs, const double *Mah, double *scores);
int gmmiv_score_twocov(gmmiv_ctx *ctx, int dim, int64_t M, int64_t S, const double *models,
                       const double *segs, const double *G, const double *H, double *scores);
int gmmiv_score_plda(gmmiv_ctx *ctx, int rf, int64_t M, int64_t S, const double *models_sum,
                     const int64_t *nsess, const double *segs, const double *FTJF, double *scores);
/* PldaTest::twoCovScoringMixPart (:3923-3949, the L3 seam of twoCovScoring): scores[m][s] += (m + s)^T G (m + s) for every
 * pair -- ACCUMULATES like the reference's `_scores(m,s) +=` (zero the array for the bare term). */
int gmmiv_score_twocov_mix_part(gmmiv_ctx *ctx, int dim, int64_t M, int64_t S, const double *models, const double *segs,
                                const double *G, double *scores);
/* PldaTest::_trials (:3437, :3591-3620): cosineDistance / mahalanobisDistance score only the listed trials (:3871, :3889), the
 * other cells keep _scores' initial 0.  All rules above fill the whole M x S block with one GEMM; this call then writes `fill`
 * into every cell whose flag trials[m*S + s] is 0 (bytes, host or device). */
int gmmiv_score_apply_trials(gmmiv_ctx *ctx, int64_t M, int64_t S, const unsigned char *trials, double fill, double *scores);
/* The fp64 GEMM every TV / JFA / PLDA step and every scoring rule above is built on (k_dgemm, csrc/tv_kernels.hip), called as they
 * call it: on the context's stream, with the context's "gemm_*" options.  Row-major, strides in doubles:
 *     C[b] = epilogue(alpha * op(A[b]) * op(B[b])) + beta * C[b],   b = 0 .. batch-1
 *     op(A)[m][k] = ta ? A[k*lda + m] : A[m*lda + k]        op(B)[k][n] = tb ? B[n*ldb + k] : B[k*ldb + n]
 *   A, B, C, rv, cv   DEVICE pointers (GMMIV_ERR_ARG otherwise); nothing is staged or copied, so an unaligned base, an odd leading
 *                     dimension or an odd batch stride reaches the kernel as given (it then takes its per-element checked loads)
 *   lda, ldb, ldc     >= the extent they stride (ta ? M : K, tb ? K : N, N); sA, sB, sC >= 0 doubles between the matrices of a batch
 *                     (0: shared)
 *   nz                1: one pass over K;  > 1: split-K over at most nz layers of K (each a multiple of 16) whose partial products go
 *                     to the context's workspace (nz * M * N doubles) and are summed in layer order (deterministic);
 *                     0: the count the library picks for its own long-K products
 *   epi_mode          0: none;  1: v * rv[m] * cv[n];  2: v + br * rv[m] + bc * cv[n] + cst   (v = alpha * the product; rv[M], cv[N])
 * GMMIV_ERR_ARG: a negative size, a leading dimension smaller than its extent, batch > 1 with nz != 1 or epi_mode != 0, nz != 1
 * with epi_mode != 0, epi_mode outside 0..2 or without rv / cv.  M, N or batch == 0: nothing is done (GMMIV_OK).  K == 0: C = beta * C,
 * zeros when beta == 0.  beta == 0: C is written, never read.  Only enqueues: gmmiv_ctx_sync (or the stream) orders the result. */
int gmmiv_dgemm(gmmiv_ctx *ctx, int ta, int tb, int M, int N, int K, double alpha, const double *A, int64_t lda, int64_t sA,
                const double *B, int64_t ldb, int64_t sB, double beta, double *C, int64_t ldc, int64_t sC, int batch, int nz,
                int epi_mode, const double *rv, const double *cv, double br, double bc, double cst);
/* Multi-GPU scoring: the M x S matrix tiles by blocks of MODELS, no collective -- rank g calls any rule above
 * with the columns [m0, m1) of `models` (and the matching nsess / rows of scores); gmmiv_shard_range gives the contiguous range
 * of rank `rank` out of `world` over n items (sizes differ by at most one), the same split as the reference's thread ranges
 * (PldaTools.cpp:4175-4183 dispatch, AccumulateTVStat.cpp:498-507). */
void gmmiv_shard_range(int64_t n, int rank, int world, int64_t *begin, int64_t *end);

/* ---- score normalisation: LIA_SpkDet/ComputeNorm (z / t / zt / tz-norm) on resident score matrices ---------------------
 * gmmiv_score_cohort_stats: DistribNorm::computeMeanStd (ComputeNorm.cpp:121-159) over every distribution of a cohort score
 * matrix scores[rows x cols] (row stride ld >= cols).
 *   axis 0: one distribution per ROW (its cols scores; z-norm: a model against the impostor segments) -> mean[rows], std[rows];
 *   axis 1: one distribution per COLUMN (its rows scores; t-norm: the cohort models against a segment) -> mean[cols], std[cols].
 *   select:   NULL, or bytes along the cohort axis (cols of them for axis 0, rows for axis 1): a score enters its distribution
 *             only where the byte is non-zero (selectImp, :436-445); n = the number of non-zero bytes.
 *   pre_mean, pre_std: NULL, or vectors along the cohort axis: the statistics are those of (x - pre_mean[j]) / pre_std[j],
 *             computed on the fly with exactly these two operations (getAllScoresFirstNormed, :466-489) -- the zt / tz chains
 *             never materialise a normalised copy of their cohort matrix.
 *   mean_mode 0: mean = sum / size, std = sqrt(sum2 / size - mean * mean) (biased, not clamped: a negative radicand gives NaN, a
 *             constant cohort gives 0 and the later division Inf / NaN, as in the reference);
 *   mean_mode 1: mean = the score at position size / 2 of the kept range, std = the mean absolute deviation from it.
 *   percent_h, percent_l in [0, 1): discardH = (unsigned long)((double)n * percent_h) highest and discardL lowest scores are left
 *             out (fp64 product, truncated); size = n - discardH - discardL.  The result is what the reference gets from a
 *             descending sort, ties included; no sort runs (an exact radix select per distribution, score_norm.hip).
 *   Quirk kept from the reference: with mean_mode 1 and BOTH percentages zero it does not sort, and its "median" is the score
 *   at position n / 2 in INPUT order.
 *   An empty kept range (n == 0 or discardH + discardL >= n) is GMMIV_ERR_ARG, checked before anything is enqueued.  The one
 *   exception: a `select` that is a DEVICE pointer is counted on the device (same fp64 product and truncation), nothing is read
 *   back, and an empty kept range then yields NaN in mean and std.
 *   Summation order differs from the reference's sequential loop (fixed, so results are bitwise reproducible): sums agree
 *   within (n - 1) 2^-53 sum|x|, and exactly whenever every partial sum is exact.  NaN scores are outside the contract.
 *   Device scratch: at most GMMIV_SCORE_NORM_SCRATCH_BYTES(ndist) = 512 * ndist + 64 bytes (+ the workspace's growth slack of 1/8),
 *   whatever the matrix: 64 bytes for the counts of a device mask, 512 per distribution for the row-slab sums of the untrimmed
 *   column pass (axis 1, mean_mode 0, no discard); the select histograms live in LDS.  Host arrays are staged like everywhere else.
 * gmmiv_score_normalize: scores[M x S] in place, every step the two IEEE operations (x - mean) / std (a true division):
 *   GMMIV_NORM_Z   (x - row_mean[m]) / row_std[m]                     GMMIV_NORM_T   (x - col_mean[s]) / col_std[s]
 *   GMMIV_NORM_ZT  t first, then z (:596-666)                          GMMIV_NORM_TZ  z first, then t (:668-751)
 *   first_out: NULL, or [M x S] that receives the score after the FIRST of the two normalisations (the reference writes both).
 * Kernel timers (gmmiv_ctx_kernel_ms, option "timing"): "k_norm_stats" and "k_norm_apply".
 * With device pointers throughout both calls only enqueue.  rows == 0 / cols == 0 / M == 0 / S == 0: nothing to do, GMMIV_OK. */
#define GMMIV_SCORE_NORM_SCRATCH_BYTES(ndist) ((size_t)512 * (size_t)(ndist) + (size_t)64)
enum { GMMIV_NORM_Z = 0, GMMIV_NORM_T = 1, GMMIV_NORM_ZT = 2, GMMIV_NORM_TZ = 3 };
int gmmiv_score_cohort_stats(gmmiv_ctx *ctx, int64_t rows, int64_t cols, const double *scores, int64_t ld, int axis,
                             const unsigned char *select, const double *pre_mean, const double *pre_std, int mean_mode,
                             double percent_h, double percent_l, double *mean, double *std);
int gmmiv_score_normalize(gmmiv_ctx *ctx, int64_t M, int64_t S, double *scores, int order, const double *row_mean,
                          const double *row_std, const double *col_mean, const double *col_std, double *first_out);
/* Bytes the context holds in the scratch slot of the score-normalisation calls (slot < 0), or in workspace slot `slot`
 * (0 when out of range): lets a caller check that a repeated call allocates nothing. */
size_t gmmiv_ctx_workspace_bytes(gmmiv_ctx *ctx, int slot);

/* ---- score normalisation on lists: sparse trials and per-entity cohorts of different lengths ------------------------------
 * The reference keeps one growing list of scores per name (DistribNorm, ComputeNorm.cpp:104-118), filled line by line
 * (getAllScores / getAllScoresFirstNormed, :446-489), and walks the test list with two name lookups per line (:542-554, :576-589,
 * :634-658, :717-742): nothing there asks for a full cross product.  These two calls are that, on a CSR list over a score array.
 * gmmiv_score_list_stats: DistribNorm::computeMeanStd (:121-159) for ndist distributions.  Distribution d owns the slots k in
 *   [off[d], off[d + 1]); slot k holds v = scores[pos ? pos[k] : k], and with pre_id the value
 *   (v - pre_mean[pre_id[k]]) / pre_std[pre_id[k]] -- exactly these two operations, computed on the fly (:480): the zt / tz chains
 *   never materialise a normalised copy.  One scores array (the llr of a gmmiv_llr_trials call, say) serves two calls through two
 *   pos tables, one grouped by model (z), one by segment (t).
 *   off:      a HOST table of ndist + 1 offsets, non-decreasing, off[0] >= 0; copied before return.  Slots before off[0] are never
 *             read (pos and pre_id are indexed by slot all the same).  Every other array is a host or a device array.
 *   mean_mode, percent_h, percent_l: as for gmmiv_score_cohort_stats, with n = off[d + 1] - off[d], discardH = (unsigned long)
 *             ((double)n * percent_h), discardL likewise and size = n - discardH - discardL taken PER DISTRIBUTION.  The quirk is
 *             kept: mean_mode 1 with both percentages zero does not sort, its "median" is the score at slot off[d] + n / 2.
 *   RESULT:   the (mean, std) of a distribution are THE BITS gmmiv_score_cohort_stats returns with axis = 0, select = NULL for a
 *             one-row matrix holding the same values in the same order (pre_mean / pre_std gathered into vectors of that length).
 *             Thread count, wave or workgroup path, staging, and with them the fp64 summation order, are functions of the
 *             distribution's own length; they do not depend on its neighbours, on ndist or on how the call groups distributions
 *             into launches.  Ties, the sum bound (n - 1) 2^-53 sum|x| and NaN (outside the contract) are therefore the dense call's.
 *   GMMIV_ERR_ARG, before anything is enqueued and naming the first offending distribution: a decreasing off; a distribution
 *             with n == 0 or an empty kept range (the reference: "Problem: empty impostor cohort"); pre_id without both pre_*
 *             vectors or the reverse; a percentage outside [0, 1); an unknown mean_mode; a HOST pos / pre_id entry outside
 *             [0, nscores) / [0, npre) (device tables are not checked); without pos, a list that ends beyond nscores.  The
 *             arguments are checked before the context is looked at.  ndist == 0 is valid.
 *   Planning: the distributions are binned on the host by length class -- the lengths that share a launch shape of the dense call
 *             -- and every class that occurs is one launch.  gmmiv_score_list_class gives the class of a length (streaming = the
 *             untrimmed mean_mode 0: 2 classes, else GMMIV_SCORE_LIST_CLASSES), its threads per workgroup and the scores its
 *             workgroups stage in LDS (0: none); gmmiv_plan_score_lists (pure host function, needs no GPU) gives cls[d], the
 *             distributions ordered by class (table order inside a class) and class_begin[GMMIV_SCORE_LIST_CLASSES + 1] into that
 *             order; each output may be NULL.  It returns the number of classes that occur, or -1 for a bad table.
 *   Device scratch: GMMIV_SCORE_LIST_SCRATCH_BYTES(ndist) = 12 ndist + 8 bytes (+ the workspace's growth slack of 1/8) in the slot
 *             gmmiv_ctx_workspace_bytes(ctx, -1) reports: off as 8-byte and the class order as 4-byte entries.  Histograms and
 *             staged keys live in LDS.  A repeated call allocates nothing.  Host arrays are staged like everywhere else.
 *   Synchronisation: the call is NOT enqueue-only: it waits for the context's stream once, after uploading its two tables (they
 *             live in host memory of the call).  With device arrays everything after that is only enqueued.
 * gmmiv_score_normalize_list: scores[i] <- (scores[i] - row_mean[row_id[i]]) / row_std[row_id[i]] and / or the same with the column
 *   vectors, i < n, in place, every step one subtraction and one true division; order GMMIV_NORM_Z / T / ZT (t first) / TZ (z first)
 *   as for gmmiv_score_normalize.  first_out: NULL, or [n] for the value after the first of two steps.  The ids and vectors an order
 *   needs must be present; a HOST id outside [0, nrow) / [0, ncol) is GMMIV_ERR_ARG.  n == 0 is valid.  Only enqueues with device
 *   arrays.
 * Kernel timers: "k_norm_stats" (summed over the launches of a call) and "k_norm_apply". */
#define GMMIV_SCORE_LIST_SCRATCH_BYTES(ndist) ((size_t)12 * (size_t)(ndist) + (size_t)8)
#define GMMIV_SCORE_LIST_CLASSES 7
int gmmiv_score_list_class(int64_t n, int streaming, int *threads /* nullable */, int64_t *stage_scores /* nullable */);
int64_t gmmiv_plan_score_lists(int64_t ndist, const int64_t *off /* ndist + 1 */, int streaming, int32_t *cls /* [ndist] */,
                               int32_t *order /* [ndist] */, int64_t *class_begin /* [GMMIV_SCORE_LIST_CLASSES + 1] */);
int gmmiv_score_list_stats(gmmiv_ctx *ctx, int64_t ndist, const int64_t *off /* HOST, ndist + 1 */,
                           const int64_t *pos /* nullable */, const double *scores, int64_t nscores,
                           const int32_t *pre_id /* nullable */, const double *pre_mean, const double *pre_std, int64_t npre,
                           int mean_mode, double percent_h, double percent_l, double *mean /* [ndist] */, double *std /* [ndist] */);
int gmmiv_score_normalize_list(gmmiv_ctx *ctx, int64_t n, double *scores, int order,
                               const int32_t *row_id, const double *row_mean, const double *row_std, int64_t nrow,
                               const int32_t *col_id, const double *col_mean, const double *col_std, int64_t ncol,
                               double *first_out /* nullable */);

/* ---- JFA (LIA_SpkTools/src/AccumulateJFAStat.cpp): model M_{s,h} = m + V y_s + U x_h + D z_s ---------------------------
 * The factor steps are the total-variability entry points under the JFA names:
 *   JFAAcc::estimateVEVT / estimateUEUT (:1266-1352, :1425-1508)                         -> gmmiv_tv_tett
 *   JFAAcc::estimateAndInverseL_EV + estimateYandV (:1970-1996, :2467-2511), _EC + estimateXandU (:2137-2163, :3040-3083)
 *                                                                                          -> gmmiv_tv_estimate_a_and_c
 *   JFAAcc::estimateY / estimateX (:2867-2957, :3262-3351)                                -> gmmiv_tv_estimate_w
 *   JFAAcc::updateVestimate / updateUestimate (:3597-3644)                                -> gmmiv_tv_update_t
 * What is specific to JFA is below.  All arrays host or device. */
/* F[r,c,:] -= N[r,c] (means[c,:] + (W[o] T)[c,:] + Dm[c,:] Z[o][c,:]),  o = owner ? owner[r] : r.  Every term is optional
 * (means, T/W, Dm/Z may be NULL).  N [rows x C], F [rows x C*D], T [R x C*D], W [nfact x R], Dm [C*D], Z [nfact x C*D].
 * Replaces JFAAcc::substractMplusDZ (:3805-3822), substractMplusVY (:3988-4005), substractMplusVYplusDZ (:4400-4422, owner =
 * the speaker of each session), the mean part of substractMplusUX (:4336-4364; its channel part is gmmiv_jfa_subtract_sessions),
 * getMplusVYplusDZ / getUX (:1803-1957). */
int gmmiv_jfa_subtract(gmmiv_ctx *ctx, int64_t rows, int C, int D, const double *N, double *F, const int64_t *owner, int64_t nfact,
                       const double *means, int R, const double *T, const double *W, const double *Dm, const double *Z);
/* F_X[s,c,:] -= sum over the sessions h in [sess_begin[s], sess_begin[s+1]) of N_h[h,c] (x_h U)[c,:]   (sessions grouped by
 * speaker, sess_begin a HOST array of nspk + 1 offsets).  Replaces JFAAcc::substractUX (:4152-4172). */
int gmmiv_jfa_subtract_sessions(gmmiv_ctx *ctx, int64_t nspk, const int64_t *sess_begin, int C, int D, const double *N_h, double *F_X,
                                int R, const double *U, const double *X);
/* tau < 0: Z = F iv D / (1 + N iv D^2) (JFAAcc::estimateZ, :3550-3573); tau >= 0: Z = tau / (tau + N) D iv F (estimateZMAP, :3576-3594). */
int gmmiv_jfa_estimate_z(gmmiv_ctx *ctx, int64_t nspk, int C, int D, const double *N, const double *F, const double *invvar, const double *Dm,
                         double tau, double *Z);
/* JFAAcc::estimateZandD (:3480-3516): Z as above (tau < 0) and D <- sum_s z F / sum_s (1 / L + z^2) N, in place. */
int gmmiv_jfa_estimate_z_and_d(gmmiv_ctx *ctx, int64_t nspk, int C, int D, const double *N, const double *F, const double *invvar, double *Dm,
                               double *Z);

/* ---- collectives of the paths that shard: RCCL over xGMI ---------------------------------------------
 * The reference merges the private accumulators of its worker threads under a mutex: MixtureStat::addAccEM
 * (LIA_SpkTools/src/AccumulateStat.cpp:286-292) for the EM statistics, `+=` of A / Cmx / R / r in the threaded
 * estimateAandC (AccumulateTVStat.cpp:1920-1937, 2036-2044).  With one rank per GPU the merge is a collective on the
 * accumulators where they lie (device memory):
 *   EM statistics (TrainWorld)        gmmiv_allreduce_f64 of the flat accumulator, gmmiv_em_acc_len() doubles (1.98 MB)
 *   T-matrix EM (TotalVariability)    gmmiv_reduce_scatter_f64 of A_packed and Cmx by blocks of Gaussians -> each rank
 *                                     solves T_c = A_c^-1 Cmx_c for its own Gaussians (updateTestimate is independent per
 *                                     Gaussian, :981-1000) -> gmmiv_allgather_f64 of the T blocks; R, r, meanW: allreduce
 * One communicator per context.  Rank 0 obtains an id (gmmiv_comm_get_unique_id) and ships its 128 bytes to the other ranks
 * over any host channel (gmmiv_comm_exchange_id_file: a file in a directory all ranks see; MPI / a TCP store work as well),
 * then EVERY rank calls gmmiv_comm_create (collective).  world == 1 needs no id and no RCCL.  The calls are enqueued on the
 * context's stream; device buffers are used in place, host buffers (allreduce / broadcast only) are staged and the call
 * returns after the result is back.  RCCL is loaded at run time (dlopen of the copy already mapped in the process, else
 * librccl.so.1; the environment variable GMMIV_RCCL_LIB, when set, names the ONLY library tried): GMMIV_ERR_UNSUPPORTED when
 * it cannot be found.
 *
 * Transports.  The id rank 0 draws selects the transport of the communicator every rank then creates from it:
 *   "rccl"  (default) RCCL over xGMI / PCIe, one rank per GPU -- the production path;
 *   "shm"   ranks of ONE host that may SHARE a GPU (RCCL refuses two ranks on one device), or a host without RCCL: buffers
 *           are staged through one mmap'ed file (GMMIV_COMM_SHM_DIR, default /dev/shm; GMMIV_COMM_SHM_SLOT_MB per rank,
 *           default 16) and every rank sums the pieces on its own device in rank order -- bitwise the same result on every
 *           rank.  It is how the multi-rank orchestration (reduce-scatter by Gaussian blocks, sharded updateTestimate,
 *           all-gather) is exercised end to end on a one-GPU machine; calls block until the exchange is complete.
 * gmmiv_comm_get_unique_id_for(transport, id): transport "rccl", "shm", or NULL = the environment variable
 * GMMIV_COMM_TRANSPORT, else "rccl"; gmmiv_comm_get_unique_id(id) = gmmiv_comm_get_unique_id_for(NULL, id).
 * A rank that waits longer than GMMIV_COMM_TIMEOUT_S (default 300) for its peers in the shm transport fails with GMMIV_ERR_HIP. */
typedef struct gmmiv_comm gmmiv_comm;
#define GMMIV_COMM_ID_BYTES 128
int gmmiv_comm_get_unique_id(void *id128);
int gmmiv_comm_get_unique_id_for(const char *transport, void *id128);
/* rank 0: creates the id and publishes it at `path` (atomically; a file already there is removed first); other ranks: wait up
 * to timeout_s for it and read it (a file last modified more than 10 minutes before the call is taken for a dead job's leftover
 * and ignored).  Rank 0 removes the file again as soon as its gmmiv_comm_create on that id has succeeded -- every rank has read
 * the id by then -- so a path can be reused by the next job. */
int gmmiv_comm_exchange_id_file(const char *path, int rank, void *id128, double timeout_s);
int gmmiv_comm_create(gmmiv_ctx *ctx, int world, int rank, const void *id128, gmmiv_comm **out);
void gmmiv_comm_destroy(gmmiv_comm *comm);
int gmmiv_comm_world(const gmmiv_comm *comm);
int gmmiv_comm_rank(const gmmiv_comm *comm);
const char *gmmiv_comm_backend(const gmmiv_comm *comm); /* "rccl: <path of the library in use>", "shm (...)", or "single rank ..." */
/* What the collective library itself says about this communicator: *rccl_version = ncclGetVersion's code (e.g. 22105), *rccl_comm_count
 * = ncclCommCount(comm), the number of ranks RCCL sees.  Both 0 for a single-rank or "shm" communicator (no RCCL behind it). */
int gmmiv_comm_info(const gmmiv_comm *comm, int *rccl_version, int *rccl_comm_count);
/* payload bytes this rank passed to collectives since the last call of this function (then reset to 0) */
double gmmiv_comm_take_bytes(gmmiv_comm *comm);
/* buf[n] <- sum over ranks (in place; host or device) */
int gmmiv_allreduce_f64(gmmiv_comm *comm, double *buf, size_t n);
/* recv[recvcount] <- block `rank` of the sum over ranks of send[world * recvcount] (device; in place when
 * recv == send + rank * recvcount) */
int gmmiv_reduce_scatter_f64(gmmiv_comm *comm, const double *send, double *recv, size_t recvcount);
/* recv[world * sendcount] <- the ranks' send[sendcount], in rank order (device; in place when send == recv + rank * sendcount) */
int gmmiv_allgather_f64(gmmiv_comm *comm, const double *send, double *recv, size_t sendcount);
/* buf[n] on every rank <- buf of rank `root` (host or device) */
int gmmiv_broadcast_f64(gmmiv_comm *comm, double *buf, size_t n, int root);
/* Overlapped forms (device buffers): *_begin orders the collective behind everything enqueued on the context's stream SO FAR and
 * runs it on the communicator's own side stream -- work enqueued on the context's stream afterwards overlaps with it;
 * gmmiv_comm_join makes the context's stream wait for every collective begun since the last join (their results may be used
 * from then on; the buffers must not be touched in between).  Same arithmetic as the plain calls: results are bitwise equal.
 * All ranks must issue begins, joins and plain collectives of one communicator in the same order.  With one rank, and on the
 * "shm" transport (whose calls block), *_begin behaves like the plain call and the join is a no-op. */
int gmmiv_allreduce_f64_begin(gmmiv_comm *comm, double *buf, size_t n);
int gmmiv_reduce_scatter_f64_begin(gmmiv_comm *comm, const double *send, double *recv, size_t recvcount);
int gmmiv_allgather_f64_begin(gmmiv_comm *comm, const double *send, double *recv, size_t sendcount);
int gmmiv_comm_join(gmmiv_comm *comm);

#ifdef __cplusplus
}
#endif
#endif /* GMMIV_H */
