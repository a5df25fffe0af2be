// gmm_kernels.h -- host-callable launchers of gmm_kernels.hip (internal; the public surface is
// include/gmmiv.h).  All pointers are device pointers; every function returns a hipError_t value.
#pragma once
#include <hip/hip_runtime.h>

#include "kopts.h"
#include "../../include/gmmiv.h" // gmmiv_model_tile

#define GMMK_KS_GENERIC 99 // "no MFMA instantiation for this vectSize": every KS > 15 / KS <= 15 test of the callers routes it to the fallback side
#define GMMK_MAX_DIM 4096  // the generic kernels keep 4 frames x D doubles in LDS
int gmmk_ks_for_dim(int D);   // k-steps (of 4 dims) of the compiled instantiation serving D, 0 = unsupported
int gmmk_rl_for_ks(int KS);   // row length (doubles) of the LDS frame tile / half-width of an EM partial row
int gmmk_pack_model(hipStream_t st, int C, int D, int KS, int nct, int Cp64, const double *w, const double *mean,
                    const double *iv, double *a, double *lwc, double *Pt, double *meanT, double *ivT);
int gmmk_llk(hipStream_t st, int KS, int x_f64, const void *x, long T, long ldx, int D, const double *Pt, int nct,
             double *lse, int use_glds, int wg_waves);
int gmmk_llk_finalize(hipStream_t st, const double *lse, long T, double lo, double hi, double *llk_out,
                      double *partial /* >= 3*256 doubles */, double scale_c, double scale_r, double *dst_clamped,
                      double *dst_raw, double scale_n = 0.0, double *dst_count = nullptr);
int gmmk_add_scalar(hipStream_t st, double *dst, double v);
int gmmk_count_dead(hipStream_t st, const double *lse, long T, unsigned long long *cnt); // *cnt += frames whose lse is not finite (zero-likelihood frames)
int gmmk_rows_sum_groups(hipStream_t st, long n, int ngroups, const int *rb, const double *src, double *dst); // dst[g] = sum of src rows [rb[g], rb[g+1])
int gmmk_stats(hipStream_t st, int KS, int sq, int x_f64, const void *x, long ldx, int D, int C, const double *Pt,
               int nct, const double *lse, double lse_shift, const long *seg_begin, int nseg, double *out0,
               double *out1, int mode, int wg_waves, double prune_arg);
int gmmk_em_reduce(hipStream_t st, const double *part, int nseg, int C, int Cp, int D, int KS, double *acc);
int gmmk_em_get(hipStream_t st, int C, int D, const double *acc, const double *prev_mean, const double *prev_cov,
                double *w, double *mean, double *cov);
int gmmk_topc_frames_per_block(int Cp64, int D);
int gmmk_topc_determine(hipStream_t st, int x_f64, const void *x, long T, long ldx, int D, int C, int Cp,
                        const double *meanT, const double *ivT, const double *lwc, const double *w, int ctop,
                        int complete, double lo, double hi, int *idx, double *lk, double *nlk, double *nllk,
                        double *nw, double *llk);
// generic statistics (capi_gmm.hip, models without an MFMA instantiation): Xa rows for the GEMM, scatter of S = gamma^T Xa
int gmmk_build_xa(hipStream_t st, int x_f64, const void *x, long ldx, int D, long n, int sq, int NC, double *Xa);
int gmmk_scatter_em(hipStream_t st, int C, int D, int NC, const double *S, double scale, double *acc);
int gmmk_scatter_nf(hipStream_t st, int C, int D, int NC, const double *S, double *Nrow, double *Frow);
size_t gmmk_topc_big_scratch_doubles(long T, int Cp);
int gmmk_topc_determine_big(hipStream_t st, int x_f64, const void *x, long T, long ldx, int D, int C, int Cp,
                            const double *meanT, const double *ivT, const double *lwc, const double *w, int ctop,
                            int complete, double lo, double hi, int *idx, double *lk, double *nlk, double *nllk,
                            double *nw, double *llk, double *zs); // any C / D / ctop: logit rows in global scratch (gmmk_topc_big_scratch_doubles)
int gmmk_topc_use_big(hipStream_t st, int x_f64, const void *x, long T, long ldx, int D, const double *mean,
                      const double *iv, const double *lwc, int C, int ctop, const int *idx, const double *nllk, int complete,
                      double lo, double hi, double *llk); // ctop > 64
int gmmk_topc_use(hipStream_t st, int x_f64, const void *x, long T, long ldx, int D, const double *mean,
                  const double *iv, const double *lwc, int C, int ctop, const int *idx, const double *nllk, int complete,
                  double lo, double hi, double *llk);
int gmmk_frame_moments(hipStream_t st, int x_f64, const void *x, long T, long ldx, int D, double *partial,
                       int max_blocks, double *acc);
int gmmk_variance_control(hipStream_t st, int C, int D, double *cov, double flooring, double ceiling,
                          const double *cov_signal, unsigned long long *counts);
int gmmk_reciprocal(hipStream_t st, long n, const double *in, double *out);
int gmmk_gather_frames(hipStream_t st, int x_f64, const void *x, long ldx, int D, const long *idx, long n, void *out);
int gmmk_segment_means(hipStream_t st, const double *v, long ld, const long *item, long nitem, double *part, const long *pair_off,
                       const long *pair_len, long npair, double *out);
int gmmk_topgauss_select(hipStream_t st, long T, int cap, double mass, int fixed_count, const double *w, int *idx, const double *lk,
                         const double *llk, int *count, double *snsw, double *snsl, unsigned long long *capped);
int gmmk_flag_frames(hipStream_t st, int x_f64, const void *x, long T, long ldx, int D, unsigned char *flag, int *any);
int gmmk_fill_chunks(hipStream_t st, long *dst, int nseg, long per, long n);
int gmmk_count_flags(hipStream_t st, const unsigned char *flag, long T, unsigned long long *cnt);
int gmmk_gather_runs(hipStream_t st, int x_f64, const void *x, long ldx, int D, const long *runs, long nrun, void *out);

// stats_z.hip / k_llk_mfma<WZ>: scaled likelihoods written once by the log-likelihood kernel, statistics from them.
// The scratch the kernel leaves them in (reserved by gmmiv_z_reserve, capi_gmm_util.h): zbuf = nct * nfb blocks of 2 KB (16 frames x 16
// Gaussians), eit = the running exponents, (nct / 2) * nfb * 16 ints, inv / efin = 1 / S_t and Efin of every frame.
// One other user: gmmk_llk_topc hands k_llk_mfma<TC> its own arrays in the same five kernel arguments (zbuf = candidate records, nfb
// unused, eit = candidate counts, inv = the slow-path sums, efin = Efin); a change of this struct has to keep that call in step.
struct gmmk_zview {
    double *zbuf;
    long nfb;
    int *eit;
    double *inv;
    int *efin;
};
int gmmk_llk_z(hipStream_t st, int KS, int x_f64, const void *x, long T, long ldx, int D, const double *Pt, int nct,
               double *lse, int use_glds, const gmmk_zview &z);
// k_llk_mfma<.., MM>: a model per segment (gmmiv_*_models).  tiles: DEVICE array of ntiles entries (gmmiv_plan_model_tiles; frame numbers
// relative to x / lse / inv / efin / zbuf block 0), Pt: the packed models of the call's chunk, pt_stride doubles apart.  zbuf / eit hold
// nfb >= ceil(last written frame / 16) blocks per Gaussian tile; only rows inside the tiles' windows are written.  -1: no instantiation
int gmmk_llk_models(hipStream_t st, int KS, int x_f64, const void *x, long ldx, int D, const double *Pt, long pt_stride, int nct,
                    const gmmiv_model_tile *tiles, long ntiles, double *lse, int use_glds);
int gmmk_llk_z_models(hipStream_t st, int KS, int x_f64, const void *x, long ldx, int D, const double *Pt, long pt_stride, int nct,
                      const gmmiv_model_tile *tiles, long ntiles, double *lse, int use_glds, const gmmk_zview &z);
// constants of G models in one launch (tables at p + g * stride, stride 0 = shared; a / lwc [G x Cp]); packed operands of the n models
// ids[0..n) (device array) into Pt + slot * nct (2 KS + 2) 64 in one launch -- the arithmetic of gmmk_pack_model, the same bits
int gmmk_const_models(hipStream_t st, int G, int C, int Cp, int D, const double *w, long sw, const double *mean, long sm, const double *iv,
                      long si, double *a, double *lwc);
int gmmk_pack_models(hipStream_t st, int n, const int *ids, int C, int Cp, int D, int KS, int nct, const double *mean, long sm,
                     const double *iv, long si, const double *a, double *Pt);
int gmmk_llk_seg_finalize(hipStream_t st, const double *lse, const long *sb, long nseg, double lo, double hi, double *llk_out, double *seg_sum,
                          double *seg_llk); // per segment [sb[s], sb[s+1]): clamped values, their sum, {sum, count} of the finite raw values
int gmmk_map_adapt_models(hipStream_t st, int G, int C, int D, const double *N, const double *F, const double *count, long count_stride,
                          const double *w0, const double *mean0, const double *cur, long cur_stride, int method, int mean_adapt,
                          int weight_adapt, double mean_reg, double weight_reg, double mean_alpha, double *mean_out, double *w_out);
// computeMAP with the variance branch (gmmiv_map_adapt_models_full): S / cur_cov / cov0 / any of the outputs nullable as the header says;
// status [G] (int32) = entries of cov_out that are not positive and finite, written on the device
int gmmk_map_adapt_models_full(hipStream_t st, int G, int C, int D, const double *N, const double *F, const double *S, const double *count,
                               long count_stride, const double *w0, const double *mean0, const double *cov0, const double *cur_mean,
                               long cur_mean_stride, const double *cur_cov, long cur_cov_stride, int method, int mean_adapt, int var_adapt,
                               int weight_adapt, double mean_reg, double var_reg, double weight_reg, double mean_alpha, double *mean_out,
                               double *cov_out, double *w_out, int *status);
// normalizeMixture towards N(0, 1) for G models in place: one thread per (model, dimension), the fold of mixtureFusion over c = 0 .. C-1
int gmmk_normalize_models(hipStream_t st, int G, int C, int D, const double *w, long w_stride, double *mean, double *cov, int nb_it,
                          int mean_only);
// three pieces of a flat EM accumulator [occ | sum g x | sum g x^2 | ..] into statistics rows (the segment walk of gmmiv_em_stats_models)
int gmmk_acc_to_rows(hipStream_t st, int C, int D, const double *acc, double *Nrow, double *Frow, double *Srow);
// k_llk_mfma<TC>: candidates of the top-C' selection collected in the log-likelihood kernel (see gmm_kernels.hip), ranked by
// gmmk_topc_rank (topc_z.hip)
int gmmk_topc_cap(void);
int gmmk_llk_topc(hipStream_t st, int KS, int x_f64, const void *x, long T, long ldx, int D, const double *Pt, int nct, int use_glds,
                  int ctop, double *cand, int *cnt, double *theta, double *slow, int *efin);
int gmmk_topc_rank(hipStream_t st, int x_f64, const void *x, long n, long ldx, int D, int C, const double *cand, const int *cnt,
                   const double *theta, const double *slow, const int *efin, const double *mean, const double *iv, const double *lwc,
                   const double *w, int ctop, int complete, double lo, double hi, int *idx, double *lk, double *nlk, double *nllk,
                   double *nw, double *llk, int *flag, long *redo, int stats, long *wide);
int gmmk_topc_scatter(hipStream_t st, long n, int ctop, const long *redo, const int *sidx, const double *slk, const double *snlk,
                      const double *snllk, const double *snw, const double *sllk, int *idx, double *lk, double *nlk, double *nllk, double *nw,
                      double *llk);
int gmmk_posteriors(hipStream_t st, int x_f64, const void *x, long T, long ldx, int D, int C, int Cp, const double *meanT,
                    const double *ivT, const double *lwc, const double *lse, double *gamma);
int gmmk_stats_z_groups(int nct);
int gmmk_stats_z_wg_per_cu(void);
int gmmk_stats_z(hipStream_t st, int KS, int sq, int x_f64, const void *x, long ldx, int D, int C, int nct, const gmmk_zview &z,
                 double scale, const long *seg_begin, int nseg, double *out0, double *out1, int mode, int accum, double prune_thr);
// the EM shape with a row epilogue: N [nseg x C], F, X2 [nseg x C*D] = sum_t gamma [1 | x | x^2] of every segment, written directly
int gmmk_stats_z_rows(hipStream_t st, int KS, int x_f64, const void *x, long ldx, int D, int C, int nct, const gmmk_zview &z,
                      const long *seg_begin, int nseg, double *N, double *F, double *X2, double prune_thr);
size_t gmmk_topc_z_lds(int nct, int D);
int gmmk_topc_from_z(hipStream_t st, int x_f64, const void *x, long n, long ldx, int D, int C, int nct, const gmmk_zview &z,
                     const double *mean, const double *iv, const double *lwc, const double *w, int ctop, int complete, double lo, double hi,
                     int *idx, double *lk, double *nlk, double *nllk, double *nw, double *llk, int *flag);
int gmmk_topc_use16(hipStream_t st, int x_f64, const void *x, long T, long ldx, int D, const double *mean, const double *iv,
                    const double *lwc, int C, int ctop, const int *idx, const double *nllk, int complete, double lo, double hi, double *llk, int four);
int gmmk_topc_use4_multi(hipStream_t st, int x_f64, const void *x, long T, long ldx, int D, const void *clients, int n_clients, int ctop,
                         const int *idx, const double *nllk, int complete, double lo, double hi, double *llk); // clients: device array of {mean, iv, lwc, (long) C}
int gmmk_post_from_z(hipStream_t st, long n, int C, int nct, const gmmk_zview &z, double *gamma);

// feat_comp.hip: frames rewritten from the posteriors (gmmiv_feat_compensate / gmmiv_feat_map / gmmiv_scatter_runs)
size_t gmmk_feat_offset_doubles(int nct, int D);
int gmmk_feat_pack_offset(hipStream_t st, const double *off, int C, int D, int nct, double *offP); // MFMA B-operand order, zero padded
int gmmk_feat_comp(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, long n, int D, int nct, const gmmk_zview &z,
                   const double *offP, void *out, long ldo); // -1: D > 64
// a model per segment (gmmiv_feat_compensate_models): the offsets of the models ids[0 .. n) of a chunk packed by one launch, and
// k_feat_comp over a tile table (gmmiv_plan_feat_tiles with gmmk_feat_blocks_per_tile blocks per entry, frames relative to x)
int gmmk_feat_pack_offsets(hipStream_t st, int n, const int *ids, const double *off, long stride, int C, int D, int nct, double *offP);
int gmmk_feat_blocks_per_tile(void);
int gmmk_feat_comp_models(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, long n, int D, int nct, const gmmk_zview &z,
                          const double *offP, long off_stride, const gmmiv_feat_tile *tiles, long ntiles, void *out, long ldo); // -1: D > 64
int gmmk_feat_sub(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, long n, int D, const double *P, const double *lse, void *out,
                  long ldo);
int gmmk_feat_map(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, long T, int D, int C, const int *best, const double *cd_mean,
                  const double *cd_cov, const double *ci_mean, const double *ci_cov, void *out, long ldo);
int gmmk_scatter_runs(hipStream_t st, int x_f64, void *x, long ldx, int D, const long *runs, long nrun, const void *in);

// feat_norm.hip: NormFeat's default mode (moments per group, mean / std, computeZeroOne) and the online mode of NormFeatWindowMode
int gmmk_moments_groups(hipStream_t st, int x_f64, const void *x, long ldx, int D, const long *runs, long nrun, long ngroups, double *partial,
                        double *acc); // partial: [nrun x 2D] scratch
int gmmk_moments_stats(hipStream_t st, long ngroups, int D, const double *acc, double *mean, double *sd);
int gmmk_feat_norm_apply(hipStream_t st, int x_f64, int o_f64, const void *x, long ldx, int D, const long *runs, long nrun, long ngroups,
                         const double *mean, const double *sd, void *out, long ldo); // mean / sd nullable
size_t gmmk_online_units(long nfiles, long frames); // upper bound of the chunks of nfiles files with `frames` frames together
long gmmk_online_chunk(void);
int gmmk_feat_norm_online(hipStream_t st, int n_cu, int x_f64, int o_f64, const void *x, long ldx, int D, const long *file_begin, long nfiles,
                          long W, long L, long max_units, long *chunk_off, double *state, double *decay, void *out, long ldo);
// energy_det.hip: EnergyDetector per file (order nullable: the file of each workgroup; max_frames < 0: the longest selection is unknown)
long gmmk_energy_stage_frames(int x_f64);
int gmmk_energy_em(hipStream_t st, int x_f64, const void *x, long ldx, const long *runs, long nrun, long nfiles, const long *order, long max_frames,
                   int C, int nb_it, double flooring, double ceiling, double alpha, double *model, double *threshold, int *status);
int gmmk_energy_select(hipStream_t st, int x_f64, const void *x, long ldx, const long *runs, long nrun, long nfiles, const double *threshold,
                       long *n_above, long *seg_count, const long *seg_off, long *seg_begin, long *seg_len);
