// capi_trials.hip -- C ABI (include/gmmiv.h): gmmiv_llr_trials, the GMM-UBM scores of a whole list of (segment, model) trials in one device
// pass, and its work list gmmiv_plan_trial_tiles.  Kernels in topc_trials.hip.  DESIGN.md section 3.16.
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "capi_gmm_util.h"
#include "gmm_kernels.h"
#include "trials_kernels.h"

extern "C" {

// ---- the tile table (pure host) ---------------------------------------------------------------------------------------------------
int64_t gmmiv_plan_trial_tiles(const int64_t *seg_begin, int64_t nseg, const int32_t *trial_seg, const int32_t *trial_model, int64_t ntrial,
                               int piece_frames, gmmiv_trial_tile *tiles, int64_t cap)
{
    if (!seg_begin || nseg < 0 || ntrial < 0 || (ntrial && (!trial_seg || !trial_model)) || piece_frames <= 0 || piece_frames % 4 || seg_begin[0] < 0) return -1;
    for (int64_t s = 0; s < nseg; ++s)
        if (seg_begin[s + 1] < seg_begin[s]) return -1;
    // the trials of every segment, in list order
    std::vector<int64_t> first((size_t)nseg + 1, 0);
    for (int64_t i = 0; i < ntrial; ++i) {
        if (trial_seg[i] < 0 || trial_seg[i] >= nseg) return -1;
        ++first[(size_t)trial_seg[i] + 1];
    }
    for (int64_t s = 0; s < nseg; ++s) first[s + 1] += first[s];
    std::vector<int64_t> of((size_t)ntrial), fill(first.begin(), first.end() - 1);
    for (int64_t i = 0; i < ntrial; ++i) of[fill[trial_seg[i]]++] = i;
    int64_t n = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t b = seg_begin[s], e = seg_begin[s + 1];
        if (first[s + 1] == first[s]) continue;
        int32_t piece = 0;
        for (int64_t f = b; f < e; f += piece_frames, ++piece) // an empty segment has no tile
            for (int64_t j = first[s]; j < first[s + 1]; ++j) {
                if (tiles && n < cap) {
                    gmmiv_trial_tile t;
                    t.lo = f;
                    t.hi = e < f + piece_frames ? e : f + piece_frames;
                    t.trial = (int32_t)of[j];
                    t.seg = (int32_t)s;
                    t.model = trial_model[of[j]];
                    t.piece = piece;
                    tiles[n] = t;
                }
                ++n;
            }
    }
    return n;
}

int gmmiv_trial_piece(const gmmiv_ctx *c)
{
    return (c && c->trials_piece >= 4 && c->trials_piece % 4 == 0 && c->trials_piece <= 0x40000000) ? (int)c->trials_piece : GMMIV_TRIAL_PIECE;
}

static int use_top_row(gmmiv_ctx *c, const gmmiv_gmm_batch *b, int g, const void *x, int dt, long n, long ldx, int ctop, const int *idx, const double *nllk,
                       int complete, double lo, double hi, double *row)
{
    // the kernels gmmiv_llk_use_top picks, on the tables of model g of the batch
    const double *mean = b->mean + (size_t)g * b->sm, *iv = b->iv + (size_t)g * b->si, *lwc = b->lwc + (size_t)g * b->Cpa;
    int krc = c->topc_z ? gmmk_topc_use16(c->stream, dt == GMMIV_F64, x, n, ldx, b->D, mean, iv, lwc, b->C, ctop, idx, nllk, complete, lo, hi, row,
                                          (int)c->topc_use_lanes)
                        : -1;
    if (krc == -1) krc = gmmk_topc_use(c->stream, dt == GMMIV_F64, x, n, ldx, b->D, mean, iv, lwc, b->C, ctop, idx, nllk, complete, lo, hi, row);
    GCHK(krc);
    return GMMIV_OK;
}

int gmmiv_llr_trials(gmmiv_ctx *c, const gmmiv_gmm *world, const gmmiv_gmm_batch *b, const void *x, int dt, int64_t T, int64_t ldx,
                     const int64_t *seg_begin, int64_t nseg, const int32_t *trial_seg, const int32_t *trial_model, int64_t ntrial, int ctop, int mode,
                     double min_llk, double max_llk, double *llr, double *client_mean, double *world_mean)
{
    const char *who = "llr_trials";
    if (!c || !world || !b) { gmmiv_set_error("%s: NULL context, world model or batch", who); return GMMIV_ERR_ARG; }
    if (world->ctx != c || b->ctx != c) { gmmiv_set_error("%s: the world model / the batch belongs to a different context", who); return GMMIV_ERR_ARG; }
    if (!b->loaded) { gmmiv_set_error("%s: the batch has no models yet (gmmiv_gmm_batch_load)", who); return GMMIV_ERR_ARG; }
    if (b->C != world->C || b->D != world->D) {
        gmmiv_set_error("%s: the batch holds models of %d x %d, the world model is %d x %d", who, b->C, b->D, world->C, world->D);
        return GMMIV_ERR_ARG;
    }
    if (T < 0 || nseg < 0 || ntrial < 0 || !seg_begin || (ntrial && (!trial_seg || !trial_model || !llr))) { gmmiv_set_error("%s: bad argument", who); return GMMIV_ERR_ARG; }
    if (gmmiv_is_device_ptr(seg_begin) || (ntrial && (gmmiv_is_device_ptr(trial_seg) || gmmiv_is_device_ptr(trial_model)))) {
        gmmiv_set_error("%s: seg_begin, trial_seg and trial_model must be host arrays", who);
        return GMMIV_ERR_ARG;
    }
    if (ctop < 1 || ctop > 64 || ctop > world->C) { gmmiv_set_error("%s: topDistribsCount %d outside 1 .. min(64, mixtureDistribCount %d)", who, ctop, world->C); return GMMIV_ERR_ARG; }
    if (mode != GMMIV_TOP_PARTIAL && mode != GMMIV_TOP_COMPLETE) { gmmiv_set_error("%s: mode must be GMMIV_TOP_PARTIAL or GMMIV_TOP_COMPLETE", who); return GMMIV_ERR_ARG; }
    if (nseg > 0x7fffffff / 64 || ntrial > 0x7fffffff / 64) { gmmiv_set_error("%s: too many segments or trials in one call", who); return GMMIV_ERR_UNSUPPORTED; }
    if (seg_begin[0] < 0 || seg_begin[nseg] > T) { gmmiv_set_error("%s: seg_begin out of range", who); return GMMIV_ERR_ARG; }
    for (int64_t s = 0; s < nseg; ++s)
        if (seg_begin[s + 1] < seg_begin[s]) { gmmiv_set_error("%s: seg_begin must be non-decreasing", who); return GMMIV_ERR_ARG; }
    for (int64_t i = 0; i < ntrial; ++i) {
        if (trial_seg[i] < 0 || trial_seg[i] >= nseg) { gmmiv_set_error("%s: trial_seg[%lld] = %d outside [0, %lld)", who, (long long)i, trial_seg[i], (long long)nseg); return GMMIV_ERR_ARG; }
        if (trial_model[i] < 0 || trial_model[i] >= b->G) { gmmiv_set_error("%s: trial_model[%lld] = %d outside [0, %d)", who, (long long)i, trial_model[i], b->G); return GMMIV_ERR_ARG; }
    }
    if (dt != GMMIV_F32 && dt != GMMIV_F64) { gmmiv_set_error("feature dtype must be GMMIV_F32 or GMMIV_F64"); return GMMIV_ERR_ARG; }
    if (ldx < b->D) { gmmiv_set_error("ldx (%ld) < D (%d)", (long)ldx, b->D); return GMMIV_ERR_ARG; }
    if (nseg == 0) return GMMIV_OK; // no segment: no trial either
    GBIND(c);
    int rc;
    const int P = gmmiv_trial_piece(c);
    const int complete = mode == GMMIV_TOP_COMPLETE;
    const int64_t f0 = seg_begin[0], span = seg_begin[nseg] - f0;
    // the frames of the segments only: a host x is copied from its row f0 on
    XView xv;
    if ((rc = xv.init(c, span > 0 ? (const char *)x + (size_t)f0 * ldx * gmmiv_esize(dt) : x, dt, span, ldx, b->D))) return rc;
    DevOut<double> o_llr, o_cm, o_wm;
    if ((rc = o_llr.init(c, WS_T0, llr, (size_t)ntrial, false))) return rc;
    if ((rc = o_cm.init(c, WS_T1, client_mean, (size_t)ntrial, false))) return rc;
    if ((rc = o_wm.init(c, WS_T2, world_mean, (size_t)nseg, false))) return rc;

    // tables: the tiles (sorted by segment, piece, trial), the slots of every trial's and every segment's partials
    const int64_t ntiles = gmmiv_plan_trial_tiles(seg_begin, nseg, trial_seg, trial_model, ntrial, P, nullptr, 0);
    if (ntiles < 0) { gmmiv_set_error("%s: bad trial list", who); return GMMIV_ERR_ARG; }
    std::vector<gmmiv_trial_tile> tiles((size_t)ntiles);
    gmmiv_plan_trial_tiles(seg_begin, nseg, trial_seg, trial_model, ntrial, P, tiles.data(), ntiles);
    auto pieces = [&](int64_t s) { return (seg_begin[s + 1] - seg_begin[s] + P - 1) / P; };
    // one host table of longs: seg_begin [nseg + 1] | seg_off [nseg + 1] | trial_off [ntrial + 1]; trial_seg goes up as it is
    std::vector<long> tab((size_t)(2 * (nseg + 1) + ntrial + 1));
    long *h_sb = tab.data(), *h_so = h_sb + nseg + 1, *h_to = h_so + nseg + 1;
    h_so[0] = 0;
    for (int64_t s = 0; s <= nseg; ++s) h_sb[s] = (long)seg_begin[s];
    for (int64_t s = 0; s < nseg; ++s) h_so[s + 1] = h_so[s] + (long)pieces(s);
    h_to[0] = 0;
    for (int64_t i = 0; i < ntrial; ++i) h_to[i + 1] = h_to[i] + (long)pieces(trial_seg[i]);
    if (h_to[ntrial] != (long)ntiles) { gmmiv_set_error("%s: internal error, %ld slots for %lld tiles", who, h_to[ntrial], (long long)ntiles); return GMMIV_ERR_ARG; }
    void *d_tiles, *d_tab, *d_part;
    if ((rc = c->scratch(WS_TR_TILES, (size_t)ntiles * sizeof(gmmiv_trial_tile), &d_tiles))) return rc;
    if ((rc = c->scratch(WS_TR_TAB, tab.size() * sizeof(long) + (size_t)ntrial * sizeof(int32_t), &d_tab))) return rc;
    if ((rc = c->scratch(WS_TR_PART, (size_t)(ntiles + h_so[nseg]) * sizeof(double), &d_part))) return rc;
    const long *d_sb = (const long *)d_tab, *d_so = d_sb + nseg + 1, *d_to = d_so + nseg + 1;
    const int *d_ts = (const int *)(d_to + ntrial + 1);
    double *part = (double *)d_part, *wpart = part + ntiles;
    if (ntiles) GCHK(hipMemcpyAsync(d_tiles, tiles.data(), (size_t)ntiles * sizeof(gmmiv_trial_tile), hipMemcpyHostToDevice, c->stream));
    GCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(long), hipMemcpyHostToDevice, c->stream));
    if (ntrial) GCHK(hipMemcpyAsync((void *)d_ts, trial_seg, (size_t)ntrial * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    GCHK(hipStreamSynchronize(c->stream)); // the tables live in host vectors / the caller's arrays

    // chunks of whole segments whose per-frame world results fit the scratch (a segment longer than that is a chunk of its own)
    const size_t per_frame = (size_t)ctop * sizeof(int32_t) + 2 * sizeof(double);
    int64_t Tc = (int64_t)((((size_t)(c->trials_scratch_mb > 0 ? c->trials_scratch_mb : 0)) << 20) / per_frame);
    if (Tc < 1) Tc = 1;
    int64_t max_frames = 0, max_seg = 0;
    std::vector<int64_t> cuts(1, 0);
    for (int64_t s0 = 0; s0 < nseg;) {
        int64_t s1 = s0 + 1;
        while (s1 < nseg && seg_begin[s1 + 1] - seg_begin[s0] <= Tc) ++s1;
        cuts.push_back(s1);
        if (seg_begin[s1] - seg_begin[s0] > max_frames) max_frames = seg_begin[s1] - seg_begin[s0];
        s0 = s1;
    }
    for (int64_t s = 0; s < nseg; ++s)
        if (seg_begin[s + 1] - seg_begin[s] > max_seg) max_seg = seg_begin[s + 1] - seg_begin[s];
    const bool fast = c->topc_z && c->topc_use_lanes == 4 && ctop <= 16 && b->D % 2 == 0;
    void *d_idx, *d_nllk, *d_llkw, *d_row = nullptr;
    const size_t nf = (size_t)(max_frames > 0 ? max_frames : 1);
    if ((rc = c->scratch(WS_TR_IDX, nf * ctop * sizeof(int32_t), &d_idx))) return rc;
    if ((rc = c->scratch(WS_TR_NLLK, nf * sizeof(double), &d_nllk))) return rc;
    if ((rc = c->scratch(WS_TR_LLKW, nf * sizeof(double), &d_llkw))) return rc;
    if (!fast && (rc = c->scratch(WS_TR_ROW, (size_t)(max_seg > 0 ? max_seg : 1) * sizeof(double), &d_row))) return rc;

    size_t tile0 = 0;
    bool first = true; // the first launch of the call restarts the "k_topc_use" timer
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        const int64_t s0 = cuts[k], s1 = cuts[k + 1], base = seg_begin[s0], n = seg_begin[s1] - base;
        size_t tile1 = tile0;
        while (tile1 < (size_t)ntiles && tiles[tile1].seg < s1) ++tile1;
        if (n > 0) {
            const void *xc = gmmiv_x_at(xv, dt, base - f0);
            // the world pass of the chunk: top set, remainder and clamped log-likelihood of every frame, as gmmiv_llk_determine_top gives them
            if ((rc = gmmiv_llk_determine_top(c, world, xc, dt, n, xv.ldx, ctop, mode, min_llk, max_llk, (int32_t *)d_idx, nullptr, nullptr, (double *)d_nllk,
                                              nullptr, (double *)d_llkw)))
                return rc;
            GCHK(gmmk_piece_sums_segs(c->stream, (const double *)d_llkw, (long)base, d_sb, d_so, (long)s0, (long)s1, h_so[s1] - h_so[s0], P, wpart));
            if (fast) {
                c->t_begin("k_topc_use", first);
                first = false;
                GCHK(gmmk_topc_use4_trials(c->stream, dt == GMMIV_F64, xv.d, (long)f0, xv.ldx, b->D, b->mean, b->sm, b->iv, b->si, b->lwc, (long)b->Cpa, b->C, ctop,
                                           (const gmmiv_trial_tile *)d_tiles + tile0, (long)(tile1 - tile0), d_to, (long)base, (const int *)d_idx,
                                           (const double *)d_nllk, complete, min_llk, max_llk, part));
                c->t_end();
            } else {
                // any shape (topDistribsCount > 16, odd vectSize): trial by trial through the kernels gmmiv_llk_use_top runs, into a row of
                // per-frame values that the same piece scheme sums.  Launch-bound: two launches per trial.
                for (int64_t i = 0; i < ntrial; ++i) {
                    const int64_t s = trial_seg[i];
                    if (s < s0 || s >= s1 || seg_begin[s + 1] == seg_begin[s]) continue;
                    const int64_t sb = seg_begin[s], ns = seg_begin[s + 1] - sb;
                    c->t_begin("k_topc_use", first);
                    first = false;
                    rc = use_top_row(c, b, trial_model[i], gmmiv_x_at(xv, dt, sb - f0), dt, (long)ns, xv.ldx, ctop, (const int *)d_idx + (size_t)(sb - base) * ctop,
                                     (const double *)d_nllk + (sb - base), complete, min_llk, max_llk, (double *)d_row);
                    c->t_end();
                    if (rc) return rc;
                    GCHK(gmmk_piece_sums_row(c->stream, (const double *)d_row, (long)ns, P, part + h_to[i]));
                }
            }
        }
        tile0 = tile1;
    }
    c->t_begin("k_trial_reduce");
    GCHK(gmmk_trial_reduce(c->stream, (long)ntrial, (long)nseg, d_ts, d_to, d_sb, d_so, part, wpart, o_llr.d, o_cm.d, o_wm.d));
    c->t_end();
    if ((rc = o_llr.finish())) return rc;
    if ((rc = o_cm.finish())) return rc;
    return o_wm.finish();
}

} // extern "C"
