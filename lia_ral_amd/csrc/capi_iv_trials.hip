// capi_iv_trials.hip -- C ABI (include/gmmiv_iv_trials.h): the i-vector scoring rules on a list of (model, segment) trials and their
// host planner gmmiv_plan_iv_trial_tiles.  Kernels in iv_trials.hip; the dense rules are capi_iv_score.hip.  DESIGN.md section 3.21.
#include <string.h>

#include <algorithm>
#include <memory>
#include <thread>
#include <vector>

#include "ctx.h"
#include "host_linalg.h"
#include "iv_trials_kernels.h"
#include "tv_kernels.h"

// ---- the work list (pure host) ------------------------------------------------------------------------------------------------------
// The trials sel[0 .. n) (list positions, increasing; sel == NULL: 0 .. n) sorted by (anchor, partner, position) and cut into pieces.
// Two stable counting passes, the partner first; a record carries its keys along, so neither pass reads the list out of order, and the
// anchors' histogram gives the runs the tiles are cut from.  Every pass scatters into as many streams as there are vectors, which one core
// does at tens of nanoseconds per trial -- at 10^7 trials far more than the kernel takes -- so long lists are planned in chunks on up to 16
// host threads (a chunk keeps the list order and the chunks' slots follow each other: the result does not depend on the thread count).
namespace {
struct IvtRec { int32_t pos, anchor, partner; };
// host threads of the planner: one below 2^18 trials, else the machine's, at most 16
int ivt_threads(int64_t n)
{
    if (n < (1 << 18)) return 1;
    const unsigned h = std::thread::hardware_concurrency();
    return h == 0 ? 1 : (h > 16 ? 16 : (int)h);
}
template <class F> void ivt_parallel(int T, F f)
{
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(f, t);
    f(0);
    for (std::thread &x : th) x.join();
}
// one STABLE counting pass over the items 0 .. n in T chunks: item i has key(i) in [0, K) and is stored by put(i, slot)
template <class Key, class Put> void ivt_pass(int T, int64_t n, int64_t K, std::vector<std::vector<int64_t> > &cnt, Key key, Put put)
{
    cnt.resize((size_t)T);
    ivt_parallel(T, [&](int c) {
        std::vector<int64_t> &h = cnt[(size_t)c];
        h.assign((size_t)K, 0);
        for (int64_t i = n * c / T, e = n * (c + 1) / T; i < e; ++i) ++h[(size_t)key(i)];
    });
    int64_t run = 0;
    for (int64_t k = 0; k < K; ++k)
        for (int c = 0; c < T; ++c) { const int64_t v = cnt[(size_t)c][(size_t)k]; cnt[(size_t)c][(size_t)k] = run; run += v; }
    ivt_parallel(T, [&](int c) {
        std::vector<int64_t> &h = cnt[(size_t)c];
        for (int64_t i = n * c / T, e = n * (c + 1) / T; i < e; ++i) put(i, h[(size_t)key(i)]++);
    });
}
struct IvtPlanner {
    std::vector<int64_t> hm, hs; // trials per model / per segment, as offsets
    std::vector<std::vector<int64_t> > cnt, cnt2;
    std::unique_ptr<IvtRec[]> rec; // grown, never cleared: every record is written before it is read
    size_t rec_cap = 0;
    int anchor = GMMIV_IV_ANCHOR_MODEL;
    // anchor_opt: GMMIV_IV_ANCHOR_MODEL / _SEG, anything else = the auto rule.  partner / pos (nullable, together): the sorted arrays
    // [n].  Leaves `anchor` and the histograms that cut() reads.
    void run(int64_t M, int64_t S, const int32_t *tm, const int32_t *ts, const int32_t *sel, int64_t n, int anchor_opt, int32_t *partner, int32_t *pos)
    {
        const int T = ivt_threads(n);
        cnt.resize((size_t)T);
        cnt2.resize((size_t)T);
        ivt_parallel(T, [&](int c) {
            std::vector<int64_t> &a = cnt[(size_t)c], &b = cnt2[(size_t)c];
            a.assign((size_t)M + 1, 0);
            b.assign((size_t)S + 1, 0);
            for (int64_t i = n * c / T, e = n * (c + 1) / T; i < e; ++i) {
                const int64_t at = sel ? sel[i] : i;
                ++a[(size_t)tm[at] + 1];
                ++b[(size_t)ts[at] + 1];
            }
        });
        hm.assign((size_t)M + 1, 0);
        hs.assign((size_t)S + 1, 0);
        for (int c = 0; c < T; ++c) {
            for (int64_t m = 1; m <= M; ++m) hm[(size_t)m] += cnt[(size_t)c][(size_t)m];
            for (int64_t k = 1; k <= S; ++k) hs[(size_t)k] += cnt2[(size_t)c][(size_t)k];
        }
        int64_t dm = 0, ds = 0; // distinct vectors: fewer distinct segments than models -> the segment side; a tie goes to the model
        for (int64_t m = 0; m < M; ++m) { dm += hm[m + 1] > 0; hm[m + 1] += hm[m]; }
        for (int64_t k = 0; k < S; ++k) { ds += hs[k + 1] > 0; hs[k + 1] += hs[k]; }
        anchor = (anchor_opt == GMMIV_IV_ANCHOR_MODEL || anchor_opt == GMMIV_IV_ANCHOR_SEG) ? anchor_opt
                                                                                           : (ds < dm ? GMMIV_IV_ANCHOR_SEG : GMMIV_IV_ANCHOR_MODEL);
        if (!partner || n <= 0) return;
        const bool by_seg = anchor == GMMIV_IV_ANCHOR_SEG;
        const int32_t *ta = by_seg ? ts : tm, *tp = by_seg ? tm : ts;
        if (rec_cap < (size_t)n) { rec.reset(new IvtRec[(size_t)n]); rec_cap = (size_t)n; }
        IvtRec *r = rec.get();
        ivt_pass(T, n, by_seg ? M : S, cnt, [&](int64_t i) { return tp[sel ? sel[i] : i]; }, // by partner: the records carry their keys along
                 [&](int64_t i, int64_t j) {
                     const int64_t at = sel ? sel[i] : i;
                     r[j].pos = (int32_t)at; r[j].anchor = ta[at]; r[j].partner = tp[at];
                 });
        ivt_pass(T, n, by_seg ? S : M, cnt, [&](int64_t i) { return r[i].anchor; },           // by anchor
                 [&](int64_t i, int64_t j) { partner[j] = r[i].partner; pos[j] = r[i].pos; });
    }
    // the tiles of the last run: runs of one anchor in pieces of at most `piece`; lo / hi count from `base`; at most cap entries are
    // written (tiles nullable).  Returns the number of tiles.
    int64_t cut(int piece, int64_t base, gmmiv_iv_trial_tile *tiles, int64_t cap) const
    {
        const std::vector<int64_t> &ha = anchor == GMMIV_IV_ANCHOR_SEG ? hs : hm;
        int64_t nt = 0;
        for (int64_t a = 0, nA = (int64_t)ha.size() - 1; a < nA; ++a)
            for (int64_t lo = ha[a], e = ha[a + 1]; lo < e; lo += piece, ++nt)
                if (tiles && nt < cap) {
                    gmmiv_iv_trial_tile t;
                    t.anchor = (int32_t)a;
                    t.reserved = 0;
                    t.lo = base + lo;
                    t.hi = base + std::min<int64_t>(e, lo + piece);
                    tiles[nt] = t;
                }
        return nt;
    }
};
} // namespace

// the first trial with an index out of range, or -1
static int64_t ivt_first_bad(int64_t M, int64_t S, const int32_t *tm, const int32_t *ts, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (tm[i] < 0 || tm[i] >= M || ts[i] < 0 || ts[i] >= S) return i;
    return -1;
}

extern "C" {

int gmmiv_iv_trial_piece(const gmmiv_ctx *c)
{
    return (c && c->iv_trials_piece > 0 && c->iv_trials_piece <= 0x40000000) ? (int)c->iv_trials_piece : GMMIV_IV_TRIAL_PIECE;
}

int gmmiv_iv_trial_anchor(int64_t M, int64_t S, const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial)
{
    if (M < 0 || S < 0 || ntrial < 0 || ntrial > 0x7fffffff || (ntrial && (!trial_model || !trial_seg))) return -1;
    if (ivt_first_bad(M, S, trial_model, trial_seg, ntrial) >= 0) return -1;
    IvtPlanner pl;
    pl.run(M, S, trial_model, trial_seg, nullptr, ntrial, GMMIV_IV_ANCHOR_AUTO, nullptr, nullptr);
    return pl.anchor;
}

int64_t gmmiv_plan_iv_trial_tiles(int64_t M, int64_t S, const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial, int anchor,
                                  int piece, int64_t *order, gmmiv_iv_trial_tile *tiles, int64_t cap)
{
    if (M < 0 || S < 0 || ntrial < 0 || ntrial > 0x7fffffff || piece < 1 || anchor < GMMIV_IV_ANCHOR_AUTO || anchor > GMMIV_IV_ANCHOR_SEG) return -1;
    if (ntrial && (!trial_model || !trial_seg)) return -1;
    if (ivt_first_bad(M, S, trial_model, trial_seg, ntrial) >= 0) return -1;
    if (ntrial == 0) return 0;
    IvtPlanner pl;
    std::vector<int32_t> pp(order ? (size_t)2 * ntrial : 0);
    pl.run(M, S, trial_model, trial_seg, nullptr, ntrial, anchor, order ? pp.data() : nullptr, order ? pp.data() + ntrial : nullptr);
    const int64_t nt = pl.cut(piece, 0, tiles, tiles ? cap : 0);
    if (order)
        for (int64_t i = 0; i < ntrial; ++i) order[i] = pp[(size_t)ntrial + i];
    return nt;
}

} // extern "C"

// ---- the calls ------------------------------------------------------------------------------------------------------------------------
// everything that can be said about the arguments without a context or a device
static int ivt_check(const char *who, int dim, int64_t M, int64_t S, const double *models, const double *segs, const int32_t *tm,
                     const int32_t *ts, int64_t ntrial, const double *scores)
{
    if (dim <= 0 || M < 0 || S < 0 || ntrial < 0) {
        gmmiv_set_error("%s: bad size (dim %d, M %lld, S %lld, ntrial %lld)", who, dim, (long long)M, (long long)S, (long long)ntrial);
        return GMMIV_ERR_ARG;
    }
    if ((M > 0 && !models) || (S > 0 && !segs)) { gmmiv_set_error("%s: models / segs == NULL", who); return GMMIV_ERR_ARG; }
    if (ntrial > 0 && (!tm || !ts || !scores)) { gmmiv_set_error("%s: trial_model / trial_seg / scores == NULL", who); return GMMIV_ERR_ARG; }
    if (ntrial > 0 && (gmmiv_is_device_ptr(tm) || gmmiv_is_device_ptr(ts))) {
        gmmiv_set_error("%s: trial_model and trial_seg must be host arrays", who);
        return GMMIV_ERR_ARG;
    }
    const int64_t bad = ivt_first_bad(M, S, tm, ts, ntrial);
    if (bad >= 0) {
        if (tm[bad] < 0 || tm[bad] >= M) gmmiv_set_error("%s: trial_model[%lld] = %d outside [0, %lld)", who, (long long)bad, tm[bad], (long long)M);
        else gmmiv_set_error("%s: trial_seg[%lld] = %d outside [0, %lld)", who, (long long)bad, ts[bad], (long long)S);
        return GMMIV_ERR_ARG;
    }
    if (M > 0x7fffffff || S > 0x7fffffff || ntrial > 0x7fffffff) { gmmiv_set_error("%s: too many vectors or trials in one call", who); return GMMIV_ERR_UNSUPPORTED; }
    return GMMIV_OK;
}

namespace {
struct IvtCall {
    gmmiv_ctx *c;
    int dim, ldr;
    int64_t M, S, ntrial;
    const int32_t *tm, *ts;
    DevIn<double> m, s;
    DevOut<double> sc;
    double *A = nullptr, *B = nullptr, *Y = nullptr, *qm = nullptr, *qs = nullptr, *mat = nullptr;
    // one class = one launch: the trials sel[0 .. n) of the list, their tiles and arrays at [e0, e0 + n) / [t0, t0 + nt) of the tables
    struct Class { std::vector<int32_t> sel; bool all = false; int64_t n = 0, e0 = 0, t0 = 0, nt = 0; int anchor = 0; };
    std::vector<Class> cls;
    const gmmiv_iv_trial_tile *d_tiles = nullptr;
    const int *d_partner = nullptr, *d_pos = nullptr;
    bool first_k = true, first_g = true;

    int init(gmmiv_ctx *ctx, int dim_, int64_t M_, int64_t S_, const double *models, const double *segs, const int32_t *tm_, const int32_t *ts_,
             int64_t ntrial_, double *scores)
    {
        c = ctx; dim = dim_; ldr = dim_ + (dim_ & 1); M = M_; S = S_; ntrial = ntrial_; tm = tm_; ts = ts_;
        int rc;
        void *p;
        if ((rc = m.init(c, WS_IVT_M, models, (size_t)dim * M)) || (rc = s.init(c, WS_IVT_S, segs, (size_t)dim * S)) ||
            (rc = sc.init(c, WS_IVT_OUT, scores, (size_t)ntrial, false))) return rc;
        if ((rc = c->scratch(WS_IVT_A, (size_t)M * ldr * 8, &p))) return rc;
        A = (double *)p;
        if ((rc = c->scratch(WS_IVT_B, (size_t)S * ldr * 8, &p))) return rc;
        B = (double *)p;
        if ((rc = c->scratch(WS_IVT_Y, (size_t)dim * std::max(M, S) * 8, &p))) return rc;
        Y = (double *)p;
        if ((rc = c->scratch(WS_IVT_Q, (size_t)(M + S) * 8, &p))) return rc;
        qm = (double *)p;
        qs = qm + M;
        if ((rc = c->scratch(WS_IVT_MAT, (size_t)4 * dim * dim * 8, &p))) return rc;
        mat = (double *)p;
        GCHK(ivk_cols_to_rows(c->stream, dim, M, m.d, M, A, ldr)); // the models as rows: never projected
        return GMMIV_OK;
    }
    // plan every class, upload the tables of all of them and wait for the copy (they live in buffers of this call)
    int upload()
    {
        const int P = gmmiv_iv_trial_piece(c);
        int64_t total = 0;
        for (Class &k : cls) { k.n = k.all ? ntrial : (int64_t)k.sel.size(); total += k.n; } // <= ntrial: a trial belongs to one class
        std::unique_ptr<int32_t[]> pp(new int32_t[(size_t)(total > 0 ? 2 * total : 1)]);
        int32_t *partner = pp.get(), *pos = partner + total;
        std::vector<gmmiv_iv_trial_tile> tiles;
        IvtPlanner pl;
        int64_t e0 = 0;
        for (Class &k : cls) {
            const int32_t *sel = k.all ? nullptr : k.sel.data();
            k.e0 = e0;
            k.t0 = (int64_t)tiles.size();
            pl.run(M, S, tm, ts, sel, k.n, (int)c->iv_trials_anchor, partner + e0, pos + e0);
            k.anchor = pl.anchor;
            k.nt = pl.cut(P, e0, nullptr, 0);
            tiles.resize((size_t)(k.t0 + k.nt));
            pl.cut(P, e0, tiles.data() + k.t0, k.nt);
            e0 += k.n;
        }
        void *p;
        int rc;
        const size_t tb = tiles.size() * sizeof(gmmiv_iv_trial_tile);
        if ((rc = c->scratch(WS_IVT_TAB, GMMIV_IV_TRIAL_TABLE_BYTES(total, tiles.size()), &p))) return rc;
        d_tiles = (const gmmiv_iv_trial_tile *)p;
        d_partner = (const int *)((char *)p + tb);
        d_pos = d_partner + total;
        if (tb) GCHK(hipMemcpyAsync(p, tiles.data(), tb, hipMemcpyHostToDevice, c->stream));
        if (total) GCHK(hipMemcpyAsync((void *)d_partner, pp.get(), (size_t)2 * total * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
        return GMMIV_OK;
    }
    // B, qm and qs of one rule: Qc, Qm, Qs on the device (dim x dim)
    int project(const double *Qc, const double *Qm, const double *Qs)
    {
        double *Qsym = mat + (size_t)3 * dim * dim;
        GCHK(tvk_dgemm(c->stream, false, false, dim, (int)M, dim, 1.0, Qm, dim, 0, m.d, M, 0, 0.0, Y, M, 0, 1));
        GCHK(tvk_coldot(c->stream, dim, M, m.d, Y, qm, M));
        GCHK(tvk_dgemm(c->stream, false, false, dim, (int)S, dim, 1.0, Qs, dim, 0, s.d, S, 0, 0.0, Y, S, 0, 1));
        GCHK(tvk_coldot(c->stream, dim, S, s.d, Y, qs, S));
        GCHK(tvk_add_transpose(c->stream, dim, Qc, Qc, Qsym));
        c->t_begin("k_dgemm(score)", first_g);
        first_g = false;
        // B [S x ldr] = segs^T (Qc + Qc^T): the rows ((Qc + Qc^T) s)^T, written in row form
        GCHK(tvk_dgemm(c->stream, true, false, (int)S, dim, dim, 1.0, s.d, S, 0, Qsym, dim, 0, 0.0, B, ldr, 0, 1));
        GCHK(ivk_zero_pad(c->stream, dim, S, B, ldr));
        c->t_end();
        return GMMIV_OK;
    }
    int launch(const Class &k, int mode, double cc, double bm, double bs, double cst)
    {
        const bool by_seg = k.anchor == GMMIV_IV_ANCHOR_SEG;
        c->t_begin("k_score_trials", first_k);
        first_k = false;
        GCHK(ivk_score_trials(c->stream, ldr, by_seg ? B : A, by_seg ? A : B, by_seg ? qs : qm, by_seg ? qm : qs, by_seg, d_tiles + k.t0, (long)k.nt,
                              d_partner, d_pos, mode, cc, bm, bs, cst, sc.d));
        c->t_end();
        return GMMIV_OK;
    }
    int whole_list()
    {
        cls.resize(1);
        cls[0].all = true;
        return upload();
    }
};
} // namespace

extern "C" {

int gmmiv_score_cosine_trials(gmmiv_ctx *c, int dim, int64_t M, int64_t S, const double *models, const double *segs,
                              const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial, double *scores)
{
    int rc = ivt_check("score_cosine_trials", dim, M, S, models, segs, trial_model, trial_seg, ntrial, scores);
    if (rc) return rc;
    if (!c) { gmmiv_set_error("score_cosine_trials: ctx == NULL"); return GMMIV_ERR_ARG; }
    if (ntrial == 0) return GMMIV_OK;
    GBIND(c);
    IvtCall a;
    if ((rc = a.init(c, dim, M, S, models, segs, trial_model, trial_seg, ntrial, scores)) || (rc = a.whole_list())) return rc;
    GCHK(ivk_cols_to_rows(c->stream, dim, S, a.s.d, S, a.B, a.ldr));
    GCHK(tvk_coldot(c->stream, dim, M, a.m.d, a.m.d, a.qm, M));
    GCHK(tvk_coldot(c->stream, dim, S, a.s.d, a.s.d, a.qs, S));
    GCHK(tvk_rsqrt_vec(c->stream, M + S, a.qm)); // qm | qs are one array
    if ((rc = a.launch(a.cls[0], 1, 0.0, 0.0, 0.0, 0.0))) return rc;
    return a.sc.finish();
}

int gmmiv_score_mahalanobis_trials(gmmiv_ctx *c, int dim, int64_t M, int64_t S, const double *models, const double *segs, const double *Mah,
                                   const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial, double *scores)
{
    int rc = ivt_check("score_mahalanobis_trials", dim, M, S, models, segs, trial_model, trial_seg, ntrial, scores);
    if (rc) return rc;
    if (!Mah) { gmmiv_set_error("score_mahalanobis_trials: Mah == NULL"); return GMMIV_ERR_ARG; }
    if (!c) { gmmiv_set_error("score_mahalanobis_trials: ctx == NULL"); return GMMIV_ERR_ARG; }
    if (ntrial == 0) return GMMIV_OK;
    GBIND(c);
    IvtCall a;
    if ((rc = a.init(c, dim, M, S, models, segs, trial_model, trial_seg, ntrial, scores)) || (rc = a.whole_list())) return rc;
    const size_t nn = (size_t)dim * dim;
    GCHK(hipMemcpyAsync(a.mat, Mah, nn * 8, hipMemcpyDefault, c->stream));
    if (!gmmiv_is_device_ptr(Mah)) GCHK(hipStreamSynchronize(c->stream)); // the caller's matrix may go away on return
    // -1/2 (m-s)' Q (m-s) = -1/2 m'Qm - 1/2 s'Qs + 1/2 m'(Q+Q')s
    if ((rc = a.project(a.mat, a.mat, a.mat)) || (rc = a.launch(a.cls[0], 2, 0.5, -0.5, -0.5, 0.0))) return rc;
    return a.sc.finish();
}

int gmmiv_score_twocov_trials(gmmiv_ctx *c, int dim, int64_t M, int64_t S, const double *models, const double *segs, const double *G,
                              const double *H, const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial, double *scores)
{
    int rc = ivt_check("score_twocov_trials", dim, M, S, models, segs, trial_model, trial_seg, ntrial, scores);
    if (rc) return rc;
    if (!G || !H) { gmmiv_set_error("score_twocov_trials: G/H == NULL"); return GMMIV_ERR_ARG; }
    if (!c) { gmmiv_set_error("score_twocov_trials: ctx == NULL"); return GMMIV_ERR_ARG; }
    if (ntrial == 0) return GMMIV_OK;
    GBIND(c);
    IvtCall a;
    if ((rc = a.init(c, dim, M, S, models, segs, trial_model, trial_seg, ntrial, scores)) || (rc = a.whole_list())) return rc;
    const size_t nn = (size_t)dim * dim;
    double *dG = a.mat, *dH = a.mat + nn, *GmH = a.mat + 2 * nn;
    GCHK(hipMemcpyAsync(dG, G, nn * 8, hipMemcpyDefault, c->stream));
    GCHK(hipMemcpyAsync(dH, H, nn * 8, hipMemcpyDefault, c->stream));
    if (!gmmiv_is_device_ptr(G) || !gmmiv_is_device_ptr(H)) GCHK(hipStreamSynchronize(c->stream));
    // (m+s)'G(m+s) - m'Hm - s'Hs = m'(G-H)m + s'(G-H)s + m'(G+G')s
    GCHK(tvk_axpby(c->stream, (long)nn, 1.0, dG, -1.0, dH, GmH));
    if ((rc = a.project(dG, GmH, GmH)) || (rc = a.launch(a.cls[0], 2, 1.0, 1.0, 1.0, 0.0))) return rc;
    return a.sc.finish();
}

int gmmiv_score_plda_trials(gmmiv_ctx *c, int rf, int64_t M, int64_t S, const double *models_sum, const int64_t *nsess, const double *segs,
                            const double *FTJF, const int32_t *trial_model, const int32_t *trial_seg, int64_t ntrial, double *scores)
{
    const char *who = "score_plda_trials";
    int rc = ivt_check(who, rf, M, S, models_sum, segs, trial_model, trial_seg, ntrial, scores);
    if (rc) return rc;
    if (!FTJF || (M > 0 && !nsess)) { gmmiv_set_error("%s: nsess/FTJF == NULL", who); return GMMIV_ERR_ARG; }
    if (M > 0 && gmmiv_is_device_ptr(nsess)) { gmmiv_set_error("%s: nsess must be a host array", who); return GMMIV_ERR_ARG; }
    for (int64_t i = 0; i < ntrial; ++i)
        if (nsess[trial_model[i]] < 1) {
            gmmiv_set_error("%s: trial %lld: nsess[%d] = %lld < 1", who, (long long)i, trial_model[i], (long long)nsess[trial_model[i]]);
            return GMMIV_ERR_ARG;
        }
    if (!c) { gmmiv_set_error("%s: ctx == NULL", who); return GMMIV_ERR_ARG; }
    if (ntrial == 0) return GMMIV_OK;
    GBIND(c);
    IvtCall a;
    if ((rc = a.init(c, rf, M, S, models_sum, segs, trial_model, trial_seg, ntrial, scores))) return rc;
    // the classes: the distinct session counts of the models that occur, in increasing order (a handful: found by a linear search)
    std::vector<int64_t> vals;
    for (int64_t i = 0; i < ntrial; ++i) {
        const int64_t L = nsess[trial_model[i]];
        if (std::find(vals.begin(), vals.end(), L) == vals.end()) vals.push_back(L);
    }
    std::sort(vals.begin(), vals.end());
    a.cls.resize(vals.size());
    if (vals.size() == 1) a.cls[0].all = true;
    else {
        std::vector<int32_t> cls_of((size_t)M, -1); // per model, looked up once
        for (int64_t i = 0; i < ntrial; ++i) {
            int32_t &k = cls_of[(size_t)trial_model[i]];
            if (k < 0) k = (int32_t)(std::lower_bound(vals.begin(), vals.end(), nsess[trial_model[i]]) - vals.begin());
            a.cls[(size_t)k].sel.push_back((int32_t)i);
        }
    }
    if ((rc = a.upload())) return rc;

    const size_t nn = (size_t)rf * rf;
    std::vector<double> hF(nn);
    // a device FTJF is read in the order of the context's stream, as in gmmiv_score_plda
    if (gmmiv_is_device_ptr(FTJF)) {
        GCHK(hipMemcpyAsync(hF.data(), FTJF, nn * 8, hipMemcpyDeviceToHost, c->stream));
        GCHK(hipStreamSynchronize(c->stream));
    } else memcpy(hF.data(), FTJF, nn * 8);
    // K_n = (n FTJF + I)^-1 and a_n = log det K_n: the context's cache, shared with gmmiv_score_plda
    typedef gmmiv_ctx::PldaK KN;
    if (c->plda_ftjf.size() != nn || memcmp(c->plda_ftjf.data(), hF.data(), nn * 8) != 0) {
        c->plda_ftjf = hF;
        c->plda_k.clear();
    }
    std::map<long, KN> &cache = c->plda_k;
    auto getK = [&](int64_t n) -> const KN * {
        auto it = cache.find((long)n);
        if (it != cache.end()) return &it->second;
        std::vector<double> t(nn);
        for (size_t e = 0; e < nn; ++e) t[e] = (double)n * hF[e];
        for (int i = 0; i < rf; ++i) t[(size_t)i * rf + i] += 1.0;
        KN kn;
        double ld;
        if (!host_spd_inverse(rf, t, kn.K, &ld)) return nullptr;
        kn.alpha = -ld;
        return &cache.emplace((long)n, std::move(kn)).first->second;
    };
    const KN *K1 = getK(1);
    if (!K1) { gmmiv_set_error("%s: FTJF + I is not positive definite", who); return GMMIV_ERR_NUMERIC; }
    double *dQc = a.mat, *dQm = a.mat + nn, *dQs = a.mat + 2 * nn;
    std::vector<double> qm(nn), qs(nn);
    for (size_t k = 0; k < vals.size(); ++k) {
        const int64_t L = vals[k];
        const KN *KL = getK(L), *KL1 = getK(L + 1);
        if (!KL || !KL1) { gmmiv_set_error("%s: K_n not positive definite", who); return GMMIV_ERR_NUMERIC; }
        // score = 1/2 m'(K_{L+1}-K_L)m + 1/2 s'(K_{L+1}-K_1)s + 1/2 m'(K_{L+1}+K_{L+1}')s + (a_{L+1} - a_L - a_1)/2
        for (size_t e = 0; e < nn; ++e) { qm[e] = KL1->K[e] - KL->K[e]; qs[e] = KL1->K[e] - K1->K[e]; }
        GCHK(hipMemcpyAsync(dQc, KL1->K.data(), nn * 8, hipMemcpyHostToDevice, c->stream));
        GCHK(hipMemcpyAsync(dQm, qm.data(), nn * 8, hipMemcpyHostToDevice, c->stream));
        GCHK(hipMemcpyAsync(dQs, qs.data(), nn * 8, hipMemcpyHostToDevice, c->stream));
        GCHK(hipStreamSynchronize(c->stream)); // qm / qs are rewritten for the next class
        const double cst = (KL1->alpha - KL->alpha - K1->alpha) / 2.0;
        if ((rc = a.project(dQc, dQm, dQs)) || (rc = a.launch(a.cls[k], 2, 0.5, 0.5, 0.5, cst))) return rc;
    }
    return a.sc.finish();
}

} // extern "C"
