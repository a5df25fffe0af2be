"""Shared by test_cpu_trials.py / test_gpu_trials.py / test_gpu_trials_elementwise.py: the segment layouts and trial lists of the
batched-ComputeTest tests, a numpy restatement of the tile planner (gmmiv_plan_trial_tiles), the reference scores of a trial list
assembled from the oracle's DETERMINE_TOP_DISTRIBS / USE_TOP_DISTRIBS passes, the documented summation order of gmmiv_llr_trials as
numpy (piece_mean, compose) and the long double per-trial reference with its bars (trial_ref)."""
import functools

import numpy as np

import gmm_ref as gr
from conftest import make_frames, make_gmm
from oracle import oracle as orc

LEAD, TRAIL = 7, 3          # frames owned by nobody at both ends
N_MODELS = 5


def piece_layout(P):
    """segments of 0, 1, P - 1, P, P + 1, 2 P + 3 frames -> (seg_begin [7], T)"""
    sb = LEAD + np.concatenate([[0], np.cumsum([0, 1, P - 1, P, P + 1, 2 * P + 3])]).astype(np.int64)
    return sb, int(sb[-1]) + TRAIL


def trial_list(nseg, skip=None, seed=0):
    """a shuffled list: every segment but `skip` against two or three of the models, one pair twice -> (trial_seg, trial_model)"""
    rng = np.random.default_rng(seed)
    pairs = [(s, int(g)) for s in range(nseg) if s != skip for g in rng.choice(N_MODELS, size=2 + s % 2, replace=False)]
    pairs.append(pairs[len(pairs) // 2])                       # a repeated trial
    order = rng.permutation(len(pairs))
    ts = np.array([pairs[i][0] for i in order], np.int32)
    tm = np.array([pairs[i][1] for i in order], np.int32)
    return ts, tm


def plan_np(seg_begin, trial_seg, trial_model, P):
    """the tiles of gmmiv_plan_trial_tiles as tuples (lo, hi, trial, seg, model, piece), sorted by (segment, piece, position in the list)"""
    out = []
    for s in range(len(seg_begin) - 1):
        b, e = int(seg_begin[s]), int(seg_begin[s + 1])
        for k, lo in enumerate(range(b, e, P)):
            out += [(lo, min(lo + P, e), i, s, int(trial_model[i]), k) for i in range(len(trial_seg)) if trial_seg[i] == s]
    return out


def make_models(world, per_model_tables, seed=11):
    """N_MODELS client models around the world (w, mean, covinv): means moved like a MAP adaptation; with per_model_tables also their own
    weights and inverse variances -> (w [G, C] or [C], mean [G, C, D], covinv [G, C, D] or [C, D])"""
    w, mean, iv = world
    rng = np.random.default_rng(seed)
    m = mean[None] + rng.normal(0.0, 0.3, (N_MODELS,) + mean.shape)
    if not per_model_tables:
        return w, m, iv
    ww = w[None] * np.exp(rng.normal(0.0, 0.2, (N_MODELS, len(w))))
    ww /= ww.sum(1, keepdims=True)
    return ww, m, iv[None] * np.exp(rng.normal(0.0, 0.1, (N_MODELS,) + iv.shape))


def model_of(models, g):
    w, m, iv = models
    return (w[g] if w.ndim == 2 else w), m[g], (iv[g] if iv.ndim == 3 else iv)


def frame_ref(world, models, x, ctop, complete=True, lo=-200.0, hi=200.0):
    """per-frame reference on ALL rows of x: (llk_w [T], llk_c [G, T]) -- the oracle's determine-top pass on the world, its use-top pass
    per model on the world's indices and remainder"""
    x = np.asarray(x, np.float64)
    d = orc.llk_determine_top(orc.Gmm(*world), x, ctop, complete, lo, hi)
    lc = np.stack([orc.llk_use_top(orc.Gmm(*model_of(models, g)), x, d["idx"], d["nontop_lk"], complete, lo, hi) for g in range(len(models[1]))])
    return d["llk"], lc


def ref_llr(llk_w, llk_c, seg_begin, trial_seg, trial_model):
    """(llr, client_mean [ntrial], world_mean [nseg]) from the per-frame values; an empty segment gives zeros"""
    mean = lambda v, s: float(np.mean(v[seg_begin[s]:seg_begin[s + 1]])) if seg_begin[s + 1] > seg_begin[s] else 0.0
    wm = np.array([mean(llk_w, s) for s in range(len(seg_begin) - 1)])
    cm = np.array([mean(llk_c[g], s) for s, g in zip(trial_seg, trial_model)])
    return (cm - wm[np.asarray(trial_seg, int)] if len(cm) else cm), cm, wm


# ---------------------------------------------------------------- the documented summation order, and the per-trial reference
SEG_LENGTHS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 16, 17, 0, 31]      # every n mod 4, zero to eight pieces of 4, an empty segment inside


def layout_of(lengths):
    """segments of the given lengths after LEAD frames that belong to nobody, TRAIL after the last -> (seg_begin, T)"""
    sb = LEAD + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return sb, int(sb[-1]) + TRAIL


def piece_mean(values, P, defect=None):
    """include/gmmiv.h, "Sums", statement for statement in float64: a piece is P frames counted from the segment's first frame; frame
    j of a piece is added, in frame order, to partial j mod 4, each partial starting from 0.0; a piece is ((p0 + p1) + p2) + p3; the
    pieces are added in order to a sum starting from 0.0; one division by n.  An empty segment gives 0.0.
    defect (tests/test_cpu_trials.py): "swap" -- a piece as ((p0 + p2) + p1) + p3; "boundary" -- the first piece boundary at P + 4;
    "tail" -- the last frame of a piece of 4k + 1 frames added to partial 1; "reverse" -- pieces added last to first; "drop_last" --
    the last frame of a segment of 4k + 3 frames left out."""
    v = [float(a) for a in np.asarray(values, np.float64)]
    n = len(v)
    if n == 0:
        return 0.0
    used = n - 1 if defect == "drop_last" and n % 4 == 3 else n
    cuts = list(range(0, used, P))
    if defect == "boundary" and len(cuts) > 1:
        cuts = [0] + [c + 4 for c in cuts[1:] if c + 4 < used]
    sums = []
    for k, lo in enumerate(cuts):
        hi = cuts[k + 1] if k + 1 < len(cuts) else used
        p = [0.0, 0.0, 0.0, 0.0]
        for j in range(hi - lo):
            slot = 1 if defect == "tail" and (hi - lo) % 4 == 1 and j == hi - lo - 1 else j % 4
            p[slot] += v[lo + j]
        sums.append(((p[0] + p[2]) + p[1]) + p[3] if defect == "swap" else ((p[0] + p[1]) + p[2]) + p[3])
    total = 0.0
    for s in (reversed(sums) if defect == "reverse" else sums):
        total += s
    return total / n


def compose(world_vals, client_vals, seg_begin, trial_seg, trial_model, P, defect=None):
    """what gmmiv_llr_trials documents, from per-frame values: -> (llr, client_mean [ntrial], world_mean [nseg]), every mean by
    piece_mean, llr = client_mean - world_mean[seg] as one subtraction.  client_vals[g]: the per-frame values of model g.
    defect: one of piece_mean's, or ("clamp_mean", lo, hi) -- world_vals / client_vals are then UNCLAMPED and the clamp is applied to
    each mean instead of to each frame."""
    clamp_mean = isinstance(defect, tuple) and defect[0] == "clamp_mean"
    pd = None if clamp_mean else defect
    mean = lambda v, s: piece_mean(v[int(seg_begin[s]):int(seg_begin[s + 1])], P, pd)
    wm = np.array([mean(world_vals, s) for s in range(len(seg_begin) - 1)], np.float64)
    cm = np.array([mean(client_vals[int(g)], int(s)) for s, g in zip(trial_seg, trial_model)], np.float64)
    if clamp_mean:
        n = np.diff(np.asarray(seg_begin))
        wm = np.where(n > 0, np.clip(wm, defect[1], defect[2]), 0.0)
        cm = np.where(n[np.asarray(trial_seg, int)] > 0, np.clip(cm, defect[1], defect[2]), 0.0) if len(cm) else cm
    return (cm - wm[np.asarray(trial_seg, int)] if len(cm) else cm), cm, wm


def frame_refs(world_ref, client_refs, idx, complete, lo, hi):
    """the clamped long double per-frame references of the chain and their bars (tests/gmm_ref.py), on the selection idx [T, ctop]:
    -> (world (value [T], bar [T]), {g: (value [T], bar [T])}).  A zero-likelihood frame of the world (a NaN feature, or the largest
    logit not above log 2^-1075) has world value exactly lo, bar 0, and remainder -inf (include/gmmiv.h, "DEGENERATE INPUTS")."""
    dead = world_ref.dead()
    v, b = world_ref.top_llk(idx, complete)
    wv, wb = gr.clamp(v, lo, hi, b)
    wv, wb = np.where(dead, gr.LD(lo), wv), np.where(dead, 0.0, wb)
    ln, mask = world_ref.nontop(idx, dead)
    out = {}
    for g, cref in client_refs.items():
        v, b = gr.use_top(cref, idx, ln, world_ref, mask, complete)
        out[g] = gr.clamp(v, lo, hi, b)
    return (wv, wb), out


def mean_bar(v, bar, lo, hi):
    """the long double mean of v[lo:hi] and its bar (sum_t bar_t + (n + 8) u sum_t |v_t|) / n + u |mean| -- Reference.llk_sum's form,
    plus the division; an empty range gives (0, 0)"""
    n = hi - lo
    if n <= 0:
        return gr.LD(0), 0.0
    m = v[lo:hi].sum() / gr.LD(n)
    return m, (float(bar[lo:hi].sum()) + (n + 8) * gr.U * float(np.abs(v[lo:hi]).sum())) / n + gr.U * abs(float(m))


def trial_ref(world_ref, client_refs, idx, seg_begin, trial_seg, trial_model, complete, lo, hi):
    """-> dict: world_mean, client_mean, llr (long double) and world_mean_b, client_mean_b, llr_b (float64 bars) of a trial list, plus
    "frames" = frame_refs(...).  An LLR's bar is client bar + world bar + u |llr|."""
    (wv, wb), cl = frame_refs(world_ref, client_refs, idx, complete, lo, hi)
    nseg = len(seg_begin) - 1
    wm = [mean_bar(wv, wb, int(seg_begin[s]), int(seg_begin[s + 1])) for s in range(nseg)]
    cm = [mean_bar(*cl[int(g)], int(seg_begin[s]), int(seg_begin[s + 1])) for s, g in zip(trial_seg, trial_model)]
    llr = [c[0] - wm[int(s)][0] for c, s in zip(cm, trial_seg)]
    llr_b = [c[1] + wm[int(s)][1] + gr.U * abs(float(l)) for c, s, l in zip(cm, trial_seg, llr)]
    arr = lambda seq, dt: np.array(list(seq), dt)
    return {"world_mean": arr((m[0] for m in wm), gr.LD), "world_mean_b": arr((m[1] for m in wm), np.float64),
            "client_mean": arr((m[0] for m in cm), gr.LD), "client_mean_b": arr((m[1] for m in cm), np.float64),
            "llr": arr(llr, gr.LD), "llr_b": arr(llr_b, np.float64), "frames": ((wv, wb), cl)}


# ---------------------------------------------------------------- the cases of the per-trial tests
WIDE = (-1e9, 1e9)
SHAPES = [(2, 2, 1), (2, 2, 2),                  # the fast kernel with one dimension pair, lanes masked
          (37, 14, 10), (37, 14, 16),            # the fast kernel, seven dimension pairs
          (128, 60, 10),                         # the production shape: the second 16-pair batch masked
          (40, 62, 16),                          # 31 dimension pairs
          (33, 13, 10),                          # odd vectSize: the any-shape path
          (128, 60, 17), (70, 20, 64)]           # topDistribsCount > 16: the any-shape path
LONG_SHAPES = [(37, 14, 10), (128, 60, 10)]      # the shapes that also run the default-piece layout (about 1200 frames)


def lengths_of(layout, P_default):
    """"short": SEG_LENGTHS; "long": the lengths of piece_layout(P_default) with 4 P + 2 appended"""
    return list(SEG_LENGTHS) if layout == "short" else [0, 1, P_default - 1, P_default, P_default + 1, 2 * P_default + 3, 4 * P_default + 2]


@functools.lru_cache(maxsize=None)
def judged_case(C, D, dtype_str, layout="short", P_default=128):
    """world, client models (shared tables: models[False]; per-model tables: models[True]), frames, segments and the long double
    references of one (shape, dtype, layout) -- built once, never modified.  Inside the longest segment frame + 5 has a NaN feature
    and frame + 11 lies 50 sigma from Gaussian 0 in every dimension."""
    world = make_gmm(C, D, seed=C + D)
    sb, T = layout_of(lengths_of(layout, P_default))
    x = make_frames(*world, T, seed=T + D, dtype=np.dtype(dtype_str).type)
    longest = int(np.argmax(np.diff(sb)))
    a = int(sb[longest])
    x[a + 5, D // 2] = np.nan
    x[a + 11] = (world[1][0] + 50.0 / np.sqrt(world[2][0])).astype(x.dtype)
    x.setflags(write=False)
    models = {pm: make_models(world, pm) for pm in (False, True)}
    refs = {pm: {g: gr.Reference(*model_of(models[pm], g), x) for g in range(N_MODELS)} for pm in (False, True)}
    return dict(world=world, models=models, sb=sb, T=T, x=x, longest=longest, wref=gr.Reference(*world, x), crefs=refs)


def biting_clamps(cs):
    """(lo, hi): the 10th and 90th percentile of the world reference's own log-likelihoods on the usable frames of the longest
    segment -- at least three of its frames then lie above hi, three below lo, and most in between"""
    s = cs["longest"]
    v = cs["wref"].llk[int(cs["sb"][s]):int(cs["sb"][s + 1])].astype(np.float64)
    v = v[np.isfinite(v) & (v > gr.ZERO_LLK)]
    return float(np.percentile(v, 10)), float(np.percentile(v, 90))


def library_like_idx(world_ref, ctop):
    """the selection the library documents, from the reference alone (for the tests without a GPU): per frame the ctop largest
    logits, ties lowest index first; a zero-likelihood frame gets 0 .. ctop - 1"""
    return np.where(world_ref.dead()[:, None], np.arange(ctop)[None, :], world_ref.top(ctop)).astype(np.int64)


def judge_frames(tref, world_vals, client_vals):
    """ratios to the per-frame bars of tref["frames"]: {"world llk": [T], "client llk": [G, T]}"""
    (wv, wb), cl = tref["frames"]
    return {"world llk": gr.ratio(np.asarray(world_vals, np.float64).astype(gr.LD) - wv, wb),
            "client llk": np.stack([gr.ratio(np.asarray(client_vals[g], np.float64).astype(gr.LD) - cl[g][0], cl[g][1]) for g in sorted(cl)])}


def judge_trials(tref, llr, client_mean, world_mean):
    """ratios to the per-trial bars of trial_ref: {"world_mean": [nseg], "client_mean": [ntrial], "llr": [ntrial]}"""
    got = {"world_mean": world_mean, "client_mean": client_mean, "llr": llr}
    return {k: gr.ratio(np.asarray(v, np.float64).astype(gr.LD) - tref[k], tref[k + "_b"]) for k, v in got.items()}
