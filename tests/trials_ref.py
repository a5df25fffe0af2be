"""Shared by test_cpu_trials.py / test_gpu_trials.py: the segment layout and trial lists of the batched-ComputeTest tests, a numpy
restatement of the tile planner (gmmiv_plan_trial_tiles) and the reference scores of a trial list assembled from the oracle's
DETERMINE_TOP_DISTRIBS / USE_TOP_DISTRIBS passes."""
import numpy as np

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
