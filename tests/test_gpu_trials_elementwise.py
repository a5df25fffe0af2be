"""Batched ComputeTest (gmmiv_llr_trials: k_topc_use4_trials, the any-shape path, k_piece_sums_*, k_trial_reduce) and the per-frame
top-C chain behind it (gmmiv_llk_determine_top, gmmiv_llk_use_top), judged trial by trial and frame by frame.

(a) THE BITS.  include/gmmiv.h documents the order of every sum ("Sums": frame j of a piece to partial j mod 4, a piece
    ((p0 + p1) + p2) + p3, pieces in order, one division by n_s) and that the per-frame values are exactly those of the single-model
    entry points.  trials_ref.compose is that paragraph in numpy; llr, client_mean and world_mean must have ITS bits on the per-frame
    values gmmiv_llk_determine_top / gmmiv_llk_use_top return for the same frames -- no tolerance -- under "trials_piece" 4, 12 and
    the default, clamps that never bite and clamps that do, shared and per-model tables, float32 and float64 frames, COMPLETE and
    PARTIAL, on every shape of trials_ref.SHAPES; and again under "trials_scratch_mb" 0, "glds" 0, "topc_use_lanes" 1, "topc_fused" 0,
    "topc_fused" 0 + "topc_z" 0, and with x as columns of a wider device matrix and the outputs between guard bands.  Two piece
    lengths must not give the same bits everywhere (the knob does something).
    The default-piece layout (trials_ref.piece_layout with 4 P + 2 appended, about 1200 frames) runs at trials_ref.LONG_SHAPES;
    the other shapes run the default piece on the short list, where every segment is one piece.
(b) PER TRIAL.  Every world_mean[s], client_mean[i] and llr[i] against the long double means of the clamped long double per-frame
    references, each under its own bar (trials_ref.trial_ref); empty segments exactly 0.
(c) PER FRAME, in every mode the trial call can run: llk_determine_top's llk per frame, lk per selected pair, the selection, and
    llk_use_top of a shifted client, for ctop in {1, 2, 10, 16, 17, min(64, C)}, COMPLETE and PARTIAL, clamps wide and biting, on
    the defaults and under "topc_use_lanes" 1, "topc_fused" 0, "topc_fused" 0 + "topc_z" 0 (references and bars: tests/gmm_ref.py).
(d) gmmiv_trial_piece: what it answers for valid and invalid "trials_piece", and that an invalid value computes with the default.

The library's own selection is judged first (selection_shortfall) and then used by the references, as in
test_gpu_gmm_elementwise.run_top; its output never sets a bar.  No trial, segment or frame of a case is left out.  The biting
clamps are the 10th and 90th percentile of the reference's own per-frame values; that they bite on both sides and leave most frames
alone is asserted from the reference alone (here for (c), in tests/test_cpu_trials_ref.py for the layouts of (a) and (b)).

A failure names case, option path, entry point, kind and the first offending unit.  With TRIALS_ERRORS_JSON set to a path the
largest ratio per (case, path, entry point, kind) is written there (profiles/r19/trials_errors.json).
"""
import functools
import json
import os
import time

import numpy as np
import pytest

import elementwise_judge as ej
import gmm_ref as gr
import trials_ref as tr
from elementwise_judge import Guarded, options, path_name

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300), pytest.mark.skipif(not gr.HAVE_LONGDOUBLE, reason=gr.SKIP_MESSAGE)]

LD = gr.LD
RATIOS = {}
SECONDS = []
CLIENT_SHIFT = 5
G = tr.N_MODELS


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    c = capi.Context(0)
    yield c
    c.close()
    _H.clear()
    path = os.environ.get("TRIALS_ERRORS_JSON")
    if path and RATIOS:
        per = {}
        for (case, p, entry, kind), v in RATIOS.items():
            for key in ("path: " + p, "entry: %s, %s" % (entry, kind)):
                per[key] = max(per.get(key, 0.0), v)
        with open(path, "w") as f:
            json.dump({"bound": "tests/gmm_ref.py per frame: share-weighted rho = (2D + 16) u S of the logits in the sum + 4u |llk| + 4u (COMPLETE: "
                                "with the world's remainder; PARTIAL: without); tests/trials_ref.py per trial: (sum_t bar_t + (n + 8) u sum_t |llk_t|) / n "
                                "+ u |mean|, an LLR client bar + world bar + u |llr|; the composition itself is held to the bits of trials_ref.compose",
                       "tests": len(SECONDS), "seconds": float("%.1f" % sum(SECONDS)), "max_ratio": float("%.4g" % max(RATIOS.values())),
                       "worst": {k: float("%.4g" % v) for k, v in sorted(per.items())},
                       "entries": {" | ".join(k): float("%.4g" % v) for k, v in sorted(RATIOS.items())}}, f, indent=1)


@pytest.fixture(autouse=True)
def _clock():
    t = time.perf_counter()
    yield
    SECONDS.append(time.perf_counter() - t)


def Judge(case, path="defaults"):
    return ej.Judge(case, path, RATIOS)


def shape_name(shape):
    return "%dx%d_top%d" % shape


def mode_name(complete):
    return "complete" if complete else "partial"


# ---------------------------------------------------------------- handles, built once per module
_H = {}


def handles(ctx, C, D, per_model):
    """the world handle, the batch of the five clients and a single-model handle per client"""
    key = (C, D, per_model)
    if key not in _H:
        cs = tr.judged_case(C, D, "float32")
        models = cs["models"][per_model]
        if (C, D) not in _H:
            _H[(C, D)] = ctx.gmm(*cs["world"])
        _H[key] = dict(world=_H[(C, D)], batch=ctx.gmm_batch(G, C, D).load(*models), one=[ctx.gmm(*tr.model_of(models, g)) for g in range(G)])
    return _H[key]


def per_frame(h, x, ctop, complete, lo, hi):
    """the per-frame values of the single-model entry points on the frames x: the world's determine-top pass and every client's
    use-top pass on the world's indices and remainder"""
    d = h["world"].llk_determine_top(x, ctop, complete, lo, hi)
    return d, {g: h["one"][g].llk_use_top(x, d["idx"], d["nontop_llk"], complete, lo, hi) for g in range(G)}


def same_as_composition(j, what, got, d, rows, sb, ts, tm, P):
    want = tr.compose(d["llk"], rows, sb, ts, tm, P)
    for name, a, b in zip(("llr", "client_mean", "world_mean"), got, want):
        j.same_bits("%s, %s" % (name, what), a, b, "the documented composition of the per-frame values")


def layouts_of(shape):
    return ("short", "long") if shape in tr.LONG_SHAPES else ("short",)


def case_of(shape, dtype, layout):
    from lia_ral_amd import capi
    return tr.judged_case(shape[0], shape[1], gr.dtype_name(dtype), layout, capi.TRIAL_PIECE)


def clamps_of(cs):
    return (("wide", tr.WIDE), ("biting", tr.biting_clamps(cs)))


def valid_selection(j, entry, ref, d, ctop, w=None):
    """indices inside the model and distinct per frame; a zero-likelihood frame 0 .. ctop - 1 with likelihoods exactly 0 and
    nontop_w = 1 - w_0 - ... - w_{ctop - 1} (ctop subtractions from 1: ctop u; include/gmmiv.h, "DEGENERATE INPUTS"); every other
    frame's j-th selected logit no further below the j-th largest than the two logits' errors -> the selection as int64, or None"""
    idx = d["idx"].astype(np.int64)
    bad = [t for t, r in enumerate(idx.tolist()) if len(set(r)) != ctop or min(r) < 0 or max(r) >= ref.C] if idx.shape == (ref.T, ctop) else [-1]
    if bad:
        j.note(entry, "indices outside the model or repeated in a row, at %d frames, first frame %d: %r" % (len(bad), bad[0], idx[bad[0]].tolist() if bad[0] >= 0 else idx.shape))
        return None
    dead = ref.dead()
    if not np.array_equal(idx[dead], np.broadcast_to(np.arange(ctop), (int(dead.sum()), ctop))):
        j.note(entry, "a zero-likelihood frame does not select 0 .. ctop - 1")
    if dead.any():
        j(entry, "zero-likelihood frame lk", gr.ratio(d["lk"][dead], 0.0))
        if w is not None:
            j(entry, "zero-likelihood frame nontop_w", gr.ratio(d["nontop_w"][dead].astype(LD) - (LD(1) - np.asarray(w[:ctop], LD).sum()), ctop * gr.U))
    short, slack = ref.selection_shortfall(np.where(dead[:, None], ref.top(ctop), idx))
    j(entry, "selection", gr.ratio(np.where(dead[:, None], 0.0, short), slack))
    return idx


# ---------------------------------------------------------------- (a) the bits of the composition
TRIAL_PARAMS = [pytest.mark.parametrize("complete", [True, False], ids=mode_name), pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name),
                pytest.mark.parametrize("shape", tr.SHAPES, ids=shape_name)]


def trial_params(f):
    for p in TRIAL_PARAMS:
        f = p(f)
    return f


@trial_params
def test_the_results_have_the_bits_of_the_documented_composition(ctx, shape, dtype, complete):
    from lia_ral_amd import capi
    C, D, ctop = shape
    j = Judge("%s %s %s" % (shape_name(shape), gr.dtype_name(dtype), mode_name(complete)))
    moved = False
    for layout in layouts_of(shape):
        cs = case_of(shape, dtype, layout)
        sb, x = cs["sb"], cs["x"]
        n = np.diff(sb)
        ts, tm = tr.trial_list(len(sb) - 1, skip=3)
        for cname, (lo, hi) in clamps_of(cs):
            for per_model in (False, True):
                h = handles(ctx, C, D, per_model)
                d, rows = per_frame(h, x, ctop, complete, lo, hi)
                res = {}
                for P in ((4, 12, 0) if layout == "short" else (0,)):
                    with options(ctx, {"trials_piece": P} if P else {}):
                        res[P] = h["batch"].llr_trials(h["world"], x, sb, ts, tm, ctop, complete, lo, hi)
                    what = "%s layout, P %s, %s clamps, %s tables" % (layout, P or "default", cname, "per-model" if per_model else "shared")
                    same_as_composition(j, what, res[P], d, rows, sb, ts, tm, P or capi.TRIAL_PIECE)
                if layout == "short":          # segments longer than both pieces: the two summation orders must show somewhere
                    moved |= bool(np.any(res[4][2][n > 12] != res[12][2][n > 12]) or np.any(res[4][1][n[ts] > 12] != res[12][1][n[ts] > 12]))
    if not moved:
        j.note("trials_piece", "pieces of 4 and of 12 frames gave the same bits on every segment longer than both")
    j.finish()


VARIANTS = ({"trials_scratch_mb": 0}, {"glds": 0}, {"topc_use_lanes": 1}, {"topc_fused": 0}, {"topc_fused": 0, "topc_z": 0})


@trial_params
def test_the_bits_hold_on_every_option_path(ctx, shape, dtype, complete):
    """each path against the per-frame entry points under the same options (so "topc_use_lanes" 1 composes k_topc_use16's values and
    the unfused world passes their own), pieces of 4 and of 12 frames, per-model tables, both clamps"""
    C, D, ctop = shape
    cs = case_of(shape, dtype, "short")
    sb, x = cs["sb"], cs["x"]
    ts, tm = tr.trial_list(len(sb) - 1, skip=3)
    h = handles(ctx, C, D, True)
    bad = []
    for opts in VARIANTS:
        j = Judge("%s %s %s" % (shape_name(shape), gr.dtype_name(dtype), mode_name(complete)), path_name(opts))
        for (cname, (lo, hi)), P in zip(clamps_of(cs), (4, 12)):
            with options(ctx, dict(opts, trials_piece=P)):
                d, rows = per_frame(h, x, ctop, complete, lo, hi)
                got = h["batch"].llr_trials(h["world"], x, sb, ts, tm, ctop, complete, lo, hi)
            same_as_composition(j, "P %d, %s clamps" % (P, cname), got, d, rows, sb, ts, tm, P)
        bad += j.bad
    assert not bad, "%d comparisons failed:\n" % len(bad) + "\n".join(bad[:30])


@trial_params
def test_the_bits_hold_on_a_wider_device_matrix_between_guard_bands(ctx, shape, dtype, complete):
    """x as the first D columns of a device matrix of D + 5 (the filler must never be read), llr / client_mean / world_mean as device
    arrays filled with a sentinel between two guard bands: the bands stay intact, every element is written -- also the world mean of
    the segment no trial names -- and the bits are those of the composition"""
    import torch
    C, D, ctop = shape
    cs = case_of(shape, dtype, "short")
    sb, x = cs["sb"], cs["x"]
    ts, tm = tr.trial_list(len(sb) - 1, skip=3)
    assert 3 not in ts
    h = handles(ctx, C, D, True)
    wide = torch.full((cs["T"], D + 5), 1e30, dtype=torch.float32 if x.dtype == np.float32 else torch.float64, device="cuda")
    wide[:, :D] = torch.from_numpy(np.array(x)).cuda()           # (a copy: the cached frames are read-only)
    xv = wide[:, :D]
    torch.cuda.synchronize()
    assert xv.stride(0) == D + 5
    j = Judge("%s %s %s ldx=D+5" % (shape_name(shape), gr.dtype_name(dtype), mode_name(complete)))
    for (cname, (lo, hi)), P in zip(clamps_of(cs), (12, 4)):
        out = [Guarded((len(ts),), fill=None), Guarded((len(ts),), fill=None), Guarded((len(sb) - 1,), fill=None)]
        with options(ctx, {"trials_piece": P}):
            d, rows = per_frame(h, xv, ctop, complete, lo, hi)
            h["batch"].llr_trials(h["world"], xv, sb, ts, tm, ctop, complete, lo, hi, llr=out[0].view, client_mean=out[1].view, world_mean=out[2].view)
            ctx.sync()
        got = [o.read(j, name) for o, name in zip(out, ("llr", "client_mean", "world_mean"))]
        same_as_composition(j, "device, P %d, %s clamps" % (P, cname), got, d, rows, sb, ts, tm, P)
    j.finish()


# ---------------------------------------------------------------- (b) per trial against long double
B_CASES = [(s, "short") for s in tr.SHAPES] + [(s, "long") for s in tr.LONG_SHAPES]


@pytest.mark.parametrize("complete", [True, False], ids=mode_name)
@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("shape,layout", B_CASES, ids=lambda v: v if isinstance(v, str) else shape_name(v))
def test_every_trial_and_segment_against_long_double(ctx, shape, layout, dtype, complete):
    C, D, ctop = shape
    cs = case_of(shape, dtype, layout)
    sb, x = cs["sb"], cs["x"]
    ts, tm = tr.trial_list(len(sb) - 1, skip=3)
    empty = np.diff(sb) == 0
    assert empty.sum() >= 1 and empty[ts].any()
    j = Judge("%s %s %s %s" % (shape_name(shape), layout, gr.dtype_name(dtype), mode_name(complete)))
    for cname, (lo, hi) in clamps_of(cs):
        for per_model in (False, True):
            h = handles(ctx, C, D, per_model)
            with options(ctx, {"trials_piece": 4} if layout == "short" else {}):
                llr, cm, wm = h["batch"].llr_trials(h["world"], x, sb, ts, tm, ctop, complete, lo, hi)
            d = h["world"].llk_determine_top(x, ctop, complete, lo, hi)
            idx = valid_selection(j, "determine_top " + mode_name(complete), cs["wref"], d, ctop, cs["world"][0])
            if idx is None:
                continue
            tref = tr.trial_ref(cs["wref"], cs["crefs"][per_model], idx, sb, ts, tm, complete, lo, hi)
            entry = "llr_trials %s %s" % (mode_name(complete), cname)
            for kind, r in tr.judge_trials(tref, llr, cm, wm).items():
                j(entry, kind, r)
            j(entry, "empty segment", gr.ratio(np.concatenate([wm[empty], cm[empty[ts]], llr[empty[ts]]]), 0.0))
    j.finish()


# ---------------------------------------------------------------- (c) the per-frame chain in every mode
C_CASES = gr.PATH_CASES + ((16, 13, 16, 2.0), (40, 61, 66, 2.0))
C_PATHS = ({}, {"topc_use_lanes": 1}, {"topc_fused": 0}, {"topc_fused": 0, "topc_z": 0})


def ctops_of(C):
    return sorted(c for c in {1, 2, 10, 16, 17, min(64, C)} if 1 <= c <= C)


@functools.lru_cache(maxsize=None)
def frame_clamps(case, dtype_str, ctop, complete):
    """the biting clamps of a (case, ctop, mode): the 10th and 90th percentile of the world reference's own per-frame values on its
    own selection; asserted from the references alone: both bite, for the world and for the client, and most frames stay unclamped"""
    ref, cref = gr.reference(case, dtype_str), gr.reference(case, dtype_str, CLIENT_SHIFT)
    idx = ref.top(ctop)
    w = ref.top_llk(idx, complete)[0].astype(np.float64)
    lo, hi = float(np.percentile(w, 10)), float(np.percentile(w, 90))
    ln, mask = ref.nontop(idx)
    c = gr.use_top(cref, idx, ln, ref, mask, complete)[0].astype(np.float64)
    for v in (w, c):
        assert (v < lo).any() and (v > hi).any() and ((v >= lo) & (v <= hi)).mean() > 0.5, (case, ctop, complete)
    return lo, hi


@pytest.mark.parametrize("opts", C_PATHS, ids=lambda o: path_name(o).replace(" ", "_"))
@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("case", C_CASES, ids=gr.case_name)
def test_the_per_frame_chain_in_every_mode_of_the_trial_call(ctx, case, dtype, opts):
    dn = gr.dtype_name(dtype)
    ref, cref = gr.reference(case, dn), gr.reference(case, dn, CLIENT_SHIFT)
    assert not ref.dead().any()
    x = gr.frames(case, dtype)
    g, client = ctx.gmm(*gr.model(case)), ctx.gmm(*gr.model(case, CLIENT_SHIFT))
    j = Judge("%s %s" % (gr.case_name(case), dn), path_name(opts))
    with options(ctx, opts):
        for ctop in ctops_of(ref.C):
            for complete in (True, False):
                for cname, (lo, hi) in (("wide", tr.WIDE), ("biting", frame_clamps(case, dn, ctop, complete))):
                    before = len(j.bad)
                    d = g.llk_determine_top(x, ctop, complete, lo, hi)
                    entry = "determine_top " + mode_name(complete)
                    idx = valid_selection(j, entry, ref, d, ctop)
                    if idx is not None:
                        v, b = ref.top_llk(idx, complete)
                        v, b = gr.clamp(v, lo, hi, b)
                        j(entry, "llk", gr.ratio(d["llk"].astype(LD) - v, b))
                        lk, lkb = ref.selected_lk(idx)
                        j(entry, "lk", gr.ratio(d["lk"].astype(LD) - lk, lkb))
                        ln, mask = ref.nontop(idx)
                        v, b = gr.use_top(cref, idx, ln, ref, mask, complete)
                        v, b = gr.clamp(v, lo, hi, b)
                        j("use_top " + mode_name(complete), "llk", gr.ratio(client.llk_use_top(x, d["idx"], d["nontop_llk"], complete, lo, hi).astype(LD) - v, b))
                    if len(j.bad) > before:
                        j.note(entry, "the failures above: ctop %d, %s clamps (%r, %r)" % (ctop, cname, lo, hi))
    client.close(); g.close()
    j.finish()


# ---------------------------------------------------------------- (d) gmmiv_trial_piece
def test_trial_piece_answers_the_piece_in_effect_and_an_invalid_value_means_the_default(ctx):
    from lia_ral_amd import capi
    assert ctx.trial_piece() == capi.TRIAL_PIECE
    for v in (0, 2, 6, -4, 2 ** 31):
        with options(ctx, {"trials_piece": v} if v else {}):
            assert ctx.trial_piece() == capi.TRIAL_PIECE, v
    for v in (4, 12, 132):
        with options(ctx, {"trials_piece": v}):
            assert ctx.trial_piece() == v
    assert ctx.trial_piece() == capi.TRIAL_PIECE
    shape = (37, 14, 10)
    cs = case_of(shape, np.float32, "long")
    ts, tm = tr.trial_list(len(cs["sb"]) - 1, skip=3)
    h = handles(ctx, 37, 14, True)
    run = lambda: h["batch"].llr_trials(h["world"], cs["x"], cs["sb"], ts, tm, 10, True, -200.0, 200.0)
    base = run()
    j = Judge("%s float32 complete long" % shape_name(shape), "trials_piece")
    for v in (2, 6, -4, 2 ** 31):
        with options(ctx, {"trials_piece": v}):
            for name, a, b in zip(("llr", "client_mean", "world_mean"), run(), base):
                j.same_bits("%s under trials_piece %d" % (name, v), a, b, "the default piece")
    with options(ctx, {"trials_piece": 132}):                    # a valid value that is not the default does change the bits
        other = run()
    if all(np.array_equal(a, b) for a, b in zip(other, base)):
        j.note("trials_piece 132", "the same bits as the default piece on every trial and segment")
    j.finish()
