"""Everything downstream of the i-vector -- the scoring rules (gmmiv_score_cosine / _mahalanobis / _twocov / _twocov_mix_part / _plda,
gmmiv_score_apply_trials), gmmiv_iv_normalize, the development-set statistics (gmmiv_dev_means / _cov_mat / _scatter_mat), the JFA
steps (gmmiv_jfa_subtract / _subtract_sessions / _estimate_z / _estimate_z_and_d) and the approximate extractors
(gmmiv_tv_norm_statistics / _subtract_m_plus_tw / _norm_t / _weighted_cov / _approximate_tctc / _estimate_w_ubm_weight / _eigen) --
judged per trial, per element and per utterance against the 80-bit restatement and the bars of tests/backend_ref.py, never against
the largest entry of an array (that is tests/test_gpu_tv.py, which stays).

What runs here for the first time: the second and later iterations of the tv_batch loops (tv_batch 4: r0 > 0 in k_gather_rows and
k_jfa_sub, the [h0, h1) windows of gmmiv_jfa_subtract_sessions with a speaker that spans three of them and empty speakers at a
window's front, the u0 > 0 accumulation of both approximate extractors, ragged last batches), an odd R in the approximate
extractors, the pad columns of ScoreArgs::even_stride, of the run gather of gmmiv_score_plda and of Y in quad_score with NaN left
in them by the call before, one device tensor as models and segments, the FTJF cache of the context across two models, the device
path of the owner map.  Device results live between guard bands that must come back untouched.

A failure names case, option path, entry point, unit kind, the first offending unit and its ratio to the bar.  With
BACKEND_ERRORS_JSON set to a path the largest ratio per (case, path, entry point, unit kind) is written there, with the relative
accuracy the target trials reach under the expansion (profiles/r16/backend_errors.json).
"""
import json
import os

import numpy as np
import pytest

import backend_ref as br
import elementwise_judge as ej
from elementwise_judge import SENTINEL, Guarded, options, path_name

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300), pytest.mark.skipif(not br.HAVE_LONGDOUBLE, reason=br.SKIP_MESSAGE)]

RATIOS = {}
TARGETS = {}          # (rule, dim) -> the largest |error| / |score| over the target trials
NOTES = {}


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    c = capi.Context(0)
    yield c
    c.close()
    path = os.environ.get("BACKEND_ERRORS_JSON")
    if path and RATIOS:
        per = {}
        for (case, p, entry, kind), v in RATIOS.items():
            for key in ("path: " + p, "entry: " + entry.split(" [")[0]):
                per[key] = max(per.get(key, 0.0), v)
        with open(path, "w") as f:
            json.dump({"bound": "tests/backend_ref.py: scoring per trial 2 (dim + 8) u S_ms; PLDA (2 (rf + 8) + 4 rf kappa) u S_q + 8 rf u max(S_c, 1); "
                                "iv_normalize, dev set, JFA, approximate extractors per element; estimate_w_ubm_weight / _eigen per utterance "
                                "16 max(err_oracle_u, 64 u)",
                       "max_ratio": float("%.4g" % max(RATIOS.values())), "worst": {k: float("%.4g" % v) for k, v in sorted(per.items())},
                       "target_trials_relative_error": {"%s dim %d" % k: float("%.3g" % v) for k, v in sorted(TARGETS.items())},
                       "notes": NOTES, "entries": {" | ".join(k): float("%.4g" % v) for k, v in sorted(RATIOS.items())}}, f, indent=1)


def Judge(case, path="defaults"):
    return ej.Judge(case, path, RATIOS)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- scoring
def run_rule(ctx, rule, p, m, s, out, which="FTJF"):
    """one scoring call; m, s: numpy arrays or device tensors; out: numpy array or device view (mix_part: holds C_in)"""
    if rule == "cosine":
        return ctx.score_cosine(m, s, out=out)
    if rule == "mahalanobis":
        return ctx.score_mahalanobis(m, s, p["Mah"], out=out)
    if rule == "twocov":
        return ctx.score_twocov(m, s, p["G"], p["H"], out=out)
    if rule == "mix_part":
        return ctx.score_twocov_mix_part(m, s, p["G"], out)
    return ctx.score_plda(m, p["nsess"], s, p[which], out=out)


def score_both_ways(ctx, j, key, rule, which="FTJF", tag=""):
    """host arrays, then device tensors with the result between guard bands -> the device result"""
    p = br.score_case(*key)
    ref, bar = br.score_reference(key, rule, which)
    mv = p["msum"] if rule == "plda" else p["m"]
    M, S = p["M"], p["S"]
    host = run_rule(ctx, rule, p, mv, p["s"], p["C_in"].copy() if rule == "mix_part" else np.full((M, S), SENTINEL), which)
    j(rule + tag + " [host]", "trial", br.ratio(br.ld(host) - ref, bar))
    g = Guarded((M, S), None, init=p["C_in"] if rule == "mix_part" else None)
    md = dev(mv)
    sd = md if p["s"] is p["m"] else dev(p["s"])              # the self-scoring case: ONE device tensor on both sides
    run_rule(ctx, rule, p, md, sd, g.view, which)
    ctx.sync()
    got = g.read(j, rule + tag + " [device]")
    j(rule + tag + " [device]", "trial", br.ratio(br.ld(got) - ref, bar))
    return got


@pytest.mark.parametrize("counts", br.SCORE_COUNTS, ids=lambda c: "%dx%d" % c)
@pytest.mark.parametrize("dim", br.SCORE_DIMS)
def test_scoring_rules_per_trial(ctx, dim, counts):
    M, S = counts
    j = Judge("score %dx%dx%d" % (dim, M, S))
    for rule in br.RULES:
        key = (dim, M, S, "cosine" if rule == "cosine" else "plain")
        got = score_both_ways(ctx, j, key, rule)
        TARGETS[(rule, dim)] = max(TARGETS.get((rule, dim), 0.0), br.target_accuracy(key, rule, got))
    j.finish()


def test_scoring_one_device_tensor_as_models_and_segments(ctx):
    key = (33, 33, 33, "self")
    j = Judge("score 33x33x33 models == segs")
    for rule in br.RULES:
        score_both_ways(ctx, j, key, rule)
    j.finish()


@pytest.mark.parametrize("rule", br.RULES)
def test_scores_do_not_depend_on_what_the_scratch_held(rule):
    """odd M and odd S: both vector matrices are copied into blocks with one pad column per row, and so are the PLDA runs and Y.
    A call of the same rule on a larger odd shape with NaN for every vector leaves NaN where those pads land; the scores must be
    the bits a fresh context gives.  (NaN is data here: no call fails.)"""
    from lia_ral_amd import capi
    key = (33, 33, 31, "cosine" if rule == "cosine" else "plain")
    p = br.score_case(*key)
    big = dict(br.score_case(33, 45, 47, "plain"))
    mv = p["msum"] if rule == "plda" else p["m"]
    j = Judge("score 33x33x31 after NaN " + rule)
    outs = []
    for dirty in (False, True):
        c = capi.Context(0)
        try:
            if dirty:
                nan_m, nan_s = np.full((33, 45), np.nan), np.full((33, 47), np.nan)
                junk = run_rule(c, rule, big, nan_m, nan_s, np.zeros((45, 47)))
                assert np.isnan(junk).all()
            outs.append(run_rule(c, rule, p, mv, p["s"], p["C_in"].copy() if rule == "mix_part" else np.full((33, 31), SENTINEL)))
        finally:
            c.close()
    j.same_bits(rule, outs[1], outs[0], "the same call on a fresh context")
    ref, bar = br.score_reference(key, rule)
    j(rule + " [host]", "trial", br.ratio(br.ld(outs[1]) - ref, bar))
    j.finish()


@pytest.mark.parametrize("counts", list(br.PLDA_COUNTS))
def test_plda_session_counts_and_a_change_of_model(ctx, counts):
    """runs of equal session counts (odd runs, a run that starts at an odd index, n = 50), then a second FTJF of the same size on the
    same context against its own reference -- a K_n kept from the first model fails -- then the first again: the bits of the first"""
    ns = br.PLDA_COUNTS[counts]
    key = (40 if len(ns) > 1 else 5, len(ns), 7, "plda " + counts)
    j = Judge("plda %s" % counts)
    first = score_both_ways(ctx, j, key, "plda", "FTJF", " first model")
    score_both_ways(ctx, j, key, "plda", "FTJF2", " second model")
    again = score_both_ways(ctx, j, key, "plda", "FTJF", " first model again")
    j.same_bits("plda first model again", again, first, "the first call")
    j.finish()


def test_apply_trials_on_top_of_two_rules(ctx):
    key = (33, 33, 31, "plain")
    p = br.score_case(*key)
    rng = np.random.default_rng(3)
    trials = rng.random((33, 31)) < 0.3
    j = Judge("apply_trials 33x33x31")
    for rule, fill in (("cosine", 0.0), ("mahalanobis", -7.5)):
        g = Guarded((33, 31), None)
        md, sd, td = dev(p["m"]), dev(p["s"]), dev(trials.astype(np.uint8))   # alive until the sync: the calls are asynchronous
        run_rule(ctx, rule, p, md, sd, g.view)
        ctx.sync()
        before = g.read(j, rule)
        ctx.score_apply_trials(td, g.view, fill)
        ctx.sync()
        after = g.read(j, rule + " masked")
        host = ctx.score_apply_trials(trials, before.copy(), fill)
        for name, a in (("device", after), ("host", host)):
            if not np.all(a[~trials] == fill):
                j.note(rule, "%s: a masked cell is not the fill value" % name)
            j.same_bits(rule + " " + name, a[trials], before[trials], "the scores before the mask")
    j.finish()


# ---------------------------------------------------------------- iv_normalize
@pytest.mark.parametrize("shape", br.IVN_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_iv_normalize_per_element(ctx, shape):
    din, dout, n = shape
    p = br.ivn_inputs(*shape)
    j = Judge("iv_normalize %dx%dx%d" % shape)
    for mean, M, ln in br.IVN_FORMS:
        mu, Mx = (p["mean"] if mean else None), (p["M"] if M else None)
        do = dout if M else din
        ref, bar = br.ivn_reference(p["X"], mu, Mx, ln)
        tag = "iv_normalize mean %d M %d length_norm %d" % (bool(mean), bool(M), ln)
        j(tag + " [host]", "element", br.ratio(br.ld(ctx.iv_normalize(p["X"], mu, Mx, ln, out=np.full((do, n), SENTINEL))) - ref, bar))
        g, Xd = Guarded((do, n), None), dev(p["X"])
        ctx.iv_normalize(Xd, mu, Mx, ln, out=g.view)
        ctx.sync()
        j(tag + " [device]", "element", br.ratio(br.ld(g.read(j, tag + " [device]")) - ref, bar))
        if not M:                                               # the output in the tensor of the input (the header allows it without a rotation)
            g = Guarded((din, n), init=p["X"])
            ctx.iv_normalize(g.view, mu, Mx, ln, out=g.view)
            ctx.sync()
            j(tag + " [device in place]", "element", br.ratio(br.ld(g.read(j, tag + " [device in place]")) - ref, bar))
    j.finish()


def test_iv_normalize_columns_of_tiny_norm(ctx):
    """norm 1e-150 (squared: a normal double) is normalised like any column.  norm 1e-170: the squared norm is 0 in double; the
    reference project's lengthNorm (double sum, sqrt, division) divides by 0, the oracle does, and so does the library: no finite
    entry in that column, where the 80-bit reference holds a unit vector.  The library follows the reference project."""
    from oracle import oracle as orc
    X = br.ivn_tiny_columns()
    ref, bar = br.ivn_reference(X, None, None, True)
    o = orc.iv_normalize(X, None, None, True)
    fin = [k for k in range(X.shape[1]) if k != 5]
    j = Judge("iv_normalize tiny columns")
    g, Xd = Guarded(X.shape, None), dev(X)
    ctx.iv_normalize(Xd, None, None, True, out=g.view)
    ctx.sync()
    for name, got in (("host", ctx.iv_normalize(X, None, None, True)), ("device", g.read(j, "device"))):
        j("iv_normalize length_norm [%s]" % name, "element", br.ratio(br.ld(got)[:, fin] - ref[:, fin], bar[:, fin]))
        NOTES["iv_normalize column of norm 1e-170, " + name] = "library %s, oracle %s, 80-bit reference finite" % (
            "finite" if np.isfinite(got[:, 5]).all() else "not finite", "finite" if np.isfinite(o[:, 5]).all() else "not finite")
        if np.isfinite(got[:, 5]).any() != np.isfinite(o[:, 5]).any():
            j.note(name, "the column whose squared norm underflows: %r, the oracle has %r" % (got[:, 5].tolist(), o[:, 5].tolist()))
    j.finish()


# ---------------------------------------------------------------- development set
@pytest.mark.parametrize("name", list(br.DEV_CASES))
def test_dev_set_statistics_per_element(ctx, name):
    X, sps = br.dev_inputs(name)
    j = Judge("dev " + name)
    for where, Xa in (("host", X), ("device", dev(X))):
        mean, sm = ctx.dev_means(Xa, sps)
        S, W, B = ctx.dev_cov_mat(Xa, sps)
        SB, SW = ctx.dev_scatter_mat(Xa, sps)
        for q, r in br.dev_judge(name, {"mean": mean, "smean": sm, "Sigma": S, "W": W, "B": B, "SB": SB, "SW": SW}).items():
            entry = "dev_means" if q in ("mean", "smean") else "dev_cov_mat" if q in ("Sigma", "W", "B") else "dev_scatter_mat"
            j("%s [%s]" % (entry, where), q + " element", r)
    j.finish()


# ---------------------------------------------------------------- JFA
BATCHES = ({"tv_batch": 4}, {})
# the 24 sessions are six full windows of 4: tv_batch 5 ends the session loop (and the 24-row forms of jfa_subtract) in a short window
JFA_BATCHES = tuple({"tv_batch": b} for b in br.JFA_BATCHES) + ({},)


@pytest.mark.parametrize("opts", JFA_BATCHES, ids=path_name)
@pytest.mark.parametrize("shape", br.JFA_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_jfa_steps_per_element(ctx, shape, opts):
    p = br.jfa_inputs(*shape)
    C, D = p["C"], p["D"]
    j = Judge("jfa %dx%dx%d" % shape, path_name(opts))
    dv = {k: dev(p[k]) for k in ("N", "F", "Nh", "Um", "X", "iv")}       # device inputs stay alive until the sync of their call
    with options(ctx, opts):
        for form in br.JFA_SUBTRACT_FORMS:
            N, F, kw = br.jfa_subtract_args(p, form)
            ref, bar = br.jfa_subtract_reference(N, F, D, **kw)
            j("jfa_subtract " + form + " [host]", "element", br.ratio(br.ld(ctx.jfa_subtract(N, F.copy(), C, D, **kw)) - ref, bar))
            g = Guarded(F.shape, init=F)
            kd = dict(kw)
            if "owner" in kd:
                kd["owner"] = dev(kd["owner"])                   # the owner map on the device: the path that is not range-checked
            ctx.jfa_subtract(dv["N"] if N is p["N"] else dv["Nh"], g.view, C, D, **kd)
            ctx.sync()
            j("jfa_subtract " + form + " [device]", "element", br.ratio(br.ld(g.read(j, "jfa_subtract " + form)) - ref, bar))
        ref, bar = br.jfa_sessions_reference(p)
        j("jfa_subtract_sessions [host]", "element",
          br.ratio(br.ld(ctx.jfa_subtract_sessions(p["sb"], p["Nh"], p["F"].copy(), p["Um"], p["X"], C, D)) - ref, bar))
        g = Guarded(p["F"].shape, init=p["F"])
        ctx.jfa_subtract_sessions(p["sb"], dv["Nh"], g.view, dv["Um"], dv["X"], C, D)
        ctx.sync()
        j("jfa_subtract_sessions [device]", "element", br.ratio(br.ld(g.read(j, "jfa_subtract_sessions")) - ref, bar))
        for tau in (-1.0, 14.0):
            ref, bar = br.jfa_z_reference(p, tau)
            g = Guarded(p["F"].shape, None)
            ctx.jfa_estimate_z(p["N"], p["F"], p["iv"], p["Dm"], C, D, tau=tau, out=g.view)
            ctx.sync()
            j("jfa_estimate_z tau %g [device]" % tau, "element", br.ratio(br.ld(g.read(j, "jfa_estimate_z")) - ref, bar))
            j("jfa_estimate_z tau %g [host]" % tau, "element", br.ratio(br.ld(ctx.jfa_estimate_z(p["N"], p["F"], p["iv"], p["Dm"], C, D, tau=tau)) - ref, bar))
        z, zbar, d, dbar = br.jfa_zd_reference(p)
        Dg = p["Dm"].copy()
        Zg = ctx.jfa_estimate_z_and_d(p["N"], p["F"], p["iv"], Dg, C, D)
        j("jfa_estimate_z_and_d [host]", "Z element", br.ratio(br.ld(Zg) - z, zbar))
        j("jfa_estimate_z_and_d [host]", "D element", br.ratio(br.ld(Dg) - d, dbar))
        gz, gd = Guarded(p["F"].shape, None), Guarded(p["Dm"].shape, init=p["Dm"])
        ctx.jfa_estimate_z_and_d(dv["N"], dv["F"], dv["iv"], gd.view, C, D, out=gz.view)
        ctx.sync()
        j("jfa_estimate_z_and_d [device]", "Z element", br.ratio(br.ld(gz.read(j, "z_and_d Z")) - z, zbar))
        j("jfa_estimate_z_and_d [device]", "D element", br.ratio(br.ld(gd.read(j, "z_and_d D")) - d, dbar))
    j.finish()


# ---------------------------------------------------------------- approximate extractors
@pytest.mark.parametrize("opts", BATCHES, ids=path_name)
@pytest.mark.parametrize("shape", br.AX_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_approximate_extractors_per_element_and_per_utterance(ctx, shape, opts):
    a = br.approx(*shape)
    U, C, D, R = shape
    j = Judge("approx %dx%dx%dx%d" % shape, path_name(opts))
    names = {"Fn": "tv_norm_statistics", "Fs": "tv_subtract_m_plus_tw", "Tn": "tv_norm_t", "Wm": "tv_weighted_cov", "Dm": "tv_approximate_tctc"}
    rng = np.random.default_rng(U + R)
    start_w = rng.normal(size=(U, R))
    start_d = rng.uniform(0.5, 2.0, (C, R))
    with options(ctx, opts):
        got = {"Fn": ctx.tv_norm_statistics(a.N, a.F.copy(), a.means, a.iv, C, D), "Fs": ctx.tv_subtract_m_plus_tw(a.N, a.F.copy(), a.means, a.T, a.Wv, C, D),
               "Tn": ctx.tv_norm_t(a.T.copy(), a.iv, C, D), "Wm": ctx.tv_weighted_cov(a.Tn, a.weight, C, D), "Dm": ctx.tv_approximate_tctc(a.Tn, a.Q, C, D)}
        for k, r in a.judge(got).items():
            j(names[k] + " [host]", "element", r)
        # the calls are asynchronous on the context's stream: every device input stays alive, and nothing is allocated, until the sync
        d = {k: dev(getattr(a, k)) for k in ("N", "means", "iv", "T", "Wv", "Tn", "Q", "Fn", "Wm", "Dm", "weight")}
        gf, gs, gd = Guarded(a.F.shape, init=a.F), Guarded(a.F.shape, init=a.F), Guarded((C, R), init=start_d)
        gt, gw, gz = Guarded(a.T.shape, init=a.T), Guarded((R, R), None), Guarded((C, R))
        ctx.tv_norm_statistics(d["N"], gf.view, d["means"], d["iv"], C, D)
        ctx.tv_subtract_m_plus_tw(d["N"], gs.view, d["means"], d["T"], d["Wv"], C, D)
        ctx.tv_norm_t(gt.view, d["iv"], C, D)
        ctx.tv_weighted_cov(d["Tn"], d["weight"], C, D, out=gw.view)
        ctx.tv_approximate_tctc(d["Tn"], d["Q"], C, D, out=gz.view)
        ctx.tv_approximate_tctc(d["Tn"], d["Q"], C, D, out=gd.view)
        ctx.sync()
        for k, r in a.judge({"Fn": gf.read(j, names["Fn"]), "Fs": gs.read(j, names["Fs"]), "Tn": gt.read(j, names["Tn"]),
                             "Wm": gw.read(j, names["Wm"]), "Dm": gz.read(j, names["Dm"])}).items():
            j(names[k] + " [device]", "element", r)
        j("tv_approximate_tctc [device, accumulating]", "element", br.ratio(br.ld(gd.read(j, "tctc")) - (a.Dm_ref + br.ld(start_d)), a.tctc_bar(start_d)))
        for which, call, extra in (("ubm", ctx.tv_estimate_w_ubm_weight, (a.Wm,)), ("eig", ctx.tv_estimate_w_eigen, (a.Dm, a.Q))):
            entry = "tv_estimate_w_" + ("ubm_weight" if which == "ubm" else "eigen")
            W = call(a.N, a.Fn, a.Tn, *extra, C, D)
            j(entry + " [host]", "W per utterance", a.w_ratios(which, W))
            if np.any(W[br.tr.EMPTY_UTT] != 0.0):
                j.note(entry, "the utterance without frames did not return w = 0")
            W = call(a.N, a.Fn, a.Tn, *extra, C, D, out=start_w.copy())
            j(entry + " [host, accumulating]", "W per utterance", a.w_ratios(which, W, start_w))
            dx = (d["Wm"],) if which == "ubm" else (d["Dm"], d["Q"])
            g0, g = Guarded((U, R)), Guarded((U, R), init=start_w)
            call(d["N"], d["Fn"], d["Tn"], *dx, C, D, out=g0.view)
            call(d["N"], d["Fn"], d["Tn"], *dx, C, D, out=g.view)
            ctx.sync()
            j(entry + " [device]", "W per utterance", a.w_ratios(which, g0.read(j, entry)))
            j(entry + " [device, accumulating]", "W per utterance", a.w_ratios(which, g.read(j, entry), start_w))
    j.finish()
