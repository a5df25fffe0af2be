"""The zero-likelihood rule of include/gmmiv.h ("DEGENERATE INPUTS") held per frame, per pair (t, c) and per element of every
accumulator, on every shape and option path that decides it: k_llk_mfma, k_stats_z, k_stats_mfma, k_posteriors, the three top-C
families, the any-shape kernels, the batched instantiation.

The frames of gmm_ref.planted: dead frames of eight kinds (a NaN, +Inf, -Inf, 1e30 in one dimension, -2e18 in the last, every
dimension 3e17, every dimension NaN, a finite frame whose largest logit is -800) at 0, T - 1, on both sides of the 16 / 64 / 128 /
256 frame boundaries and over the whole 16-frame block 32 .. 47, and up to two ALIVE frames at largest logit -700 next to them.  The
reference is gmm_ref.RuleReference: the long double log-domain reference with the rule applied -- on a dead frame every bar is 0, so
llk must be exactly min_llk = -1000, the posterior row exactly 0, and an utterance or segment of dead frames a row of zeros; every
other frame, the -700 ones included, is judged under its own bars as in test_gpu_gmm_elementwise.py.  The conditions all this rests
on (gmm_ref.planted_conditions) are asserted in every test, from the references alone.

gmm_ref.DEAD_CASES x both frame types run the default paths through Gmm.llk (+ sums: every frame counts, a dead one with min_llk),
Gmm.occ, Gmm.em_accumulate (weights 1, 0.5, 1 then 0.5; llk and count over the alive frames only), Gmm.tv_stats (gmm_ref.dead_layouts:
every dead frame an utterance of its own, ragged utterances that cut the dead block, one utterance) and the top-C chain for
ctop = min(10, C) and min(17, C); gmm_ref.DEAD_PATH_CASES run each of the 14 option paths of test_gpu_gmm_elementwise.PATHS on the
entry points it reaches.  Around every call the counters "zero_llk_frames" and "screened_frames" are reset and read and must hold
exactly what the header says.  Then: "assume_finite" 1 gives the bits of 0; GmmBatch.llk / tv_stats / em_stats with a segment that
is the dead block, a bound between a dead and an alive frame and a segment ending on the dead last frame; tv_stats_lines rows are
still the left fold of the tv_stats rows.

llk_use_top sees a frame only through the client's logits of the selected Gaussians and the world's remainder: on a frame that is
dead under the world it returns the clamp of the client's log-sum over the Gaussians 0 .. ctop - 1 (remainder -inf) -- min_llk on
every kind-(1) frame (its logits lie near -1e19), and on a -800 frame the client's own value where that lies above min_llk = -1000.
It is judged against exactly that (gmm_ref.use_top, gmm_ref.clamp_below), and the header's table says so now.

With DEAD_ERRORS_JSON set to a path the largest ratio per (case, path, entry point) is written there
(profiles/r25/dead_frames_errors.json).
"""
import contextlib
import json
import os
import time

import numpy as np
import pytest

import gmm_ref as gr
import test_gpu_gmm_elementwise as ew
from test_gpu_gmm_elementwise import ALL, DEFAULTS, PATHS, label, options, run_em, run_occ
from test_gpu_gmm_services_elementwise import LINES, fold

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300), pytest.mark.skipif(not gr.HAVE_LONGDOUBLE, reason=gr.SKIP_MESSAGE)]

LD = gr.LD
LO, HI = gr.DEAD_LO, gr.DEAD_HI
CLIENT_SHIFT = ew.CLIENT_SHIFT
BATCH_SHIFTS = ew.BATCH_SHIFTS
RATIOS = {}
JUDGED = [0]
assert len(PATHS) == 14 and DEFAULTS["assume_finite"] == 0


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    t0 = time.time()
    c = capi.Context(0)
    yield c
    c.close()
    path = os.environ.get("DEAD_ERRORS_JSON")
    if path and RATIOS:
        per_path, per_entry = {}, {}
        for (case, p, entry), v in RATIOS.items():
            per_path[p] = max(per_path.get(p, 0.0), v)
            per_entry[entry] = max(per_entry.get(entry, 0.0), v)
        with open(path, "w") as f:
            json.dump({"bound": "tests/gmm_ref.py, RuleReference: the bars of Reference on the alive frames, 0 on a dead frame",
                       "max_ratio": float("%.4g" % max(RATIOS.values())), "judged_elements": JUDGED[0], "module_seconds": round(time.time() - t0, 1),
                       "paths": {k: float("%.4g" % v) for k, v in sorted(per_path.items())},
                       "entry_points": {k: float("%.4g" % v) for k, v in sorted(per_entry.items())},
                       "entries": {" | ".join(k): float("%.4g" % v) for k, v in sorted(RATIOS.items())}}, f, indent=1)


class Judge(ew.Judge):
    """test_gpu_gmm_elementwise.Judge, with the largest ratios kept in this module's own record"""

    def __call__(self, entry, axes, got, ref, bar):
        key = (self.case, self.path, entry)
        theirs = ew.RATIOS.pop(key, None)
        super().__call__(entry, axes, got, ref, bar)
        RATIOS[key] = max(RATIOS.get(key, 0.0), ew.RATIOS.pop(key))
        JUDGED[0] += int(np.size(got))
        if theirs is not None:
            ew.RATIOS[key] = theirs

    def equal(self, entry, got, want, what):
        got = np.asarray(got)
        if not np.array_equal(got, np.broadcast_to(want, got.shape)):
            bad = np.argwhere(got != np.broadcast_to(want, got.shape))
            self.note(entry, "%s: %d of %d differ, first at %s: %r" % (what, len(bad), got.size, tuple(int(v) for v in bad[0]), got[tuple(bad[0])]))
        JUDGED[0] += int(got.size)


@contextlib.contextmanager
def counted(ctx, j, entry, zero, screened):
    """reset both counters, run, read: exactly (zero, screened) frames were counted (include/gmmiv.h: kind (2) AND kind (1) frames in
    "zero_llk_frames" by the entry points that drop a frame from a sum, none by the top-C entry points; kind (1) frames in
    "screened_frames" once per frame-consuming call while "assume_finite" is 0)"""
    ctx.set_option("zero_llk_frames", 0); ctx.set_option("screened_frames", 0)
    yield
    got = (ctx.set_option("zero_llk_frames", 0), ctx.set_option("screened_frames", 0))
    if got != (zero, screened):
        j.note(entry + " counters", "zero_llk_frames, screened_frames = %r, the header says %r" % (got, (zero, screened)))


def setup(case, dtype, floor=gr.PHI, shifts=(0, CLIENT_SHIFT)):
    """-> (planted frames, the world's RuleReference, dead frames, kind-(1) frames); the conditions of the case asserted first"""
    dn = gr.dtype_name(dtype)
    gr.planted_conditions(case, dn, shifts)
    ref = gr.rule_reference(case, dn, 0, floor)
    return gr.planted(case, dn)["x"], ref, int(ref.dead().sum()), int(ref.unusable.sum())


# ---------------------------------------------------------------- the entry points
def run_llk(j, g, x, ref):
    sums = np.zeros(2)
    got = g.llk(x, LO, HI, sums=sums)
    j("llk", "(t)", got, ref.llk, ref.B)                        # B = 0 on a dead frame: exactly LO
    s, sb = ref.llk_sum(every=True)
    j("llk sums", "()", sums[0], s, sb)
    if sums[1] != ref.T:
        j.note("llk sums", "frame count %r, expected %d (every frame counts)" % (sums[1], ref.T))


def run_tv(j, g, x, ref):
    for name, ub in gr.dead_layouts(ref.T):
        N, F = g.tv_stats(x, ub)
        Nr, Fr, Nb, Fb = ref.utt_stats(ub)
        j("tv(%s) N" % name, "(u, c)", N, Nr, Nb)
        j("tv(%s) F" % name, "(u, c, d)", F.reshape(Fr.shape), Fr, Fb)


def run_top(ctx, j, g, client, x, ref, cref, ctop, w, ns):
    """DETERMINE_TOP_DISTRIBS (COMPLETE) on the world, USE_TOP_DISTRIBS of the shifted client on its selection, the dead-aware checks
    of test_gpu_trials_elementwise.valid_selection; the selection is checked for range and repeats BEFORE it is handed on"""
    e = "top%d" % ctop
    dead = ref.dead()
    nd = int(dead.sum())
    with counted(ctx, j, e + " determine", 0, ns):
        d = g.llk_determine_top(x, ctop, True, LO, HI)
    idx = d["idx"].astype(np.int64)
    bad = [t for t, r in enumerate(idx.tolist()) if len(set(r)) != ctop or min(r) < 0 or max(r) >= ref.C]
    if bad:
        j.note(e + " idx", "indices outside the model or repeated in a row at %d frames, first frame %d: %r" % (len(bad), bad[0], idx[bad[0]].tolist()))
        return
    j.equal(e + " idx dead", idx[dead], np.arange(ctop)[None, :], "a zero-likelihood frame does not select 0 .. ctop - 1")
    j(e + " lk dead", "(dead t, j)", d["lk"][dead], 0.0, 0.0)
    j(e + " nontop_lk dead", "(dead t)", d["nontop_lk"][dead], 0.0, 0.0)
    j.equal(e + " nontop_llk dead", d["nontop_llk"][dead], -np.inf, "the remainder of a zero-likelihood frame is not -inf")
    j(e + " nontop_w dead", "(dead t)", d["nontop_w"][dead], LD(1) - np.asarray(w[:ctop], LD).sum(), ctop * gr.U)
    short, slack = ref.selection_shortfall(np.where(dead[:, None], ref.top(ctop), idx))
    j(e + " idx", "(t, j)", np.where(dead[:, None], 0.0, short), 0.0, slack)
    j(e + " llk", "(t)", d["llk"], ref.llk, ref.B)
    lk, lkb = ref.selected_lk(idx)
    j(e + " lk", "(alive t, j)", d["lk"][~dead], lk[~dead], lkb[~dead])
    ln, mask = ref.nontop(idx, dead)
    want, bar = gr.clamp_below(*gr.use_top(cref, idx, ln, ref, mask), LO, HI)
    with counted(ctx, j, e + " use_top", 0, ns):
        got = client.llk_use_top(x, d["idx"], d["nontop_llk"], True, LO, HI)
    j(e + " use_top llk", "(t)", got, want, bar)


def run_entries(ctx, j, case, dtype, entries, floor=gr.PHI):
    x, ref, nd, ns = setup(case, dtype, floor)
    w, mean, iv = gr.model(case)
    g = ctx.gmm(w, mean, iv)
    for e in entries:
        if e == "llk":
            with counted(ctx, j, "llk", nd, ns):
                run_llk(j, g, x, ref)
        elif e == "occ":
            with counted(ctx, j, "occ", nd, ns):
                run_occ(j, g, x, ref)
        elif e == "em":
            with counted(ctx, j, "em (three calls)", 3 * nd, 3 * ns):
                run_em(j, g, x, ref)
        elif e == "tv":
            with counted(ctx, j, "tv (three calls)", 3 * nd, 3 * ns):
                run_tv(j, g, x, ref)
        else:
            client = ctx.gmm(*gr.model(case, CLIENT_SHIFT))
            cref = gr.rule_reference(case, gr.dtype_name(dtype), CLIENT_SHIFT, floor)
            for ctop in sorted({min(10, ref.C), min(17, ref.C)}):
                run_top(ctx, j, g, client, x, ref, cref, ctop, w, ns)
            client.close()
    g.close()


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("case", gr.DEAD_CASES, ids=gr.case_name)
def test_default_paths_hold_the_rule_per_frame_pair_and_element(ctx, case, dtype):
    j = Judge(label(case, dtype), "defaults")
    run_entries(ctx, j, case, dtype, ALL)
    j.finish()


@pytest.mark.parametrize("case", gr.DEAD_PATH_CASES, ids=gr.case_name)
@pytest.mark.parametrize("path", list(PATHS), ids=lambda p: p.replace(" ", "_"))
def test_option_paths_hold_the_rule_per_frame_pair_and_element(ctx, path, case):
    opts, entries, floor = PATHS[path]
    j = Judge(label(case, np.float32), path)
    with options(ctx, opts):
        run_entries(ctx, j, case, np.float32, entries, floor)
    j.finish()


def test_assume_finite_1_gives_the_bits_of_0_on_planted_frames(ctx):
    """include/gmmiv.h: "RESULTS do not depend on it" -- the option only skips the pass that counts the kind-(1) frames, so
    "screened_frames" stays 0 under it and "zero_llk_frames" counts as before"""
    case = gr.DEAD_PATH_CASES[0]
    x, ref, nd, ns = setup(case, np.float32)
    g, client = ctx.gmm(*gr.model(case)), ctx.gmm(*gr.model(case, CLIENT_SHIFT))
    ub = gr.dead_layouts(ref.T)[1][1]
    j = Judge(label(case, np.float32), "assume_finite 1")

    def run(screened):
        out = {}
        with counted(ctx, j, "llk", nd, screened):
            out["llk"] = g.llk(x, LO, HI)
        with counted(ctx, j, "occ", nd, screened):
            out["occ"] = g.occ(x)
        with counted(ctx, j, "em", nd, screened):
            out["em"] = g.em_accumulate(x, weight=0.5)
        with counted(ctx, j, "tv", nd, screened):
            out["tv N"], out["tv F"] = g.tv_stats(x, ub)
        with counted(ctx, j, "top", 0, 2 * screened):
            d = g.llk_determine_top(x, 10, True, LO, HI)
            out["use_top"] = client.llk_use_top(x, d["idx"], d["nontop_llk"], True, LO, HI)
        out.update(("top " + k, d[k].astype(np.float64)) for k in ("idx", "lk", "nontop_lk", "nontop_llk", "nontop_w", "llk"))
        return out

    base = run(ns)
    with options(ctx, {"assume_finite": 1}):
        other = run(0)
    for k in base:
        j.same_bits(k, other[k], base[k], "assume_finite 0")
    client.close(); g.close()
    j.finish()


def batch_segments(T):
    """six segments: a bound at 17 between the dead frame 16 and an alive one, one segment that is exactly the dead block 32 .. 47
    (every row 0), an empty one, one that ends on the dead last frame; the frames 0 .. 2 (0 is dead) belong to no segment"""
    return np.array([3, 17, 32, 48, 48, (48 + T) // 2, T], np.int64), np.array([1, 2, 0, 2, 0, 1], np.int32)


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("case", gr.BATCH_CASES, ids=gr.case_name)
def test_a_model_per_segment_holds_the_rule(ctx, case, dtype):
    """GmmBatch.llk / tv_stats / em_stats: each segment under its own model's rule reference.  seg_sum is the sum of the clamped
    per-frame values, so a dead frame enters with min_llk; seg_llk leaves the dead frames out of the sum and of its frame count
    (include/gmmiv.h, gmmiv_tv_stats_models)"""
    C, D, T, _ = case
    dn = gr.dtype_name(dtype)
    x, _, _, _ = setup(case, dtype, shifts=BATCH_SHIFTS)
    models = [gr.model(case, s) for s in BATCH_SHIFTS]
    refs = [gr.rule_reference(case, dn, s) for s in BATCH_SHIFTS]
    sb, sm = batch_segments(T)
    assert refs[0].dead()[32:48].all() and refs[0].dead()[16] and not refs[0].dead()[17] and refs[0].dead()[T - 1] and sb[-1] == T
    nd, ns = int(refs[0].dead()[sb[0]:].sum()), int(refs[0].unusable[sb[0]:].sum())
    b = ctx.gmm_batch(3, C, D).load(np.stack([m[0] for m in models]), np.stack([m[1] for m in models]), np.stack([m[2] for m in models]))
    j = Judge(label(case, dtype), "batch")
    with counted(ctx, j, "batch llk", nd, ns):
        llk, ssum = b.llk(x, sb, sm, LO, HI)
    with counted(ctx, j, "batch tv", nd, ns):
        N, F, sl = b.tv_stats(x, sb, sm)
    with counted(ctx, j, "batch em_stats", nd, ns):
        Ne, Fe, Se, sle = b.em_stats(x, sb, sm)
    if not np.isnan(llk[:sb[0]]).all():
        j.note("batch llk", "a frame outside every segment was written")
    for s, m in enumerate(sm):
        lo, hi, r = int(sb[s]), int(sb[s + 1]), refs[m]
        j("batch llk seg %d" % s, "(t - %d)" % lo, llk[lo:hi], r.llk[lo:hi], r.B[lo:hi])
        j("batch llk seg_sum %d" % s, "()", ssum[s], *r.llk_sum(lo, hi, every=True))
        q = r.sums(lo, hi)
        for name, (Ns, Fs, Ss, L) in (("tv", (N, F, None, sl)), ("em_stats", (Ne, Fe, Se, sle))):
            j("batch %s seg_llk %d" % (name, s), "()", L[s, 0], *r.llk_sum(lo, hi))
            if L[s, 1] != r.alive_count(lo, hi):
                j.note("batch %s seg_llk %d" % (name, s), "frame count %r, expected the %d alive frames of %d" % (L[s, 1], r.alive_count(lo, hi), hi - lo))
            j("batch %s N seg %d" % (name, s), "(c)", Ns[s], q["occ"], q["occ_b"])
            j("batch %s F seg %d" % (name, s), "(c, d)", Fs[s].reshape(C, D), q["sx"], q["sx_b"])
            if Ss is not None:
                j("batch %s S seg %d" % (name, s), "(c, d)", Ss[s].reshape(C, D), q["sxx"], q["sxx_b"])
    assert not refs[0].sums(32, 48)["occ_b"].any()                   # the dead block: bars of 0, so its rows above were held to exactly 0
    b.close()
    j.finish()


def test_tv_stats_lines_rows_are_still_the_fold_of_their_file_rows(ctx):
    """the property of test_gpu_gmm_services_elementwise.py on planted frames: file 0 ends inside the dead block, file 4 is the dead
    last frame alone (a row of zeros), and every line row has the bits of 0.0 + r_1 + r_2 .. over the gmmiv_tv_stats rows"""
    case = (300, 60, 130, 2.0)
    x, ref, nd, ns = setup(case, np.float32)
    fb = gr.ragged_bounds(case[2])
    assert len(fb) == 6 and 32 < fb[1] < 48 and fb[4] == case[2] - 1 and ref.dead()[fb[4]]
    g = ctx.gmm(*gr.model(case))
    j = Judge(label(case, np.float32), "tv_stats_lines")
    Nf, Ff = g.tv_stats(x, fb)
    Nr, Fr, Nb, Fb = ref.utt_stats(fb)
    j("tv files N", "(u, c)", Nf, Nr, Nb)
    j("tv files F", "(u, c, d)", Ff.reshape(Fr.shape), Fr, Fb)
    with counted(ctx, j, "tv_stats_lines", nd, ns):
        N, F = g.tv_stats_lines(x, fb, LINES)
    for l, files in enumerate(LINES):
        j.same_bits("N line %d" % l, N[l], fold(Nf, files), "the fold over the file rows")
        j.same_bits("F line %d" % l, F[l], fold(Ff, files), "the fold over the file rows")
    g.close()
    j.finish()
