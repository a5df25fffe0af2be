"""Results do not depend on what a context did before ("Results do not depend on a context's history").

The workspaces of a context are grow-only and never cleared; a fresh hipMalloc comes back zeroed, so on a context that has done
nothing else a read of memory the call has not written sees 0 -- and every other GPU file of this suite runs on such contexts.
Here the programme of tests/ws_history.py (54 steps: every frame-consuming entry point, the batched models, the front end -- windowed
NormFeat and TurnDetection included, whose tile offsets, run bases, staged decisions, run partials and smoothed curve live in slots
the back end shares --, the score normalisation and the i-vector back end: the T-matrix chain, the development set, PLDA, the scoring rules on matrices and on trial
lists, JFA) runs on contexts with different histories and the outputs are compared BIT FOR BIT, no reference and no tolerance:

    fresh_small, fresh_small_again        the judged shapes on two fresh contexts: the precondition (they must agree)
    fresh_large                           the dirtying shapes alone: NaN / Inf / 1e30 / far frames, chunked scratch, finite back-end inputs,
                                          then one NaN-as-data call per back-end family
    large_then_small, .._reversed         the judged shapes on every slot the large pass left dirty  == fresh_small
    small_then_large                      every slot freed and reallocated in mid-life               == fresh_large
    large_moved_then_small                the large pass with an option moved for one step each and put back == fresh_small

One test per sequence runs it (on one context, kept for the rest of the module) and holds that every step of its plan ran; one test
per programme step and form then compares every output of the step in every sequence; the non-vacuity test holds what keeps
them from passing emptily (no slot grew in the small pass, the large pass touched every slot the small one uses, the NaN calls
returned NaN or "not positive definite" as each must, the planted frames were counted, the chunked steps launched twice, the E-step
under tv_batch 16 ran its short batches).  With WS_HISTORY_JSON set to a path the outcome per step, the seconds, the workspace tables
and the launch counts are written there (profiles/r23/ws_history.json; profiles/r29/ws_history.json with the two steps of windowed
NormFeat and TurnDetection: on an MI355X on 2026-10-21, parent 32904a4, the module takes 11.1 s for 123 tests, 10.5 s for 119 before; a
large pass spends 0.015 s in either form of "normfeat window" and 0.007 s in "turn detection", and 30 NaN-as-data calls finish it).
"""
import json
import os
import time

import numpy as np
import pytest

import elementwise_judge as ej
import gmm_ref as gr
import ws_history as wh

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

MOVED = {"llk": {"glds": 0}, "em_accumulate": {"wg_waves": 4}, "occ": {"short_calls": 0}, "tv_stats": {"z_waves": 4},
         "batch llk": {"models_scratch_mb": 0}, "llr_trials per-model tables": {"trials_scratch_mb": 0},
         # the back end: a step that does not set the option itself (the bracket of elementwise_judge.options expects the default)
         "tv e-step": {"tv_batch": 48}, "tv m-step": {"tv_mstep_solve": 0, "tv_md_device": 0}, "tv tett": {"tv_tett_direct": 0},
         "tv estimate_w": {"chol_gemm": 1}, "dgemm split-K": {"gemm_nt80": 0}}
wh.SEQUENCES["large_moved_then_small"] = wh.SEQUENCES["large_then_small"]
# sequence -> (the sequence whose results it must repeat, the cases compared)
AGAINST = {"fresh_small_again": ("fresh_small", wh.SMALL), "large_then_small": ("fresh_small", wh.SMALL),
           "large_then_small_reversed": ("fresh_small", wh.SMALL), "large_moved_then_small": ("fresh_small", wh.SMALL),
           "small_then_large": ("fresh_large", wh.LARGE)}
RUNS, RATIOS, EQUAL, COMPARED = {}, {}, {}, set()


FAILED = []                      # the first exception a sequence or a handle test met on the GPU


def gpu_is_usable():
    """nothing of this module starts on the GPU after a call on it has failed: the failure is reported again instead"""
    if FAILED:
        raise RuntimeError("not run: an earlier GPU call of this module failed: %r" % (FAILED[0],))


def sequence(name):
    """the sequence, run once per module"""
    if name not in RUNS:
        gpu_is_usable()
        try:
            RUNS[name] = wh.run_sequence(name, moved=MOVED if name == "large_moved_then_small" else None)
            print("\n[ws_history] %s: %.1f s" % (name, RUNS[name]["total"]))
        except Exception as e:        # noqa: BLE001
            FAILED.append(e)
            raise
    return RUNS[name]


@pytest.fixture(scope="module", autouse=True)
def record():
    t0 = time.perf_counter()
    yield
    total = time.perf_counter() - t0
    print("\n[ws_history] module: %.1f s" % total)
    path = os.environ.get("WS_HISTORY_JSON")
    if not path:
        return
    runs = {k: v for k, v in RUNS.items() if isinstance(v, dict)}
    steps = {}
    for (step, form), eq in sorted(EQUAL.items()):
        secs = {s: round(sum(v for (c, st, f), v in r["seconds"].items() if st == step and f == form), 4) for s, r in runs.items()}
        steps["%s | %s" % (step, form)] = {"equal": eq, "seconds": secs}
    with open(path, "w") as f:
        json.dump({"criterion": "bitwise equality with the same step on a fresh context; no tolerance",
                   "module_seconds": round(total, 1), "sequence_seconds": {s: round(r["total"], 1) for s, r in runs.items()},
                   "steps": steps, "outputs_compared": len(COMPARED),
                   "workspace_bytes": {s: [{"after": p, "bytes": t} for p, t in r["ws"]] for s, r in runs.items()},
                   "launches ((k_llk_mfma, k_stats_z); k_dgemm(L) after either call of an E-step)":
                       {s: {" | ".join(k): v for k, v in r["log"].items()} for s, r in runs.items()},
                   "nan_calls_answered_as_they_must": {s: r["nan_ok"] for s, r in runs.items() if r["nan_ok"] is not None},
                   "nan_calls": sorted(set().union(*[r.get("nan", {}) for r in runs.values()]))}, f, indent=1)


def compare(j, step, form, name):
    base_name, cases = AGAINST[name]
    got, base = sequence(name)["results"], sequence(base_name)["results"]
    before = len(j.bad)
    for case in cases:
        if not step.applies(case):
            continue
        key = (case["name"], step.name, form)
        a, b = got[key], base[key]
        j.case, j.path = case["name"], "%s | %s | %s" % (name, step.name, form)
        if set(a) != set(b):
            j.note("outputs", "the step returned %s here and %s on %s" % (sorted(a), sorted(b), base_name))
        for out in sorted(set(a) & set(b)):
            j.same_bits(out, a[out], b[out], base_name)
            COMPARED.add((name,) + key + (out,))
    EQUAL.setdefault((step.name, form), {})[name] = len(j.bad) == before


@pytest.mark.parametrize("name", list(wh.SEQUENCES))
def test_sequence_runs_every_step_of_its_plan(name):
    """one context per sequence, run here and kept for the comparisons below: no test of this module takes longer than one sequence"""
    r = sequence(name)
    want = [(c["name"], s.name, f) for cases, reverse in wh.SEQUENCES[name] for c, s, f in wh.plan(cases, reverse)]
    assert want and set(r["results"]) == set(want) and [p for p, _ in r["ws"]] == ["large" if cases is wh.LARGE else "small" for cases, _ in wh.SEQUENCES[name]]
    assert all(r["results"][k] for k in want), "a step returned nothing"


STEP_FORMS = [(s.name, f) for s in wh.PROGRAMME for f in s.forms]


@pytest.mark.parametrize("name,form", STEP_FORMS, ids=["%s-%s" % (n.replace(" ", "_"), f) for n, f in STEP_FORMS])
def test_step_gives_the_bits_of_a_fresh_context_in_every_sequence(name, form):
    """precondition first: two fresh contexts agree (an output that does not is a finding to explain from the code, not a reason to
    relax -- DESIGN lists such outputs, and the list is empty); then every used context against the fresh one"""
    step = wh.STEPS[name]
    j = ej.Judge("", "", RATIOS)
    for seq in ("fresh_small_again", "large_then_small", "large_then_small_reversed", "small_then_large", "large_moved_then_small"):
        compare(j, step, form, seq)
    j.finish()


def test_no_output_of_any_step_was_left_uncompared():
    """every (sequence, case, step, form, output) of the compared sequences went through same_bits"""
    for name, form in STEP_FORMS:
        j = ej.Judge("", "", RATIOS)
        for seq in AGAINST:
            compare(j, wh.STEPS[name], form, seq)
    for seq, (base, cases) in AGAINST.items():
        res = sequence(seq)["results"]
        want = {(seq,) + key + (out,) for key, outs in res.items() if key[0] in {c["name"] for c in cases} for out in outs}
        assert want and want <= COMPARED, sorted(want - COMPARED)[:10]
        for c in cases:
            ran = {k[1:] for k in res if k[0] == c["name"]}
            assert ran == {(s.name, f) for s in wh.PROGRAMME if s.applies(c) for f in s.forms}, "a step did not run on " + c["name"]


def test_the_comparisons_are_not_vacuous():
    large = sequence("fresh_large")
    ws_small, ws_large = sequence("fresh_small")["ws"][0][1], large["ws"][0][1]
    # every slot the small pass uses was dirtied by the large pass alone
    cold = [i for i in range(64) if ws_small[i] and not ws_large[i]]
    assert not cold, "slots the small pass uses and the large pass leaves untouched: %s" % cold
    assert any(ws_small)
    # no slot grew in the small pass: all of them were reused as they were, none handed out fresh and cleared
    for name in ("large_then_small", "large_then_small_reversed", "large_moved_then_small"):
        (p0, after_large), (p1, after_small) = sequence(name)["ws"]
        assert (p0, p1) == ("large", "small")
        grown = [(i, after_large[i], after_small[i]) for i in range(64) if after_small[i] != after_large[i]]
        assert not grown, "%s: slots changed in the small pass (slot, bytes before, after): %s" % (name, grown)
    # the growth path did grow: the small pass left the fresh small table, the large pass freed and reallocated slots in mid-life
    (_, s0), (_, s1) = sequence("small_then_large")["ws"]
    regrown = [i for i in range(64) if s1[i] > s0[i] > 0]
    print("\n[ws_history] slots in use after the small pass: %d, freed and reallocated by the large pass: %d" % (sum(1 for v in s0 if v), len(regrown)))
    assert s0 == ws_small and regrown and all(b >= a for a, b in zip(s0, s1)), (s0, s1)
    # the small pass of the back end allocated nothing either: its slots alone, step by step -- every back-end step of the judged cases ran
    # in both forms after the large pass, and the table did not move (the check above), so each reused what the large pass left
    ran = [k for k in sequence("large_then_small")["results"] if k[0] in {c["name"] for c in wh.SMALL}]
    names = [s.name for s in wh.PROGRAMME]
    back_end = names[names.index(wh.BACKEND_FROM):]
    assert len(back_end) == 20 and {(c["name"], n, f) for c in wh.SMALL for n in back_end for f in wh.FORMS} <= set(ran)
    # the NaN-as-data calls answered as they must wherever a large pass ran: NaN everywhere, or "not positive definite" and nothing else
    for name in ("fresh_large", "large_then_small", "large_then_small_reversed", "small_then_large", "large_moved_then_small"):
        r = sequence(name)
        assert r["nan_ok"] is True and len(r["nan"]) == 30, (name, sorted(k for k, v in r["nan"].items() if not v))
    families = ("tv_estimate_a_and_c", "tv_update_t", "tv_min_divergence", "dev_cov_mat", "dev_mahalanobis", "iv_normalize", "jfa_subtract",
                "jfa_estimate_z_and_d", "score_cosine_trials", "score_mahalanobis_trials", "score_twocov_trials", "score_plda_trials", "plda_em_iteration",
                "feat_norm_window", "turn_curve", "turn_pick", "a finite call after them")
    assert set(families) <= set(large["nan"])
    # the short-batch E-step ran its batches: k_dgemm(L) is launched once per batch, and the timer holds the launches of the last call --
    # 64 and 65 utterances under tv_batch 16 are 4 and 4 + a batch of one; the default E-step is one batch per call
    timed = [c for c in wh.LARGE if c["opts"].get("timing")]
    assert timed
    for case in timed:
        assert case["iv"]["tv"][-1][3] == 129
        for form in wh.FORMS:
            assert large["log"][(case["name"], "e-step in batches", form)] == wh.estep_batches(case, wh.TV_BATCH) == [4, 5]
            assert large["log"][(case["name"], "e-step", form)] == [1, 1]
            assert large["log"][(case["name"], "e-step chol_gemm", form)] == [1, 1]
        moved = sequence("large_moved_then_small")["log"]
        assert moved[(case["name"], "e-step", "host")] == wh.estep_batches(case, MOVED["tv e-step"]["tv_batch"]) == [2, 2]
    # the planted frames were seen and counted (llk: two calls per step)
    for case in wh.LARGE:
        k1, k2 = wh.planted(case)
        assert len(k1) == 8 and len(k2) == 2
        for form in wh.FORMS:
            for step, calls in (("llk", 2), ("occ", 1)):
                r = large["results"][(case["name"], step, form)]
                assert r["delta zero_llk_frames"][0] == calls * (len(k1) + len(k2)), (case["name"], step, form, r["delta zero_llk_frames"])
                assert r["delta screened_frames"][0] == calls * len(k1), (case["name"], step, form, r["delta screened_frames"])
            assert large["results"][(case["name"], "frame_moments", form)]["unusable frames"][0] == len(k1)
    # the chunked large steps were chunked
    chunked = [c for c in wh.LARGE if c["opts"].get("z_scratch_mb")]
    assert chunked
    for case in chunked:
        for form in wh.FORMS:
            for entry in ("em", "tv"):
                n_llk, n_z = large["log"][(case["name"], entry, form)][0]
                assert n_llk >= 2 and n_z >= 2, (case["name"], entry, form, n_llk, n_z)


# ---------------------------------------------------------------------------------------------------------------- used handles
def _batch_bits(b, case, x, sb, sm):
    C, D = case["gcase"][:2]
    llk, ssum = b.llk(x, sb, sm, *wh.WIDE, out=np.full(len(x), ej.SENTINEL))
    N, F, S, sl = b.em_stats(x, sb, sm)
    out = {"llk": llk, "seg_sum": ssum, "em N": N, "em F": F, "em S": S, "em seg_llk": sl}
    if D <= 80:                                                     # above: the generic kernels, no packed MFMA operands
        out.update({"packed(%d)" % g: b.packed(g) for g in range(b.G)})
    return out


@pytest.mark.parametrize("case", wh.SMALL, ids=lambda c: c["name"])
def test_a_batch_loaded_again_has_the_bits_of_a_new_handle(case):
    """per-model tables first, then shared tables (stride 0) of OTHER models; and the content of G models first, then of fewer (a
    batch of one shape, its tables reloaded with two distinct models instead of three): packed(g), llk and em_stats of the reloaded
    handle against a new handle loaded once"""
    from lia_ral_amd import capi
    C, D, T, _ = case["gcase"]
    G = case["G"]
    w, m, iv = wh._batch_models(case["name"])
    other = [gr.model(case["gcase"], 30 + k) for k in range(G)]
    m2 = np.stack([o[1] for o in other])
    x = wh.frames(case, "host")
    sb, sm = wh.seg_table(case)
    fewer = (np.stack([w[0]] * G), np.stack([m2[0], m2[1]] + [m2[0]] * (G - 2)), np.stack([iv[1]] * G))
    loads = {"shared after per-model": ((w, m, iv), (other[0][0], m2, other[0][2])), "per-model after shared": ((w[0], m, iv[0]), (w, m2, iv)),
             "fewer distinct models": ((w, m, iv), fewer)}
    j = ej.Judge(case["name"], "", RATIOS)
    gpu_is_usable()
    ctx = capi.Context(0)
    try:
        for tag, (first, second) in loads.items():
            j.path = tag
            used = ctx.gmm_batch(G, C, D).load(*first)
            _batch_bits(used, case, x, sb, sm)                      # the handle is used before it is loaded again
            used.load(*second)
            got = _batch_bits(used, case, x, sb, sm)
            new = ctx.gmm_batch(G, C, D).load(*second)
            want = _batch_bits(new, case, x, sb, sm)
            for k in want:
                j.same_bits(k, got[k], want[k], "a new handle loaded once")
            used.close(); new.close()
    except capi.GmmivError as e:
        if "error -2" in str(e):                                    # GMMIV_ERR_HIP: the device may be unusable from here on
            FAILED.append(e)
        raise
    finally:
        ctx.close()
    j.finish()


@pytest.mark.parametrize("case", wh.SMALL, ids=lambda c: c["name"])
def test_a_model_set_again_has_the_bits_of_a_new_handle(case):
    """Gmm.set / set_cov on a used handle: llk, occ and llk_determine_top against a handle created with the new tables"""
    from lia_ral_amd import capi
    w2, m2, iv2 = gr.model(case["gcase"], 31)
    iv2 = iv2 * 1.25
    x = wh.frames(case, "host")

    def bits(g):
        out = {"llk": g.llk(x, *wh.WIDE), "occ": g.occ(x)}
        out.update({"top " + k: v for k, v in g.llk_determine_top(x, 10, True, *wh.WIDE).items()})
        return out
    j = ej.Judge(case["name"], "", RATIOS)
    gpu_is_usable()
    ctx = capi.Context(0)
    try:
        new = ctx.gmm(w2, m2, iv2)
        want = bits(new)
        for tag in ("set", "set_cov"):
            j.path = tag
            used = ctx.gmm(*gr.model(case["gcase"]))
            bits(used)
            if tag == "set":
                used.set(w2, m2, iv2)
            else:
                used.set_cov(w2, m2, 1.0 / iv2)
                want = bits(ctx.gmm(w2, m2, 1.0 / (1.0 / iv2)))    # set_cov inverts on the device: 1 / (1 / iv) is the table it holds
            got = bits(used)
            for k in want:
                j.same_bits(k, got[k], want[k], "a new handle")
    except capi.GmmivError as e:
        if "error -2" in str(e):                                    # GMMIV_ERR_HIP: the device may be unusable from here on
            FAILED.append(e)
        raise
    finally:
        ctx.close()
    j.finish()
