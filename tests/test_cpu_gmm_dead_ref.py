"""The zero-likelihood rule of tests/gmm_ref.py (RuleReference, planted, restate_rule) checked on its own, without a GPU: the
conditions the planted cases rest on, for every case and both frame types; a float64 restatement of the kernels' arithmetic with the
rule applied, which must sit well below every bar that tests/test_gpu_gmm_dead_frames.py judges; and seven planted defects in that
restatement, each of which the per-element judge must reject.

What the per-array criteria of tests/test_gpu_degenerate.py (max|a - b| / max|b| < 1e-9 over an accumulator) make of the same
defects is computed and printed next to it.  Three of them leave occ / sx / sxx untouched -- lo of a dead frame in the EM llk sum, a
dead frame in the EM frame count, a dead frame that keeps the reference's top list -- and so pass rel < 1e-9 on every array; that
module sees them only through its scalar checks, at its one shape.  The gap this closes is the other one: every defect that moves an
array is visible to rel < 1e-9 only through the few Gaussians that carry most frames, and tests/test_gpu_degenerate.py runs one
shape on six paths."""
import numpy as np
import pytest

import gmm_ref as gr

pytestmark = pytest.mark.skipif(not gr.HAVE_LONGDOUBLE, reason=gr.SKIP_MESSAGE)

READERS = (0, 5, 11, 12)        # the world, the shifted client of the top-C chain, the other two models of a batch
BATCH_ONLY = tuple(c for c in gr.BATCH_CASES if c not in gr.DEAD_CASES)
DEFECT_CASE = (300, 60, 130, 2.0)
CTOP = 10


def test_the_case_table_and_the_planted_positions():
    assert len(gr.DEAD_CASES) == 11 and len(gr.DEAD_PATH_CASES) == 3
    for case in gr.DEAD_CASES + BATCH_ONLY:
        T = case[2]
        p = gr.planted(case, "float32")
        assert p == gr.planted(case, "float32") and not p["x"].flags.writeable
        assert p["dead"][:2] == (T - 1, 0) and 16 in p["dead"] and 15 in p["dead"] and not set(p["dead"]) & set(p["far"])
        assert len(p["dead"]) == min(max(1, T // 3), len(set(q if q >= 0 else q + T for q in gr.DEAD_CANDIDATES if q < T)))
        for a, b in ((64, 63), (128, 127), (256, 255)):
            assert (a in p["dead"]) == (a < T) and (b in p["dead"]) == (b < T)
        assert T < 48 or set(range(32, 48)) <= set(p["dead"])                   # a whole dead 16-frame block
        assert T < 48 or len(set(p["kind"].values())) == 8                      # every kind is planted
        assert gr.planted(case, "float64")["dead"] == p["dead"] and gr.planted(case, "float64")["kind"] == p["kind"]


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("case", gr.DEAD_CASES + BATCH_ONLY, ids=gr.case_name)
def test_the_conditions_of_a_planted_case_hold(case, dtype):
    """the planted set is dead() under every model that reads the frames, no largest logit within 20 of the threshold, at least half
    of the frames ordinary, at most 1 % of their pairs floor-only, the -700 frames alive with their largest posterior under a bar
    above the floor, the -800 frames at -800"""
    c = gr.planted_conditions(case, gr.dtype_name(dtype), READERS)
    print("%-18s %-8s %s" % (gr.case_name(case), gr.dtype_name(dtype), "  ".join("%s %.4g" % kv for kv in c.items())))
    r = gr.rule_reference(case, gr.dtype_name(dtype))
    d = r.dead()
    assert not r.gamma[d].any() and not r.g64[d].any() and not r.dgamma[d].any() and not r.B[d].any() and np.all(r.llk[d] == gr.DEAD_LO)
    assert np.isfinite(r.gamma.astype(np.float64)).all() and np.isfinite(r.dgamma).all() and np.isfinite(r.B).all()
    for name, ub in gr.dead_layouts(r.T):
        N, F, Nb, Fb = r.utt_stats(ub)
        gone = np.array([d[ub[u]:ub[u + 1]].all() for u in range(len(ub) - 1)])
        assert np.isfinite(Fb).all() and not N[gone].any() and not F[gone].any() and not Nb[gone].any() and not Fb[gone].any()
        assert name != "a" or gone.sum() == d.sum()
        assert name != "b" or r.T <= 41 or 40 in ub                             # (b) cuts the dead block
    every, alive = r.llk_sum(every=True)[0], r.llk_sum()[0]
    assert abs(float(every - alive) - gr.DEAD_LO * d.sum()) < 1e-6 and r.count_bar((1.0, 0.5))[0] == 1.5 * (r.T - d.sum())


def test_the_restatement_with_the_rule_applied_meets_every_bar():
    worst, worst_far = 0.0, 0.0
    for case in gr.DEAD_CASES:
        for dt in gr.DTYPES:
            dn = gr.dtype_name(dt)
            ref, p = gr.rule_reference(case, dn), gr.planted(case, dn)
            w, mean, iv = gr.model(case)
            ctop = min(CTOP, case[0])
            got = gr.restate_rule(w, mean, iv, p["x"], ctop)
            assert np.array_equal(got["dead"], ref.dead())
            j = gr.judge_rule(ref, got)
            # the top-C chain as the kernels evaluate it (restate_top), world and shifted client, on the reference's own selection
            idx = np.where(ref.dead()[:, None], np.arange(ctop)[None, :], ref.top(ctop))
            cref = gr.rule_reference(case, dn, 5)
            wl, cl = gr.restate_top((w, mean, iv), [gr.model(case, 5)], p["x"], idx, True, gr.DEAD_LO, gr.DEAD_HI)
            j["top llk"] = float(gr.ratio(wl.astype(gr.LD) - ref.llk, ref.B).max())
            ln, mask = ref.nontop(idx, ref.dead())
            v, b = gr.clamp_below(*gr.use_top(cref, idx, ln, ref, mask), gr.DEAD_LO, gr.DEAD_HI)
            j["use_top llk"] = float(gr.ratio(cl[0].astype(gr.LD) - v, b).max())
            far = list(p["far"])
            jf = float(gr.ratio(got["gamma"][far].astype(gr.LD) - ref.gamma[far], ref.dgamma[far]).max())
            print("%-18s %-8s far %.3g  %s" % (gr.case_name(case), dn, jf, "  ".join("%s %.3g" % kv for kv in j.items())))
            assert max(j.values()) <= 1.0, (case, dn, j)
            worst, worst_far = max(worst, max(j.values())), max(worst_far, jf)
    print("largest ratio of the restatement to a bar: %.3g; on the -700 frames: %.3g" % (worst, worst_far))
    assert worst < 0.5 and worst_far < 0.5


def old_rel(got, ref):
    """tests/test_gpu_degenerate.py's criterion: the largest of max|a - b| / max|b| over occ, sx, sxx"""
    s = ref.sums()
    return max(float(np.abs(got[k] - s[k].astype(np.float64)).max() / np.abs(s[k].astype(np.float64)).max()) for k in ("occ", "sx", "sxx"))


def test_every_planted_defect_is_rejected_by_the_judge():
    ref, p = gr.rule_reference(DEFECT_CASE, "float32"), gr.planted(DEFECT_CASE, "float32")
    w, mean, iv = gr.model(DEFECT_CASE)
    clean = gr.judge_rule(ref, gr.restate_rule(w, mean, iv, p["x"], CTOP))
    assert max(clean.values()) <= 1.0, clean
    passes_old = []
    for defect in gr.RULE_DEFECTS:
        got = gr.restate_rule(w, mean, iv, p["x"], CTOP, defect=defect)
        j = gr.judge_rule(ref, got)
        rel = old_rel(got, ref)
        beyond = {k: v for k, v in j.items() if not v <= 1.0}
        print("%-48s old rel-to-max %.3g;  outside their bars: %s" % (defect, rel, "  ".join("%s %.3g" % kv for kv in beyond.items())))
        assert beyond, defect
        if rel < 1e-9:
            passes_old.append(defect)
    print("pass rel < 1e-9 on occ / sx / sxx: %s" % "; ".join(passes_old))
    assert passes_old == [gr.RULE_DEFECTS[1], gr.RULE_DEFECTS[2], gr.RULE_DEFECTS[6]]
