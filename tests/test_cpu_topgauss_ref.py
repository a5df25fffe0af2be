"""tests/topgauss_ref.py without a GPU: a float64 numpy restatement of gmmiv_topgauss_compute sits below ratio 1 on every case,
mode and setting of top_gauss; three planted defects fail, each on a named case; and the case table is not vacuous -- the count
varies from frame to frame, the capped case has capped and uncapped frames, the clamp reaches the planted frame, and the reference
itself has no ambiguous frame.  gmm_ref.use_top with a per-frame count is held to its old results."""
import numpy as np
import pytest

import gmm_ref as gr
import topgauss_ref as tg
from elementwise_judge import Judge

pytestmark = pytest.mark.skipif(not tg.HAVE_LONGDOUBLE, reason=tg.SKIP_MESSAGE)

MODES = (True, False)


def mode_name(complete):
    return "COMPLETE" if complete else "PARTIAL"


def run(case, dtype, complete, top_gauss, defect=None, ratios=None):
    ref = tg.reference(case, np.dtype(dtype).name)
    w, mean, iv = gr.model(case[:4])
    got = tg.restate_compute(w, mean, iv, tg.frames(case, dtype), case[4], top_gauss, complete, defect=defect)
    j = Judge("%s %s" % (tg.case_name(case), np.dtype(dtype).name), "%s top_gauss %g" % (mode_name(complete), top_gauss),
              {} if ratios is None else ratios)
    share = tg.judge(j, tg.Expected(ref, case[4], top_gauss, complete), got, w)
    return j, share, got


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("case", tg.CASES, ids=tg.case_name)
def test_float64_restatement_is_inside_every_bar(case, dtype):
    ratios = {}
    for complete in MODES:
        for top_gauss in tg.settings(case):
            j, share, got = run(case, dtype, complete, top_gauss, ratios=ratios)
            j.finish()
            assert share == 0.0, "the reference has ambiguous frames: %r" % share
    print("%s %s: largest ratio %.3g" % (tg.case_name(case), np.dtype(dtype).name, max(ratios.values())))
    assert max(ratios.values()) <= 1.0


# defect -> (case, complete, top_gauss): where it must fail
DEFECTS = {
    "test_behind_addition": ((33, 16, 257, 0.5, 33), True, 0.9),
    "snsl_not_floored": ((33, 16, 257, 0.5, 33), True, 33.0),
    "snsw_by_position": ((65, 33, 64, 0.3, 64), True, 0.999),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defects_fail(defect):
    case, complete, top_gauss = DEFECTS[defect]
    j, _, _ = run(case, np.float32, complete, top_gauss)
    j.finish()
    j, _, _ = run(case, np.float32, complete, top_gauss, defect=defect)
    assert j.bad, "the defect %s passes on %s" % (defect, tg.case_name(case))
    with pytest.raises(AssertionError):
        j.finish()


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("case", tg.CASES, ids=tg.case_name)
def test_cases_are_not_vacuous(case, dtype):
    ref = tg.reference(case, np.dtype(dtype).name)
    cap = case[4]
    p = tg.plant_at(case)
    assert -745.0 < float(ref.llk[p]) < tg.LO and not ref.dead()[p], "the planted frame does not reach the clamp"
    for complete in MODES:
        e = tg.Expected(ref, cap, 0.999, complete)
        assert float(e.llk[p]) == tg.LO and e.capped[p] and e.n_ref[p] == cap
        distinct = len(set(e.n_ref.tolist()))
        print("%s %s %s: %d distinct counts at mass 0.999, %d of %d frames capped"
              % (tg.case_name(case), np.dtype(dtype).name, mode_name(complete), distinct, int(e.capped.sum()), ref.T))
        if case[0] > 1:
            assert distinct >= 8, distinct
        assert (e.n_ref == 1).any() or case[0] > 1
    if case == tg.CAPPED_CASE:
        e = tg.Expected(ref, cap, 0.999, True)
        others = np.delete(e.capped, p)
        assert others.any() and not others.all(), "the capped case needs capped and uncapped frames besides the planted one"


def test_use_top_with_a_count_keeps_its_results_and_drops_the_tail():
    """count = ctop everywhere: the bits of the call without a count; a shorter count: the log-sum over the prefix, whatever
    stands behind it"""
    case = (37, 17, 300, 2.0)
    ref, cref = gr.reference(case, "float32"), gr.reference(case, "float32", 5)
    idx = ref.top(10)
    ln, mask = ref.nontop(idx)
    for complete in MODES:
        a, ab = gr.use_top(cref, idx, ln, ref, mask, complete)
        b, bb = gr.use_top(cref, idx, ln, ref, mask, complete, count=np.full(ref.T, 10))
        assert np.array_equal(a, b) and np.array_equal(ab, bb)
    count = 1 + np.arange(ref.T) % 10
    tail = np.where(np.arange(10)[None, :] < count[:, None], idx, -1)
    got, bar = gr.use_top(cref, tail, ln, None, None, False, count=count)
    for t in (0, 7, 9, 299):
        z = cref.z[t, idx[t, :count[t]]]
        want = z.max() + np.log(np.exp(z - z.max()).sum())
        assert abs(float(got[t] - want)) <= 4 * gr.U * abs(float(want)) and bar[t] > 0
    full, _ = gr.use_top(cref, tail, ln, None, None, True, count=count)
    assert np.all(full >= got) and np.any(full > got)
