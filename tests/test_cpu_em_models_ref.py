"""tests/em_models_ref.py checked on its own, without a GPU: the bars of the variance branch of computeMAP and of normalizeMixture
against a float64 numpy restatement of the kernels' arithmetic, three value-only defects that the bars reject by orders of magnitude,
and the floor share of every (case, dtype, segment) the GPU tests judge."""
import numpy as np
import pytest

import em_models_ref as er
import gmm_ref as gr

pytestmark = pytest.mark.skipif(not gr.HAVE_LONGDOUBLE, reason=gr.SKIP_MESSAGE)

REG = (14.0, 9.0, 20.0)


def stats_of(case, dtype):
    """float64 statistics rows of the case's segments (the reference's own, rounded), counts, the a-priori and the current models"""
    C, D, T, _ = case
    sb, sm = er.segments(case)
    rows = er.segment_rows(case, gr.dtype_name(dtype))
    G = len(sm)
    N, F, S = np.zeros((G, C)), np.zeros((G, C, D)), np.zeros((G, C, D))
    for s, r in enumerate(rows):
        if r is not None:
            N[s], F[s], S[s] = r["occ"].astype(np.float64), r["sx"].astype(np.float64), r["sxx"].astype(np.float64)
    N[0, C // 2] = 0.0                                              # a Gaussian without occupancy keeps its current mean / variance
    count = np.diff(sb).astype(np.float64)
    w0, mean0, iv0 = er.model(case, 0)
    ws, means, ivs = er.models(case)
    return N, F, S, count, w0, mean0, 1.0 / iv0, means[sm], 1.0 / ivs[sm]


def test_at_most_one_percent_of_the_pairs_of_a_segment_are_judged_by_the_floor_alone():
    for case in er.EM_CASES:
        sb, sm = er.segments(case)
        assert sb[2] == sb[1] and len(set(sm.tolist())) == 3          # an empty segment, all three models in use
        for dt in gr.DTYPES:
            for s in range(len(sm)):
                share = er.floor_share(case, gr.dtype_name(dt), s)
                print("%-18s %-8s segment %d model %d: floor share %.4f" % (gr.case_name(case), gr.dtype_name(dt), s, sm[s], share))
                assert share <= 0.01, (case, s, share)


def test_the_models_of_a_case_differ_in_means_and_variances():
    for case in er.EM_CASES:
        ws, means, ivs = er.models(case)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert not np.array_equal(means[a], means[b]) and not np.array_equal(ivs[a], ivs[b])
        assert np.all(ivs > 0)


@pytest.mark.parametrize("method", er.METHODS)
def test_the_float64_restatement_of_compute_map_meets_every_bar(method):
    worst = 0.0
    for case in er.EM_CASES:
        for dt in gr.DTYPES:
            args = stats_of(case, dt)
            for var, weight in ((True, True), (True, False), (False, True)):
                ref = er.map_ld(*args, method, True, var, weight, REG, 0.6)
                mo, co, wo = er.map_np(*args, method, True, var, weight, REG, 0.6)
                r = {k: float(gr.ratio(g.astype(gr.LD) - ref[k], ref[k + "_b"]).max()) for k, g in (("mean", mo), ("cov", co), ("w", wo))}
                print("%-18s %-8s %-13s var %d weight %d: %s" % (gr.case_name(case), gr.dtype_name(dt), method, var, weight,
                                                                   "  ".join("%s %.3g" % kv for kv in r.items())))
                worst = max(worst, max(r.values()))
    print("largest ratio of the restatement to a bar: %.3g" % worst)
    assert worst < 0.5                                              # a bar the restatement only just met would be a tuned one


def test_value_only_defects_of_the_variance_branch_miss_the_bar_by_orders_of_magnitude():
    for case in er.EM_CASES:
        args = stats_of(case, np.float32)
        ref = er.map_ld(*args, "MAPOccDep", True, True, False, REG, 0.6)
        for defect in ("drop", "swap", "fp32"):
            _, co, _ = er.map_np(*args, "MAPOccDep", True, True, False, REG, 0.6, defect=defect)
            r = gr.ratio(co.astype(gr.LD) - ref["cov"], ref["cov_b"])
            print("%-18s %-5s largest error / bar %.3g, median %.3g" % (gr.case_name(case), defect, r.max(), np.median(r)))
            assert r.max() >= 1e3, (case, defect, float(r.max()))


def test_the_float64_restatement_of_normalize_mixture_meets_every_bar():
    worst = 0.0
    for case in er.EM_CASES:
        ws, means, ivs = er.models(case)
        for k in range(3):
            for mean_only in (False, True):
                m, c = means[k], 1.0 / ivs[k]
                for it in range(2):                                  # the second iteration on the first one's output
                    nm, nc, mb, cb = er.normalize_ld(ws[k], m, c, mean_only)
                    gm, gc = er.normalize_np(ws[k], m, c, mean_only)
                    rm = float(gr.ratio(gm.astype(gr.LD) - nm, mb).max())
                    rc = float(gr.ratio(gc.astype(gr.LD) - nc, cb).max())
                    print("%-18s model %d mean_only %d it %d: mean %.3g cov %.3g" % (gr.case_name(case), k, mean_only, it, rm, rc))
                    worst = max(worst, rm, rc)
                    m, c = gm, gc
                    bad_m, bad_c = er.normalize_np(ws[k], m, c, mean_only, fp32=True)
                    nm2, nc2, mb2, cb2 = er.normalize_ld(ws[k], m, c, mean_only)
                    bad = float(gr.ratio(bad_m.astype(gr.LD) - nm2, mb2).max())
                    print("%-18s model %d mean_only %d it %d: fp32 variance table in the fold, mean %.3g" % (gr.case_name(case), k, mean_only, it + 1, bad))
                    assert bad >= 1e2, (case, k, bad)                 # orders beyond, also where the bar grows with C = 129
    print("largest ratio of the restatement to a bar: %.3g" % worst)
    assert worst < 0.5


def test_normalize_reference_reaches_zero_mean_and_unit_variance():
    case = er.EM_CASES[0]
    ws, means, ivs = er.models(case)
    nm, nc, _, _ = er.normalize_ld(ws[1], means[1], 1.0 / ivs[1])
    tm, tc = er.fusion_ld(ws[1], nm.astype(np.float64), nc.astype(np.float64))
    assert np.abs(tm).max() < 1e-12 and np.abs(tc - 1).max() < 1e-12
