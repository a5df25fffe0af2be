"""tests/gmm_ref.py checked on its own, without a GPU: the per-pair bars against a float64 restatement of the kernels' arithmetic and
against the CPU oracle, the case table's floor share, and three value-only defects that the bars reject by orders of magnitude while
the criteria the suite had before (1e-9 absolute on a per-frame log-likelihood, max|a - b| / max|b| < 1e-9 over a whole array of
occupancies / first- / second-order sums) do not see them."""
import numpy as np
import pytest

import gmm_ref as gr
from oracle import oracle as orc

pytestmark = pytest.mark.skipif(not gr.HAVE_LONGDOUBLE, reason=gr.SKIP_MESSAGE)

ORACLE_FLOOR = 1e-250          # the oracle is linear-domain: below this its values are not reliable
DEFECT_CASE = (300, 60, 130, 2.0)


def test_at_most_one_percent_of_the_pairs_of_a_case_are_judged_by_the_floor_alone():
    assert len(gr.CASES) == 17 and all(c in gr.CASES for c in gr.PATH_CASES + gr.BATCH_CASES + (gr.WIDE_CASE,))
    for case in gr.CASES:
        for dt in gr.DTYPES:
            share = gr.reference(case, gr.dtype_name(dt)).floor_share()
            print("%-18s %-8s floor share %.4f" % (gr.case_name(case), gr.dtype_name(dt), share))
            assert share <= 0.01, (case, share)


def test_the_float64_restatement_of_the_expanded_form_meets_every_bar():
    """derived, not tuned: the same arithmetic in numpy's order stays well inside every bar, on every case"""
    worst = 0.0
    for case in gr.CASES:
        for dt in gr.DTYPES:
            ref = gr.reference(case, gr.dtype_name(dt))
            w, mean, iv = gr.model(case)
            j = gr.judge(ref, gr.restate(w, mean, iv, gr.frames(case, dt)))
            print("%-18s %-8s %s" % (gr.case_name(case), gr.dtype_name(dt), "  ".join("%s %.3g" % kv for kv in j.items())))
            worst = max(worst, max(j.values()))
            assert max(j.values()) <= 1.0, (case, j)
    print("largest ratio of the restatement to a bar: %.3g" % worst)
    assert worst < 0.5                                         # a bar the restatement only just met would be a tuned one


def _above(ref_values):
    return np.abs(ref_values.astype(np.float64)) > ORACLE_FLOOR


def test_the_oracle_meets_the_bars_above_its_linear_domain_floor():
    """oracle.llk / occ / em_accumulate / tv_stats, per pair and element, wherever the reference value is above 1e-250"""
    worst = {}
    for case in gr.CASES:
        for dt in gr.DTYPES:
            ref = gr.reference(case, gr.dtype_name(dt))
            w, mean, iv = gr.model(case)
            x = gr.frames(case, dt).astype(np.float64)
            og = orc.Gmm(w, mean, iv)
            got = {"llk": gr.ratio(orc.llk(og, x, -1e9, 1e9).astype(gr.LD) - ref.llk, ref.B)}
            got["occ"] = np.where(_above(ref.gamma), gr.ratio(orc.occ(og, x).astype(gr.LD) - ref.gamma, ref.dgamma), 0.0)
            em = orc.em_accumulate(og, x)
            s = ref.sums()
            for k in ("occ", "sx", "sxx"):
                got["em " + k] = np.where(_above(s[k]), gr.ratio(em[k].astype(gr.LD) - s[k], s[k + "_b"]), 0.0)
            ub = gr.ragged_bounds(ref.T)
            utt = np.repeat(np.arange(len(ub) - 1), np.diff(ub))
            No, Fo = orc.tv_stats(og, x, utt, len(ub) - 1)
            N, F, Nb, Fb = ref.utt_stats(ub)
            got["tv N"] = np.where(_above(N), gr.ratio(No.astype(gr.LD) - N, Nb), 0.0)
            got["tv F"] = np.where(_above(F), gr.ratio(Fo.reshape(F.shape).astype(gr.LD) - F, Fb), 0.0)
            for k, r in got.items():
                worst[k] = max(worst.get(k, 0.0), float(r.max()))
                assert r.max() <= 1.0, (case, gr.dtype_name(dt), k, float(r.max()), np.unravel_index(int(np.argmax(r)), r.shape))
    print("oracle, largest ratio per result: " + "  ".join("%s %.3g" % kv for kv in worst.items()))


def old_criteria(got, ref):
    """what the suite held before: -> (max |llk - ref|, the largest of max|a - b| / max|b| over occ, sx, sxx)"""
    s = ref.sums()
    rel = max(float(np.abs(got[k] - s[k].astype(np.float64)).max() / np.abs(s[k].astype(np.float64)).max()) for k in ("occ", "sx", "sxx"))
    return float(np.abs(got["llk"] - ref.llk.astype(np.float64)).max()), rel


def _drop_x2_term(tab):
    tab["neg_half_iv"][3, -1] = 0.0                              # Gaussian 3 loses the x^2 term of its last dimension


def _carriers(ref):
    """Gaussians that carry some frame (a posterior above 1e-12 somewhere): a defect in their rows is what the old criteria can see"""
    return (ref.g64 > 1e-12).any(0)


def _fp32_table(ref):
    def f(tab):
        rows = ~_carriers(ref)
        assert rows.sum() > 100
        tab["mu_iv"][rows] = tab["mu_iv"][rows].astype(np.float32).astype(np.float64)
    return f


def _row15_from_row14(ref):
    def f(gamma):
        out = gamma.copy()
        t = np.arange(15, gamma.shape[0], 16)
        near_zero = (gamma[t] < 1e-20) & (gamma[t - 1] < 1e-20)
        assert near_zero.mean() > 0.5
        out[t] = np.where(near_zero, gamma[t - 1], gamma[t])
        return out
    return ("gamma", f)


def test_value_only_defects_pass_the_old_criteria_and_miss_the_bars_by_orders_of_magnitude():
    """(1) one Gaussian's x^2 term dropped in one dimension of the packed table; (2) the mu iv table rounded to float32 -- in the rows
    of the Gaussians that carry no frame: rounded in EVERY row it moves the per-frame log-likelihoods by 1e-6 and the old 1e-9 does
    see it; (3) the posteriors of frame row 15 of each 16-frame block taken from row 14 for the Gaussians of near-zero posterior.
    Each leaves llk within 1e-9 and occ / sx / sxx within 1e-9 of the largest entry, and misses a per-pair bar by >= 10^3."""
    ref = gr.reference(DEFECT_CASE, "float32")
    w, mean, iv = gr.model(DEFECT_CASE)
    x = gr.frames(DEFECT_CASE, np.float32)
    clean = gr.restate(w, mean, iv, x)
    assert max(gr.judge(ref, clean).values()) <= 1.0
    for name, defect in (("x^2 term dropped", _drop_x2_term), ("fp32 mu iv rows", _fp32_table(ref)), ("row 15 from row 14", _row15_from_row14(ref))):
        got = gr.restate(w, mean, iv, x, defect)
        dl, rel = old_criteria(got, ref)
        j = gr.judge(ref, got)
        print("%-20s old criteria: llk abs %.3g, statistics rel-to-max %.3g;  ratios to the bars: %s"
              % (name, dl, rel, "  ".join("%s %.3g" % kv for kv in j.items())))
        assert dl < 1e-9 and rel < 1e-9, (name, dl, rel)         # the old criteria are satisfied
        assert j["gamma"] >= 1e3 and max(j["occ"], j["sx"], j["sxx"]) >= 1e3, (name, j)   # the bars are not, posteriors AND sums


def test_ratio_treats_an_empty_sum_and_a_nan_as_it_must():
    r = gr.ratio(np.array([0.0, 1e-300, np.nan, 1.0]), np.array([0.0, 0.0, 1.0, 2.0]))
    assert r[0] == 0.0 and r[1] == np.inf and r[2] == np.inf and r[3] == 0.5
