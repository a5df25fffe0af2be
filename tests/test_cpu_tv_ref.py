"""tests/tv_ref.py checked on its own, without a GPU: two independent double-precision restatements of the E-step chain -- the CPU
oracle (Gauss-Jordan) and float64 numpy through np.linalg.inv (LU) -- stay within a quarter of every bar on every case, so the bars
are not fitted to one algorithm; and value-only defects of the numpy restatement miss a bar by >= 100 x while the criteria the
suite held this chain to before (max|a - b| / max|b| < 1e-9 over W, A, Cmx, Rm, r; 1e-12 on TETt) read below their thresholds."""
import numpy as np
import pytest

import spd_ref as sr
import tv_ref as tr
from oracle import oracle as orc

pytestmark = pytest.mark.skipif(not tr.HAVE_LONGDOUBLE, reason=tr.SKIP_MESSAGE)

# the order-160 reference takes 10 s of CPU: the GPU file builds it, this one leaves it out
CPU_CASES = tuple(c for c in tr.ESTEP_CASES if c[2] <= 100)
DEFECT_CASE = tr.ESTEP_CASES[4]            # 8 x 12 x 92 x 129
QUARTER = 0.25


def oracle_acc(p, U):
    o = orc.tv_estimate_a_and_c(p.N[:U], p.F0[:U], p.Tm, p.invvar, p.te_full)
    o["A"] = sr.pack(o["A"].reshape(p.C, p.R, p.R))
    o["meanW"] = o["r"]                    # the library returns the sum, the oracle the mean
    return o


@pytest.mark.parametrize("case", CPU_CASES, ids=tr.case_name)
def test_both_restatements_stay_within_a_quarter_of_every_bar(case):
    p = tr.case_problem(case)
    assert len(tr.ESTEP_CASES) == 10 and len(CPU_CASES) == 9
    N = p.N
    # the inputs are what the file says they are
    assert not N[tr.EMPTY_UTT].any() and (N > 0).any(0).all() and 0.2 < (N == 0).mean() < 0.45
    loud = N.sum(1)
    assert loud[loud > 0].max() / loud[loud > 0].min() >= 1e6
    others = np.delete(N, p.faint, 1)
    assert N[:, p.faint].max() < 1e-6 * others.max()
    for U in case[3]:
        assert (N[:min(U, 5)] > 0).any(0).all()
        for name, got in (("oracle", oracle_acc(p, U)), ("numpy inv", tr.restate(p, U))):
            j = tr.judge(p, got, U)
            print("%-14s U %-4d cond(L_u) %s  %-9s %s" % (tr.case_name(case), U, p.cond_stats(U), name, "  ".join("%s %.3g" % kv for kv in j.items())))
            assert max(j.values()) <= QUARTER, (name, U, j)
            assert not np.asarray(got["W"])[tr.EMPTY_UTT].any()
    # the links before and after the E-step: the oracle in its own order
    U = max(case[3])
    F0o = orc.tv_subtract_m(p.N, p.F, p.means)
    assert tr.ratio(F0o.astype(tr.LD) - p.F0_ref, p.F0_bar).max() <= 1.0          # 2 u is the bound itself: two roundings
    teo = sr.pack(orc.tv_tett(p.Tm, p.invvar, p.C, p.D))
    r = tr.ratio(teo.astype(tr.LD) - p.te_ref, p.te_bar).max()
    print("%-14s oracle TETt %.3g of its bar" % (tr.case_name(case), r))
    assert r <= QUARTER
    m = p.mstep(U)
    A_full = sr.unpack(m["A"], p.R)
    Cb = m["Cmx"].reshape(p.R, p.C, p.D)
    Tn = np.stack([np.linalg.solve(A_full[c], Cb[:, c, :]) for c in range(p.C)], 1).reshape(p.R, p.C * p.D)
    r = p.mstep_ratios(Tn, m).max()
    print("%-14s update_t: oracle error at most %.3g, numpy solve %.3g of its bar" % (tr.case_name(case), m["err_oracle"].max(), r))
    assert r <= QUARTER


def test_value_only_defects_pass_the_old_criteria_and_miss_the_bars_by_two_orders_of_magnitude():
    """(1) A += N^T E reads the faint Gaussian's column of N one utterance off; (2) the i-vector of the quietest utterance off by
    1e-6; (3) one utterance dropped from the faint Gaussian's block of Cmx -- each leaves every old criterion satisfied and misses
    a bar by >= 100 x.  (4) TETt of the faint Gaussian without its last k term is seen by both: TETt does not scale with the
    occupancy, so the old 1e-12 on TETt reads 0.2, and it moves W past 1e-9 too.  It is reported and does not count."""
    p = tr.case_problem(DEFECT_CASE)
    U = max(DEFECT_CASE[3])
    clean = tr.restate(p, U)
    assert max(tr.judge(p, clean, U).values()) <= QUARTER
    assert all(v < t for v, t in tr.old_criteria(p, clean, U).values())
    unseen_and_caught = []
    for d in tr.DEFECTS:
        got = tr.restate(p, U, d)
        j = tr.judge(p, got, U)
        old = tr.old_criteria(p, got, U)
        seen = [k for k, (v, t) in old.items() if not v < t]
        print("%-14s old criteria: %s (%s);  ratios to the bars: %s" % (d, "  ".join("%s %.2g" % (k, v[0]) for k, v in old.items()),
                                                                     "seen by " + ", ".join(seen) if seen else "all satisfied",
                                                                     "  ".join("%s %.3g" % kv for kv in j.items())))
        assert max(j.values()) >= 100.0, (d, j)                 # every defect misses a bar
        if not seen:
            unseen_and_caught.append(d)
    assert unseen_and_caught == ["A neighbour", "quiet w", "Cmx utterance"]


def test_the_faint_gaussian_and_the_quiet_utterance_are_where_the_old_criterion_is_blind():
    """what the table of defects rests on: the faint Gaussian's rows of A and Cmx are 1e-6 or less of the largest entry of their
    arrays, and the quietest i-vector is decades below the loudest"""
    p = tr.case_problem(DEFECT_CASE)
    U = max(DEFECT_CASE[3])
    s = p.sums(U)
    A = np.abs(s["A"].astype(np.float64))
    Cm = np.abs(s["Cmx"].astype(np.float64)).reshape(p.R, p.C, p.D)
    assert A[p.faint].max() < 1e-6 * A.max() and Cm[:, p.faint].max() < 1e-6 * Cm.max()
    wn = p.wn.astype(np.float64)
    assert wn[tr.quiet_utterance(p, U)] < 1e-3 * wn.max()


def test_min_divergence_bars_hold_for_a_float64_restatement_and_reject_a_defect():
    for R in tr.MD_RANKS:
        m = tr.md_problem(R)
        n = m["n"]
        rn = m["r"] / n
        Rn = m["Rm"] / n - np.outer(rn, rn)
        Ch = np.linalg.cholesky(Rn).T                             # LAPACK's factor, BLAS products
        j = {k: float(v.max()) for k, v in tr.md_judge(m, Rn, rn, m["means"] + m["meanW"] @ m["T"], Ch @ m["T"]).items()}
        print("R %d: oracle Ch T error at most %.3g;  numpy: %s" % (R, m["err_oracle"].max(), "  ".join("%s %.3g" % kv for kv in j.items())))
        assert max(j.values()) <= 1.0 and j["mean"] <= QUARTER and j["Ch T"] <= QUARTER     # Rn and r / n are bounds on 2-4 roundings
        # the last row of Ch (its diagonal entry alone) scaled by 1 + 1e-8: the last row of Ch T moves, far below the old 1e-7
        Cd = Ch.copy()
        Cd[-1] *= 1.0 + 1e-8
        Td = Cd @ m["T"]
        jd = tr.md_judge(m, Rn, rn, m["means"], Td)
        assert jd["Ch T"].max() >= 100.0 and tr.relerr(Td, m["Tn"]) < 1e-7


def test_ratio_treats_an_empty_sum_and_a_nan_as_it_must():
    r = tr.ratio(np.array([0.0, 1e-300, np.nan, 1.0]), np.array([0.0, 0.0, 1.0, 2.0]))
    assert r[0] == 0.0 and r[1] == np.inf and r[2] == np.inf and r[3] == 0.5
