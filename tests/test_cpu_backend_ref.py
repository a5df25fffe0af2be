"""tests/backend_ref.py checked on its own, without a GPU: a float64 numpy restatement of the device's formulation (the expansion of
the scoring rules, BLAS sums, LAPACK inverses) and the double oracle stay within a quarter of every bar on every case and every
element -- the bars that ARE the count of a pointwise formula's roundings within the ceiling that count allows (CEILING) --
and four value-only defects pass the whole-array criterion tests/test_gpu_tv.py applies to their entry point while they miss the
new bar by >= 10 x."""
import numpy as np
import pytest

import backend_ref as br

pytestmark = pytest.mark.skipif(not br.HAVE_LONGDOUBLE, reason=br.SKIP_MESSAGE)

QUARTER = 0.25
# Where a bar IS the count of the roundings of a pointwise formula a quarter cannot hold; the ceiling is then the share of the bar
# that the formula's own roundings can reach at worst:
CEILING = {"centring": 1.0,         # one rounding against u (|x| + |mu|)
           "mean": 0.5,             # a mean of two vectors: two roundings against (2 + 2) u; longer sums err as random walks, far below
           "estimate_z": 0.625,     # tau form: five roundings against 8 u; the other form's seven are damped by n v d^2 / (1 + n v d^2)
           "m + DZ": 0.5,           # no factor product: D Z, + m, * N, F - ..: four roundings against 8 u
           "norm_statistics": 0.75}  # m N, the difference, sqrt, the product: u |m N| + 3 u |F - m N| <= 3 u (|F| + |m N|) against 4 u (..)


def worst(r):
    return float(np.max(r)) if np.size(r) else 0.0


# ---------------------------------------------------------------- scoring
@pytest.mark.parametrize("dim", br.SCORE_DIMS)
def test_scoring_restatement_and_oracle_stay_within_a_quarter_of_every_trials_bar(dim):
    top, acc = {}, {}
    for M, S in br.SCORE_COUNTS:
        for rule in br.RULES:
            key = (dim, M, S, "cosine" if rule == "cosine" else "plain")
            ref, bar = br.score_reference(key, rule)
            assert np.all(bar > 0) and np.all(np.isfinite(ref.astype(np.float64)))
            for name, got in (("numpy", br.score_restate(key, rule)), ("oracle", br.score_oracle(key, rule))):
                r = worst(br.ratio(br.ld(got) - ref, bar))
                top[(rule, name)] = max(top.get((rule, name), 0.0), r)
                assert r <= QUARTER, (rule, name, M, S, r)
            acc[rule] = max(acc.get(rule, 0.0), br.target_accuracy(key, rule, br.score_restate(key, rule)))
    print("dim %-3d error / bar: %s;  target trials |error| / |score|: %s"
          % (dim, "  ".join("%s %s %.3g" % (k[0], k[1], v) for k, v in sorted(top.items())), "  ".join("%s %.2g" % kv for kv in sorted(acc.items()))))


def test_scoring_inputs_are_what_the_file_says():
    p = br.score_case(33, 33, 31)
    m, s = p["m"], p["s"]
    assert p["exact"] == 0 and np.array_equal(m[:, 0], s[:, 0]) and p["fm"] == 16 and p["fs"] == 15
    nm, ns = np.linalg.norm(m, axis=0), np.linalg.norm(s, axis=0)
    assert nm[16] < 1e-4 * np.median(nm) and ns[15] < 1e-4 * np.median(ns) and ns[30] > 0.1 * np.median(ns)
    for i in p["targets"][1:]:
        assert 1e-4 < np.linalg.norm(m[:, i] - s[:, i]) / nm[i] < 1e-2
    assert len(p["targets"]) == 29
    q = br.score_case(33, 33, 33, "self")
    assert q["s"] is q["m"]


@pytest.mark.parametrize("counts", list(br.PLDA_COUNTS))
def test_plda_session_counts_and_a_second_model(counts):
    ns = br.PLDA_COUNTS[counts]
    key = (40 if len(ns) > 1 else 5, len(ns), 7, "plda " + counts)
    for which in ("FTJF", "FTJF2"):
        ref, bar = br.score_reference(key, "plda", which)
        for name, got in (("numpy", br.score_restate(key, "plda", which)), ("oracle", br.score_oracle(key, "plda", which))):
            r = worst(br.ratio(br.ld(got) - ref, bar))
            print("plda %-22s %-5s %-6s kappa %.3g  error / bar %.3g" % (counts, which, name, br.plda_model(key, which, int(max(ns)))[3], r))
            assert r <= QUARTER
    # a stale K_n (the first model's on the second model's call) misses the bar: what the FTJF cache of the context must not do
    ref2, bar2 = br.score_reference(key, "plda", "FTJF2")
    assert worst(br.ratio(br.ld(br.score_restate(key, "plda", "FTJF")) - ref2, bar2)) > 10.0


def test_two_scoring_defects_pass_the_old_criterion_and_miss_the_trials_bar():
    """(1) s^T Q_s s of the last segment (the column next to the pad, a quiet segment at 0.05 of the others) off by 1e-9 relative,
    Mahalanobis; (2) the cross term of the trial (faint model, faint segment) off by 1e-3 relative, two-covariance"""
    for key, rule, defect in (((33, 33, 31, "quiet last"), "mahalanobis", br.SCORE_DEFECTS[0]), ((33, 33, 31, "plain"), "twocov", br.SCORE_DEFECTS[1])):
        ref, bar = br.score_reference(key, rule)
        clean, bad = br.score_restate(key, rule), br.score_restate(key, rule, defect=defect)
        assert worst(br.ratio(br.ld(clean) - ref, bar)) <= QUARTER
        old, new = br.relerr(bad, ref), worst(br.ratio(br.ld(bad) - ref, bar))
        print("%-34s %-12s old criterion %.3g (threshold %.0e);  error / bar %.3g" % (defect, rule, old, br.OLD_SCORE_THRESHOLD[rule], new))
        assert old < br.OLD_SCORE_THRESHOLD[rule] and new >= 10.0


# ---------------------------------------------------------------- iv_normalize
@pytest.mark.parametrize("shape", br.IVN_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_iv_normalize_restatement_and_oracle(shape):
    from oracle import oracle as orc
    p = br.ivn_inputs(*shape)
    for mean, M, ln in br.IVN_FORMS:
        mu, Mx = (p["mean"] if mean else None), (p["M"] if M else None)
        ref, bar = br.ivn_reference(p["X"], mu, Mx, ln)
        for name, got in (("numpy", br.ivn_restate(p["X"], mu, Mx, ln)), ("oracle", orc.iv_normalize(p["X"], mu, Mx, ln))):
            r = worst(br.ratio(br.ld(got) - ref, bar))
            print("iv_normalize %s mean %-5s M %-5s length_norm %-5s %-6s error / bar %.3g" % (shape, bool(mean), bool(M), ln, name, r))
            # no mean, no M, no length_norm: a copy (bar 0); the mean alone: ONE rounding, u (|x| + |mu|) is the bound itself
            assert r <= (QUARTER if (M or ln) else CEILING["centring"] if mean else 0.0)


def test_iv_normalize_tiny_columns_in_double_and_in_long_double():
    """norm 1e-150: the squared norm 1e-300 is a normal double, the column is normalised like any other.  norm 1e-170: the squared
    norm is 0 in double, so the reference project's lengthNorm (a double sum, sqrt, a division: PldaTools.cpp:3706-3751) divides
    by 0 and the oracle with it; the long-double reference holds a unit vector.  The library is held to the reference project."""
    from oracle import oracle as orc
    X = br.ivn_tiny_columns()
    ref, bar = br.ivn_reference(X, None, None, True)
    assert np.all(np.isfinite(ref.astype(np.float64))) and abs(float(br.norm2(ref[:, 5])) - 1.0) < 1e-15
    o = orc.iv_normalize(X, None, None, True)
    fin = [j for j in range(7) if j != 5]
    assert worst(br.ratio(br.ld(o)[:, fin] - ref[:, fin], bar[:, fin])) <= QUARTER
    assert not np.isfinite(o[:, 5]).any()


# ---------------------------------------------------------------- development set
@pytest.mark.parametrize("name", list(br.DEV_CASES))
def test_dev_set_restatement_and_oracle(name):
    X, sps = br.dev_inputs(name)
    assert X.shape[1] == sps.sum()
    for who, got in (("numpy", br.dev_restate(name)), ("oracle", br.dev_oracle(name))):
        j = {q: worst(r) for q, r in br.dev_judge(name, got).items()}
        print("%-24s %-6s %s" % (name, who, "  ".join("%s %.3g" % kv for kv in j.items())))
        assert max(v for q, v in j.items() if q not in ("mean", "smean")) <= QUARTER and max(j["mean"], j["smean"]) <= CEILING["mean"], (who, j)
    if name == "1x[1]":
        r = br.dev_reference(name)
        assert not r["W"][0].any() and not r["B"][0].any() and not br.dev_oracle(name)["W"].any()


def test_dev_set_defect_in_a_faint_dimension():
    name = br.DEV_DEFECT_CASE
    ref = br.dev_reference(name)
    W = ref["W"][0].astype(np.float64)
    assert abs(W[5, 7]) < 1e-9 * W[0, 0]                       # the faint dimensions against dimension 0
    bad = br.dev_restate(name, br.DEV_DEFECT)
    old, new = br.relerr(bad["W"], ref["W"][0]), worst(br.dev_judge(name, {"W": bad["W"]})["W"])
    print("%s: old criterion %.3g (threshold 1e-12);  error / bar %.3g" % (br.DEV_DEFECT, old, new))
    assert old < 1e-12 and new >= 10.0


# ---------------------------------------------------------------- JFA
@pytest.mark.parametrize("shape", br.JFA_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_jfa_restatement_and_oracle(shape):
    from oracle import oracle as orc
    p = br.jfa_inputs(*shape)
    C, D = p["C"], p["D"]
    f = br.jfa_faint(C)
    assert p["Nh"][:, f].max() < 1e-8 * np.delete(p["Nh"], f, 1).max() and (p["Nh"] == 0).sum() == 1
    j = {}
    for form in br.JFA_SUBTRACT_FORMS:
        N, F, kw = br.jfa_subtract_args(p, form)
        ref, bar = br.jfa_subtract_reference(N, F, D, **kw)
        j["subtract " + form + " numpy"] = worst(br.ratio(br.ld(br.jfa_subtract_restate(N, F, D, **kw)) - ref, bar))
        j["subtract " + form + " oracle"] = worst(br.ratio(br.ld(orc.jfa_subtract(N, F, kw.get("owner"), kw.get("means"), kw.get("T"), kw.get("W"),
                                                                              kw.get("Dm"), kw.get("Z"))) - ref, bar))
    ref, bar = br.jfa_sessions_reference(p)
    j["sessions numpy"] = worst(br.ratio(br.ld(br.jfa_sessions_restate(p)) - ref, bar))
    j["sessions oracle"] = worst(br.ratio(br.ld(orc.jfa_subtract_sessions(p["sb"], p["Nh"], p["F"], p["Um"], p["X"])) - ref, bar))
    print("jfa %s: %s" % (shape, "  ".join("%s %.3g" % kv for kv in j.items())))
    assert max(v for q, v in j.items() if "m + DZ " not in q) <= QUARTER and max(j.values()) <= CEILING["m + DZ"], j
    k = {}
    for tau in (-1.0, 14.0):
        ref, bar = br.jfa_z_reference(p, tau)
        k["z tau %g numpy" % tau] = worst(br.ratio(br.ld(br.jfa_z_restate(p, tau)) - ref, bar))
        k["z tau %g oracle" % tau] = worst(br.ratio(br.ld(orc.jfa_estimate_z(p["N"], p["F"], p["iv"], p["Dm"], tau)) - ref, bar))
    z, zbar, d, dbar = br.jfa_zd_reference(p)
    zn, dn = br.jfa_zd_restate(p)
    zo, do = orc.jfa_estimate_z_and_d(p["N"], p["F"], p["iv"], p["Dm"])
    k["z_and_d Z numpy"], k["z_and_d Z oracle"] = worst(br.ratio(br.ld(zn) - z, zbar)), worst(br.ratio(br.ld(zo) - z, zbar))
    k["z_and_d D numpy"], k["z_and_d D oracle"] = worst(br.ratio(br.ld(dn) - d, dbar)), worst(br.ratio(br.ld(do) - d, dbar))
    print("jfa %s: %s" % (shape, "  ".join("%s %.3g" % kv for kv in k.items())))
    assert max(k.values()) <= CEILING["estimate_z"] and max(k["z_and_d D numpy"], k["z_and_d D oracle"]) <= QUARTER, k


def test_jfa_defect_on_the_straddling_speaker_and_the_faint_gaussian():
    p = br.jfa_inputs(6, 5, 3)
    ref, bar = br.jfa_sessions_reference(p)
    bad = br.jfa_sessions_restate(p, br.JFA_DEFECT)
    old, new = br.relerr(bad, ref), worst(br.ratio(br.ld(bad) - ref, bar))
    print("%s: old criterion %.3g (threshold 1e-12);  error / bar %.3g" % (br.JFA_DEFECT, old, new))
    assert old < 1e-12 and new >= 10.0
    # what the batch sizes of the GPU file are there for: under both the straddler spans three windows; 4 gives full windows with
    # empty speakers at a window's front, in its middle and in a run; 5 a short last window of sessions and of jfa_subtract's rows
    sb, nsess, nspk = p["sb"], p["nsess"], p["nspk"]
    assert nsess == sb[-1] == 24 and br.JFA_BATCHES == (4, 5)
    assert all(len(br.jfa_windows_spanned(br.JFA_STRADDLER, b)) == 3 for b in br.JFA_BATCHES)
    assert nsess % 4 == 0 and nspk % 4 != 0 and nsess % 5 != 0 and nspk % 5 != 0
    empty = [i for i in range(nspk) if sb[i] == sb[i + 1]]
    assert empty == [1, 6, 7] and sb[6] % 4 == 0 and sb[1] % 4 != 0


# ---------------------------------------------------------------- approximate extractors
@pytest.mark.parametrize("shape", br.AX_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_approximate_extractors_restatement_and_oracle(shape):
    a = br.approx(*shape)
    re, orc_ = a.restate(), a.oracle()
    for who, got in (("numpy", re), ("oracle", orc_)):
        j = {k: worst(v) for k, v in a.judge(got).items()}
        print("approx %s %-6s %s  cond(L) max %.3g" % (shape, who, "  ".join("%s %.3g" % kv for kv in j.items()), a.cond.max()))
        assert max(j[k] for k in ("Fs", "Wm", "Dm", "Tn")) <= QUARTER and j["Fn"] <= CEILING["norm_statistics"], j
    for which in ("ubm", "eig"):
        r = worst(a.w_ratios(which, re[which]))
        print("approx %s estimate_w %s numpy: error / bar %.3g (oracle error at most %.3g)" % (shape, which, r, a.err_oracle[which].max()))
        assert r <= QUARTER
        assert not np.asarray(re[which])[br.tr.EMPTY_UTT].any()


def test_ratio_treats_a_zero_bar_and_a_nan_as_it_must():
    r = br.ratio(np.array([0.0, 1e-300, np.nan, 1.0]), np.array([0.0, 0.0, 1.0, 2.0]))
    assert r[0] == 0.0 and r[1] == np.inf and r[2] == np.inf and r[3] == 0.5
