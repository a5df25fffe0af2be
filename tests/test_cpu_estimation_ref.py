"""The references and bars of tests/estimation_ref.py, shown to bite without a GPU.

* every case completes in the 80-bit reference, the float64 restatement and the oracle (no "not positive definite"), and the
  restatement and the oracle pass every bar on every unit of every case -- the EM iteration over two iterations, the second from
  the oracle's own doubles after the first;
* the route tv_orthonormalize_t must take is stated for every case from dmin / dmax of the 80-bit factor, and the restatement takes it;
* each of six planted defects of the restatement is rejected by its bar, and at least half of them pass the whole-array criterion
  tests/test_gpu_tv.py applies to the same entry point (the share is printed): the gap the per-unit files close is real.
"""
import numpy as np
import pytest

import estimation_ref as er

pytestmark = pytest.mark.skipif(not er.HAVE_LONGDOUBLE, reason=er.SKIP_MESSAGE)


def relerr(a, b):
    """the criterion of tests/test_gpu_tv.py"""
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def top(r):
    return max((float(np.max(v, initial=0.0)) for v in r.values()), default=0.0)


# ---------------------------------------------------------------- every case, the restatement and the oracle
@pytest.mark.parametrize("entry", list(er.ENTRIES))
def test_the_restatement_and_the_oracle_pass_every_bar(entry):
    e = er.ENTRIES[entry]
    worst, gap, bad = {}, {}, []
    for key in e.cases:
        for who, got in (("restatement", e.restate(key)), ("oracle", e.oracle(key))):
            for kind, r in er.judge(entry, key, got).items():
                w = float(np.max(r, initial=0.0))
                worst[(who, kind)] = max(worst.get((who, kind), 0.0), w)
                if not w <= 1.0:
                    bad.append("%s | %s | %s | %s: %.3g" % (entry, er.case_name(key), who, kind, w))
        d, o = er.err_double(entry, key), er.err_oracle(entry, key)
        for kind in d:
            if not kind.startswith("!") and d[kind].size:
                floor = 64 * er.u
                g = np.maximum(o[kind], floor) / np.maximum(d[kind], floor)
                gap[kind] = (max(gap.get(kind, (1.0, 1.0))[0], float(g.max())), min(gap.get(kind, (1.0, 1.0))[1], float(g.min())))
    for (who, kind), w in sorted(worst.items()):
        print("%-20s %-12s %-28s worst |error| / bar %.3g" % (entry, who, kind, w))
    for kind, (hi, lo) in sorted(gap.items()):
        print("%-20s err_oracle / err_double (both floored at 64 u), %-22s between %.3g and %.3g" % (entry, kind, lo, hi))
    assert not bad, "\n".join(bad[:30])


@pytest.mark.parametrize("name", list(er.EM_CASES))
def test_em_iterations_complete_and_pass_every_bar(name):
    """two iterations, the second from the oracle's doubles; also from the restatement's: a state that is symmetric only to rounding"""
    for chain in ("oracle", "restatement"):
        state = er.em_inputs(name)
        for it in range(2):
            ref, dbl, orc = er.em_bars(state)
            outs = {"restatement": er.em_restate(*state), "oracle": er.em_oracle(*state)}
            for who, got in outs.items():
                assert np.array_equal(got[0].view(np.int64), er.em_centred(state).view(np.int64)), (name, it, who, "centred X is not X - Delta")
                r = er.em_judge(state, got)
                print("%-22s from the %s's state, iteration %d, %-12s %s" % (name, chain, it + 1, who, {k: float("%.3g" % v.max()) for k, v in r.items()}))
                assert top(r) <= 1.0, (name, chain, it, who, r)
            assert np.isfinite(np.linalg.cond(outs["oracle"][3])) and np.linalg.cond(outs["oracle"][3]) <= 1e4
            o = outs[chain]
            state = (o[0], state[1], o[1], o[2], o[3], o[4])


def test_only_sets_with_more_than_two_sessions_per_dimension_go_to_the_inverses():
    assert [s for s in er.DEV_SETS if er.invertible(s)] == list(er.INV_DEV_SETS) and not er.invertible("3x[1,2,1]")
    assert sorted({er.dev_set(s)[0].shape[0] for s in er.INV_DEV_SETS}) == [1, 2, 5, 8, 33, 34, 65]


def test_the_references_are_what_the_units_are_measured_against():
    """eigen: the 80-bit pairs have no residual, are orthonormal and reproduce the matrix; efr whitens; lda solves B l = lambda W l"""
    for mkey in (("spd", 33, 1e6), ("dev", "33x257 scaled", "Sigma"), ("repeated", 3, 0)):
        A = er.ld(er.eigen_matrix(mkey))
        vect, val = er.eigen_reference((mkey, A.shape[0]))
        scale = float(np.max(np.abs(val)))
        assert float(np.max(np.abs(er.mm(A, vect) - vect * val))) <= 2.0 ** -56 * scale
        assert float(np.max(np.abs(er.mm(vect.T, vect) - np.eye(A.shape[0])))) <= 2.0 ** -56
        if mkey[0] != "repeated":
            M = er.efr_reference(mkey)
            assert float(np.max(np.abs(er.mm(er.mm(M, A), M.T) - np.eye(A.shape[0])))) <= 2.0 ** -56 * float(val[0] / val[-1])    # times cond(S)
    for mkey in (("spd", 33, 1e6), ("dev", "65x[2]*100", "W,B")):
        W, B = (er.ld(a) for a in er.lda_inputs(mkey))
        rows, val = er.lda_reference((mkey, W.shape[0]))
        res = er.mm(rows, B.T) - val[:, None] * er.mm(rows, W.T)
        assert float(np.max(np.abs(res))) <= 2.0 ** -60 * W.shape[0] * float(np.max(np.abs(B)) + np.max(val) * np.max(np.abs(W)))     # the terms that cancel
        assert float(np.max(np.abs(er.nrm(rows, 1) - 1))) <= 2.0 ** -60


# ---------------------------------------------------------------- the routes of tv_orthonormalize_t
def test_the_route_of_every_orthonormalize_case_is_stated_and_the_restatement_takes_it():
    for R, SV in er.ORTHO_SHAPES:
        assert er.ortho_route((R, SV, "plain")) == "gram"
        ratio = er.ortho_reference((R, SV, "row at 2e-4"))[1]
        assert er.ortho_route((R, SV, "row at 2e-4")) == "gram" and (R == 1 or abs(ratio / 2e-4 - 1) < 1e-9)
        ratio = er.ortho_reference((R, SV, "row at 5e-5"))[1]
        assert er.ortho_route((R, SV, "row at 5e-5")) == ("gram" if R == 1 else "step") and (R == 1 or abs(ratio / 5e-5 - 1) < 1e-9)
    for key in er.ORTHO_CASES:
        if key[2].startswith("zero row"):
            assert er.ortho_route(key) == "step" and not er.ortho_restate(key)[int(key[2].split()[-1])].any()
        T = er.ortho_inputs(key)
        try:                                                   # the route the float64 factor chooses is the one the 80-bit factor states
            d = np.diag(np.linalg.cholesky(T @ T.T))
            took = "gram" if d.min() > er.ROUTE_THRESHOLD * d.max() else "step"
        except np.linalg.LinAlgError:
            took = "step"
        assert took == er.ortho_route(key), key
    assert max(SV for _, SV in er.ORTHO_SHAPES) > 512 * 256       # the grid-stride loop of k_gs_update takes a second trip


# ---------------------------------------------------------------- planted defects
def em_defect(variant, defect):
    state = er.em_inputs(variant)
    got = er.em_restate(*state, defect=defect)
    r = dict(er.em_judge(state, got))
    r["!bits of X - Delta"] = np.array([0.0 if np.array_equal(got[0].view(np.int64), er.em_centred(state).view(np.int64)) else np.inf])
    o = er.em_oracle(*state)
    old = all(relerr(g, w) < 1e-8 for g, w in zip(got, o) if w.size)          # test_plda_em_iterations_match_oracle
    return r, old


def mahalanobis_defect():
    name = "33x257 scaled"
    got = er.mahalanobis_restate(name, er.INVERSE_DEFECT)
    from oracle import oracle as orc
    X, sps = er.dev_set(name)
    old = relerr(got, np.linalg.inv(orc.dev_cov_mat(X, sps)[1])) < 1e-8                      # test_backend_estimation_matches_oracle
    return er.judge("dev_mahalanobis", name, got), old


def ortho_defect():
    key = (24, 1000, "zero row 12")
    got = er.ortho_restate(key, er.ORTHO_DEFECT)
    keep = [i for i in range(24) if i != 12]
    old = relerr(got, er.ortho_oracle(key)) < 1e-10 and np.allclose(got[keep] @ got[keep].T, np.eye(23), atol=1e-10) and not got[12].any()
    return er.judge("tv_orthonormalize_t", key, got), old


def eigen_defect():
    key = (("spd", 33, 1e3), 33)
    vect, val = er.eigen_restate(key, er.EIGEN_DEFECT)
    S = er.eigen_matrix(key[0])
    ov, ol = er.eigen_oracle(key)
    old = (np.all(np.diff(val) <= 0) and np.allclose(vect @ np.diag(val) @ vect.T, S, atol=1e-10 * val[0]) and relerr(val, ol) < 1e-12
           and relerr(np.abs(vect), np.abs(ov)) < 1e-8)                                        # test_efr_lda_and_eigen
    return er.judge("sym_eigen", key, (vect, val)), old


DEFECTS = {
    er.INVERSE_DEFECT: mahalanobis_defect,
    er.EM_DEFECTS[0]: lambda: em_defect("33x7x3 257 speakers, 257th a twin of the 1st", er.EM_DEFECTS[0]),
    er.EM_DEFECTS[1]: lambda: em_defect("8x3x2 [600,1,2], last of the 600 sessions faint", er.EM_DEFECTS[1]),
    er.EM_DEFECTS[2]: lambda: em_defect("5x2x1 [1,2,1,3], Delta 1e-10", er.EM_DEFECTS[2]),
    er.ORTHO_DEFECT: ortho_defect,
    er.EIGEN_DEFECT: eigen_defect,
}


@pytest.fixture(scope="module")
def defects():
    return {name: fn() for name, fn in DEFECTS.items()}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_each_planted_defect_is_rejected_by_its_bar(defects, name):
    r, old = defects[name]
    print("%-95s |error| / bar %.3g in %r; the whole-array criterion of test_gpu_tv.py %s it" % (
        name, top(r), max(r, key=lambda k: np.max(r[k], initial=0.0)), "passes" if old else "rejects"))
    assert top(r) > 1.0, (name, {k: float(np.max(v, initial=0.0)) for k, v in r.items()})


def test_the_variants_of_the_em_defects_pass_without_the_defect():
    for variant in er.EM_VARIANTS:
        r, old = em_defect(variant, None)
        assert top(r) <= 1.0 and old, (variant, r)


def test_at_least_half_of_the_defects_pass_the_whole_array_thresholds(defects):
    passed = [name for name, (_, old) in defects.items() if old]
    print("%d of %d planted defects pass the whole-array thresholds of tests/test_gpu_tv.py: %s" % (len(passed), len(defects), "; ".join(passed)))
    assert 2 * len(passed) >= len(defects)
