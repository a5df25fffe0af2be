"""The list form of the i-vector scoring rules (include/gmmiv_iv_trials.h), the parts that need no GPU: the symbols, the argument checks
(made before the context is looked at), the host planner against its numpy mirror, the ndx loader of the host layer, two source checks
and the yardstick of the GPU test: a float64 emulation of the documented summation order against the bars of tests/backend_ref.py."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import backend_ref as br
import iv_trials_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL = ct.c_void_p(0)
RULE_SYMBOLS = ("gmmiv_score_cosine_trials", "gmmiv_score_mahalanobis_trials", "gmmiv_score_twocov_trials", "gmmiv_score_plda_trials")


def _p(a):
    return ct.c_void_p(a.ctypes.data)


def _call(rule, dim, M, S, tm, ts, nsess=None, ctx=NULL, ntrial=None):
    """one list call with a NULL context on host arrays -> (rc, message); nothing may be written"""
    from lia_ral_amd import capi
    m, s = np.ones((dim, max(M, 1))), np.ones((dim, max(S, 1)))
    Q = np.eye(dim)
    tm, ts = np.ascontiguousarray(tm, np.int32), np.ascontiguousarray(ts, np.int32)
    n = len(tm) if ntrial is None else ntrial
    out = np.full(max(len(tm), 1), 99.0)
    head = (ctx, dim, ct.c_int64(M), ct.c_int64(S), _p(m))
    tail = (_p(tm), _p(ts), ct.c_int64(n), _p(out))
    if rule == "cosine":
        rc = capi.lib.gmmiv_score_cosine_trials(*head, _p(s), *tail)
    elif rule == "mahalanobis":
        rc = capi.lib.gmmiv_score_mahalanobis_trials(*head, _p(s), _p(Q), *tail)
    elif rule == "twocov":
        rc = capi.lib.gmmiv_score_twocov_trials(*head, _p(s), _p(Q), _p(Q), *tail)
    else:
        ns = np.ascontiguousarray(np.ones(max(M, 1)) if nsess is None else nsess, np.int64)
        rc = capi.lib.gmmiv_score_plda_trials(*head, _p(ns), _p(s), _p(Q), *tail)
    assert np.all(out == 99.0)
    return rc, capi.lib.gmmiv_last_error().decode()


def test_symbols_of_the_new_header_are_exported():
    from lia_ral_amd import capi
    hdr = open(os.path.join(ROOT, "include", "gmmiv_iv_trials.h")).read()
    assert '#include "gmmiv.h"' in hdr
    names = set(re.findall(r"^(?:int|int64_t)\s+(gmmiv_\w+)\s*\(", hdr, re.M))
    assert set(RULE_SYMBOLS) | {"gmmiv_plan_iv_trial_tiles", "gmmiv_iv_trial_anchor", "gmmiv_iv_trial_piece"} == names
    for name in names:
        assert hasattr(capi.lib, name), name
    for name in ("score_cosine_trials", "score_mahalanobis_trials", "score_twocov_trials", "score_plda_trials", "iv_trial_piece"):
        assert hasattr(capi.Context, name), name
    assert capi.IV_TRIAL_PIECE == int(re.search(r"#define GMMIV_IV_TRIAL_PIECE (\d+)", hdr).group(1))
    main = open(os.path.join(ROOT, "include", "gmmiv.h")).read()
    assert not any(n in main for n in names)                            # the prototypes live in the new header alone


@pytest.mark.parametrize("rule", ir.LIST_RULES)
def test_bad_arguments_are_refused_before_the_context_is_looked_at(rule):
    rc, msg = _call(rule, 4, 3, 5, [0, 1, 2], [0, 4, 1])
    assert rc == -1 and "ctx == NULL" in msg                            # a good list: the context is the last check
    rc, msg = _call(rule, 4, 3, 5, [], [])
    assert rc == -1 and "ctx == NULL" in msg
    rc, msg = _call(rule, 4, 3, 5, [0, 3, 7], [0, 1, 9])
    assert rc == -1 and "trial_model[1] = 3 outside [0, 3)" in msg      # the FIRST offending trial
    rc, msg = _call(rule, 4, 3, 5, [0, 2, 2], [0, 5, -1])
    assert rc == -1 and "trial_seg[1] = 5 outside [0, 5)" in msg
    rc, msg = _call(rule, 4, 3, 5, [-1], [0])
    assert rc == -1 and "trial_model[0] = -1 outside [0, 3)" in msg
    rc, msg = _call(rule, 4, 0, 0, [0], [0])
    assert rc == -1 and "trial_model[0] = 0 outside [0, 0)" in msg
    rc, msg = _call(rule, 0, 3, 5, [0], [0])
    assert rc == -1 and "bad size" in msg
    rc, msg = _call(rule, 4, 3, 5, [0], [0], ntrial=-1)
    assert rc == -1 and "bad size" in msg


def test_plda_refuses_a_session_count_below_one_only_on_a_model_with_a_trial():
    rc, msg = _call("plda", 4, 3, 5, [0, 2], [0, 1], nsess=[1, 0, 2])
    assert rc == -1 and "ctx == NULL" in msg                            # model 1 has no trial: its count is not looked at
    rc, msg = _call("plda", 4, 3, 5, [0, 2, 1, 1], [0, 1, 4, 2], nsess=[1, 0, 2])
    assert rc == -1 and "trial 2: nsess[1] = 0 < 1" in msg


# ---------------------------------------------------------------- the planner
PLAN_LISTS = [(M, S, kind) for (M, S) in ((1, 1), (3, 7), (7, 3), (33, 31), (34, 130)) for kind in ir.LISTS]


@pytest.mark.parametrize("M,S,kind", PLAN_LISTS, ids=lambda v: str(v).replace(" ", "_"))
def test_planner_against_its_numpy_mirror(M, S, kind):
    from lia_ral_amd import capi
    tm, ts = ir.trial_list(kind, M, S)
    n = len(tm)
    for anchor in (ir.ANCHOR_AUTO, ir.ANCHOR_MODEL, ir.ANCHOR_SEG):
        for piece in (1, 4, 7, capi.IV_TRIAL_PIECE):
            order, tiles, count = capi.plan_iv_trial_tiles(M, S, tm, ts, anchor, piece)
            want_order, want_tiles = ir.plan(tm, ts, anchor, piece)
            assert np.array_equal(order, want_order) and tiles == want_tiles and count == len(want_tiles)
            # the properties themselves, not only the mirror
            assert sorted(order.tolist()) == list(range(n))                                   # every trial once
            side = anchor if anchor else ir.anchor_rule(tm, ts)
            ta, tp = (ts, tm) if side == ir.ANCHOR_SEG else (tm, ts)
            keys = list(zip(ta[order].tolist(), tp[order].tolist(), order.tolist()))
            assert keys == sorted(keys)                                                       # (anchor, partner, position)
            covered = np.zeros(n, np.int64)
            for a, lo, hi in tiles:
                assert 0 < hi - lo <= piece and np.all(ta[order[lo:hi]] == a)
                covered[lo:hi] += 1
            assert np.all(covered == 1)                                                       # every trial in exactly one tile
            anchors = [t[0] for t in tiles]
            assert anchors == sorted(anchors)                                                 # the tiles of one anchor are adjacent


def test_anchor_rule_and_its_tie():
    from lia_ral_amd import capi
    assert capi.iv_trial_anchor(5, 9, [0, 1, 2], [4, 4, 4]) == capi.IV_ANCHOR_SEG             # 3 models, 1 segment
    assert capi.iv_trial_anchor(5, 9, [3, 3, 3], [4, 5, 6]) == capi.IV_ANCHOR_MODEL
    assert capi.iv_trial_anchor(5, 9, [0, 1, 0, 1], [7, 8, 8, 7]) == capi.IV_ANCHOR_MODEL     # 2 and 2: the model
    assert capi.iv_trial_anchor(5, 9, [0, 0, 1], [7, 7, 7]) == capi.IV_ANCHOR_SEG             # distinct vectors count, not trials
    assert capi.iv_trial_anchor(5, 9, [], []) == capi.IV_ANCHOR_MODEL
    for M, S, kind in PLAN_LISTS:
        tm, ts = ir.trial_list(kind, M, S)
        assert capi.iv_trial_anchor(M, S, tm, ts) == ir.anchor_rule(tm, ts)
    with pytest.raises(capi.GmmivError):
        capi.iv_trial_anchor(5, 9, [5], [0])


def test_planner_one_anchor_with_every_trial_empty_list_cap_and_bad_arguments():
    from lia_ral_amd import capi
    tm, ts = ir.trial_list("one model", 3, 1000)
    order, tiles, count = capi.plan_iv_trial_tiles(3, 1000, tm, ts, capi.IV_ANCHOR_MODEL, 4)
    assert count == 250 and all(a == 2 and hi - lo == 4 for a, lo, hi in tiles) and np.array_equal(ts[order], np.arange(1000))
    order, tiles, count = capi.plan_iv_trial_tiles(3, 1000, tm, ts, capi.IV_ANCHOR_MODEL, 512)
    assert [(a, hi - lo) for a, lo, hi in tiles] == [(2, 512), (2, 488)]
    order, tiles, count = capi.plan_iv_trial_tiles(3, 1000, tm, ts, capi.IV_ANCHOR_AUTO, 512)       # one model: it is the anchor
    assert count == 2
    order, tiles, count = capi.plan_iv_trial_tiles(3, 1000, tm, ts, capi.IV_ANCHOR_SEG, 512)
    assert count == 1000 and np.array_equal(order, np.argsort(ts, kind="stable"))
    order, tiles, count = capi.plan_iv_trial_tiles(3, 5, [], [])                                    # ntrial = 0 is valid
    assert len(order) == 0 and tiles == [] and count == 0
    assert capi.plan_iv_trial_tiles(0, 0, [], [])[2] == 0
    # entries beyond cap are counted, not written (the binding keeps guard entries behind cap and checks them)
    order, tiles, count = capi.plan_iv_trial_tiles(3, 1000, tm, ts, capi.IV_ANCHOR_MODEL, 4, cap=10)
    assert count == 250 and len(tiles) == 10 and tiles == ir.plan(tm, ts, ir.ANCHOR_MODEL, 4)[1][:10]
    order, tiles, count = capi.plan_iv_trial_tiles(3, 1000, tm, ts, capi.IV_ANCHOR_MODEL, 4, cap=0)
    assert count == 250 and tiles == []
    a = np.zeros(2, np.int32)
    f = capi.lib.gmmiv_plan_iv_trial_tiles
    bad = [(-1, 5, 2, 1, 4), (3, -1, 2, 1, 4), (3, 5, -1, 1, 4), (3, 5, 2, 3, 4), (3, 5, 2, -1, 4), (3, 5, 2, 1, 0), (3, 5, 2, 1, -4)]
    for M, S, n, anchor, piece in bad:
        assert f(ct.c_int64(M), ct.c_int64(S), _p(a), _p(a), ct.c_int64(n), anchor, piece, NULL, NULL, ct.c_int64(0)) == -1
    assert f(ct.c_int64(3), ct.c_int64(5), NULL, _p(a), ct.c_int64(2), 1, 4, NULL, NULL, ct.c_int64(0)) == -1
    for tm_bad, ts_bad in (([0, 3], [0, 0]), ([0, 0], [0, 5]), ([-1, 0], [0, 0])):
        with pytest.raises(capi.GmmivError):
            capi.plan_iv_trial_tiles(3, 5, tm_bad, ts_bad)
    assert capi.lib.gmmiv_iv_trial_piece(NULL) == capi.IV_TRIAL_PIECE


def test_planner_on_a_list_long_enough_for_its_host_threads():
    """from 2^18 trials on the counting passes run in chunks on several threads: the same order, whatever their number"""
    from lia_ral_amd import capi
    rng = np.random.default_rng(11)
    M, S, n = 300, 700, (1 << 18) + 12345
    tm, ts = rng.integers(0, M, n).astype(np.int32), rng.integers(0, S, n).astype(np.int32)      # pairs repeat: position decides
    for anchor in (ir.ANCHOR_MODEL, ir.ANCHOR_SEG):
        order, tiles, count = capi.plan_iv_trial_tiles(M, S, tm, ts, anchor, 512)
        want_order, want_tiles = ir.plan(tm, ts, anchor, 512)
        assert np.array_equal(order, want_order) and tiles == want_tiles and count == len(want_tiles)
    assert capi.iv_trial_anchor(M, S, tm, ts) == capi.IV_ANCHOR_MODEL


# ---------------------------------------------------------------- the sources
def test_the_kernel_source_has_no_atomic_and_the_makefile_names_the_new_files():
    src = open(os.path.join(ROOT, "lia_ral_amd", "csrc", "iv_trials.hip")).read()
    assert "k_score_trials" in src and "atomic" not in src.lower()
    assert "__shared__" not in src.split("k_cols_to_rows")[0]                                 # the gather kernel uses no LDS
    mk = open(os.path.join(ROOT, "lia_ral_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, re.M).group(1).split()
    assert "iv_trials.hip" in srcs and "capi_iv_trials.hip" in srcs and "../../include/gmmiv_iv_trials.h" in hdrs


# ---------------------------------------------------------------- the yardstick
EMU_DIMS = (1, 5, 33, 64, 127, 128, 129, 130, 257)


@pytest.mark.skipif(not br.HAVE_LONGDOUBLE, reason=br.SKIP_MESSAGE)
@pytest.mark.parametrize("dim", EMU_DIMS)
def test_the_documented_order_in_float64_stays_under_a_quarter_of_the_bar(dim):
    """the bars of backend_ref leave room for the formulation of the list calls: 64 strided partials, the butterfly, the epilogue"""
    worst = 0.0
    for M, S in ((7, 5), (3, 7)):
        tm, ts = ir.trial_list("full", M, S)
        for rule in ir.LIST_RULES:
            key = ir.case_key(dim, M, S, rule)
            r, i = ir.worst_ratio(ir.emulate(key, rule, tm, ts), key, rule, tm, ts)
            assert r <= 0.25, (dim, M, S, rule, "trial %d = (%d, %d)" % (i, tm[i], ts[i]), r)
            worst = max(worst, r)
    for kind in ir.PLDA_KINDS:
        M = len(br.PLDA_COUNTS[kind])
        tm, ts = ir.trial_list("full", M, 7)
        key = (dim, M, 7, "plda " + kind)
        r, i = ir.worst_ratio(ir.emulate(key, "plda", tm, ts), key, "plda", tm, ts)
        assert r <= 0.25, (dim, kind, "trial %d = (%d, %d)" % (i, tm[i], ts[i]), r)
        worst = max(worst, r)
    print("dim %d: the emulation reaches %.3f of the bar" % (dim, worst))


# ---------------------------------------------------------------- the ndx loader of the host layer
def _write(path, lines):
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return str(path)


def test_host_symbols_are_exported():
    from lia_ral_amd import host_capi
    for name in ("liagpu_iv_test_trials", "liagpu_iv_test_ndx", "liagpu_iv_test_ndx_load"):
        assert hasattr(host_capi.lib, name), name
    for name in ("iv_test_trials", "iv_test_ndx", "load_iv_test_ndx"):
        assert hasattr(host_capi, name), name
    with pytest.raises(host_capi.HostError, match="pldaScoring must be: native OR enrollMean"):
        host_capi.iv_test(np.zeros((2, 2)), [2], np.zeros((2, 1)), [1], np.zeros((2, 1)), scoring="plda", plda_scoring="ScoreFusion")


def test_ndx_without_a_target_list_first_appearance_and_duplicates(tmp_path):
    from lia_ral_amd import host_capi
    ndx = _write(tmp_path / "a.ndx", ["segB spk2 spk1", "", "segA spk1 spk3 spk1", "segB spk3 spk2", "segC"])
    nx = host_capi.load_iv_test_ndx(ndx)
    assert nx["segs"] == ["segB", "segA", "segC"]                       # first appearance; a segment without a model is still a segment
    assert nx["models"] == ["spk2", "spk1", "spk3"] and nx["sessions"] == [["spk2"], ["spk1"], ["spk3"]]
    # duplicates removed (segA spk1 twice, segB spk2 twice), order of first appearance
    assert list(zip(nx["trial_model"].tolist(), nx["trial_seg"].tolist())) == [(0, 0), (1, 0), (1, 1), (2, 1), (2, 0)]
    assert nx["dropped"] == 0 and nx["max_sessions"] == 1


def test_ndx_with_a_target_list_descending_sort_and_the_dropped_trial(tmp_path):
    from lia_ral_amd import host_capi
    ids = _write(tmp_path / "t.lst", ["m1 e1", "m2 e2 e3 e4", "m3 e5", "m4 e6 e7", "m1 e8 e9"])
    ndx = _write(tmp_path / "b.ndx", ["s1 m3 m9 m1", "s2 m2 m9", "s1 m4 m3"])
    nx = host_capi.load_iv_test_ndx(ndx, ids)
    # lines by element count, descending, equal counts in file order (assumed stable): m2 (4), m4 (3), m1 e8 e9 (3), m1 e1 (2), m3 (2)
    assert nx["models"] == ["m2", "m4", "m1", "m3"]
    assert nx["sessions"] == [["e2", "e3", "e4"], ["e6", "e7"], ["e8", "e9", "e1"], ["e5"]]
    assert nx["max_sessions"] == 3 and nx["segs"] == ["s1", "s2"]
    assert nx["dropped"] == 2                                           # m9 twice: no enrolment session
    assert list(zip(nx["trial_model"].tolist(), nx["trial_seg"].tolist())) == [(3, 0), (2, 0), (0, 1), (1, 0)]
    with pytest.raises(host_capi.HostError, match="cannot open the ndx file"):
        host_capi.load_iv_test_ndx(str(tmp_path / "missing.ndx"))
