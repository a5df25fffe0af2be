"""The yardstick of the TurnDetection tests is checked before anything is judged by it (tests/turn_ref.py), and what include/gmmiv_turn.h
promises without a GPU: the header, the symbols, the NULL context, the planner, the host twin.

Largest |fp64 restatement - long double| / bar on the case table: profiles/r28/turn_errors.json (rewritten by every run)."""
import ctypes as ct
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import turn_ref as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRITS = (tr.GLR, tr.DGLR, tr.BIC)
FUNCTIONS = ("gmmiv_turn_tile_positions", "gmmiv_plan_turn_positions", "gmmiv_turn_curve", "gmmiv_turn_pick", "gmmiv_turn_segments")


def test_both_fp64_orders_stay_within_the_bar_of_the_long_double_restatement():
    worst = dict(reference_order=0.0, documented_order=0.0, logcov_ratio=0.0)
    for D, W, S in tr.CASES:
        for x in tr.case_frames(D, W, S):
            worst["logcov_ratio"] = max(worst["logcov_ratio"], tr.logcov_ratio(x, W))
            for crit in CRITS:
                r = tr.value_ld(x, W, crit)
                assert r["status"] == 0
                b = tr.bar(r, D, W, S)
                worst["reference_order"] = max(worst["reference_order"], float(abs(tr.value_ref64(x, W, crit) - r["value"])) / b)
                worst["documented_order"] = max(worst["documented_order"], float(abs(tr.value_doc64(x, W, S, crit) - r["value"])) / b)
    out = os.path.join(ROOT, "profiles", "r28")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "turn_errors.json"), "w") as f:
            json.dump(dict(what="largest |fp64 restatement - long double| / bar over tests/turn_ref.py CASES x 3 positions x 3 criteria", **worst), f, indent=1)
            f.write("\n")
    except OSError:
        pass                                                                # a read-only checkout still runs the test
    assert worst["logcov_ratio"] <= 1.4, "the derivation's sum |log cov| <= 1.4 sum (1 + kappa) does not hold on the case table"
    assert worst["reference_order"] <= 0.5 and worst["documented_order"] <= 0.5, worst


@pytest.mark.parametrize("defect,crit", [("unbiased", tr.DGLR), ("short12", tr.GLR), ("logw", tr.BIC)])
def test_a_planted_defect_in_the_value_exceeds_the_bar(defect, crit):
    over = 0
    for D, W, S in tr.CASES:
        for x in tr.case_frames(D, W, S):
            r = tr.value_ld(x, W, crit)
            for f in (lambda: tr.value_ref64(x, W, crit, defect=defect), lambda: tr.value_doc64(x, W, S, crit, defect=defect)):
                over += float(abs(f() - r["value"])) > tr.bar(r, D, W, S)
    assert over >= 1


def pick_curves():
    rng = np.random.default_rng(5)
    return [[4.0] * 6, [2.0, 9, 5, 1, 7, 3], [0.0, 5, 9, 5, 0], [9.0, 1, 8, 0, 7, 2, 6], [1.0, 4, 4, 4, 1, 1, 6, 6, 2, 2, 7, 0], [0.0, 4, 8, 4, 0, 4, 8, 4, 0]] + \
        [list(rng.integers(-9, 9, n).astype(np.float64)) for n in (5, 9, 30, 100)]


@pytest.mark.parametrize("defect", ["index0", "ge"])
def test_a_planted_defect_in_the_pick_loop_changes_a_decision(defect):
    changed = 0
    for cv in pick_curves():
        for alpha in (0.25, 0.5, 1.0, 2.0):
            changed += bool((tr.pick_as_written(cv, alpha)[1] != tr.pick_as_written(cv, alpha, defect=defect)[1]).any())
    assert changed >= 1


def test_the_pick_loop_keeps_the_ends_the_nan_and_the_short_curves():
    for cv in ([5.0], [5.0, 9.0], [1.0, 8.0, 2.0]):
        sm, dec, mean, std = tr.pick_as_written(cv, 0.5)
        assert dec[0] == 0 and dec[-1] == 0 and (len(cv) < 3 or np.array_equal(sm[[0, -1]], [cv[0], cv[-1]]))
    sm, dec, mean, std = tr.pick_as_written([1.0, 8.0, 2.0], 0.5)
    assert sm[1] == 0.25 * 1 + 0.25 * 2 + 0.5 * 8 and dec[1] == 0              # the left walk never looks at index 0: minL = v'[1] and |0| > thr is false
    assert tr.pick_as_written([1.0, 8.0, 2.0], 0.5, defect="index0")[1][1] == 1
    sm, dec, mean, std = tr.pick_as_written([4.0, 9, 2, 7, float("nan"), 8, 1, 6, 3], 0.5)
    assert np.isnan(mean) and np.isnan(std) and not dec.any()                   # every comparison with a NaN std is false


def test_the_random_curves_of_the_gpu_test_leave_fewer_than_one_percent_to_the_margin():
    from test_gpu_turn import random_curves
    left = total = 0
    for cv in random_curves():
        sm, dec, mean, std = tr.pick_as_written(cv, 0.7)
        mar, wid = tr.pick_margins(sm, 0.7, float(std), len(cv))
        left += int((mar <= wid).sum())
        total += len(cv)
    assert left <= 0.01 * total and total > 2000, (left, total)


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_header_declares_and_the_library_exports_the_entry_points():
    from lia_ral_amd import capi
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "gmmiv_turn.h")).read(), flags=re.S)
    assert '#include "gmmiv.h"' in hdr
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(capi.lib, name), name
    for const, v in (("GMMIV_TURN_GLR", 0), ("GMMIV_TURN_DGLR", 1), ("GMMIV_TURN_BIC", 2), ("GMMIV_TURN_BAD_COV", 1), ("GMMIV_TURN_CLAMPED", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (const, v), hdr), const
    assert "DELTABIC" not in re.sub(r"\s+", " ", " ".join(re.findall(r"#define[^\n]*", hdr)))
    with pytest.raises(capi.GmmivError, match="DELTABIC"):
        capi.turn_crit("DELTABIC")


def test_every_call_refuses_a_null_context_with_a_status_and_a_message():
    from lia_ral_amd import capi
    lib, null, i64 = capi.lib, ct.c_void_p(0), ct.c_int64
    runs = np.array([[0, 30, 0]], np.int64)
    po = capi.plan_turn_positions(runs, 1, 4, 2)
    n = int(po[-1])
    v, st, dec = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    x = np.zeros((30, 3))
    p = capi._ptr
    rc = lib.gmmiv_turn_curve(null, p(x), capi.F64, i64(3), 3, p(runs), i64(1), i64(1), p(po), i64(n), i64(4), i64(2), 1, ct.c_double(-200), ct.c_double(200), p(v), p(st))
    assert rc != 0 and b"NULL context" in lib.gmmiv_last_error()
    rc = lib.gmmiv_turn_pick(null, p(v), p(po), i64(1), i64(n), ct.c_double(0.5), null, p(dec), null, null)
    assert rc != 0 and b"NULL context" in lib.gmmiv_last_error()
    rc = lib.gmmiv_turn_segments(null, p(runs), i64(1), i64(1), p(po), i64(n), p(dec), i64(4), i64(2), null, null, null, null)
    assert rc != 0 and b"NULL context" in lib.gmmiv_last_error()
    # host tables are validated before the context is looked at: the message names the run
    bad = np.array([[0, 30, 0], [40, 30, 0]], np.int64)
    po2 = np.array([0, n, n + 3], np.int64)
    rc = lib.gmmiv_turn_curve(null, p(x), capi.F64, i64(3), 3, p(bad), i64(2), i64(1), p(po2), i64(n + 3), i64(4), i64(2), 1, ct.c_double(-200), ct.c_double(200), p(v), p(st))
    assert rc != 0 and b"run 1" in lib.gmmiv_last_error()


def test_the_planner_matches_the_loop_as_written():
    from lia_ral_amd import capi
    for W in range(1, 9):
        for S in range(1, 7):
            lens = np.arange(1, 41)
            runs = np.stack([np.cumsum(lens) + 3, lens, np.zeros_like(lens)], 1).astype(np.int64)
            po = capi.plan_turn_positions(runs, 1, W, S)
            assert list(np.diff(po)) == [tr.positions_as_written(int(L), W, S, int(b)) for b, L, _ in runs], (W, S)
    assert list(capi.plan_turn_positions(np.zeros((0, 3), np.int64), 0, 50, 5)) == [0]


@pytest.mark.parametrize("runs,nfiles,W,S,msg", [
    ([[0, 30, 1], [40, 30, 0]], 2, 4, 2, "run 1"), ([[0, 30, 2]], 2, 4, 2, "run 0"), ([[0, 30, 0], [5, -1, 0]], 1, 4, 2, "run 1"),
    ([[-1, 30, 0]], 1, 4, 2, "run 0"), ([[0, 30, 0]], 1, 0, 2, "W"), ([[0, 30, 0]], 1, 4, 0, "step")])
def test_the_planner_refuses_a_bad_table_with_a_message(runs, nfiles, W, S, msg):
    from lia_ral_amd import capi
    with pytest.raises(capi.GmmivError, match=msg):
        capi.plan_turn_positions(np.array(runs, np.int64), nfiles, W, S)


# ---------------------------------------------------------------------------------------------------------------- the host twin
def test_the_host_twin_reproduces_the_loop_as_written_on_its_own_curves():
    """liagpu::turnDetection (host only): its segments, smoothed curves, statistics and decisions are those of the as-written restatement
    run on the values the twin computed itself -- exactly; and its values stay under the bar of the long double restatement"""
    from lia_ral_amd import host_capi as h
    rng = np.random.default_rng(0)
    D, W, S = 4, 6, 4
    x = tr.draw_frames(rng, 300, D, np.float32)
    x[150:] += np.float32(2.0)
    segs = (np.array([3, 20, 40, 200]), np.array([10, 13, 150, 61]))
    turns = 0
    for crit, alpha in (("DGLR", 0.5), ("BIC", 0.7), ("GLR", 0.25)):
        out = h.turn_detection_batch([x, x[:50]], [segs, (np.array([0]), np.array([50]))], crit, W, S, alpha, twin=True)
        assert [len(c["value"]) for c in out[0]["curves"]] == [tr.positions_as_written(int(n), W, S) for n in segs[1]]
        want = []
        for (b, n), c in zip(zip(*segs), out[0]["curves"]):
            b, n = int(b), int(n)
            if len(c["value"]):
                sm, dec, mean, std = tr.pick_as_written(c["value"], alpha)
                assert np.array_equal(sm, c["smoothed"]) and np.array_equal(dec, c["dec"]) and mean == c["mean"] and std == c["std"]
                turns += int(dec.sum())
                for k, v in enumerate(c["value"]):
                    r = tr.value_ld(x[b + k * S:b + k * S + 2 * W], W, tr.TURN_NAMES[crit])
                    assert abs(tr.LD(v) - r["value"]) <= tr.bar(r, D, W, S)
            want += tr.segments_as_written(b, n, W, S, c["dec"])
        assert list(zip(out[0]["begin"].tolist(), out[0]["length"].tolist())) == want
        assert list(zip(out[1]["begin"].tolist(), out[1]["length"].tolist())) == tr.segments_as_written(0, 50, W, S, out[1]["curves"][0]["dec"])
    assert turns >= 3
    with pytest.raises(h.HostError, match="DELTABIC"):
        h.turn_detection_batch([x], [segs], "DELTABIC", twin=True)


def test_the_integration_block_compiles_against_the_stub_and_the_header(tmp_path):
    """the TurnDetection block of INTEGRATION.md (fenced as c++: its prototypes are not in gmmiv.h, which is what the document test holds
    the cpp blocks to) behind the cpp blocks it builds on, with the document test's own compiler line"""
    from test_cpu_integration_doc import compile_tu, cpp_blocks
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    mine = re.findall(r"```c\+\+\n(.*?)```", text, flags=re.S)
    assert len(mine) == 1 and '#include "gmmiv_turn.h"' in mine[0]
    src = '#include "alize_stub.h"\n' + "\n".join(cpp_blocks()) + "\n" + mine[0]
    r = compile_tu(src, tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    called = set(re.findall(r"\b(gmmiv_turn_[a-z0-9_]+|gmmiv_plan_turn_[a-z0-9_]+)\s*\(", mine[0]))
    assert called == {"gmmiv_plan_turn_positions", "gmmiv_turn_curve", "gmmiv_turn_pick", "gmmiv_turn_segments"}
    drifted = mine[0].replace("npos, winSize, winStep, c,", "npos, winSize, c, winStep, &value[0],")
    assert drifted != mine[0] and compile_tu('#include "alize_stub.h"\n' + "\n".join(cpp_blocks()) + "\n" + drifted, tmp_path).returncode != 0
