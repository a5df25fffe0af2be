"""NormFeat's windowMode without a GPU (include/gmmiv_feat_window.h): the header, the argument checks (NULL context), the planner
against the literal restatement of the schedule (tests/normwin_ref.py), the schedule's properties, four planted defects, and the
documented fp64 order against the long-double restatement under the derived bar of normwin_ref."""
import ctypes as ct
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normwin_ref as nr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = ("gmmiv_plan_norm_windows", "gmmiv_feat_norm_window")


def capi():
    from lia_ral_amd import capi as c
    return c


# ---------------------------------------------------------------------------------------------------------------- the header
def test_the_header_declares_what_the_library_exports_and_gmmiv_h_does_not():
    hdr = open(os.path.join(ROOT, "include", "gmmiv_feat_window.h")).read()
    main = open(os.path.join(ROOT, "include", "gmmiv.h")).read()
    assert '#include "gmmiv.h"' in hdr
    body = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gmmiv_[a-z0-9_]+)\s*\(", body))
    assert declared == set(PROTOS)
    lib = capi().lib
    for name in PROTOS:
        assert getattr(lib, name) is not None
        assert not re.search(r"\b%s\b" % name, main)
    assert "GMMIV_NORMWIN_CMS 1" in hdr and "GMMIV_NORMWIN_VAR 2" in hdr and "one compute unit" in hdr
    mk = open(os.path.join(ROOT, "lia_ral_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "capi_feat_window.hip" in srcs and "feat_norm_window.hip" in srcs


def test_the_kernel_source_has_no_atomics_and_no_restrict_on_the_frames():
    src = open(os.path.join(ROOT, "lia_ral_amd", "csrc", "feat_norm_window.hip")).read()
    assert "atomic" not in src.lower()
    assert "__restrict__" not in src and "nontemporal" not in src
    assert "fp contract(off)" in src


# ---------------------------------------------------------------------------------------------------------------- argument checks
def _i64(a):
    return np.ascontiguousarray(a, np.int64)


def _call(dt=0, ldx=4, D=4, runs=None, nfiles=1, step_off=None, steps=None, alpha=None, flags=0, x=1 << 20, nrun=None, nsteps=None):
    """gmmiv_feat_norm_window with a NULL context -> (status, message)"""
    c = capi()
    runs = _i64([[0, 5, 0], [7, 5, 0]]) if runs is None else _i64(runs).reshape(-1, 3)
    step_off = _i64([0, 1]) if step_off is None else _i64(step_off)
    steps = _i64([[0, 2, 0, 2]]) if steps is None else _i64(steps).reshape(-1, 4)
    alpha = np.ascontiguousarray([1.0] * len(steps) if alpha is None else alpha, np.float64)
    rc = c.lib.gmmiv_feat_norm_window(None, ct.c_void_p(x), dt, ct.c_int64(ldx), D, c._ptr(runs), ct.c_int64(len(runs) if nrun is None else nrun),
                                      ct.c_int64(nfiles), c._ptr(step_off), c._ptr(steps), c._ptr(alpha), ct.c_int64(len(steps) if nsteps is None else nsteps),
                                      flags, None, None)
    return rc, c.lib.gmmiv_last_error().decode()


def test_argument_checks_come_in_order_dtype_tables_context():
    ERR_ARG = -1
    rc, msg = _call(dt=7, runs=[[0, 5, 3]])                                          # a bad dtype wins over a bad table
    assert rc == ERR_ARG and "x_dtype must be GMMIV_F32 or GMMIV_F64" in msg
    rc, msg = _call()                                                                # valid tables: the NULL context is what is left
    assert rc == ERR_ARG and "NULL context" in msg
    rc, msg = _call(flags=3)
    assert rc == ERR_ARG and "cmsOnly and varOnly are not compatible" in msg
    assert "flags must be" in _call(flags=4)[1]
    assert "ldx < D" in _call(ldx=3)[1] and "bad argument" in _call(nrun=-1)[1]
    rc, msg = _call(runs=[[0, 5, 0], [7, 5, 1]])                                     # the tables come before the context
    assert rc == ERR_ARG and "run 1" in msg and "outside [0, 1)" in msg
    assert "run 1" in _call(runs=[[0, 5, 1], [7, 5, 0]], nfiles=2, step_off=[0, 1, 1])[1]
    assert "run 0 has a negative first frame or length" in _call(runs=[[-1, 5, 0]], steps=[[0, 1, 0, 1]])[1]
    assert "step_off[0] must be 0" in _call(step_off=[1, 1])[1]
    assert "non-decreasing (file 1)" in _call(nfiles=2, step_off=[0, 2, 1])[1]
    assert "step_off ends at 2, not at nsteps = 1" in _call(step_off=[0, 2])[1]
    assert "step 0" in _call(steps=[[0, 3, 0, 2]])[1]                                # the window leaves the table
    assert "step 0" in _call(steps=[[1, 2, 0, 2]])[1]                                # the apply range leaves the window
    assert "step 0" in _call(steps=[[0, 2, 1, 1]])[1]                                # nothing to normalise
    rc, msg = _call(runs=[[0, 5, 0], [7, 5, 1]], nfiles=2, step_off=[0, 1, 2], steps=[[0, 1, 0, 1], [0, 2, 1, 2]])
    assert rc == ERR_ARG and "step 1 of file 1 names runs outside the file's runs [1, 2)" in msg
    # nothing to do is valid, but only with a context
    assert "NULL context" in _call(nfiles=0, runs=np.zeros((0, 3)), step_off=[0], steps=np.zeros((0, 4)))[1]


def test_the_planner_refuses_what_the_reference_cannot_run():
    c = capi()
    ok = [[10, 5, 0], [15, 5, 0], [30, 5, 1]]
    off, st, al = c.plan_norm_windows(ok, 2, [10, 28], 0.05)
    assert off[-1] == len(st) == len(al) > 0

    def refused(runs, first=(10, 28), nfiles=2, **kw):
        with pytest.raises(c.GmmivError) as e:
            c.plan_norm_windows(runs, nfiles, list(first), **kw)
        return str(e.value)
    assert "run 1" in refused([[10, 5, 0], [10, 5, 0]]) and "strictly increasing" in refused([[10, 5, 0], [10, 5, 0]])      # equal begins
    assert "strictly increasing" in refused([[15, 5, 0], [10, 5, 0]])
    m = refused([[10, 5, 0], [14, 5, 0], [30, 5, 1]])
    assert "run 1" in m and "overlaps" in m
    assert "run 2" in refused([[10, 5, 0], [15, 5, 0], [27, 5, 1]]) and "before its file" in refused([[10, 5, 0], [15, 5, 0], [27, 5, 1]])
    assert "run 1 has length 0" in refused([[10, 5, 0], [15, 0, 0]])
    assert "run 1" in refused([[30, 5, 1], [10, 5, 0]]) and "run 0" in refused([[10, 5, 2]])
    assert "window_duration" in refused(ok, window_duration=-1.0) and "frame_length" in refused(ok, frame_length=0.0)
    # the same begin in two DIFFERENT files is fine
    c.plan_norm_windows([[10, 5, 0], [38, 5, 1]], 2, [0, 28])


# ---------------------------------------------------------------------------------------------------------------- planner == restatement
def _tables(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        runs, first, T = nr.random_table(rng, int(rng.integers(1, 6)))
        yield runs, first, float(rng.choice(nr.DURATIONS)), float(rng.choice((1.0, 0.5, 0.9))), float(rng.choice((0.01, 0.016)))


def test_the_planner_equals_the_restatement_on_random_tables():
    c = capi()
    nsteps = nonzero_first = 0
    for runs, first, wd, comp, fl in _tables(3000, 2027):
        off, st, al = c.plan_norm_windows(runs, len(first), first, wd, comp, fl)
        o2, s2, a2 = nr.plan(runs, len(first), first, wd, comp, fl)
        assert np.array_equal(off, o2) and np.array_equal(st, s2), (runs.tolist(), first.tolist(), wd, fl)
        assert al.tobytes() == a2.tobytes()                                          # alpha bit for bit
        assert len(al) <= len(runs)                                                  # arrays of nrun steps always suffice
        nsteps += len(al)
        nonzero_first += int((first > 0).any())
    assert nsteps > 10000 and nonzero_first > 1000
    # a planner on absolute frames would differ: T() truncates, and 0.016 s frames make the truncation depend on the origin
    runs = np.array([[1000 + 7 * i, 7, 0] for i in range(40)], np.int64)
    a_rel = c.plan_norm_windows(runs, 1, [1000], 0.5, 1.0, 0.016)
    a_abs = c.plan_norm_windows(runs, 1, [0], 0.5, 1.0, 0.016)
    assert a_rel[2].tobytes() != a_abs[2].tobytes()
    # the counting call (no arrays) returns the same number
    n = c.lib.gmmiv_plan_norm_windows(c._ptr(runs), ct.c_int64(len(runs)), ct.c_int64(1), c._ptr(np.array([1000], np.int64)), ct.c_double(0.5),
                                      ct.c_double(1.0), ct.c_double(0.016), None, None, None)
    assert n == len(a_rel[2])


def test_the_schedule_properties_hold():
    """begins strictly increasing, no overlap: contiguous windows and apply ranges (asserted inside schedule()), the apply ranges
    partition the segments in order, the reference's exception never fires, and most steps normalise nothing"""
    rng = np.random.default_rng(5)
    all_steps = kept = 0
    for _ in range(2000):
        n = int(rng.integers(1, 40))
        length = [int(v) for v in rng.choice(nr.LENGTHS, n)]
        gaps = [int(v) for v in rng.choice(nr.GAPS, n)]
        begin = list(np.cumsum([int(rng.integers(0, 9))] + [l + g for l, g in zip(length[:-1], gaps[:-1])]))
        steps = nr.schedule(begin, length, float(rng.choice(nr.DURATIONS)), 1.0, float(rng.choice((0.01, 0.016))))
        em = nr.emitted(steps)
        pos = 0
        for wlo, whi, alo, ahi, a in em:
            assert alo == pos and wlo <= alo < ahi <= whi
            pos = ahi
        assert pos == n and len(em) <= n
        all_steps += len(steps)
        kept += len(em)
    print("steps %d, of which %d normalise something" % (all_steps, kept))
    assert kept < all_steps


# ---------------------------------------------------------------------------------------------------------------- the fp64 order
def _case(dtype, seed=11):
    """5 files, short segments, windows long enough that they read rewritten frames"""
    rng = np.random.default_rng(seed)
    runs, first, pos = [], [], 3
    for f in range(5):
        first.append(pos)
        p = pos + (2 if f % 2 else 0)
        for _ in range((0, 1, 25, 40, 60)[f]):
            n = int(rng.choice((1, 2, 7, 15, 16, 17, 30, 33)))
            runs.append((p, n, f))
            p += n + int(rng.choice((0, 1, 5, 40)))
        pos = p + 2
    runs = np.array(runs, np.int64)
    D = 3
    x = rng.normal(rng.uniform(-3, 3, D), rng.uniform(0.5, 2, D), (pos, D)).astype(dtype)
    return runs, np.array(first, np.int64), x


def _ratios(e, l):
    return dict(frames=nr.worst_ratio(e["out"], l["out"], l["bar"]), step_stat=nr.worst_ratio(e["step_stat"], l["step_stat"], l["sbar"]),
                gstat=nr.worst_ratio(e["gstat"], l["gstat"], l["gbar"]))


def test_the_documented_order_stays_within_the_bar_of_the_long_double_restatement():
    c = capi()
    worst = dict(frames=0.0, step_stat=0.0, gstat=0.0)
    for dtype in (np.float32, np.float64):
        runs, first, x = _case(dtype)
        for wd, comp, flags in ((0.5, 1.0, {}), (5.0, 1.0, {}), (1.0, 0.5, {}), (3.0, 1.0, dict(cms=True)), (3.0, 0.5, dict(var=True))):
            off, st, al = c.plan_norm_windows(runs, len(first), first, wd, comp, 0.01)
            e, l = nr.emulate(x, runs, len(first), off, st, al, **flags), nr.longdouble(x, runs, len(first), off, st, al, **flags)
            sel = np.concatenate([np.arange(b, b + n) for b, n, f in runs if f != 1])        # file 1 is one run: its window is the file
            assert np.isfinite(l["bar"][sel]).all() and np.isfinite(l["out"][sel]).all()
            r = _ratios(e, l)
            print(dtype.__name__, wd, comp, flags, r)
            for k in worst:
                worst[k] = max(worst[k], r[k])
            # untouched: frames outside the runs
            rows = np.concatenate([np.arange(b, b + n) for b, n, f in runs])
            rest = np.setdiff1d(np.arange(len(x)), rows)
            assert e["out"][rest].tobytes() == x[rest].tobytes() and l["out"][rest].tobytes() == x[rest].tobytes()
    assert max(worst.values()) <= 1.0, worst
    assert worst["step_stat"] > 0.0                                                          # the comparison is not vacuous
    try:
        os.makedirs(os.path.join(ROOT, "profiles", "r27"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r27", "feat_norm_window_errors.json"), "w") as f:
            json.dump(dict(what="fp64 emulation of the documented order against the long-double restatement: worst |difference| / derived bar",
                           worst_ratio=worst), f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def test_planted_defects_are_caught():
    c = capi()
    # (1), (2): the blend and the buffer the window reads -- fp64 frames, 3 s windows over 0.3 s segments
    rng = np.random.default_rng(3)
    runs = np.array([[5 + 35 * i, 30, 0] for i in range(40)], np.int64)
    x = rng.normal([1.0, -2.0], [1.0, 0.5], (5 + 35 * 40, 2))
    x[700:] += 1.5                                                                   # the file drifts: windows differ from the global statistics
    off, st, al = c.plan_norm_windows(runs, 1, [0], 3.0, 0.8, 0.01)
    l = nr.longdouble(x, runs, 1, off, st, al)
    assert max(_ratios(nr.emulate(x, runs, 1, off, st, al), l).values()) <= 1.0
    for defect in ("unblended", "original"):
        r = _ratios(nr.emulate(x, runs, 1, off, st, al, defect=defect), l)
        print(defect, r)
        assert r["frames"] > 1e3 and r["step_stat"] > 1e3, defect
    # (3): alpha not capped.  floor(A) - floor(B) >= floor(A - B): in exact arithmetic T(frames) never exceeds the window's length, and
    # 10 ms and 16 ms frames are exact.  With 11 ms frames the product 23 * 1000 * 0.011 rounds below 253, T(23) loses a millisecond and
    # the window [1, 23) is 0.241 s long for 0.242 s of frames.
    fl = 0.011
    assert nr.T(23, fl) == 0.252 and nr.T(22, fl) == 0.242 and nr.T(1, fl) == 0.011
    runs = np.array([[1 + 22 * i, 22, 0] for i in range(30)], np.int64)
    good = c.plan_norm_windows(runs, 1, [0], 0.2, 1.0, fl)
    bad = nr.plan(runs, 1, [0], 0.2, 1.0, fl, cap=False)
    assert np.array_equal(good[1], bad[1]) and bad[2].max() > 1.001 and good[2].max() == 1.0
    x = rng.normal(0.5, 1.0, (1 + 22 * 30, 2))
    x[300:] += 1.0
    l = nr.longdouble(x, runs, 1, *good)
    assert max(_ratios(nr.emulate(x, runs, 1, *good), l).values()) <= 1.0
    assert _ratios(nr.emulate(x, runs, 1, *bad), l)["frames"] > 1e3
    # (4): T without the truncation -- other alphas (and, on other tables, other windows)
    runs = np.array([[1 + 12 * i, 7, 0] for i in range(60)], np.int64)
    x = rng.normal(0.5, 1.0, (1 + 12 * 60, 2))
    x[300:] += 1.0
    good = c.plan_norm_windows(runs, 1, [0], 0.5, 0.9, 0.0125)
    l = nr.longdouble(x, runs, 1, *good)
    bad = nr.plan(runs, 1, [0], 0.5, 0.9, 0.0125, trunc=False)
    assert len(bad[2]) != len(good[2]) or bad[2].tobytes() != good[2].tobytes()
    if np.array_equal(bad[0], good[0]) and np.array_equal(bad[1], good[1]):
        assert _ratios(nr.emulate(x, runs, 1, *bad), l)["frames"] > 1e3
