"""Batched ComputeTest without a GPU: the tile planner of gmmiv_llr_trials against a numpy restatement, the reference scores the GPU
tests compare with, and the argument errors of the host layer that need no device."""
import os

import numpy as np
import pytest

import trials_ref as tr
from conftest import make_frames, make_gmm


def _tuples(tiles):
    return [(t["lo"], t["hi"], t["trial"], t["seg"], t["model"], t["piece"]) for t in tiles]


@pytest.mark.parametrize("P", [4, 64, 128])
def test_planner_matches_numpy(P):
    from lia_ral_amd import capi
    sb, T = tr.piece_layout(P)                                  # 0, 1, P - 1, P, P + 1, 2 P + 3 frames; nobody's frames at both ends
    assert sb[0] == tr.LEAD and T == sb[-1] + tr.TRAIL
    ts, tm = tr.trial_list(len(sb) - 1, skip=3)                 # a segment without a trial, a repeated trial, shuffled
    assert 3 not in ts and len(set(zip(ts.tolist(), tm.tolist()))) == len(ts) - 1 and not np.array_equal(ts, np.sort(ts))
    got = _tuples(capi.plan_trial_tiles(sb, ts, tm, P))
    ref = tr.plan_np(sb, ts, tm, P)
    assert got == ref and len(got) > 0
    assert capi.plan_trial_tiles(sb, ts, tm, P, count_only=True) == len(ref)      # tiles = NULL: the count alone
    # sorted by (segment, piece, position); pieces cover each trial's segment once; the empty segment has no tile
    assert [(t[3], t[5], t[2]) for t in got] == sorted((t[3], t[5], t[2]) for t in got)
    for i, s in enumerate(ts):
        mine = sorted((t[0], t[1]) for t in got if t[2] == i)
        n = sb[s + 1] - sb[s]
        assert len(mine) == -(-n // P)
        if n:
            assert mine[0][0] == sb[s] and mine[-1][1] == sb[s + 1] and all(a[1] == b[0] for a, b in zip(mine, mine[1:]))
            assert all(hi - lo == P for lo, hi in mine[:-1])


def test_planner_default_piece_and_layout_of_the_gmm_models_tests():
    from lia_ral_amd import capi
    import models_ref as mr
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gmmiv.h")).read()
    assert capi.TRIAL_PIECE == int(re.search(r"#define GMMIV_TRIAL_PIECE (\d+)", header).group(1))      # read from the library, not a copy
    assert capi.TRIAL_PIECE % 4 == 0 and 64 <= capi.TRIAL_PIECE <= 512
    sb, _, _ = mr.seg_layout()
    ts, tm = tr.trial_list(len(sb) - 1, seed=2)
    assert _tuples(capi.plan_trial_tiles(sb, ts, tm)) == tr.plan_np(sb, ts, tm, capi.TRIAL_PIECE)


def test_planner_edges():
    from lia_ral_amd import capi
    assert capi.plan_trial_tiles([0], [], [], 128) == []                          # no segment, no trial
    assert capi.plan_trial_tiles([5, 5, 9], [], [], 128) == []                    # segments, no trial
    assert capi.plan_trial_tiles([5, 5], [0, 0], [1, 2], 128) == []               # trials of an empty segment
    for bad in [dict(sb=[0, 10, 9], P=128), dict(sb=[0, 10], P=0), dict(sb=[0, 10], P=-4), dict(sb=[0, 10], P=6), dict(sb=[-1, 10], P=128)]:
        with pytest.raises(capi.GmmivError):
            capi.plan_trial_tiles(bad["sb"], [0], [0], bad["P"])
    with pytest.raises(capi.GmmivError):
        capi.plan_trial_tiles([0, 10], [1], [0], 128)                             # a trial of a segment that does not exist


def test_reference_scores_are_consistent(golden_dir):
    """the reference the GPU tests use: a client that is the world scores 0, one-frame segments give the per-frame differences, and the
    two segments of KAT-1 give the reference tool's LLRs"""
    world = make_gmm(37, 14, seed=3)
    models = tr.make_models(world, False)
    models = (models[0], np.concatenate([models[1][:-1], world[1][None]]), models[2])      # the last model IS the world
    x = make_frames(*world, 90, seed=4)
    lw, lc = tr.frame_ref(world, models, x, 10)
    sb = np.array([3, 3, 40, 41, 90])
    ts = np.array([2, 0, 1, 3, 1], np.int32); tm = np.array([4, 1, 4, 2, 0], np.int32)
    llr, cm, wm = tr.ref_llr(lw, lc, sb, ts, tm)
    assert llr[1] == 0 and cm[1] == 0 and wm[0] == 0                              # the empty segment
    assert abs(llr[0]) < 1e-12 and abs(llr[2]) < 1e-12                            # world against world
    assert llr[0] == lc[4][40] - lw[40]                                           # a one-frame segment
    assert abs(llr[3] - (lc[2][41:90].mean() - lw[41:90].mean())) < 1e-12
    k = np.load(os.path.join(golden_dir, "kat1_computetest.npz"))
    kw = (k["w"], k["mean_world"], k["covinv"])
    km = (np.stack([k["w_client"], k["w"]]), np.stack([k["mean_client"], k["mean_world"]]), np.stack([k["covinv_client"], k["covinv"]]))
    lw, lc = tr.frame_ref(kw, km, k["x"], int(k["top_c"]))
    for b, n, want in zip(k["seg_begin"], k["seg_len"], k["expected_llr"]):
        llr, _, _ = tr.ref_llr(lw, lc, np.array([b, b + n]), [0, 0], [0, 1])
        assert abs(llr[0] - want) < float(k["abs_tol"]) and abs(llr[1]) < 1e-12


def test_host_layer_refuses_bad_trial_lists_without_a_device():
    from lia_ral_amd import host_capi as h
    world = make_gmm(8, 12, seed=1)
    x = make_frames(*world, 40, seed=2)
    wm = (world[0], world[1], 1.0 / world[2])
    with pytest.raises(h.HostError, match="names client 2 of 2"):
        h.compute_test_batch(x, [[0]], [[40]], wm, [wm, wm], [[0, 2]])
    with pytest.raises(h.HostError, match="names client -1"):
        h.compute_test_batch(x, [[0]], [[40]], wm, [wm, wm], [[-1]])
    with pytest.raises(h.HostError, match="per line"):
        h.compute_test_batch(x, [[0], [10]], [[40]], wm, [wm], [[0]])
    with pytest.raises(h.HostError, match="1 segment begins and 2 lengths"):
        h.compute_test_batch(x, [[0]], [[20, 20]], wm, [wm], [[0]])
    assert h.lib.liagpu_compute_test_ndx and h.lib.liagpu_bench_computetest
    with pytest.raises(h.HostError, match="cannot open the ndx file"):
        h.compute_test_ndx("none.gmm", os.path.join(os.sep, "nonexistent", "x.ndx"), "", "", "")


def test_ndx_buffers_are_sized_from_the_ndx(tmp_path, golden_dir):
    """the count that sizes compute_test_ndx's buffers (host only): scores = selected segments x clients over all lines, whatever their
    number -- 70 000 here, more than any fixed buffer the binding once had"""
    import ctypes as ct
    from lia_ral_amd import host_capi as h
    ref = os.path.join(golden_dir, "ref_files")
    ndx = str(tmp_path / "big.ndx")
    ids = " ".join("client%05d" % i for i in range(35))
    with open(ndx, "w") as f:
        f.write("".join("test1 %s\n" % ids for _ in range(1000)) + "\ntest1\n")
    n = ct.c_long(0); nb = ct.c_long(0)
    assert h.lib.liagpu_compute_test_ndx_count(ndx.encode(), os.path.join(ref, "computetest_").encode(), b".lbl", b"male", ct.c_double(0.01), b"M",
                                               ct.byref(n), ct.byref(nb)) == 0
    assert n.value == 1000 * 35 * 2                              # the label file selects two segments
    longest = len("M client00000 1 test1 0.30 0.41 -1.23456789012345678e-300\n")
    assert nb.value >= n.value * longest
