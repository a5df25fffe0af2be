"""Batched models, the parts that need no GPU: the tile table of the per-segment log-likelihood kernel (gmmiv_plan_model_tiles, a pure
host function) and the numpy restatement of the batched MAP formula against the host layer's computeMAP."""
import itertools

import numpy as np
import pytest

from models_ref import SEG_LEN, SEG_MODEL, map_adapt_np, relerr, seg_layout

LENGTHS = [0, 1, 3, 15, 16, 17, 255, 256, 257]
STARTS = [0, 5, 16, 250]
TILE = 256


def check_tiles(sb, sm, tiles, tile=TILE):
    """every segment frame in exactly one (tile, row); no empty window; starts on 16-frame blocks; and the rows WRITTEN to the likelihood
    scratch (window + pads) are disjoint and fill every 16-frame block that a segment touches"""
    sb = np.asarray(sb)
    T = int(sb[-1]) + 32
    owner = np.full(T, -1)
    written = np.zeros(T + 32, int)
    for t in tiles:
        assert t["first"] % 16 == 0 and t["first"] >= 0
        assert t["first"] <= t["lo"] < t["hi"] <= t["first"] + tile, t
        s = t["seg"]
        assert sb[s] <= t["lo"] and t["hi"] <= sb[s + 1] and t["model"] == sm[s]
        assert np.all(owner[t["lo"]:t["hi"]] == -1), "a frame is covered twice"
        owner[t["lo"]:t["hi"]] = s
        assert 0 <= t["pad_lo"] < 16 and 0 <= t["pad_hi"] < 16
        assert t["lo"] - t["pad_lo"] >= t["first"] and t["hi"] + t["pad_hi"] <= t["first"] + tile
        written[t["lo"] - t["pad_lo"]:t["hi"] + t["pad_hi"]] += 1
    for s in range(len(sm)):
        assert np.all(owner[sb[s]:sb[s + 1]] == s), "segment %d is not covered" % s
    assert np.all(owner[:sb[0]] == -1) and np.all(owner[sb[-1]:] == -1)
    assert written.max(initial=0) <= 1
    blocks = np.unique(np.nonzero(owner >= 0)[0] // 16)
    for b in blocks:
        assert np.all(written[16 * b:16 * b + 16] == 1), "block %d has rows nobody writes" % b


@pytest.mark.parametrize("start", STARTS)
def test_tile_table_single_segment(start):
    from lia_ral_amd import capi
    for n in LENGTHS:
        sb, sm = [start, start + n], [3]
        tiles = capi.plan_model_tiles(sb, sm, TILE)
        assert len(tiles) == (0 if n == 0 else (start % 16 + n + TILE - 1) // TILE)
        check_tiles(sb, sm, tiles)


@pytest.mark.parametrize("start", STARTS)
def test_tile_table_segment_sequences(start):
    """all ordered pairs and one long run of the lengths, back to back from `start`: neighbours share 16-frame blocks"""
    from lia_ral_amd import capi
    for a, b in itertools.product(LENGTHS, LENGTHS):
        sb = np.cumsum([start, a, b])
        check_tiles(sb, [0, 1], capi.plan_model_tiles(sb, [0, 1], TILE))
    lens = LENGTHS + LENGTHS[::-1] + [0, 0, 1, 0]
    sb = np.cumsum([start] + lens)
    sm = np.arange(len(lens)) % 4
    tiles = capi.plan_model_tiles(sb, sm, TILE)
    check_tiles(sb, sm, tiles)
    assert [t["seg"] for t in tiles] == sorted(t["seg"] for t in tiles)          # segment order, tiles of a segment in frame order


def test_tile_table_of_the_gpu_tests_and_bad_arguments():
    from lia_ral_amd import capi
    sb, sm, T = seg_layout()
    tiles = capi.plan_model_tiles(sb, sm, TILE)
    check_tiles(sb, sm, tiles)
    assert sum(t["hi"] - t["lo"] for t in tiles) == sum(SEG_LEN) and {t["model"] for t in tiles} == set(SEG_MODEL)
    assert tiles[0]["pad_lo"] == sb[0] % 16 and tiles[-1]["pad_hi"] == (-sb[-1]) % 16
    assert all(t["pad_lo"] == 0 for t in tiles[1:]) and all(t["pad_hi"] == 0 for t in tiles[:-1])
    check_tiles(sb, sm, capi.plan_model_tiles(sb, sm, 128), tile=128)               # another tile length
    assert capi.plan_model_tiles([4, 4, 4], [0, 0], TILE) == []                     # only empty segments
    with pytest.raises(capi.GmmivError):
        capi.plan_model_tiles([10, 5], [0], TILE)                                   # decreasing bounds
    with pytest.raises(capi.GmmivError):
        capi.plan_model_tiles([0, 5], [0], 100)                                     # a tile is whole waves of 32 frames


def test_batched_map_formula_matches_compute_map():
    """map_adapt_np (tests/models_ref.py) states what gmmiv_map_adapt_models computes: the ML estimate from N / F / count, then
    computeMAP.  host_capi.compute_map -- the host layer's computeMAP, itself held to the oracle by test_cpu_plumbing.py -- is the
    reference, model by model.  All four methods, mean only and mean + weight, one Gaussian with N = 0, a count that is not whole."""
    from lia_ral_amd import host_capi as h
    rng = np.random.default_rng(11)
    G, C, D = 3, 12, 6
    w0 = rng.dirichlet(np.ones(C)); mean0 = rng.normal(size=(C, D)); cov0 = rng.uniform(0.5, 2.0, (C, D))
    count = np.array([731.0, 40.0, 2999.5])
    N = rng.dirichlet(np.ones(C), G) * count[:, None]
    N[1, 4] = 0.0
    F = (mean0 + rng.normal(0, 0.3, (G, C, D))) * N[:, :, None]
    cur = mean0 + rng.normal(0, 0.1, (G, C, D))
    reg = (14.0, 9.0, 20.0)
    for method in ("MAPOccDep", "MAPModelBased", "MAPConst", "MAPConst2", "none"):
        for weight in (False, True):
            m, w = map_adapt_np(N, F, count, w0, mean0, cur, method, True, weight, reg, 0.6)
            for g in range(G):
                wml = N[g] / count[g]
                ml = np.where(N[g][:, None] > 0, F[g] / np.where(N[g] > 0, N[g], 1.0)[:, None], cur[g])
                rw, rm, _ = h.compute_map(method, (w0, mean0, cov0), (wml, ml, cov0), count[g], mean=True, weight=weight, reg=reg, alpha_mean=0.6)
                assert relerr(m[g], rm) < 1e-14 and relerr(w[g], rw) < 1e-14, (method, weight, g)
            assert np.array_equal(m[1, 4], cur[1, 4]) or method != "none"
    m, w = map_adapt_np(N, F, count, w0, mean0, cur, "MAPOccDep", False, False, reg, 0.6)
    assert np.array_equal(m, np.broadcast_to(mean0, m.shape)) and np.array_equal(w, np.broadcast_to(w0, w.shape))
