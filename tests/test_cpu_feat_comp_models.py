"""Batched channel compensation (gmmiv_feat_compensate_models), the parts that need no GPU: the two C ABI symbols, the refusal of a
NULL context or batch, and the host planner gmmiv_plan_feat_tiles against a brute-force restatement that assigns every frame of every
16-frame block to its segment and cuts each segment's blocks into runs of blocks_per_tile."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_refuse_null_handles():
    from lia_ral_amd import capi
    lib = capi.lib
    hdr = open(os.path.join(ROOT, "include", "gmmiv.h")).read()
    assert hasattr(lib, "gmmiv_feat_compensate_models") and re.search(r"\bint gmmiv_feat_compensate_models\(gmmiv_ctx \*ctx, const gmmiv_gmm_batch \*b", hdr)
    assert hasattr(lib, "gmmiv_plan_feat_tiles") and re.search(r"\bint64_t gmmiv_plan_feat_tiles\(const int64_t \*seg_begin", hdr)
    assert "typedef struct gmmiv_feat_tile" in hdr and "waits once for its table" in hdr
    assert hasattr(capi.GmmBatch, "feat_compensate") and hasattr(capi, "plan_feat_tiles")
    null, i64 = ct.c_void_p(0), ct.c_int64
    buf = (ct.c_double * 8)()
    sb = (ct.c_int64 * 2)(0, 1)
    sm = (ct.c_int32 * 1)(0)
    rc = lib.gmmiv_feat_compensate_models(null, null, buf, 1, i64(1), i64(4), sb, sm, i64(1), buf, i64(0), buf, 1, i64(4))
    assert rc == -1 and b"feat_compensate_models" in lib.gmmiv_last_error()         # GMMIV_ERR_ARG, with a message


def brute(seg_begin, seg_model, bpt):
    """every (segment, block) pair that shares a frame, found frame by frame; then runs of bpt blocks from the segment's first block"""
    sb = [int(v) for v in seg_begin]
    out = []
    for s in range(len(sb) - 1):
        frames = list(range(sb[s], sb[s + 1]))
        if not frames:
            continue
        blocks = sorted({t // 16 for t in frames})
        first = blocks[0]
        for run in sorted({first + (b - first) // bpt * bpt for b in blocks}):
            mine = [t for t in frames if run <= t // 16 < run + bpt]
            out.append(dict(block=run, lo=mine[0], hi=mine[-1] + 1, model=int(seg_model[s]), seg=s))
    return out


def invariants(seg_begin, seg_model, bpt, tiles):
    sb = [int(v) for v in seg_begin]
    assert [(t["seg"], t["block"]) for t in tiles] == sorted((t["seg"], t["block"]) for t in tiles)
    for s in range(len(sb) - 1):
        mine = [t for t in tiles if t["seg"] == s]
        if sb[s + 1] == sb[s]:
            assert not mine                                                         # an empty segment has no entry
            continue
        assert mine[0]["block"] == sb[s] // 16 and mine[0]["lo"] == sb[s] and mine[-1]["hi"] == sb[s + 1]
        for a, b in zip(mine, mine[1:]):
            assert a["hi"] == b["lo"] and b["block"] == a["block"] + bpt            # disjoint, ordered, no gap
        for t in mine:
            assert 16 * t["block"] <= t["lo"] < t["hi"] <= 16 * (t["block"] + bpt)
            assert sb[s] <= t["lo"] and t["hi"] <= sb[s + 1]                        # no entry spans two segments
            assert t["model"] == int(seg_model[s])


HAND = {
    "three segments inside one block": ([5, 6, 9, 13], [0, 1, 2]),
    "a segment of 1 frame": ([31, 32], [3]),
    "an empty segment": ([0, 20, 20, 45], [0, 1, 2]),
    "empty segments at both ends and mid-block": ([7, 7, 7, 30, 30], [0, 1, 2, 0]),
    "a segment starting mid-block": ([23, 100], [1]),
    "exactly 16 frames": ([16, 32], [0]),
    "exactly 16 frames, mid-block": ([8, 24], [0]),
    "the issue's lengths after 5 leading frames": (np.cumsum([5, 1, 3, 4, 0, 16, 17, 40, 15, 130, 33]), [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]),
}


@pytest.mark.parametrize("bpt", [1, 2, 4])
def test_planner_matches_the_brute_force_restatement(bpt):
    from lia_ral_amd import capi
    tables = dict(HAND)
    tables["exactly 16 blocks_per_tile frames"] = ([0, 16 * bpt], [0])
    tables["exactly 16 blocks_per_tile frames, then one more segment"] = ([16, 16 + 16 * bpt, 16 + 16 * bpt + 1], [1, 0])
    rng = np.random.default_rng(100 + bpt)
    for k in range(40):
        nseg = int(rng.integers(0, 12))
        lens = rng.choice([0, 1, 2, 15, 16, 17, 16 * bpt, 16 * bpt + 1, 33, 100], nseg)
        tables["random %d" % k] = (np.cumsum(np.r_[rng.integers(0, 50), lens]), rng.integers(0, 5, nseg))
    for name, (sb, sm) in tables.items():
        tiles = capi.plan_feat_tiles(sb, sm, bpt)
        assert tiles == brute(sb, sm, bpt), name
        invariants(sb, sm, bpt, tiles)
        # entries beyond cap are counted, not written; tiles may be NULL
        assert capi.plan_feat_tiles(sb, sm, bpt, count_only=True) == len(tiles), name
        for cap in (0, 1, len(tiles)):
            n, head = capi.plan_feat_tiles(sb, sm, bpt, cap=cap)
            assert n == len(tiles) and head == tiles[:cap], (name, cap)


def test_planner_leaves_the_entries_beyond_cap_alone_and_refuses_bad_tables():
    from lia_ral_amd import capi
    lib = capi.lib
    sb = np.array([3, 40, 41, 90], np.int64)
    sm = np.array([2, 0, 1], np.int32)
    args = (sb.ctypes.data_as(ct.c_void_p), sm.ctypes.data_as(ct.c_void_p), ct.c_int64(3))
    buf = (capi.FeatTile * 8)()
    for t in buf:
        t.block = -99
    n = lib.gmmiv_plan_feat_tiles(*args, 1, ct.cast(buf, ct.c_void_p), ct.c_int64(2))
    assert n == 3 + 1 + 4 and buf[1].block == 1 and all(buf[i].block == -99 for i in range(2, 8))
    # the three -1 cases: a decreasing table, blocks_per_tile < 1, nseg < 0
    dec = np.array([3, 40, 39, 90], np.int64)
    assert lib.gmmiv_plan_feat_tiles(dec.ctypes.data_as(ct.c_void_p), args[1], args[2], 2, None, ct.c_int64(0)) == -1
    assert lib.gmmiv_plan_feat_tiles(*args, 0, None, ct.c_int64(0)) == -1
    assert lib.gmmiv_plan_feat_tiles(args[0], args[1], ct.c_int64(-1), 2, None, ct.c_int64(0)) == -1
    with pytest.raises(capi.GmmivError):
        capi.plan_feat_tiles(dec, sm, 2)
    assert lib.gmmiv_plan_feat_tiles(args[0], args[1], ct.c_int64(0), 2, None, ct.c_int64(0)) == 0          # nseg = 0 is valid


def test_segment_aware_kernel_keeps_the_single_model_arithmetic():
    """source checks in the manner of tests/test_cpu_feat_comp.py: the segment-aware form is the SAME kernel body (one summation order,
    no atomics, no split of the Gaussian sum), its offsets are packed by one launch per chunk, and the C entry checks its arguments
    before the first workspace request, copy or launch"""
    csrc = os.path.join(ROOT, "lia_ral_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "feat_comp.hip")).read())
    assert len(re.findall(r"void k_feat_comp\(", code)) == 1 and "bool SEG" in code
    k = code[code.index("void k_feat_comp("):code.index("static int launch_feat_comp")]
    assert "tiles[" in k and "off_stride" in k and "for (int ct = 0; ct < nct; ++ct)" in k and "atomic" not in k
    pk = code[code.index("int gmmk_feat_pack_offsets("):]
    pk = pk[:pk.index("\n}\n")]
    assert pk.count("<<<") == 1 and "for (" not in pk                               # one launch for all models of the chunk
    src = open(os.path.join(csrc, "capi_models.hip")).read()
    body = src[src.index("int gmmiv_feat_compensate_models("):]
    body = body[:body.index("\n}\n")]
    first_work = min(body.index(tok) for tok in ("xv.init(", "c->scratch(", ".init(c, WS_", "upload_plan("))
    for chk in ("check_batch(", "check_segments(", "offset == NULL", "gmmiv_feat_check_args("):
        assert 0 < body.index(chk) < first_work, chk
    assert "plan_chunks(" in body and "OneModel" in body and "never evaluated" in body
