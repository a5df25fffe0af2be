"""tests/dgemm_ref.py checked on its own, without a GPU: the exact references against a long double product, the per-element bound
against float64 numpy, the port of k_dgemm's tile orders as a bijection, and the case table of tests/test_gpu_dgemm.py against the
dispatch mirror -- every path launch_dgemm / tvk_dgemm_splitk can take must be reached by some case."""
import json
import os
import re

import numpy as np
import pytest

import dgemm_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ld = pytest.mark.skipif(not dr.HAVE_LONGDOUBLE, reason=dr.SKIP_MESSAGE)


def _pick(group, **kw):
    return [c for c in dr.CASES if c.group == group and all(getattr(c, k) == v for k, v in kw.items())]


SAMPLE = (_pick("tiles", M=131, N=129, K=33, real=False) + _pick("tiles", M=3, N=300, K=60, real=False) + _pick("batch", M=130, real=False) +
          _pick("splitk", K=100, real=False) + _pick("splitk", K=4096, real=False) + _pick("epi", M=131, real=False) + _pick("degenerate"))
REAL_SAMPLE = (_pick("tiles", M=131, N=129, K=33, real=True) + _pick("tiles", M=194, N=200, K=60, real=True) + _pick("batch", M=130, real=True) +
               _pick("splitk", K=101, real=True) + _pick("splitk", K=4096, real=True) + _pick("epi", M=131, real=True))


@needs_ld
def test_exact_references_equal_a_long_double_product():
    """the float64 / int64 reference of an exact case is the mathematical result: equal to the same expression in long double, and
    every value an integer multiple of 2^-7 below 2^40 (so nothing was rounded on the way)"""
    assert len(SAMPLE) >= 40
    for c in SAMPLE:
        d = dr.exact_case(c)
        oa, ob = dr._op(c, d["A"].astype(dr.LD), d["B"].astype(dr.LD))
        v = dr.LD(c.alpha) * np.matmul(oa, ob)
        if c.epi == 1:
            v = v * d["rv"].astype(dr.LD)[None, :, None] * d["cv"].astype(dr.LD)[None, None, :]
        elif c.epi == 2:
            v = v + d["br"] * d["rv"].astype(dr.LD)[None, :, None] + d["bc"] * d["cv"].astype(dr.LD)[None, None, :] + d["cst"]
        v = v + dr.LD(c.beta) * d["C"].astype(dr.LD)
        assert d["ref"].shape == (c.batch, c.M, c.N) and d["ref"].dtype == np.float64
        assert np.array_equal(d["ref"].astype(dr.LD), np.broadcast_to(v, d["ref"].shape)), c.name
        q = d["ref"] * 128.0
        assert np.array_equal(q, np.rint(q)) and np.abs(d["ref"]).max() < 2.0 ** 40, c.name


@needs_ld
def test_the_bound_holds_for_float64_numpy_with_a_margin():
    """numpy's float64 product (BLAS, its own summation order) stays inside the per-element bound on the real cases, and not by
    accident: below a fifth of it.  A result with one term of the dot product dropped is outside it."""
    worst = 0.0
    for c in REAL_SAMPLE:
        d = dr.real_case(c)
        oa, ob = dr._op(c, d["A"], d["B"])
        v = c.alpha * np.matmul(oa, ob)
        if c.epi == 1:
            v = v * d["rv"][None, :, None] * d["cv"][None, None, :]
        elif c.epi == 2:
            v = v + d["br"] * d["rv"][None, :, None] + d["bc"] * d["cv"][None, None, :] + d["cst"]
        if c.beta != 0:
            v = v + c.beta * d["C"]
        v = np.broadcast_to(v, d["ref"].shape)
        ratio = (np.abs(v.astype(dr.LD) - d["ref"]) / d["bound"]).astype(np.float64)
        assert d["bound"].min() > 0 and ratio.max() <= 0.2, (c.name, ratio.max())
        worst = max(worst, ratio.max())
        # one term of every dot product dropped (k = 0): far outside, in nearly every element
        drop = (c.alpha * oa[:, :, :1] * ob[:, :1, :]) * (d["rv"][None, :, None] * d["cv"][None, None, :] if c.epi == 1 else 1.0)
        rd = (np.abs((v - drop).astype(dr.LD) - d["ref"]) / d["bound"]).astype(np.float64)
        assert np.median(rd) > 1e3, (c.name, np.median(rd))
    print("largest float64-numpy error / bound over %d real cases: %.3f" % (len(REAL_SAMPLE), worst))


def test_the_elements_of_a_real_case_span_many_orders_of_magnitude():
    d = dr.real_case(_pick("tiles", M=194, N=200, K=60, real=True)[0])
    a = np.abs(d["ref"].astype(np.float64))
    assert a.max() / np.median(a) > 1e6 and np.median(a) / a.min() > 1e6


@pytest.mark.parametrize("remap", (1, 2))
def test_the_tile_orders_are_bijections(remap):
    """every grid up to 149 x 39 tiles: each tile is worked on exactly once, and inside the grid"""
    for Nt in range(1, 150):
        for Mt in range(1, 40):
            by, bx = np.divmod(np.arange(Nt * Mt), Nt)
            tx, ty = dr.remap_tile(remap, Nt, Mt, bx, by)
            assert tx.min() >= 0 and tx.max() < Nt and ty.min() >= 0 and ty.max() < Mt, (remap, Nt, Mt)
            assert np.array_equal(np.sort(ty * Nt + tx), np.arange(Nt * Mt)), (remap, Nt, Mt)
    assert [tuple(int(v) for v in dr.remap_tile(remap, 20, 3, x, y)) for x, y in ((0, 0), (8, 0), (9, 1), (19, 2))] == \
        [(0, 0), (0, 1), (13, 0), (19, 2)]      # by hand from the kernel: G = 2, 48 remapped ids, 12 left over


def test_embed_keeps_offsets_strides_and_fill():
    x = np.arange(24.0).reshape(2, 3, 4)
    flat, view, (s, ld) = dr.embed(x, (3, 5), np.nan, 1)
    assert (s, ld) == (3 * 7 + 5, 7) and flat.size == 2 * dr.MARGIN + 1 + 2 * s and np.array_equal(view, x)
    assert view.__array_interface__["data"][0] - flat.__array_interface__["data"][0] == 8 * (dr.MARGIN + 1)
    assert np.isnan(flat).sum() == flat.size - 24
    flat, view, (s, ld) = dr.embed(x[0], (2, 4), 7.0, 0, shared=3)
    assert s == 0 and view.shape == (3, 3, 4) and np.array_equal(view[2], x[0]) and (flat == 7.0).sum() == flat.size - 12 + (x[0] == 7.0).sum()
    for c in dr.CASES[::97]:
        lay = dr.layouts(c)
        for key in "ABC":
            (b, r, cc), (s, ld), off = lay[key]
            assert ld >= cc + 2 and (s == 0 or s >= r * ld + 4)
        assert lay["A"][1][1] % 2 == c.ald and lay["B"][1][1] % 2 == c.bld and lay["C"][1][1] % 2 == c.cld


def test_plan_on_known_calls():
    """hand-derived from launch_dgemm: R = 400 products of the i-vector path"""
    ls, red = dr.plan(True, False, 400, 122880, 1024, 400, 122880)               # Cmx += W^T F: interior + a 16-row bottom strip of 32-row tiles
    assert not red and [(l.mode, l.am, l.an, l.grid, l.m_off, l.n_off, l.side) for l in ls] == [
        (2, 1, 4, (960, 1, 1), 384, 0, True), (0, 4, 4, (960, 3, 1), 0, 0, False)] and all(l.remap == 1 for l in ls)
    ls, red = dr.plan(False, True, 1024, 400, 122880, 122880, 122880, nz=0)       # aux = F (T Sigma^-1)^T: nt80, split-K
    assert red and len(ls) == 1 and ls[0].inst == "k_dgemm<false, true, 0, 2, 5, 4, 1>" and ls[0].grid[:2] == (5, 8) and ls[0].grid[2] == len(ls[0].layers)
    assert all(ke - kb == ls[0].layers[0][1] and krem == 0 for kb, ke, nkt, krem in ls[0].layers[:-1])
    ls, red = dr.plan(False, True, 130, 160, 100, 102, 102, nz=3)
    assert red and [l.layers for l in ls][0] == ((0, 48, 3, 0), (48, 96, 3, 0), (96, 100, 1, 4))
    ls, red = dr.plan(False, False, 131, 129, 18, 20, 132)                         # odd N, n-fastest B: no clamp
    assert [(l.mode, l.grid, l.m_off, l.n_off) for l in ls] == [(1, (1, 2, 1), 0, 128), (1, (1, 1, 1), 128, 0), (0, (1, 1, 1), 0, 0)]
    assert dr.plan(False, False, 0, 5, 3, 4, 6) == ([], False) and dr.plan(False, False, 5, 5, 0, 2, 6)[0][0].mode == 1


def test_the_case_table_reaches_every_dispatch_path():
    """CASES through the mirror: each target of dgemm_ref.targets() -- every MODE x tile shape per transpose pair, every k-tail
    parity, both tile orders' ragged blocks, split-K's ragged range, the batch strides and each way out of the aligned loads --
    is reached by at least one case, and by an exact one."""
    reached, reached_real = set(), set()
    for c in dr.CASES:
        (reached_real if c.real else reached).update(dr.features(c))
    missing = [t for t in dr.targets() if t not in reached]
    assert not missing, "no exact case of dgemm_ref.CASES reaches: " + "; ".join(missing)
    inst = sorted(t for t in dr.targets() if t.startswith("inst k_dgemm"))
    assert len(inst) == 21
    missing = [t for t in inst if t not in reached_real]
    assert not missing, "no real-valued case reaches: " + "; ".join(missing)
    # nothing the mirror can produce is outside the list of instantiations the library compiles
    extra = sorted(t for t in reached | reached_real if t.startswith("inst ") and t not in dr.targets())
    assert not extra, extra


def test_the_case_table_is_the_one_the_issue_lists():
    g = {}
    for c in dr.CASES:
        g.setdefault(c.group, []).append(c)
    ex = [c for c in g["tiles"] if not c.real]
    assert len(ex) == 4 * 8 * 10 * 6 and {(c.M, c.N) for c in ex} == set(dr.TILE_SHAPES) and {c.K for c in ex} == set(dr.TILE_KS)
    assert {(c.alpha, c.beta) for c in ex} == {(a, b) for a in (1.0, -0.5) for b in (0.0, 1.0, -2.0)}
    assert len([c for c in g["options"] if not c.real]) == 2 * 4 * 2 * 10 * 6
    assert {dict(c.opts).get("gemm_remap", 1) for c in g["order"]} == {0, 1, 2} and {(c.M, c.N, c.K) for c in g["order"]} == {(1186, 9384, 18), (300, 2448, 16)}
    assert all(dr.plan_case(c)[0][0].inst != "k_dgemm<false, true, 0, 2, 5, 4, 1>" for c in g["splitk"] if c.ald or dict(c.opts).get("gemm_nt80") == 0)
    assert max(c.K for c in dr.CASES) == 4096


def test_the_records_of_the_gpu_run_match_the_mirror():
    """profiles/r12: the kernel trace of tests/test_gpu_dgemm.py lists exactly the instantiations the mirror predicts for CASES (one
    it lacks would mean the mirror is wrong, one it has beyond them a path nobody planned), and every real case has its measured
    ratio to the bound on record, all below 1."""
    text = open(os.path.join(ROOT, "profiles", "r12", "dgemm_kernel_stats.txt")).read()
    traced = set(re.findall(r"^(k_dgemm<[^>]*>|k_splitk_reduce)\(", text, re.M))
    expected = {t[5:] for t in dr.targets() if t.startswith("inst ")}
    assert len(expected) == 22
    assert not expected - traced, "predicted, not in the trace: %s" % sorted(expected - traced)
    assert not traced - expected, "in the trace, not predicted: %s" % sorted(traced - expected)
    rec = json.load(open(os.path.join(ROOT, "profiles", "r12", "dgemm_errors.json")))
    assert set(rec["cases"]) == {c.name for c in dr.CASES if c.real}
    assert 0 < max(rec["cases"].values()) <= 1.0 and abs(rec["max_ratio"] - max(rec["cases"].values())) < 1e-3
