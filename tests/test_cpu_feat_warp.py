"""Feature warping without a GPU: KAT-7 (the histogram rule against NormFeat/test/01New.histo), the restatement of warping()
(tests/warp_ref.py) against a Gaussian column, the .histo layout, planted defects the yardstick must catch, and what
include/ext/gmmiv_feat_warp.h promises before a context is looked at."""
import ctypes as ct
import os

import numpy as np
import pytest

import warp_ref as W
from conftest import GOLDEN, ROOT

from lia_ral_amd import capi
from lia_ral_amd import feat_warp as fw

lib = capi.lib
ERR_ARG = -1
H01 = os.path.join(GOLDEN, "01New.histo")
HG = os.path.join(GOLDEN, "table_gaussN.histo")


@pytest.fixture(scope="module")
def chain():
    return W.box_muller_chain(1000000)


@pytest.fixture(scope="module")
def gauss_column():
    rng = np.random.default_rng(7)
    return 3.0 + 2.0 * rng.standard_normal(100000)


# ------------------------------------------------------------------------------------------------------------------------ KAT-7
def test_glibc_rand_first_draws():
    assert list(W.glibc_rand(5)) == [1804289383, 846930886, 1681692777, 1714636915, 1957747793]  # the well-known default-seed stream


def test_kat7_bounds(chain):
    """01New.histo is makeGausHisto(10^6, 0, 1, 20).  Pinned: min and max exact at the printed precision; bound[i] = d[i k] reproduces
    16 of the 19 interior bounds; the other three (i = 5, 10, 13) lie strictly inside (d[i k - 1], d[i k]) -- carried as assumed."""
    tok = open(H01).read().split()
    nb = int(tok[0])
    printed = tok[1:1 + 2 * nb:2] + [tok[-1]]
    b, c, st = W.histo(chain, nb)
    assert st == 0
    assert "%g" % b[0] == printed[0] == "-4.77555" and "%g" % b[-1] == printed[-1] == "4.85599"
    hit = [i for i in range(1, nb) if "%g" % b[i] == printed[i]]
    print("interior bounds reproduced at %%g: %d of %d, missed %s" % (len(hit), nb - 1, sorted(set(range(1, nb)) - set(hit))))
    assert len(hit) >= 16
    d = np.sort(chain)
    k = len(d) // nb
    for i in set(range(1, nb)) - set(hit):       # a miss is a value inside the gap just below the order statistic, nothing else
        assert d[i * k - 1] < float(printed[i]) < d[i * k]


def test_kat7_area_identity(chain):
    """count is a density: count[i] * width[i] * nbBin = 1 in the file (to its printed digits) and in the restatement (to rounding)."""
    fb, fc = W.read_histo(H01)
    nb = len(fc)
    half = lambda v: 0.5 * 10.0 ** (np.floor(np.log10(np.abs(v))) - 5)        # half a unit of the sixth printed digit (%g)
    bar = (half(fb[:-1]) + half(fb[1:])) / np.diff(fb) + half(fc) / fc
    print("file: |count * width * nbBin - 1| / bar, worst bin: %.3f" % np.max(np.abs(fc * np.diff(fb) * nb - 1) / bar))
    assert np.all(np.abs(fc * np.diff(fb) * nb - 1) <= 1.01 * bar)
    b, c, _ = W.histo(chain, nb)
    assert np.max(np.abs(c * np.diff(b) * nb - 1)) < 1e-14
    assert np.max(np.abs(c / fc - 1)) < 1e-4   # a displaced bound moves < 1e-5 of a bin >= 0.127 wide (8e-5), the printed digits 3e-6
    bl, cl, _ = W.histo(chain, nb, np.longdouble)
    assert np.array_equal(bl.astype(np.float64), b) and np.max(np.abs((cl - c) / cl)) < 4 * 2.0 ** -53


def test_histo_remainder_and_degenerate():
    rng = np.random.default_rng(0)
    v = rng.standard_normal(107).astype(np.float32)
    b, c, st = W.histo(v, 10)
    d = np.sort(v).astype(np.float64)
    assert st == 0 and np.array_equal(b, np.r_[d[0:100:10], d[-1]])
    assert abs(np.sum(c * np.diff(b)) - 1) < 1e-15 and abs(c[-1] * (b[-1] - b[-2]) - 17 / 107) < 1e-16   # the last bin holds 10 + 7
    assert W.histo(v[:9], 10)[2] == W.DEGENERATE                       # n < nbBin
    assert W.histo(np.full(50, 2.5), 10)[2] == W.DEGENERATE             # constant
    t = np.arange(100.0)
    t[30:41] = 30.0                                                     # d[30] == d[40]: bin 3 has no width
    bt, ct_, stt = W.histo(t, 10)
    assert stt == W.DEGENERATE and np.sum(np.diff(bt) == 0) == 1
    v2 = v.copy()
    v2[5] = np.nan                                                      # +NaN sorts last: the last bound
    b2, _, st2 = W.histo(v2, 10)
    assert st2 == W.DEGENERATE and np.isnan(b2[-1]) and not np.isnan(b2[:-1]).any()
    v2[5] = -np.nan if np.signbit(-np.nan) else np.copysign(np.nan, -1.0)
    b3, _, st3 = W.histo(v2, 10)
    assert st3 == W.DEGENERATE and np.isnan(b3[0]) and not np.isnan(b3[1:]).any()


# ------------------------------------------------------------------------------------------------------------------- warping()
def test_histo_round_trip(tmp_path):
    for path in (H01, HG):
        b, c = W.read_histo(path)
        out = str(tmp_path / os.path.basename(path))
        fw.write_histo(out, b, c)
        assert open(out).read().split() == open(path).read().split()    # token for token: %g is the file's precision
        b2, c2 = fw.read_histo(out)
        assert np.array_equal(b, b2) and np.array_equal(c, c2)
    b, c = W.read_histo(HG)
    assert len(c) == 700 and b[0] == -3.5 and b[-1] == 3.5 and np.allclose(np.diff(b), 0.01, atol=1e-12)
    assert np.all(c > 0) and abs(np.sum(c * np.diff(b)) - 1) < 1e-3   # a density on [-3.5, 3.5], renormalised to area 1


def test_warp_gaussianises(gauss_column):
    """10^5 samples of N(3, 2^2) through their own histogram onto table_gaussN.histo: N(0, 1) within sampling error.  1000 bins: the
    source's cumulative curve is linear inside a bin, which squeezes the two tail bins towards their inner edge -- with 40 bins each
    tail bin holds 2.5 % of the mass and the output's std drops to 0.96 (the method's, not an error); with 0.1 % it loses < 0.002.  The
    bars: the mean of n N(0,1) samples has sd 1/sqrt(n) = 0.0032, their std has sd 1/sqrt(2n) = 0.0022; five sd each, plus what the
    table itself loses -- it stops at +-3.5 (mass 4.7e-4 missing, std of the truncated normal 0.9985) and is piecewise constant."""
    tb, tc = W.read_histo(HG)
    b, c, st = W.histo(gauss_column, 1000)
    assert st == 0
    y = W.warp_column(gauss_column, b, c, tb, tc)
    print('warped N(3, 4): mean %.5f std %.5f' % (y.mean(), y.std()))
    assert np.all(np.isfinite(y)) and y.min() >= -3.5 and y.max() <= 3.5
    assert abs(y.mean()) < 5 * 0.0032 + 0.002 and abs(y.std() - 1) < 5 * 0.0022 + 0.004
    order = np.argsort(gauss_column)
    assert np.all(np.diff(y[order]) >= -4e-4)   # monotone up to the jump of the as-written back-off at a target bin edge
    q = np.quantile(y, [0.1, 0.5, 0.9])
    assert np.max(np.abs(q - np.array([-1.2816, 0.0, 1.2816]))) < 0.02


def test_vector_form_is_the_loop(gauss_column):
    """warp_column (what the device is compared with) against warping() loop for loop, bit for bit, fp64 and long double."""
    tb, tc = W.read_histo(HG)
    x = gauss_column[:3000]
    for fp in (np.float64, np.longdouble):
        b, c, _ = W.histo(x, 40, fp)
        tbf, tcf = tb.astype(fp), tc.astype(fp)
        y = W.warp_column(x, b, c, tbf, tcf, fp)
        pick = np.r_[np.argsort(x)[[0, 1, 74, 75, 76, 1499, 2998, 2999]], np.arange(0, 3000, 97)]
        for i in pick:
            assert W.warping(x[i], b, c, tbf, tcf) == y[i]
    y64 = W.warp_column(x, *W.histo(x, 40)[:2], tb, tc)
    yld = W.warp_column(x, *W.histo(x, 40, np.longdouble)[:2], tb, tc, np.longdouble)
    assert np.max(np.abs(y64 - yld.astype(np.float64))) < 4e-4   # at worst one flipped bin decision (the back-off's jump); rounding otherwise


# --------------------------------------------------------------------------------------------------------- planted defects
def test_defect_bound_one_below(chain):
    tok = open(H01).read().split()
    nb = int(tok[0])
    printed = tok[1:1 + 2 * nb:2] + [tok[-1]]
    b = W.histo(chain, nb, bound_shift=-1)[0]
    hit = sum("%g" % b[i] == printed[i] for i in range(1, nb))
    assert hit < 16


def test_defect_raw_count(chain):
    fb, fc = W.read_histo(H01)
    b, c, _ = W.histo(chain, 20, density=False)
    assert np.max(np.abs(c * np.diff(b) * 20 - 1)) > 1 and np.max(np.abs(c / fc - 1)) > 1


def test_defect_missing_backoff(gauss_column):
    tb, tc = W.read_histo(HG)
    x = gauss_column[:5000]
    b, c, _ = W.histo(x, 40)
    good, bad = W.warp_column(x, b, c, tb, tc), W.warp_column(x, b, c, tb, tc, backoff=False)
    assert np.mean(good != bad) > 0.9       # the loop stops one bin late: without the step back nearly every value has other bits
    i = int(np.argsort(x)[2500])
    assert W.warping(x[i], b, c, tb, tc, backoff=False) == bad[i] != good[i]


# ------------------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_symbols():
    h = open(os.path.join(ROOT, "include", "ext", "gmmiv_feat_warp.h")).read()
    assert '#include "../gmmiv.h"' in h and "include/ext/" in h.split("*/")[0] and "lia_ral_amd/feat_warp.py" in h.split("*/")[0]
    for name in ("gmmiv_feat_warp_hist", "gmmiv_feat_warp_apply"):
        assert name in h and hasattr(lib, name)
    assert "GMMIV_WARP_DEGENERATE 1" in h and fw.WARP_DEGENERATE == 1 and fw.WARP_FORCE_SELECT == 1
    assert not os.path.exists(os.path.join(ROOT, "include", "gmmiv_feat_warp.h"))
    assert "feat_warp" not in open(os.path.join(ROOT, "lia_ral_amd", "capi.py")).read()


def _hist(ctx=None, dt=capi.F32, ldx=4, D=3, runs=((0, 10, 0),), nunits=1, nbin=4, flags=0, out=True):
    r = np.ascontiguousarray(runs, np.int64).reshape(-1, 3)
    b, c, s = np.zeros((max(nunits, 1), max(D, 1), nbin + 1)), np.zeros((max(nunits, 1), max(D, 1), max(nbin, 1))), np.zeros((max(nunits, 1), max(D, 1)), np.int32)
    p = capi._ptr
    rc = lib.gmmiv_feat_warp_hist(ctx, None, dt, ldx, D, p(r) if len(r) else None, len(r), nunits, nbin, flags, *(map(p, (b, c, s)) if out else (None,) * 3))
    return rc, lib.gmmiv_last_error().decode()


def _apply(ctx=None, dt=capi.F32, odt=capi.F32, ldx=4, ldo=4, D=3, runs=((0, 10, 0),), nunits=1, nbin=4, tb=(0.0, 1.0, 2.0), tc=(0.5, 0.5), x=None, out=None):
    r = np.ascontiguousarray(runs, np.int64).reshape(-1, 3)
    b, c, s = np.zeros((max(nunits, 1), max(D, 1), nbin + 1)), np.zeros((max(nunits, 1), max(D, 1), max(nbin, 1))), np.zeros((max(nunits, 1), max(D, 1)), np.int32)
    tb, tc = np.array(tb, np.float64), np.array(tc, np.float64)
    p = capi._ptr
    rc = lib.gmmiv_feat_warp_apply(ctx, x, dt, ldx, out, odt, ldo, D, p(r) if len(r) else None, len(r), nunits, nbin, p(b), p(c), p(s), len(tc), p(tb), p(tc))
    return rc, lib.gmmiv_last_error().decode()


def test_null_context_is_refused_last():
    for call in (_hist, _apply):
        rc, msg = call()
        assert rc == ERR_ARG and "NULL context" in msg


def test_argument_checks_come_before_the_context():
    for call, name in ((_hist, "feat_warp_hist"), (_apply, "feat_warp_apply")):
        for kw, word in ((dict(dt=7), "dtype"), (dict(D=0), "bad argument"), (dict(ldx=2), "bad argument"), (dict(nbin=0), "nbin"),
                         (dict(nbin=fw.WARP_MAX_BINS + 1), "nbin"), (dict(nunits=-1), "bad argument"),
                         (dict(runs=((0, 5, 0), (-1, 2, 0))), "run 1 has a negative"),
                         (dict(runs=((0, 5, 0), (9, 2, 1), (20, 2, 0)), nunits=2), "run 2: unit 0 is below"),
                         (dict(runs=((0, 5, 0), (9, 2, 2)), nunits=2), "run 1: unit 2"),
                         (dict(runs=((0, 5, 0), (9, 5, 0), (12, 2, 0))), "run 2 of unit 0 overlaps"),
                         (dict(runs=((0, 5, 0), (9, 5, 1), (3, 2, 1)), nunits=2), "run 2 of unit 1 begins before")):
            rc, msg = call(**kw)
            assert rc == ERR_ARG and word in msg and name in msg and "NULL context" not in msg, (kw, msg)
    assert "flags" in _hist(flags=2)[1] and "NULL" in _hist(out=False)[1] and "context" not in _hist(out=False)[1]
    # the target (a host table) and the overlap rule
    assert "target bin 1: its upper bound" in _apply(tb=(0.0, 1.0, 0.5))[1]
    assert "target bin 0: its count" in _apply(tc=(-0.5, 0.5))[1] and "target bin 1: its count" in _apply(tc=(0.5, float("nan")))[1]
    assert "nbin_t" in _apply(tb=(0.0,), tc=())[1]
    buf = np.zeros(256, np.float32)
    base = buf.ctypes.data
    assert "same dtype and stride" in _apply(x=base, out=base, odt=capi.F64)[1] and "same dtype and stride" in _apply(x=base, out=base, ldo=5)[1]
    assert "overlaps x without being x" in _apply(x=base, out=base + 16)[1]
    assert "overlaps x without being x" in _apply(x=base + 4 * 36, out=base)[1]                      # the last frame of out reaches x
    assert "NULL context" in _apply(x=base, out=base)[1] and "NULL context" in _apply(x=base, out=base + 4 * 40)[1]
    # empty calls are valid shapes: only the context is missing
    assert "NULL context" in _hist(runs=(), nunits=0)[1] and "NULL context" in _apply(runs=(), nunits=0)[1]
