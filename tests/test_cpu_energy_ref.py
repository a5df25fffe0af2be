"""tests/energy_ref.py against what is known without a GPU: KAT-6's golden, the sequential fp64 restatement, and the distance of every
case of the GPU list from the decisions two correct implementations could take differently."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_ref as er  # noqa: E402
from test_oracle_kat import energy_select_frames, kat6_normalised  # noqa: E402


@pytest.fixture(scope="module")
def ref():
    from lia_ral_amd import capi
    return er.reference(capi.energy_stage_frames(capi.F32), capi.energy_stage_frames(capi.F64))


def test_chain80_reproduces_kat6(golden_dir):
    k = np.load(os.path.join(golden_dir, "kat6_energydetector_assumed.npz"))
    C = len(k["init_w"])
    w0, m0, c0 = er.init_model(C, np.float64)
    assert np.array_equal(w0, k["init_w"]) and np.array_equal(m0, k["init_mean"]) and np.array_equal(c0, k["init_cov"])   # energyMixtureInit
    assert float(k["variance_flooring"]) == er.FLOORING and float(k["variance_ceiling"]) == er.CEILING
    for over_file in (False, True):
        e = kat6_normalised(k, over_file)
        rows = np.concatenate([np.arange(b, b + n) for b, n in zip(k["seg_begin"], k["seg_len"])])
        r = er.chain(e[rows], C, int(k["nb_train_it"]), float(k["alpha"]))
        th = float(r["threshold"])
        assert np.array_equal(np.nonzero(e[:26] > th)[0], k["expected_frames"])
        assert energy_select_frames(e, th, k["seg_begin"], k["seg_len"]) == [tuple(k["expected_seg"])]


def test_chain80_agrees_with_the_fp64_restatement(ref):
    """1e-9 max(1, max x^2): five orders above the rounding of either chain, four below 1 / n of the longest file -- where a wrong formula
    (biased against unbiased variance, a missing - mean^2, floor and ceiling swapped) shows"""
    worst = 0.0
    for g in ref:
        for f in g["ref"]:
            if len(f["x"]) == 0:
                continue
            r64 = er.seq64(f["x"], g["C"], g["nb_it"], g["alpha"])
            tol = 1e-9 * max(1.0, float(np.max(f["x"].astype(np.float64) ** 2)))
            for q in ("w", "mean", "cov", "threshold"):
                d = float(np.max(np.abs(np.asarray(r64[q], er.LD) - f["r80"][q])))
                worst = max(worst, d / tol)
                assert d <= tol, (g["name"], len(f["x"]), q, d)
    print("largest |fp64 restatement - 80-bit| / tolerance: %.3g" % worst)


def test_every_case_is_1000_bars_from_every_decision(ref):
    ncase, least = 0, np.inf
    for g in ref:
        for i, f in enumerate(g["ref"]):
            n, m, b, r = len(f["x"]), f["margins"], f["bar"], f["r80"]
            ncase += 1
            if n == 0:
                assert r["status"] == er.EMPTY
                continue
            worst_bar = max(float(np.max(b[q])) for q in b)
            checks = dict(cov=m["cov"] / float(np.max(b["cov"])), mean=m["mean"] / float(np.max(b["mean"])),
                          threshold=float(np.min(np.abs(f["x"].astype(er.LD) - r["threshold"]))) / float(b["threshold"]),
                          llk=m["llk"] / worst_bar)
            if g["nb_it"] == 0:
                checks.pop("cov"); checks.pop("llk")                    # no iteration: no floor, ceiling or likelihood decision
            for what, v in checks.items():
                least = min(least, v)
                assert v >= 1000.0, (g["name"], i, n, what, v)
            assert not r["status"] & (er.EMPTY | er.NONFINITE)
    assert ncase == sum(len(g["files"]) for g in ref) and ncase >= 38
    print("%d cases, the closest decision at %.3g bars" % (ncase, least))
