"""The batched EnergyDetector's C ABI without a GPU: the symbols, and the argument checks that come before anything is enqueued."""
import ctypes as ct
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def _lib():
    from lia_ral_amd import capi
    return capi


def test_symbols_are_declared_and_exported():
    capi = _lib()
    hdr = open(os.path.join(ROOT, "include", "gmmiv.h")).read()
    for name in ("gmmiv_energy_train", "gmmiv_energy_select", "gmmiv_energy_stage_frames"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(capi.lib, name)
    for name, v in (("GMMIV_ENERGY_EMPTY", capi.ENERGY_EMPTY), ("GMMIV_ENERGY_NONFINITE", capi.ENERGY_NONFINITE), ("GMMIV_ENERGY_FLOORED", capi.ENERGY_FLOORED),
                    ("GMMIV_ENERGY_CEILED", capi.ENERGY_CEILED), ("GMMIV_ENERGY_MAX_C", capi.ENERGY_MAX_C)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr), name
    table = hdr[hdr.index("DEGENERATE INPUTS: what every"):hdr.index("gmmiv_count_unusable_frames: the counting pass")]
    assert "gmmiv_energy_train" in table and "gmmiv_energy_select" in table
    from lia_ral_amd import host_capi
    for name in ("liagpu_energy_detector_batch", "liagpu_energy_detector_files"):
        assert getattr(host_capi.lib, name)
    assert "energy_det.hip" in open(os.path.join(ROOT, "lia_ral_amd", "csrc", "Makefile")).read()


def test_stage_boundary_query():
    capi = _lib()
    b32, b64 = capi.energy_stage_frames(capi.F32), capi.energy_stage_frames(capi.F64)
    assert b32 == 2 * b64 > 0 and b64 * 8 <= 160 * 1024       # one staging budget in bytes, inside the CU's LDS
    assert capi.energy_stage_frames(77) == 0


def _train(capi, ctx, runs, nfiles, C=3, x=1):
    r = np.ascontiguousarray(runs, np.int64).reshape(-1, 3)
    model, th, st = np.zeros(max(1, nfiles) * 3 * 8), np.zeros(max(1, nfiles)), np.zeros(max(1, nfiles), np.int32)
    return capi.lib.gmmiv_energy_train(ctx, ct.c_void_p(x), capi.F32, ct.c_int64(1), r.ctypes.data_as(ct.c_void_p), ct.c_int64(len(r)), ct.c_int64(nfiles), C, 10,
                                       ct.c_double(0.5), ct.c_double(10.0), ct.c_double(0.0), model.ctypes.data_as(ct.c_void_p), th.ctypes.data_as(ct.c_void_p),
                                       st.ctypes.data_as(ct.c_void_p))


def _select(capi, ctx, runs, nfiles):
    r = np.ascontiguousarray(runs, np.int64).reshape(-1, 3)
    th, cnt = np.zeros(max(1, nfiles)), np.zeros(max(1, nfiles), np.int64)
    return capi.lib.gmmiv_energy_select(ctx, ct.c_void_p(1), capi.F32, ct.c_int64(1), r.ctypes.data_as(ct.c_void_p), ct.c_int64(len(r)), ct.c_int64(nfiles),
                                        th.ctypes.data_as(ct.c_void_p), None, cnt.ctypes.data_as(ct.c_void_p), None, None, None)


def test_a_null_context_is_refused():
    capi = _lib()
    good = [(0, 5, 0), (9, 3, 1)]
    assert _train(capi, None, good, 2) == ERR_ARG and b"NULL context" in capi.lib.gmmiv_last_error()
    assert _select(capi, None, good, 2) == ERR_ARG and b"NULL context" in capi.lib.gmmiv_last_error()


def test_broken_host_tables_and_gaussian_counts_are_refused_before_the_context_is_touched():
    """the checks run before the context is looked at: a NULL context would be the NEXT error, so ERR_ARG with another message proves the order"""
    capi = _lib()
    for bad in ([(0, 5, 1), (9, 3, 0)],            # file ids decrease
                [(0, 5, 0), (9, 3, 2)],            # file id outside [0, nfiles)
                [(0, -1, 0)],                      # negative length
                [(-4, 2, 0)]):                     # negative first frame
        for call in (_train, _select):
            assert call(capi, None, bad, 2) == ERR_ARG
            assert b"NULL context" not in capi.lib.gmmiv_last_error(), bad
    for C in (0, 9, -1):
        assert _train(capi, None, [(0, 5, 0)], 1, C=C) == ERR_ARG and b"outside 1 .. 8" in capi.lib.gmmiv_last_error()
