"""Score normalisation, the parts that need no GPU: the two C ABI symbols and their argument checks, the NIST result-line reader
of the host layer, the refusal of lists that are not full cross products, and a source check of score_norm.hip."""
import ctypes as ct
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_refuse_a_null_context():
    from lia_ral_amd import capi
    lib = capi.lib
    for name in ("gmmiv_score_cohort_stats", "gmmiv_score_normalize", "gmmiv_ctx_workspace_bytes"):
        assert hasattr(lib, name), name
    null = ct.c_void_p(0)
    buf = (ct.c_double * 4)()
    rc = lib.gmmiv_score_cohort_stats(null, ct.c_int64(1), ct.c_int64(4), buf, ct.c_int64(4), 0, null, null, null, 0,
                                      ct.c_double(0.0), ct.c_double(0.0), buf, buf)
    assert rc == -1 and b"score_cohort_stats" in lib.gmmiv_last_error()          # GMMIV_ERR_ARG, with a message
    rc = lib.gmmiv_score_normalize(null, ct.c_int64(1), ct.c_int64(4), buf, 0, buf, buf, null, null, null)
    assert rc == -1 and b"score_normalize" in lib.gmmiv_last_error()
    assert capi.lib.gmmiv_ctx_workspace_bytes(null, -1) == 0
    assert (capi.NORM_Z, capi.NORM_T, capi.NORM_ZT, capi.NORM_TZ) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, "include", "gmmiv.h")).read()
    assert re.search(r"GMMIV_NORM_Z = 0, GMMIV_NORM_T = 1, GMMIV_NORM_ZT = 2, GMMIV_NORM_TZ = 3", hdr)
    assert "GMMIV_SCORE_NORM_SCRATCH_BYTES(ndist) ((size_t)512 * (size_t)(ndist) + (size_t)64)" in hdr
    assert capi.norm_scratch_bytes(2000) == 512 * 2000 + 64


def test_result_line_reader_round_trips_and_honours_field_positions():
    from lia_ral_amd import host_capi
    line, f = host_capi.result_line(1.5, "spk01", "seg_a", "F", threshold=0.0)
    assert line == "F spk01 1 seg_a 1.5"
    assert f == dict(name="spk01", seg="seg_a", gender="F", decision=1, llr=1.5)
    line, f = host_capi.result_line(-0.25, "spk02", "seg_b", "M", threshold=0.0, times=(0.5, 12.0), fields=(0, 1, 2, 3, 6))
    assert line == "M spk02 0 seg_b 0.5 12 -0.25"
    assert f == dict(name="spk02", seg="seg_b", gender="M", decision=0, llr=-0.25)
    # another layout: score first, then segment, model, gender
    _, f = host_capi.result_line(0.0, "x", "y", parse="-3.75e-2 segZ modelQ F 1", fields=(3, 2, 4, 1, 0))
    assert f == dict(name="modelQ", seg="segZ", gender="F", decision=1, llr=-0.0375)
    with pytest.raises(host_capi.HostError, match="no field 4"):
        host_capi.result_line(0.0, "x", "y", parse="M a 0 b")
    with pytest.raises(host_capi.HostError, match="not a score"):
        host_capi.result_line(0.0, "x", "y", parse="M a 0 b high")


def _write(path, lines):
    with open(path, "w") as f:
        f.write("".join(l + "\n" for l in lines))
    return str(path)


def test_compute_norm_files_refuses_lists_that_are_not_cross_products(tmp_path):
    """checked on the host before a device is opened: this runs on a machine without one"""
    from lia_ral_amd import host_capi
    models, segs, imps = ["m1", "m2", "m3"], ["s1", "s2"], ["i1", "i2", "i3", "i4"]
    test = ["M %s 0 %s %g" % (m, s, 0.1 * i) for i, (m, s) in enumerate((m, s) for m in models for s in segs)]
    zn = ["M %s 0 %s %g" % (m, s, 0.2 * i) for i, (m, s) in enumerate((m, s) for m in models for s in imps)]
    out = str(tmp_path / "out")
    t = _write(tmp_path / "test.nist", test)
    # one model lacks one impostor segment: a ragged cohort
    with pytest.raises(host_capi.HostError, match="not a full cross product"):
        host_capi.compute_norm_files(t, out, "znorm", znorm_nist_file=_write(tmp_path / "z1.nist", zn[:-1]))
    # a pair listed twice in place of another one
    with pytest.raises(host_capi.HostError, match="not a full cross product"):
        host_capi.compute_norm_files(t, out, "znorm", znorm_nist_file=_write(tmp_path / "z2.nist", zn[:-1] + [zn[0]]))
    # a cohort list about a model the test list does not have
    with pytest.raises(host_capi.HostError, match="not a full cross product"):
        host_capi.compute_norm_files(t, out, "znorm", znorm_nist_file=_write(tmp_path / "z3.nist", zn + ["M m9 0 i1 0.5"]))
    # the test list itself
    with pytest.raises(host_capi.HostError, match="not a full cross product"):
        host_capi.compute_norm_files(_write(tmp_path / "t2.nist", test[1:]), out, "znorm", znorm_nist_file=_write(tmp_path / "z4.nist", zn))
    with pytest.raises(host_capi.HostError, match="unknown normalization mode"):
        host_capi.compute_norm_files(t, out, "snorm", znorm_nist_file=_write(tmp_path / "z5.nist", zn))
    assert not os.path.exists(out + ".znorm")


def test_score_norm_source_has_no_floating_point_atomic():
    """determinism is structural: the only atomics are integer adds into the LDS histograms"""
    src = open(os.path.join(ROOT, "lia_ral_amd", "csrc", "score_norm.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "unsafeAtomicAdd" not in code and "atomicAdd_system" not in code and "__hip_atomic" not in code
    calls = re.findall(r"atomic\w*\s*\(([^;]*);", code)
    assert calls, "the radix select counts with LDS atomics"
    for c in calls:
        assert re.match(r"&hist\[[^\]]*\], 1u\)", c.strip()) or re.match(r"&s_nc\[[^\]]*\], 1\)", c.strip()), c
    assert re.search(r"unsigned \*hist = \(unsigned \*\)sbuf;", code)             # what they add to: 32-bit counters in LDS,
    assert re.search(r"__shared__ int s_nc\[", code)                               # and the lengths of the candidate lists
    assert "#pragma clang fp contract(off)" in src
