"""Model-based feature compensation, the parts that need no GPU: the three C ABI symbols and their argument checks, the host
arithmetic of JFAAcc::getUX / getSpeakerModel against numpy, and source checks of feat_comp.hip."""
import ctypes as ct
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lia_ral_amd", "csrc")


def test_symbols_are_declared_exported_and_refuse_a_null_context():
    from lia_ral_amd import capi
    lib = capi.lib
    hdr = open(os.path.join(ROOT, "include", "gmmiv.h")).read()
    for name in ("gmmiv_feat_compensate", "gmmiv_feat_map", "gmmiv_scatter_runs"):
        assert hasattr(lib, name) and re.search(r"\bint %s\(gmmiv_ctx \*ctx" % name, hdr), name
    null, i64 = ct.c_void_p(0), ct.c_int64
    buf = (ct.c_double * 8)()
    rc = lib.gmmiv_feat_compensate(null, null, buf, 1, i64(1), i64(4), buf, buf, 1, i64(4))
    assert rc == -1 and b"feat_compensate" in lib.gmmiv_last_error()              # GMMIV_ERR_ARG, with a message
    rc = lib.gmmiv_feat_map(null, null, buf, buf, buf, buf, buf, 1, i64(1), i64(4), buf, 1, i64(4), null)
    assert rc == -1 and b"feat_map" in lib.gmmiv_last_error()
    rc = lib.gmmiv_scatter_runs(null, buf, 1, i64(4), 4, null, i64(0), buf)
    assert rc == -1 and b"scatter_runs" in lib.gmmiv_last_error()
    for name in ("feat_compensate", "feat_map"):                                    # methods of the Python binding
        assert hasattr(capi.Gmm, name)
    assert hasattr(capi.Context, "scatter_runs")
    for row in ("gmmiv_feat_compensate         the frame is COPIED THROUGH", "gmmiv_feat_map                NOT screened"):
        assert row in hdr                                                           # the degenerate-input table names both


def test_dtype_errors_come_first_and_argument_checks_precede_any_enqueue():
    """a wrong dtype is refused whatever else is passed; in the source, feat_check (strides, T, the overlap rule) runs before the
    first workspace request, copy or launch of both entry points (the overlap rule itself needs a model: tests/test_gpu_feat_comp.py)"""
    from lia_ral_amd import capi
    lib = capi.lib
    null, i64 = ct.c_void_p(0), ct.c_int64
    buf = (ct.c_double * 8)()
    for xdt, odt in ((2, 1), (1, -1), (7, 7)):
        assert lib.gmmiv_feat_compensate(null, null, buf, xdt, i64(1), i64(4), buf, buf, odt, i64(4)) == -1
        assert b"must be GMMIV_F32 or GMMIV_F64" in lib.gmmiv_last_error()
        assert lib.gmmiv_feat_map(null, null, buf, buf, buf, buf, buf, xdt, i64(1), i64(4), buf, odt, i64(4), null) == -1
        assert b"must be GMMIV_F32 or GMMIV_F64" in lib.gmmiv_last_error()
    assert lib.gmmiv_scatter_runs(null, buf, 5, i64(4), 4, null, i64(0), buf) == -1
    src = open(os.path.join(CSRC, "capi_feat.hip")).read()
    for fn in ("gmmiv_feat_compensate", "gmmiv_feat_map"):
        body = src[src.index("int %s(" % fn):]
        body = body[:body.index("\n}\n")]
        first_work = min(body.index(tok) for tok in ("xv.init(", "c->scratch(", "o.init(", ".init(c, WS_") if tok in body)
        assert 0 < body.index("feat_check(") < first_work and 0 < body.index("feat_check_dtype(") < body.index("check_model(")
    chk = src[src.index("static int feat_check("):]
    chk = chk[:chk.index("\n}\n")]
    assert "x == out && xdt == odt && ldx == ldo" in chk and "GMMIV_ERR_ARG" in chk and "hip" not in chk


def test_session_model_host_arithmetic_matches_numpy():
    """getUX (ux = U^T x_h, the `+=` overload normalizeFeatures calls) and getSpeakerModel (m + V y + D z + U x) of the host layer"""
    from lia_ral_amd import host_capi
    rng = np.random.default_rng(5)
    C, D, RV, RC = 7, 5, 3, 4
    SV = C * D
    m, V, U, Dm = rng.normal(size=SV), rng.normal(size=(RV, SV)), rng.normal(size=(RC, SV)), rng.normal(size=SV)
    y, x, z = rng.normal(size=RV), rng.normal(size=RC), rng.normal(size=SV)
    ux, sp = host_capi.jfa_session_model_host(m, V, y, Dm, z, U, x)
    ux_ref = np.zeros(SV)
    for j in range(RC):                                                            # the reference's order: j inside, `+=`
        ux_ref += U[j] * x[j]
    assert np.array_equal(ux, ux_ref)
    assert np.allclose(ux, x @ U, rtol=0, atol=1e-14 * np.abs(U).sum(0).max())
    vy = np.zeros(SV)
    for j in range(RV):
        vy += V[j] * y[j]
    assert np.array_equal(sp, (m + vy + Dm * z) + ux_ref)
    assert np.allclose(sp, m + y @ V + Dm * z + x @ U, rtol=1e-13, atol=1e-13)
    # one eigenchannel, one eigenvoice, zero factors
    ux1, sp1 = host_capi.jfa_session_model_host(m, V[:1], np.zeros(1), Dm, np.zeros(SV), U[:1], np.zeros(1))
    assert np.array_equal(ux1, np.zeros(SV)) and np.array_equal(sp1, m)


def test_new_kernels_have_no_floating_point_atomics_and_no_split_of_the_gaussian_sum():
    src = open(os.path.join(CSRC, "feat_comp.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"atomic|unsafeAtomic|__hip_atomic", code)                 # no atomics of any kind in the file
    assert "#pragma clang fp contract(off)" in code                                 # the map expression: separately rounded operations
    k = code[code.index("void k_feat_comp("):code.index("static int launch_feat_comp")]
    assert "for (int ct = 0; ct < nct; ++ct)" in k and "blockIdx.y" not in k        # one wave walks every Gaussian tile, in order
    assert "__syncthreads" not in k and "__shared__ double tile[4][FB][16 * 17]" in k
    assert "hipFuncSetAttribute" not in code                                        # static LDS below the default limit (lds_attr.h)
