"""NormFeat's default mode and the online mode of NormFeatWindowMode, the parts that need no GPU: the four C ABI symbols, the order of
their argument checks (nothing is enqueued before they pass), the validation of a host run table, and source checks of feat_norm.hip."""
import ctypes as ct
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lia_ral_amd", "csrc")
NAMES = ("gmmiv_frame_moments_groups", "gmmiv_frame_moments_stats", "gmmiv_feat_norm_apply", "gmmiv_feat_norm_online")
null, i64 = ct.c_void_p(0), ct.c_int64


def _calls(lib, buf, runs, fb, xdt=1, odt=1, ngroups=2):
    """the four entry points with a NULL context and otherwise valid host arguments -> {name: status}"""
    return {
        "frame_moments_groups": lib.gmmiv_frame_moments_groups(null, buf, xdt, i64(4), 4, runs, i64(2), i64(ngroups), buf),
        "frame_moments_stats": lib.gmmiv_frame_moments_stats(null, i64(ngroups), 4, buf, buf, buf),
        "feat_norm_apply": lib.gmmiv_feat_norm_apply(null, buf, xdt, i64(4), 4, runs, i64(2), i64(ngroups), buf, buf, buf, odt, i64(4)),
        "feat_norm_online": lib.gmmiv_feat_norm_online(null, buf, xdt, i64(4), 4, fb, i64(2), i64(300), i64(0), buf, odt, i64(4)),
    }


def test_symbols_are_declared_exported_and_refuse_a_null_context():
    from lia_ral_amd import capi, host_capi
    lib = capi.lib
    hdr = open(os.path.join(ROOT, "include", "gmmiv.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and re.search(r"\bint %s\(gmmiv_ctx \*ctx" % name, hdr), name
    buf = (ct.c_double * 64)()
    runs = (ct.c_int64 * 6)(0, 2, 0, 2, 2, 1)
    fb = (ct.c_int64 * 3)(0, 2, 4)
    for who in ("frame_moments_groups", "frame_moments_stats", "feat_norm_apply", "feat_norm_online"):
        rc = _calls(lib, buf, runs, fb)[who]                                        # (the message is the last call's: one at a time)
        assert rc == -1, who                                                        # GMMIV_ERR_ARG
    for who, fn in (("frame_moments_groups", lambda: lib.gmmiv_frame_moments_groups(null, buf, 1, i64(4), 4, runs, i64(2), i64(2), buf)),
                    ("frame_moments_stats", lambda: lib.gmmiv_frame_moments_stats(null, i64(2), 4, buf, buf, buf)),
                    ("feat_norm_apply", lambda: lib.gmmiv_feat_norm_apply(null, buf, 1, i64(4), 4, runs, i64(2), i64(2), buf, buf, buf, 1, i64(4))),
                    ("feat_norm_online", lambda: lib.gmmiv_feat_norm_online(null, buf, 1, i64(4), 4, fb, i64(2), i64(300), i64(0), buf, 1, i64(4)))):
        assert fn() == -1
        msg = lib.gmmiv_last_error()
        assert who.encode() in msg and b"NULL context" in msg, msg
    for name in ("frame_moments_groups", "frame_moments_stats", "feat_norm_apply", "feat_norm_online"):
        assert hasattr(capi.Context, name)                                          # methods of the Python binding
    for name in ("norm_feat", "norm_feat_online", "norm_feat_files"):
        assert hasattr(host_capi, name) and hasattr(host_capi.lib, "liagpu_" + name)
    for row in ("gmmiv_frame_moments_groups    NOT screened", "gmmiv_feat_norm_apply         NOT screened", "gmmiv_feat_norm_online        NOT screened"):
        assert row in hdr                                                           # the degenerate-input table names all three
    assert "every file starts from the caller's W" in hdr                           # the quirk that is not kept is stated


def test_dtype_errors_come_first_and_argument_checks_precede_any_enqueue():
    """a wrong dtype is refused whatever else is passed; in the source the dtype check, the table validation and the overlap rule of
    both frame-rewriting entry points run before the first workspace request, copy or launch"""
    from lia_ral_amd import capi
    lib = capi.lib
    buf = (ct.c_double * 64)()
    runs = (ct.c_int64 * 6)(0, 2, 0, 2, 2, 1)
    fb = (ct.c_int64 * 3)(0, 2, 4)
    for xdt, odt in ((2, 1), (1, -1), (7, 7)):
        for who in ("feat_norm_apply", "feat_norm_online"):
            assert _calls(lib, buf, runs, fb, xdt, odt)[who] == -1
        assert lib.gmmiv_feat_norm_apply(null, buf, xdt, i64(4), 4, runs, i64(2), i64(2), buf, buf, buf, odt, i64(4)) == -1
        assert b"feat_norm_apply: x_dtype / out_dtype must be GMMIV_F32 or GMMIV_F64" in lib.gmmiv_last_error()
        assert lib.gmmiv_feat_norm_online(null, buf, xdt, i64(4), 4, fb, i64(2), i64(300), i64(0), buf, odt, i64(4)) == -1
        assert b"feat_norm_online: x_dtype / out_dtype must be GMMIV_F32 or GMMIV_F64" in lib.gmmiv_last_error()
    assert lib.gmmiv_frame_moments_groups(null, buf, 5, i64(4), 4, runs, i64(2), i64(2), buf) == -1
    assert b"x_dtype must be" in lib.gmmiv_last_error()
    # scalar arguments: a stride below D, window < 1, a negative look-ahead
    assert lib.gmmiv_feat_norm_apply(null, buf, 1, i64(3), 4, runs, i64(2), i64(2), buf, buf, buf, 1, i64(4)) == -1 and b"bad argument" in lib.gmmiv_last_error()
    assert lib.gmmiv_feat_norm_online(null, buf, 1, i64(4), 4, fb, i64(2), i64(0), i64(0), buf, 1, i64(4)) == -1 and b"bad argument" in lib.gmmiv_last_error()
    assert lib.gmmiv_feat_norm_online(null, buf, 1, i64(4), 4, fb, i64(2), i64(300), i64(-1), buf, 1, i64(4)) == -1 and b"bad argument" in lib.gmmiv_last_error()
    src = open(os.path.join(CSRC, "capi_feat.hip")).read()
    for fn, table in (("gmmiv_feat_norm_apply", "norm_check_runs("), ("gmmiv_feat_norm_online", "file_begin[f + 1] < file_begin[f]")):
        body = src[src.index("int %s(" % fn):]
        body = body[:body.index("\n}\n")]
        first_work = min(body.index(tok) for tok in ("GBIND(", "c->scratch(", ".init(c, WS_", "gmmk_", "hipMem") if tok in body)
        assert 0 < body.index("feat_check_dtype(") < body.index(table) < body.index("norm_check_overlap(") < first_work
        assert body.index("x == out && (dt != odt || ldx != ldo)") < first_work
    body = src[src.index("int gmmiv_frame_moments_groups("):]
    body = body[:body.index("\n}\n")]
    assert 0 < body.index("norm_check_runs(") < min(body.index(tok) for tok in ("GBIND(", "c->scratch(", ".init(c, WS_", "gmmk_"))
    chk = src[src.index("static int norm_check_overlap("):]
    chk = chk[:chk.index("\n}\n")]
    assert "x == out && xdt == odt && ldx == ldo" in chk and "GMMIV_ERR_ARG" in chk and "hip" not in chk


def test_a_host_table_that_breaks_the_group_rule_is_refused():
    """group ids non-decreasing and inside [0, ngroups), lengths and first frames non-negative -- checked on a host table before the
    context is even looked at; a file table must be non-decreasing"""
    from lia_ral_amd import capi
    lib = capi.lib
    buf = (ct.c_double * 64)()
    ok = (ct.c_int64 * 9)(0, 2, 0, 2, 1, 0, 3, 1, 2)                                # groups 0, 0, 2: group 1 is empty
    for bad, what in (((ct.c_int64 * 6)(0, 2, 1, 2, 2, 0), b"non-decreasing"),       # a decreasing group id
                      ((ct.c_int64 * 6)(0, 2, 0, 2, 2, 3), b"outside [0, 3)"),       # a group id >= ngroups
                      ((ct.c_int64 * 6)(0, 2, -1, 2, 2, 0), b"non-decreasing"),      # a negative group id
                      ((ct.c_int64 * 6)(0, -2, 0, 2, 2, 0), b"negative first frame or length"),
                      ((ct.c_int64 * 6)(-1, 2, 0, 2, 2, 0), b"negative first frame or length")):
        assert lib.gmmiv_frame_moments_groups(null, buf, 1, i64(4), 4, bad, i64(2), i64(3), buf) == -1
        assert b"frame_moments_groups" in lib.gmmiv_last_error() and what in lib.gmmiv_last_error(), lib.gmmiv_last_error()
        assert lib.gmmiv_feat_norm_apply(null, buf, 1, i64(4), 4, bad, i64(2), i64(3), buf, buf, buf, 1, i64(4)) == -1
        assert b"feat_norm_apply" in lib.gmmiv_last_error() and what in lib.gmmiv_last_error()
    assert lib.gmmiv_frame_moments_groups(null, buf, 1, i64(4), 4, ok, i64(3), i64(3), buf) == -1
    assert b"NULL context" in lib.gmmiv_last_error()                                # the valid table gets as far as the context check
    fb = (ct.c_int64 * 3)(0, 5, 4)
    assert lib.gmmiv_feat_norm_online(null, buf, 1, i64(4), 4, fb, i64(2), i64(300), i64(0), buf, 1, i64(4)) == -1
    assert b"non-decreasing" in lib.gmmiv_last_error()


def test_feat_norm_kernels_have_no_atomics_no_lds_attribute_and_separately_rounded_expressions():
    src = open(os.path.join(CSRC, "feat_norm.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"atomic|unsafeAtomic|__hip_atomic", code)                 # no atomics of any kind in the file
    assert "hipFuncSetAttribute" not in code and "extern __shared__" not in code    # static LDS below the default limit (lds_attr.h)
    for kern in ("void k_moments_stats(", "void k_feat_norm_apply(", "void k_moments_groups(", "void k_online_replay(", "void k_online_sums(",
                 "void k_online_carry("):
        body = code[code.index(kern):]
        body = body[:body.index("\n}\n")]
        assert "#pragma clang fp contract(off)" in body, kern                      # a product and a sum stay two roundings
    stats = code[code.index("void k_moments_stats("):]
    stats = stats[:stats.index("\n}\n")]
    assert "/ n" in stats and "m * m" in stats and "__builtin_sqrt(q - mm)" in stats
    apply_ = code[code.index("void k_feat_norm_apply("):]
    apply_ = apply_[:apply_.index("\n}\n")]
    assert "- m[k]" in apply_ and "d / s[k]" in apply_ and "fma" not in apply_      # one subtraction, one true division
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "feat_norm.hip" in mk
