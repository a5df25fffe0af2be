"""gmmiv_topgauss_compute (k_topgauss_select behind the three top-C paths) and gmmiv_llk_use_top / _multi on the stored selection it
leaves -- the first count[t] entries of a row, -1 behind them: what TopGauss::compute writes and TopGauss::get evaluates -- judged
per frame against the long double restatement and the derived bars of tests/topgauss_ref.py, through capi directly.

compute      every case of topgauss_ref.CASES, float32 and float64 frames, COMPLETE and PARTIAL, the masses 0.5 / 0.9 / 0.999 and the
             fixed counts 1 and cap, on the fused, the stored-likelihood and the direct top-C path (and the 4-wave shapes and
             short_calls 0 on one case): count, idx, snsw, snsl, llk per frame, n_capped, at most 1 % ambiguous frames.
device form  every output a device tensor between guard bands (idx and count in int32 buffers of their own), the frames as columns
             of a wider device matrix: the bits of the host-array call, guard bands untouched.
get          llk_use_top(ctop = cap, idx, log(snsl)) of three clients on exactly the arrays compute returned, against a long
             double log-sum over the first count[t] entries (+ snsl[t], COMPLETE) of those same doubles; both lane layouts; the rows
             of llk_use_top_multi have the bits of the single calls; on the UBM itself get gives back compute's llk.
degenerate   a NaN frame and a far frame follow the zero-likelihood rule, their neighbours keep their bits.

With TOPGAUSS_ERRORS_JSON set to a path the largest ratio per (case, path, entry, kind) is written there
(profiles/r24/topgauss_errors.json)."""
import ctypes as ct
import json
import os
import time

import numpy as np
import pytest

import gmm_ref as gr
import topgauss_ref as tg
from elementwise_judge import GUARD, Guarded, Judge, options, path_name

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300), pytest.mark.skipif(not tg.HAVE_LONGDOUBLE, reason=tg.SKIP_MESSAGE)]

LD = gr.LD
U = gr.U
RATIOS = {}
JUDGED = [0]
PATHS = ({}, {"topc_fused": 0}, {"topc_fused": 0, "topc_z": 0})
MORE_PATHS_CASE = (65, 33, 64, 0.3, 64)
MORE_PATHS = ({"wg_waves": 4}, {"short_calls": 0})
MODES = (True, False)
CLIENT_SHIFTS = (5, 11, 12)
GET_CASES = ((17, 2, 129, 2.0, 16), (65, 33, 64, 0.3, 64), (96, 81, 70, 0.3, 40))
BATCHED_CASE = (17, 2, 129, 2.0, 16)      # cap <= 16 and an even D: gmmiv_llk_use_top_multi takes its one-launch kernel
I32_SENTINEL = -77777


class CountingJudge(Judge):
    def __call__(self, entry, kind, ratios):
        JUDGED[0] += int(np.asarray(ratios).size)
        super().__call__(entry, kind, ratios)


def mode_name(complete):
    return "COMPLETE" if complete else "PARTIAL"


def label(case, dtype, extra=""):
    return "%s %s%s" % (tg.case_name(case), gr.dtype_name(dtype), extra)


@pytest.fixture(scope="module")
def ctx():
    from lia_ral_amd import capi
    t0 = time.time()
    c = capi.Context(0)
    yield c
    c.close()
    path = os.environ.get("TOPGAUSS_ERRORS_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"bound": "tests/topgauss_ref.py", "max_ratio": float("%.4g" % max(RATIOS.values())), "judged_elements": JUDGED[0],
                       "module_seconds": round(time.time() - t0, 1),
                       "entries": {" | ".join(k): float("%.4g" % v) for k, v in sorted(RATIOS.items())}}, f, indent=1)


def run_compute(ctx, j, g, case, dtype, paths):
    ref = tg.reference(case, gr.dtype_name(dtype))
    x = tg.frames(case, dtype)
    w = gr.model(case[:4])[0]
    cap = case[4]
    for complete in MODES:
        for top_gauss in tg.settings(case):
            e = tg.Expected(ref, cap, top_gauss, complete)
            for opts in paths:
                j.path = "%s | %s top_gauss %g" % (path_name(opts), mode_name(complete), top_gauss)
                with options(ctx, opts):
                    got = g.topgauss_compute(x, cap, top_gauss, complete, tg.LO, tg.HI)
                tg.judge(j, e, got, w)


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
@pytest.mark.parametrize("case", tg.CASES, ids=tg.case_name)
def test_compute_per_frame_on_every_top_c_path(ctx, case, dtype):
    j = CountingJudge(label(case, dtype), "", RATIOS)
    g = ctx.gmm(*gr.model(case[:4]))
    run_compute(ctx, j, g, case, dtype, PATHS + (MORE_PATHS if case == MORE_PATHS_CASE else ()))
    g.close()
    j.finish()


class GuardedI32:
    """an int32 device result between two guard bands (elementwise_judge.Guarded holds doubles)"""

    def __init__(self, shape):
        import torch
        self.n, self.shape = int(np.prod(shape)), tuple(shape)
        self.buf = torch.full((self.n + 2 * GUARD,), I32_SENTINEL, dtype=torch.int32, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.n].view(*shape)
        torch.cuda.synchronize()

    def read(self, j, entry):
        import torch
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        if not (np.all(h[:GUARD] == I32_SENTINEL) and np.all(h[GUARD + self.n:] == I32_SENTINEL)):
            j.note(entry, "a guard band around the device result was written")
        out = h[GUARD:GUARD + self.n].reshape(self.shape).copy()
        if np.any(out == I32_SENTINEL):
            j.note(entry, "%d elements of the result were never written" % int((out == I32_SENTINEL).sum()))
        return out


@pytest.mark.parametrize("complete", MODES, ids=mode_name)
def test_device_outputs_between_guard_bands_have_the_bits_of_the_host_call(ctx, complete):
    import torch
    from lia_ral_amd import capi
    case, dtype, mass = (65, 33, 64, 0.3, 64), np.float32, 0.9
    C, D, T, _, cap = case
    x = tg.frames(case, dtype)
    g = ctx.gmm(*gr.model(case[:4]))
    host = g.topgauss_compute(x, cap, mass, complete, tg.LO, tg.HI)
    j = CountingJudge(label(case, dtype, " ldx=D+5"), "device outputs | %s top_gauss %g" % (mode_name(complete), mass), RATIOS)
    wide = torch.full((T, D + 5), 1e30, dtype=torch.float32, device="cuda")       # the filler must never be read as a feature
    wide[:, :D] = torch.from_numpy(x.copy()).cuda()                               # (the shared frames are read-only)
    idx, cnt = GuardedI32((T, cap)), GuardedI32((T,))
    snsw, snsl, llk = Guarded((T,), fill=None), Guarded((T,), fill=None), Guarded((T,), fill=None)
    n_capped = ct.c_int64(-1)
    torch.cuda.synchronize()
    capi._chk(capi.lib.gmmiv_topgauss_compute(ctx._h, g._h, ct.c_void_p(wide.data_ptr()), capi.F32, ct.c_int64(T), ct.c_int64(D + 5), cap,
                                              ct.c_double(mass), capi.TOP_COMPLETE if complete else capi.TOP_PARTIAL, ct.c_double(tg.LO),
                                              ct.c_double(tg.HI), ct.c_void_p(idx.view.data_ptr()), ct.c_void_p(cnt.view.data_ptr()),
                                              ct.c_void_p(snsw.view.data_ptr()), ct.c_void_p(snsl.view.data_ptr()),
                                              ct.c_void_p(llk.view.data_ptr()), ct.byref(n_capped)))
    ctx.sync()
    dev = dict(idx=idx.read(j, "idx"), count=cnt.read(j, "count"), snsw=snsw.read(j, "snsw"), snsl=snsl.read(j, "snsl"),
               llk=llk.read(j, "llk"), n_capped=int(n_capped.value))
    for k in ("idx", "count", "snsw", "snsl", "llk"):
        j.same_bits(k, dev[k], host[k], "the host-array call")
    if dev["n_capped"] != host["n_capped"]:
        j.note("n_capped", "%d on the device form, %d on the host form" % (dev["n_capped"], host["n_capped"]))
    tg.judge(j, tg.Expected(tg.reference(case, "float32"), cap, mass, complete), dev, gr.model(case[:4])[0])
    g.close()
    j.finish()


def get_reference(cref, got, complete):
    """TopGauss::get on exactly the arrays of one compute call: the clamped long double log-sum over the first count[t] listed
    Gaussians of the client (+ snsl[t], COMPLETE) and its bar (gmm_ref.use_top with a count; the remainder is the caller's double)"""
    idx, count = got["idx"].astype(np.int64), got["count"].astype(np.int64)
    want, bar = gr.use_top(cref, idx, np.log(got["snsl"]).astype(LD), None, None, complete, count=count)
    return gr.clamp(want, tg.LO, tg.HI, bar)


@pytest.mark.parametrize("complete", MODES, ids=mode_name)
@pytest.mark.parametrize("case", GET_CASES, ids=tg.case_name)
def test_get_on_the_stored_selection_of_compute(ctx, case, complete):
    from lia_ral_amd import capi
    dtype, mass = np.float32, 0.9
    cap = case[4]
    x = tg.frames(case, dtype)
    g = ctx.gmm(*gr.model(case[:4]))
    got = g.topgauss_compute(x, cap, mass, complete, tg.LO, tg.HI)
    assert (got["count"] == cap).any() and (got["count"] == 1).any(), "a frame with count == cap and one with count == 1 are needed"
    assert (got["idx"] == -1).any()
    nontop = np.log(got["snsl"])
    clients = [ctx.gmm(*gr.model(case[:4], s)) for s in CLIENT_SHIFTS]
    j = CountingJudge(label(case, dtype), "", RATIOS)
    for lanes in (4, 1):
        opts = {} if lanes == 4 else {"topc_use_lanes": 1}
        with options(ctx, opts):
            single = []
            for s, cl in zip(CLIENT_SHIFTS, clients):
                j.path = "%s | %s get client %d" % (path_name(opts), mode_name(complete), s)
                out = cl.llk_use_top(x, got["idx"], nontop, complete, tg.LO, tg.HI)
                want, bar = get_reference(tg.reference(case, "float32", s), got, complete)
                j("use_top llk", "frames", gr.ratio(out.astype(LD) - want, bar))
                single.append(out)
            multi = capi.Gmm.llk_use_top_multi(clients, x, got["idx"], nontop, complete, tg.LO, tg.HI)
            j.path = "%s | %s get" % (path_name(opts), mode_name(complete))
            for i, s in enumerate(CLIENT_SHIFTS):
                j.same_bits("use_top_multi row %d" % i, multi[i], single[i], "the single call")
    if case == BATCHED_CASE:      # the conditions of the one-launch kernel (gmmiv.h): it is the one that saw the -1 tail above
        assert cap <= 16 and case[1] % 2 == 0
    if complete:                  # on the UBM itself get gives back compute's llk, frame by frame, within the two bars
        j.path = "defaults | COMPLETE get on the UBM"
        ref = tg.reference(case, "float32")
        out = g.llk_use_top(x, got["idx"], nontop, True, tg.LO, tg.HI)
        want, bar = get_reference(ref, got, True)
        j("use_top llk", "frames", gr.ratio(out.astype(LD) - want, bar))
        e = tg.Expected(ref, cap, mass, True)
        j("get = compute llk", "frames", gr.ratio(out.astype(LD) - got["llk"].astype(LD), bar + e.B))
    for cl in clients:
        cl.close()
    g.close()
    j.finish()


DEGENERATE_CASE = (65, 33, 64, 0.3, 64)
NAN_AT, FAR_AT = 10, 20


@pytest.mark.parametrize("dtype", gr.DTYPES, ids=gr.dtype_name)
def test_a_nan_frame_and_a_far_frame_follow_the_zero_likelihood_rule(ctx, dtype):
    case = DEGENERATE_CASE
    C, D, T, _, cap = case
    clean = tg.frames(case, dtype)
    x = clean.copy()
    x[NAN_AT, 7] = np.nan
    x[FAR_AT, :] = 3e17                  # finite and inside the screening bound: every logit is about -1e36
    w, mean, iv = gr.model(case[:4])
    ref = gr.Reference(w, mean, iv, x)
    assert ref.dead()[[NAN_AT, FAR_AT]].all() and ref.dead().sum() == 2
    keep = np.setdiff1d(np.arange(T), [NAN_AT, FAR_AT])
    g = ctx.gmm(w, mean, iv)
    j = CountingJudge(label(case, dtype, " + NaN, far"), "", RATIOS)
    for complete in MODES:
        for top_gauss in (0.9, 1.0, float(cap)):
            e = tg.Expected(ref, cap, top_gauss, complete)
            for opts in PATHS:
                j.path = "%s | %s top_gauss %g" % (path_name(opts), mode_name(complete), top_gauss)
                with options(ctx, opts):
                    got = g.topgauss_compute(x, cap, top_gauss, complete, tg.LO, tg.HI)
                    base = g.topgauss_compute(clean, cap, top_gauss, complete, tg.LO, tg.HI)
                tg.judge(j, e, got, w)
                for t in (NAN_AT, FAR_AT):
                    n = int(got["count"][t])
                    if top_gauss < 1 and n != cap:
                        j.note("count", "zero-likelihood frame %d has count %d under a mass threshold, not cap" % (t, n))
                    if got["llk"][t] != tg.LO or got["idx"][t, :n].tolist() != list(range(n)):
                        j.note("idx", "zero-likelihood frame %d: llk %r, idx %r" % (t, got["llk"][t], got["idx"][t, :n].tolist()))
                    if top_gauss < 1 and abs(got["snsl"][t] - np.exp(tg.LO)) > 8 * U * np.exp(tg.LO):
                        j.note("snsl", "zero-likelihood frame %d: snsl %r, not exp(lo)" % (t, got["snsl"][t]))
                for k in ("idx", "count", "snsw", "snsl", "llk"):
                    j.same_bits(k + " of the neighbours", got[k][keep], base[k][keep], "the call on the clean frames")
    g.close()
    j.finish()
