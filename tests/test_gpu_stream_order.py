"""Every entry point reads and writes its device arrays in the order of the context's stream (include/gmmiv.h, "STREAM ORDER").

Per (judged case of ws_history.SMALL x step of its programme, plus the "handles" step of stream_order.py), on one context with a
private non-blocking stream: the step runs once plainly on device tensors -- the wanted bits, and every workspace allocated, so no
hipMalloc waits for the device during the second run -- and once LATE (stream_order.LateLib in place of capi.lib): before every call
the context is synchronised, every floating-point input tensor of the step (and every integer table for which the header makes 0 valid)
is overwritten with poison, and the true data comes back only on the context's stream, behind a spin kernel of SPIN_CYCLES.  A probe
on another non-blocking stream must still read the poison at the moment of the call (an assertion: without it the test proves nothing).

(a) reads     every array the late run returns has the bits of the plain run and the three counter deltas agree; an error return of
              the late run is a failure of this rule (a poisoned matrix is "not positive definite").
(b) writes    a snapshot of every output and in/out tensor, enqueued on the context's stream right behind a call, equals what the buffer
              holds once the context is synchronised (before the next call of the step, or at its end).  This catches only a writer
              that was never joined with the context's stream: a pass on (b) is much weaker evidence than a pass on (a).
(c) the table stream_order.ENQUEUE_ONLY transcribes what the header says of each function.  Where it says the call only enqueues with
              device pointers throughout, every such late call returned with the stream still busy (an event behind the restoring
              copies had not completed).  For the others nothing is asserted; the observed column is printed at the end of the module.

What the mode cannot see: a chain of two library calls inside one step (the context is synchronised before each call), mixed host /
device calls, several threads.  An in/out array is late for the first call that writes it and is left alone afterwards.

Measured on an MI355X on 2026-10-20, on the commit that adds this module (parent 9e362e0): SPIN_CYCLES = 2e7 is 8.3 ms of spin (a call
that waits for the stream returns after 8.26 .. 8.30 ms); the longest host-side part of a call that returned with the stream busy was
0.089 ms (gmmiv_score_twocov; 0.049 ms among the functions the header calls enqueue-only, gmmiv_em_accumulate), so the spin outlasts it
about ninety times.  The probe held on every one of the 578 late calls and rule (c) on every enqueue-only row.  One spin per call: no
parametrised test takes longer than 0.1 s after its context exists, the 159 of them 10 s together.  On the parent's library the three
"score rules" tests fail with "score_plda: FTJF + I is not positive definite" (gmmiv_score_plda copied FTJF on the NULL stream and read
the poison); "score trials" passes there too: gmmiv_score_plda_trials made the same copy, but behind the wait for its table upload.

Measured again on 2026-10-21 with the steps "normfeat window" and "turn detection" in the programme (parent 32904a4;
profiles/r29/stream_order.json): 602 late calls, 24 of them new -- gmmiv_feat_norm_window 6, gmmiv_turn_curve 3, gmmiv_turn_pick 6,
gmmiv_turn_segments 9, all with device arrays throughout and all back with the stream busy.  The longest host-side part of a busy
return among the new calls was 0.018 ms (gmmiv_turn_curve; 0.010 ms gmmiv_feat_norm_window, 0.008 ms gmmiv_turn_pick, 0.007 ms
gmmiv_turn_segments) next to the 0.089 ms above (0.100 ms in this run, gmmiv_score_twocov again): the 8.3 ms spin outlasts them four
hundred times.  The probe held on every call; 165 tests, the module 10.3 s, the six new cases 0.1 s each at most.
"""
import time

import pytest

import elementwise_judge as ej
import stream_order as so
import ws_history as wh

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

OBSERVED = {}                    # function -> [calls, with device arrays throughout, of those: returned busy, longest seconds on the host of a busy return]
FAILED = []
T0 = [None]
PARAMS = [(c["name"], s.name) for c in wh.SMALL for s in so.LATE_PROGRAMME if s.applies(c)]
LATE_STEPS = {s.name: s for s in so.LATE_PROGRAMME}


@pytest.fixture(scope="module", autouse=True)
def table():
    T0[0] = time.perf_counter()
    yield
    print("\n[stream_order] spin %d cycles; module %.1f s" % (so.SPIN_CYCLES, time.perf_counter() - T0[0]))
    print("[stream_order] %-36s %-9s %6s %10s %6s %9s" % ("function", "header", "calls", "throughout", "busy", "busy: ms"))
    for fn in sorted(OBSERVED):
        n, thr, busy, sec = OBSERVED[fn]
        print("[stream_order] %-36s %-9s %6d %10d %6d %9.3f" % (fn, so.ENQUEUE_ONLY.get(fn, ("handle",))[0], n, thr, busy, 1e3 * sec))
    if OBSERVED:
        print("[stream_order] longest host-side part of a call that returned with the stream busy: %.3f ms" % (1e3 * max(v[3] for v in OBSERVED.values())))


@pytest.mark.parametrize("case_name,step_name", PARAMS, ids=["%s-%s" % (c, s.replace(" ", "_")) for c, s in PARAMS])
def test_step_reads_and_writes_in_stream_order(case_name, step_name, monkeypatch):
    from lia_ral_amd import capi
    if FAILED:
        raise RuntimeError("not run: an earlier GPU call of this module failed: %r" % (FAILED[0],))
    case, step = wh.CASES[case_name], LATE_STEPS[step_name]
    j = ej.Judge(case_name, step_name, {})
    ctx = capi.Context(0)
    h = wh.Handles(ctx)
    try:
        plain = step.run(ctx, h, case, "device")
        rec = so.Recorder(so.TorchBackend(capi.lib, ctx))
        lib = so.LateLib(capi.lib, rec, ctx._h, step.name)
        late = None
        with monkeypatch.context() as m:
            m.setattr(wh, "RECORDER", rec)
            m.setattr(capi, "lib", lib)
            try:
                late = step.run(ctx, h, case, "device")
                lib.finish()
            except capi.GmmivError as e:
                if "error -2" in str(e):          # a HIP error is no data: nothing more of this module runs on the GPU
                    FAILED.append(e)
                    raise
                j.note("late run", "the call on late inputs failed (it read them before they were there): %s" % e)
        for r in lib.records:
            o = OBSERVED.setdefault(r["fn"], [0, 0, 0, 0.0])
            o[0] += 1
            o[1] += bool(r["throughout"])
            o[2] += bool(r["throughout"] and r["busy"])
            o[3] = max(o[3], r["seconds"] if r["busy"] else 0.0)
        print("\n[stream_order] %s | %s: %d late calls, %d tensors, longest host part %.3f ms" %
              (case_name, step_name, len(lib.records), len(rec.items), 1e3 * max([r["seconds"] for r in lib.records] or [0.0])))
        assert lib.records and any(r["late"] for r in lib.records), "no call of the step had a late input"
        # (a)
        if late is not None:
            if set(late) != set(plain):
                j.note("outputs", "the late run returned %s, the plain run %s" % (sorted(late), sorted(plain)))
            for out in sorted(set(late) & set(plain)):
                j.same_bits(out, late[out], plain[out], "the plain run")
        # (b) and the probe
        for text in lib.faults:
            j.note("late run", text)
        # (c)
        for r in lib.records:
            if so.ENQUEUE_ONLY.get(r["fn"], ("",))[0] == so.E and r["throughout"] and not r["busy"]:
                j.note(r["fn"], "the header says the call only enqueues with device pointers throughout; it returned with the stream idle "
                                "after %.3f ms on the host" % (1e3 * r["seconds"]))
        j.finish()
    except Exception as e:           # noqa: BLE001
        if isinstance(e, (capi.GmmivError, RuntimeError)) and not FAILED:      # a HIP error: nothing more of this module runs on the GPU
            FAILED.append(e)
        raise
    finally:
        if not FAILED:
            h.close()
            ctx.close()


def test_every_step_ran_late_and_reached_its_entry_points():
    """the late programme reached every judged function through the proxy (the CPU side holds the same from `reaches`)"""
    from test_cpu_judged_inventory import JUDGED
    if FAILED:
        raise RuntimeError("not run: an earlier GPU call of this module failed: %r" % (FAILED[0],))
    forwarded = {n for n in JUDGED if so.plain(n)}        # pure host: the proxy hands it on untouched and keeps no record of it
    assert forwarded == {"gmmiv_plan_norm_windows"}
    missing = sorted(set(JUDGED) - forwarded - set(OBSERVED))
    assert not missing, "judged functions that no late step called: %s" % missing
