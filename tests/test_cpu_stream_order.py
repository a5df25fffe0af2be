"""What tests/test_gpu_stream_order.py relies on, checked without a GPU: which functions the proxy leaves alone, that the late programme
reaches every judged function, that the table of what the headers of include/ say has a row for each, that the tables of integer arguments name real steps and
parameters, the poison, and -- with a fake library and numpy arrays in place of tensors -- the order of the proxy's steps."""
import ctypes as ct
import re

import numpy as np

import stream_order as so
import test_cpu_judged_inventory as inv
import ws_history as wh
from test_cpu_ws_history import abi_functions


def test_the_proxy_leaves_alone_exactly_the_context_planner_and_communicator_functions():
    want = {n for n, r in inv.EXEMPT.items() if r in (inv._CTX, inv._PLAN, inv._COMM)}
    got = {n for n in abi_functions() if so.plain(n)}
    # one planner is judged, not exempt (it hands back doubles): pure host, so the proxy forwards it like the others
    judged_planners = got - want
    assert judged_planners == {"gmmiv_plan_norm_windows"} <= set(inv.JUDGED) and not want - got, (sorted(got - want), sorted(want - got))
    assert all(so.plain(n) for n in ("gmmiv_plan_norm_windows", "gmmiv_plan_turn_positions", "gmmiv_turn_tile_positions"))
    assert not any(re.search(r"gmmiv_(ctx|gmm|gmm_batch)\b", abi_functions()[n]) for n in judged_planners)
    for n in ("gmmiv_gmm_create", "gmmiv_gmm_set", "gmmiv_gmm_set_cov", "gmmiv_gmm_batch_load", "gmmiv_gmm_batch_load_cov"):
        assert not so.plain(n) and inv.EXEMPT[n] == inv._HANDLE


def test_every_judged_function_is_reached_by_a_late_step_and_has_a_row_of_the_header_table():
    abi = set(abi_functions())
    reached = {e for s in so.LATE_PROGRAMME for e in s.reaches}
    assert not set(inv.JUDGED) - reached, sorted(set(inv.JUDGED) - reached)
    assert {"gmmiv_gmm_set", "gmmiv_gmm_set_cov", "gmmiv_gmm_batch_load", "gmmiv_gmm_batch_load_cov"} <= set(so.HANDLES.reaches) <= abi
    assert so.LATE_PROGRAMME[:-1] == wh.PROGRAMME and so.HANDLES.forms == wh.FORMS and all(so.HANDLES.applies(c) for c in wh.SMALL)
    assert set(so.ENQUEUE_ONLY) <= abi, sorted(set(so.ENQUEUE_ONLY) - abi)
    assert not set(inv.JUDGED) - set(so.ENQUEUE_ONLY), sorted(set(inv.JUDGED) - set(so.ENQUEUE_ONLY))
    for name, (kind, sentence) in so.ENQUEUE_ONLY.items():
        assert kind in (so.E, so.W, so.S) and sentence, name
    # the sentences quoted for the enqueue-only rows are in the headers, word for word
    import os
    from conftest import ROOT
    from test_cpu_ws_history import HEADERS
    text = " ".join(" ".join(open(os.path.join(ROOT, "include", h)).read().replace(" * ", " ").split()) for h in HEADERS)
    for name, (kind, sentence) in so.ENQUEUE_ONLY.items():
        m = re.search(r"'(.*)'", sentence)                # from the first apostrophe to the last: the quotes hold "context's"
        if m:
            assert " ".join(m.group(1).split()) in text, (name, m.group(1))
            head = re.match(r"(gmmiv_\w+\.h): ", sentence)   # a row that names its header quotes that header
            if head:
                own = " ".join(open(os.path.join(ROOT, "include", head.group(1))).read().replace(" * ", " ").split())
                assert " ".join(m.group(1).split()) in own, (name, head.group(1))
        else:
            assert kind != so.E, "an enqueue-only row quotes its sentence: %s" % name


def test_the_integer_tables_name_real_steps_and_parameters():
    protos = so.prototypes()
    params = {p for ps in protos.values() for p, kind in ps if kind in ("read", "written")}
    steps = {s.name for s in so.LATE_PROGRAMME}
    for step, param, reason in so.NOT_LATE:
        assert step in steps and param in params and reason.strip(), (step, param)
        fns = [f for f in {s.name: s for s in so.LATE_PROGRAMME}[step].reaches if any(p == param for p, _ in protos[f])]
        assert fns, (step, param)
        assert all(re_int(abi_functions()[f], param) for f in fns), "NOT_LATE holds integer tables only: %s %s" % (step, param)
    for param, reason in so.ZERO_IS_VALID.items():
        assert param in params and reason.strip(), param
        assert all(re_int(text, param) for f, text in abi_functions().items() if any(p == param and k != "scalar" for p, k in protos[f])), param


def re_int(args, param):
    """whether the parameter of that name is an integer or byte pointer in the argument text of a prototype"""
    return bool(re.search(r"\b(int64_t|int32_t|int|unsigned char|uint8_t)\s*\*\s*%s\b" % param, args))


def test_the_prototypes_tell_read_from_written():
    p = so.prototypes()
    assert p["gmmiv_tv_subtract_m"] == [("ctx", "handle"), ("U", "scalar"), ("C", "scalar"), ("D", "scalar"), ("N", "read"), ("F", "written"),
                                        ("ubm_means", "read")]
    assert dict(p["gmmiv_score_plda"])["FTJF"] == "read" and dict(p["gmmiv_score_plda"])["scores"] == "written"
    assert dict(p["gmmiv_gmm_set"])["g"] == "handle" and dict(p["gmmiv_llk_use_top_multi"])["clients"] == "handle"
    assert dict(p["gmmiv_scatter_runs"])["x"] == "written" and dict(p["gmmiv_scatter_runs"])["runs"] == "read"


def test_the_poison_is_finite_and_differs_in_every_element():
    rng = np.random.default_rng(0)
    for a in (rng.normal(size=1000), rng.normal(size=1000).astype(np.float32), np.zeros(7), np.array([1e30, -1e30, 1e-300, -1.0, 1.0, 3e38], np.float32),
              np.array([1e300, -1e300, 5e-324, -0.0])):
        b = so.poison(a)
        assert b.dtype == a.dtype and np.isfinite(b).all() and (b != a).all()
    planted = np.array([np.nan, np.inf, -np.inf, 2.0])                                      # NaN statistics (mllr_ref.generate): the poison stays finite
    assert np.isfinite(so.poison(planted)).all() and not (so.poison(planted) == planted).any()
    assert (so.poison(np.arange(5, dtype=np.int64)) == 0).all() and so.poison(np.ones(3, np.uint8)).dtype == np.uint8
    # the one fixed point of the recipe is refused at registration
    rec = so.Recorder(NumpyBackend([]))
    try:
        rec.register(np.array([-0.5]), "in")
    except AssertionError:
        pass
    else:
        raise AssertionError("-0.5 is its own poison and was accepted")
    # and no input of the judged cases holds it
    for case in wh.SMALL:
        assert not (wh.frames(case, "device") == -0.5).any()


class NumpyBackend:
    """numpy arrays for tensors; `queue` holds what is enqueued on the context's stream until ctx_sync runs it"""

    def __init__(self, log):
        self.log, self.queue = log, []

    def ctx_sync(self, h):
        for fn in self.queue:
            fn()
        self.queue = []

    def clone(self, t):
        return t.copy()

    def empty_like(self, t):
        return np.empty_like(t)

    def all_true(self, m):
        return bool(np.all(m))

    def first(self, t):
        return t.reshape(-1)[0].item() if t.size else None

    def span(self, t):
        return t.ctypes.data, t.nbytes

    def on_device(self, a):
        return True

    def write_now(self, dst, src):
        dst[...] = src

    def spin(self, n):
        self.queue.append(lambda: None)

    def enqueue_copy(self, dst, src):
        self.queue.append(lambda: dst.__setitem__(Ellipsis, src))

    def mark(self):
        return lambda: bool(self.queue)

    def busy(self, ev):
        return ev()

    def probe(self, t):
        return t.reshape(-1)[0].item()

    def same_bits(self, a, b):
        return a.tobytes() == b.tobytes()


class FakeLib:
    """gmmiv_tv_subtract_m as a stream-ordered call (F -= N means once the queue runs), or as one that reads N at once"""

    def __init__(self, be, arrays, stream_ordered=True):
        self.be, self.a, self.ordered, self.calls = be, arrays, stream_ordered, []

    def gmmiv_ctx_sync(self, h):
        self.be.ctx_sync(h)
        return 0

    def gmmiv_ctx_set_option(self, *args):
        self.calls.append("set_option")
        return 0

    def gmmiv_tv_subtract_m(self, h, U, C, D, N, F, means):
        N, F, means = (self.a[p.value] for p in (N, F, means))
        self.calls.append("subtract_m")
        if self.ordered:
            self.be.queue.append(lambda: F.__isub__(N * means))
        else:
            early = N.copy()
            self.be.queue.append(lambda: F.__isub__(early * means))
        return 0


def run_fake(stream_ordered):
    log = []
    be = NumpyBackend(log)
    rec = so.Recorder(be)
    N, F, means, out = np.arange(1.0, 5.0), np.full(4, 10.0), np.full(4, 2.0), np.full(4, -7.0)
    table = np.arange(4, dtype=np.int64)
    arrays = {a.ctypes.data: a for a in (N, F, means)}
    for a, role in ((N, "in"), (F, "inout"), (means, "in"), (out, "out"), (table, "in")):
        rec.register(a, role)
    lib = so.LateLib(FakeLib(be, arrays, stream_ordered), rec, None, "tv centre", spin=5)
    ptr = lambda a: ct.c_void_p(a.ctypes.data)
    assert lib.gmmiv_ctx_set_option(None, b"x", 0) == 0 and lib.log == []                    # forwarded, no lateness
    assert lib.gmmiv_tv_subtract_m(None, 1, 4, 1, ptr(N), ptr(F), ptr(means)) == 0
    lib.finish()
    return lib, rec, F


def test_the_proxy_does_its_steps_in_order_and_keeps_inputs_and_outputs_apart():
    lib, rec, F = run_fake(True)
    assert [len(rec.inputs()), len(rec.outputs())] == [3, 2] and [it.role for it in rec.items] == ["in", "inout", "in", "out", "in"]
    kinds = [e[0] for e in lib.log]
    # sync, poison x3 (N, F, means: the integer table was passed to no call and is left alone), spin, restore x3, probe, forward, busy, snapshots
    assert kinds == ["sync"] + ["poison"] * 3 + ["spin"] + ["restore"] * 3 + ["probe", "forward", "busy"] + ["snapshot"] * 2, kinds
    ids = [id(it) for it in rec.items]
    assert [e[1] for e in lib.log if e[0] == "poison"] == ids[:3] and [e[1] for e in lib.log if e[0] == "snapshot"] == [ids[1], ids[3]]
    assert lib.records == [dict(fn="gmmiv_tv_subtract_m", throughout=True, busy=True, seconds=lib.records[0]["seconds"], late=3)]
    assert not lib.faults and np.array_equal(F, 10.0 - np.arange(1.0, 5.0) * 2.0)
    assert rec.items[1].written and not rec.items[0].written and rec.items[0].param == "N" and rec.items[4].param is None
    assert lib.real.calls == ["set_option", "subtract_m"]
    # a call that reads an input when it is made reads the poison: rule (a) sees it
    lib, rec, F = run_fake(False)
    assert np.array_equal(F, 10.0 - (-np.arange(1.0, 5.0) - 1.0) * 2.0)


def test_ws_history_registers_nothing_and_changes_nothing_without_a_recorder():
    import inspect
    assert wh.RECORDER is None
    src = inspect.getsource(wh.dev)
    assert "if RECORDER is not None:" in src and inspect.signature(wh.dev).parameters["role"].default == "in"
    assert 'dev(a, "out")' in inspect.getsource(wh.buf) and 'dev(a, "inout")' in inspect.getsource(wh.mut)
    a = np.arange(3.0)
    assert wh.to("host", a) is a and wh.mut("host", a) is not a and np.array_equal(wh.mut("host", a), a)
    assert wh.buf("host", (2,), np.float32)[0] == np.float32(wh.SENT32) and wh.buf("host", (2,), np.int32)[0] == -77
