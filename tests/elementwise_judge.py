"""What the per-element GPU files share (test_gpu_tv_elementwise.py, test_gpu_backend_elementwise.py,
test_gpu_estimation_elementwise.py, test_gpu_trials_elementwise.py, test_gpu_ws_history.py / ws_history.py): the option bracket, the
collector of ratios to a bar and the device buffer between two guard bands.  No test lives here."""
import contextlib

import numpy as np

DEFAULTS = {"tv_batch": 1024, "tv_acc_mb": 8192, "gemm_nt80": 1, "tv_tett_direct": 1, "tv_mstep_solve": 1, "tv_md_device": 1, "chol_gemm": 0,
            "trials_piece": 0, "trials_scratch_mb": 2048, "topc_use_lanes": 4, "topc_z": 1, "topc_fused": 1, "glds": 1,
            "stats_z": 1, "z_scratch_mb": 16384, "models_scratch_mb": 2048, "wg_waves": 8, "z_waves": 8, "short_calls": 1, "timing": 0}
GUARD = 64                    # doubles on either side of a device result (a multiple of 2: the result keeps its 16-byte alignment)
SENTINEL = -1.2345678e300


@contextlib.contextmanager
def options(ctx, opts):
    """set, run, restore (as test_gpu_gmm_elementwise.options): set_option hands back what was there"""
    try:
        for k, v in opts.items():
            prev = ctx.set_option(k, v)
            assert prev == DEFAULTS[k], "option %s was %r, expected the default %r" % (k, prev, DEFAULTS[k])
        yield
    finally:
        for k, v in opts.items():
            back = ctx.set_option(k, DEFAULTS[k])
            assert back == v, "option %s read back %r after it was set to %r" % (k, back, v)


def path_name(opts):
    return " ".join("%s %d" % kv for kv in opts.items()) or "defaults"


class Judge:
    """collects the failures of one test; every comparison is a ratio to a bar; the largest ratio per (case, path, entry, kind)
    goes to `ratios`, the record of the module that runs the test"""

    def __init__(self, case, path, ratios):
        self.case, self.path, self.bad, self.ratios = case, path, [], ratios

    def __call__(self, entry, kind, ratios):
        r = np.asarray(ratios, np.float64)
        worst = float(r.max()) if r.size else 0.0
        key = (self.case, self.path, entry, kind)
        self.ratios[key] = max(self.ratios.get(key, 0.0), worst)
        if not worst <= 1.0:
            i = tuple(int(v) for v in np.argwhere(~(r <= 1.0))[0])
            self.bad.append("%s | %s | %s | %s: %d of %d outside the bar, first at %s: |error| / bar = %.3g (largest %.3g)"
                            % (self.case, self.path, entry, kind, int((~(r <= 1.0)).sum()), r.size, i, float(r[i]), worst))

    def same_bits(self, entry, a, b, what):
        a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
        if a.shape != b.shape or not np.array_equal(a.view(np.int64), b.view(np.int64)):
            i = tuple(int(v) for v in np.argwhere(a.view(np.int64) != b.view(np.int64))[0]) if a.shape == b.shape else ()
            self.bad.append("%s | %s | %s: not the bits of %s, first at %s: %r against %r"
                            % (self.case, self.path, entry, what, i, float(a[i]) if i else a.shape, float(b[i]) if i else b.shape))

    def note(self, entry, text):
        self.bad.append("%s | %s | %s: %s" % (self.case, self.path, entry, text))

    def finish(self):
        assert not self.bad, "%d comparisons failed:\n" % len(self.bad) + "\n".join(self.bad[:30])


class Guarded:
    """a device result of `shape` between two guard bands of GUARD doubles; fill = None leaves the sentinel in the result too (an
    output the call must write completely); shift = 1 moves the result one double off its 16-byte alignment"""

    def __init__(self, shape, fill=0.0, shift=0, init=None):
        import torch
        self.n = int(np.prod(shape))
        self.lo = GUARD + shift
        self.buf = torch.full((self.n + 2 * GUARD + shift,), SENTINEL, dtype=torch.float64, device="cuda")
        self.view = self.buf[self.lo:self.lo + self.n].view(*shape)
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init, np.float64)))
        elif fill is not None:
            self.view.fill_(fill)
        torch.cuda.synchronize()

    def read(self, j, entry, complete=True):
        import torch
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        if not (np.all(h[:self.lo] == SENTINEL) and np.all(h[self.lo + self.n:] == SENTINEL)):
            j.note(entry, "a guard band around the device result was written")
        out = h[self.lo:self.lo + self.n].reshape(tuple(self.view.shape)).copy()
        if complete and np.any(out == SENTINEL):
            j.note(entry, "%d elements of the result were never written" % int((out == SENTINEL).sum()))
        return out
