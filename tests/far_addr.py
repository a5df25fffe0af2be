"""The far buffer of tests/test_gpu_far_addressing.py: one device allocation in which a window handed to an entry point starts 2^31
float64 elements (2^32 float32 elements, 16 GiB) above the base, so that the frames a call addresses lie beyond 2^32 bytes, 2^31 elements
and (float32) 2^32 elements from the pointer it was given.

Everything the window does not hold is POISON: the 32-bit word 0x40490FDB repeated.  As float32 it reads 3.1415927, as float64
50.12387...: an ordinary finite value (the degenerate-input rules never see it) that no generated frame takes (put() checks).  An index
that loses its high word, wraps negative or is truncated to 32 bits therefore still lands inside the allocation -- the guard below the
window is as long as the largest negative 32-bit index, the allocation above it as long as the largest unsigned one that the sizes in
use can produce -- and reads poison or writes over it: a wrong number or a failed sweep, never a fault.

run() (run_flat() for one contiguous matrix of 16 GiB, filled and checked on the device) is the only way a test touches the buffer: it
writes the input cells, makes the call, copies out the cells the call may write,
puts poison back into both and then checks EVERY byte of the allocation, in slabs of 1 GiB (no temporary of the buffer's size exists).
"""
import struct

import numpy as np
import pytest

GIB = 1 << 30
POISON_WORD = 0x40490FDB
POISON = {np.float32: struct.unpack("<f", struct.pack("<I", POISON_WORD))[0],
          np.float64: struct.unpack("<d", struct.pack("<II", POISON_WORD, POISON_WORD))[0]}
GUARD_BYTES = 16 * GIB                  # below every window: 2^31 float64 elements, 2^32 float32 elements
ALLOC_BYTES = 33 * GIB + (1 << 20)      # guard + the largest window (float64 wide rows, 17 GiB) + slack; at most 34 GiB
SLAB_WORDS = 1 << 28                    # 1 GiB of 32-bit words per fill / check step

WIDE_LD = 1 << 22                       # row stride of the wide-rows layout, in elements
WIDE_T = {np.float32: 1056,             # frame 256 at 2^32 bytes, 512 at 2^31 elements, 1024 at 2^32 elements; 16.5 GiB
          np.float64: 544}              # frame 128 at 2^32 bytes, 512 at 2^31 elements; 17 GiB
# element offsets from the window's first element that the far-frames layout crosses
THRESHOLDS = {np.float32: (1 << 30, 1 << 31, 1 << 32),      # 2^32 bytes, 2^31 elements, 2^32 elements
              np.float64: (1 << 29, 1 << 31)}               # 2^32 bytes, 2^31 elements (2^32 float64 elements would need 32 GiB more)

assert ALLOC_BYTES <= 34 * GIB and ALLOC_BYTES % 4 == 0
assert all(np.isfinite(v) and abs(v) < 1e18 for v in POISON.values())


def tdtype(dtype):
    import torch
    return {np.float32: torch.float32, np.float64: torch.float64}[dtype]


class FarBuffer:
    def __init__(self):
        import torch
        free, _ = torch.cuda.mem_get_info()
        try:
            self.raw = torch.empty(ALLOC_BYTES, dtype=torch.uint8, device="cuda")
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            pytest.skip("the far buffer needs %d bytes in one device allocation, %d are free" % (ALLOC_BYTES, free))
        self.words = self.raw.view(torch.int32)
        self.typed = {dt: self.raw.view(tdtype(dt)) for dt in POISON}
        self.calls = 0
        for lo in range(0, self.words.numel(), SLAB_WORDS):
            self.words[lo:lo + SLAB_WORDS].fill_(POISON_WORD)
        self.sweep("the fill")

    def close(self):
        import torch
        self.words = self.typed = self.raw = None
        torch.cuda.empty_cache()

    # ---- windows
    def view(self, dtype, shape, strides):
        """a strided view (sizes and strides in elements) whose first element lies GUARD_BYTES above the allocation's base"""
        import torch
        size = np.dtype(dtype).itemsize
        off = GUARD_BYTES // size
        last = off + sum((n - 1) * s for n, s in zip(shape, strides))
        assert all(n >= 1 for n in shape) and (last + 1) * size <= ALLOC_BYTES, (shape, strides)
        return torch.as_strided(self.typed[dtype], tuple(shape), tuple(strides), off)

    def wide(self, dtype, D, T=None):
        """wide rows: [T, D] with a row stride of 2^22 elements; only the first D columns of a row ever hold data"""
        return self.view(dtype, (WIDE_T[dtype] if T is None else T, D), (WIDE_LD, 1))

    def dense(self, dtype, D, frames):
        """far frames: a dense ldx = D matrix of `frames` rows; the tests write a few short runs of it"""
        return self.view(dtype, (frames, D), (D, 1))

    # ---- the call
    def _poison(self, cells):
        cells.fill_(POISON[{4: np.float32, 8: np.float64}[cells.element_size()]])

    def run(self, what, fn, inputs=(), outputs=()):
        """inputs: (cells, numpy data) pairs written before the call; outputs: cells the call is allowed to write (an in-place call names
        its cells in both) -> (what fn returned, [numpy copy of every output]).  Afterwards the whole allocation is poison again."""
        import torch
        for cells, data in inputs:
            data = np.ascontiguousarray(data)
            assert tuple(cells.shape) == data.shape and cells.element_size() == data.itemsize, (what, tuple(cells.shape), data.shape)
            words = data.view(np.uint32)
            assert not (words == POISON_WORD).any(), "%s: the data holds the poison word" % what
            cells.copy_(torch.from_numpy(data).to(cells.device))
        for cells, data in inputs[:1]:      # the fixture itself: the first input reads back as written
            assert np.array_equal(cells.cpu().numpy().view(np.uint32), np.ascontiguousarray(data).view(np.uint32)), "%s: the far view does not hold its data" % what
        try:
            res = fn()
            torch.cuda.synchronize()
            got = [c.cpu().numpy() for c in outputs]
        finally:
            for cells, _ in inputs:
                self._poison(cells)
            for cells in outputs:
                self._poison(cells)
        self.sweep(what)
        self.calls += 1
        return res, got

    def run_flat(self, what, flat, value, fn, check):
        """run() for a contiguous 1-D view too large to pass through the host: value(lo, hi) -> the device values of elements [lo, hi),
        written slab by slab; fn() is the call; check(flat) looks at the result on the device and returns what the test needs.  Poison goes
        back slab by slab and the whole allocation is swept, as in run()."""
        import torch
        n, step = flat.numel(), SLAB_WORDS * 4 // flat.element_size()
        try:
            for lo in range(0, n, step):
                flat[lo:lo + step] = value(lo, min(lo + step, n))
            res = fn()
            torch.cuda.synchronize()
            seen = check(flat)
        finally:
            for lo in range(0, n, step):
                self._poison(flat[lo:lo + step])
        self.sweep(what)
        self.calls += 1
        return res, seen

    def sweep(self, what):
        """every byte of the allocation is poison"""
        import torch
        bad = torch.zeros((), dtype=torch.int64, device=self.words.device)
        for lo in range(0, self.words.numel(), SLAB_WORDS):
            bad += (self.words[lo:lo + SLAB_WORDS] != POISON_WORD).sum()
        n = int(bad.item())
        if n:
            where = []
            for lo in range(0, self.words.numel(), SLAB_WORDS):
                hit = (self.words[lo:lo + SLAB_WORDS] != POISON_WORD).nonzero()[:4, 0]
                where += [4 * (lo + int(i)) for i in hit.tolist()]
                if hit.numel():
                    self.words[lo:lo + SLAB_WORDS].fill_(POISON_WORD)       # the next call starts from a clean buffer again
            raise AssertionError("%s: %d 32-bit words of the far buffer are not poison after the call (outside the cells it may write); first at "
                                 "byte offsets %s from the base, the window starts at %d" % (what, n, where[:8], GUARD_BYTES))


def same_bits(what, got, want):
    """bit for bit, with the first offending index in the message"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        a, b = got.reshape(-1).view(np.uint8).reshape(got.size, -1), want.reshape(-1).view(np.uint8).reshape(want.size, -1)
        bad = np.flatnonzero((a != b).any(1))
        i = np.unravel_index(int(bad[0]), got.shape) if got.ndim else ()
        raise AssertionError("%s: %d of %d values differ in their bits from the dense call, first at %s: far %r, dense %r"
                             % (what, bad.size, got.size, tuple(int(v) for v in i), got[i], want[i]))


def far_runs(dtype, D, lens=(9, 13, 11)):
    """far-frames layout: [(first frame, length)] -- one run near frame 0, then per threshold a run that ends below the frame holding the
    threshold element, one that straddles it and one that begins above it -- and the number of frames the dense view needs.  Runs are
    sorted and disjoint, two frames apart."""
    runs = [(3, lens[0])]
    for e in THRESHOLDS[dtype]:
        f = e // D                          # the frame that holds element e (for D = 1 the frame NUMBER is the threshold)
        below = f - 2 - lens[0] - lens[1] // 2
        runs += [(below, lens[0]), (f - lens[1] // 2, lens[1]), (f + lens[1] - lens[1] // 2 + 2, lens[2])]
    assert all(a[0] + a[1] < b[0] for a, b in zip(runs, runs[1:])), runs
    return runs, runs[-1][0] + runs[-1][1] + 1


def compact(runs, align=64):
    """the dense twin of a far run table: the same runs moved next to each other, every first frame congruent to its far one modulo
    `align` (a run keeps its place inside the 16-frame blocks and tiles the kernels cut) -> ([(first, length)], frames)"""
    out, cur = [], 0
    for first, n in runs:
        cur += (first - cur) % align
        out.append((cur, n))
        cur += n + 1
    return out, cur
