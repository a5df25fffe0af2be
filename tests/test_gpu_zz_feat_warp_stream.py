"""gmmiv_feat_warp_hist / gmmiv_feat_warp_apply read device inputs in stream order (the suite-wide rule of tests/test_gpu_stream_order.py,
applied here because include/ext/gmmiv_feat_warp.h is not under include/ yet).

The test needs a context with a private stream and a second stream beside it.  It does nothing on torch's default stream between the
spin and the calls (the poison value it compares with is taken before), so it does not depend on which hardware queue its stream
shares.  The file is collected after the older stream-order tests, which do depend on the streams created before them (DESIGN.md
section 9, item 7)."""
import numpy as np
import pytest

import warp_ref as W

pytestmark = pytest.mark.gpu

from lia_ral_amd import capi                    # noqa: E402
from lia_ral_amd import feat_warp as fw         # noqa: E402
import test_gpu_feat_warp as base               # noqa: E402  (helpers only: nothing of it is collected here)


def test_device_tables_written_late_on_the_stream():
    """every array a device pointer: both calls only enqueue and read their inputs in stream order -- they hold poison when the calls are
    made and become right behind a spin kernel on the context's stream (the helpers of tests/stream_order.py, as test_gpu_turn.py)"""
    import torch
    import stream_order as so
    D, nb, U = 7, 40, 3
    x, runs = base.make(D, [500, 41, 90], np.float64, 41, pad=0)
    tb, tc = base.target()
    bits, dev = base.bits, base.dev
    c = capi.Context(0)                                                     # a private stream
    be = so.TorchBackend(capi.lib, c)
    true = [dev(x), dev(runs), dev(tb), dev(tc)]

    def outputs(fill):
        return dict(b=torch.full((U, D, nb + 1), fill, dtype=torch.float64, device="cuda"), c=torch.full((U, D, nb), fill, dtype=torch.float64, device="cuda"),
                    s=torch.full((U, D), 9, dtype=torch.int32, device="cuda"), out=torch.full(x.shape, fill, dtype=torch.float64, device="cuda"))

    def chain(xd, r, tbd, tcd, o):
        fw.warp_hist(c, xd, r, U, nb, bounds=o["b"], count=o["c"], status=o["s"])
        fw.warp_apply(c, xd, r, U, o["b"], o["c"], o["s"], tbd, tcd, out=o["out"])

    ref = outputs(-7.0)
    torch.cuda.synchronize()
    chain(*true, ref)
    c.sync()
    live = [t.clone() for t in true]
    got = outputs(-7.0)
    bad = [so.poison(src) for src in true]
    bad0 = bad[0].flatten()[0].item()
    assert bad0 != true[0].flatten()[0].item()
    torch.cuda.synchronize()
    for t, p in zip(live, bad):
        be.write_now(t, p)
    be.spin(so.SPIN_CYCLES)
    for t, src in zip(live, true):
        be.enqueue_copy(t, src)
    ev = be.mark()
    seen = be.probe(live[0])                                                # on the stream beside: the restoring copies wait behind the spin
    chain(*live, got)
    busy = be.busy(ev)
    c.sync()
    torch.cuda.synchronize()
    assert seen == bad0
    assert busy, "the calls returned after the stream had drained: they did not only enqueue"
    for name in ref:
        assert np.array_equal(bits(ref[name].cpu().numpy()), bits(got[name].cpu().numpy())), name
    c.close()
    host = base.run_dev(x, D, runs, U, nb, out_dtype=np.float64)            # and the device tables give the bits of the host tables
    assert np.array_equal(bits(host[1]), bits(ref["b"].cpu().numpy())) and np.array_equal(host[3], ref["s"].cpu().numpy())
    rows = np.concatenate([W.unit_rows(runs, u) for u in range(U)])
    assert np.array_equal(bits(host[0][rows]), bits(ref["out"].cpu().numpy()[rows]))
