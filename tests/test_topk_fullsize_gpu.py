"""Top-k at size: the livejournal stand-in with the 10 sources of a top1000 file as one source group (configs[2] as
bench.py runs it). The device selection equals numpy over group_read for every source, and costs a fraction of the
dense read it replaces."""
import ctypes as C
import time

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng, stream as st
from tests.test_fullsize_gpu import stand_in
from tests.test_topk_gpu import assert_same

pytestmark = pytest.mark.gpu


def test_livejournal_ten_source_group_topk():
    V, e1, e2, cfg, wl = stand_in("livejournal", 1)
    W, c, eps = wl.window, wl.per_batch, 1e-9
    sources = [int(x) for x in datagen.ranked_sources(V, e1, e2, W, cfg.directed, 10, 1000, 10)]
    e = eng.Engine(V, W, cfg.directed, c)
    ss = st.SlidingStream(V, e1, e2, cfg.directed, wl)
    e.load_window(*ss.serialize_edge_stream())
    gid = e.add_source_group(sources)
    e.group_init_solve(gid, eps)
    assert not ss.stream_updates()
    e.set_batch(*ss.batch_arrays())
    e.slide(*ss.new_arrays())
    e.group_update(gid, eps)
    dense = [e.group_read(gid, i) for i in range(len(sources))]
    for k in (100, 8192):
        res = e.group_topk(gid, k)
        for i, (p, r) in enumerate(dense):
            assert_same(res[i], p, r, k, 0.0, f"livejournal source {i}")

    # the dense route this replaces: p of all 10 sources through group_read (no r), against the group top-k (k = 8192)
    L, dp = eng.lib(), C.POINTER(C.c_double)
    buf = np.empty(V)

    def dense_read():
        for i in range(len(sources)):
            assert L.dppr_group_read(e._h, gid, i, buf.ctypes.data_as(dp), None) == 0

    def best_of(fn, reps=3):
        fn()  # (warm: workspace, map copies)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return min(t) * 1e3

    t_read = best_of(dense_read)
    t_top = best_of(lambda: e.group_topk(gid, 8192))
    t_top100 = best_of(lambda: e.group_topk(gid, 100))
    print(f"[topk] livejournal 10-source group: group_topk k=8192 {t_top:.3f} ms, k=100 {t_top100:.3f} ms (call, host "
          f"included); dense group_read of p for 10 sources {t_read:.3f} ms")
    assert t_top < 0.25 * t_read, (t_top, t_read)
