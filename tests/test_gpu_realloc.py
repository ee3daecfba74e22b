"""The context's reallocation paths: on one context (flow_capacity 1 << 15, max_batch_packets 1,024) a call at a
small size, the same call at a size that takes every scratch past its floor, then the small size again -- and every
result equals, field for field, what a fresh context gives for the same calls.

  SMALL  batches of 1,000 frames (inside what fb_create allocated)
  LARGE  batches of 70,000 frames: more than the 65,536-frame floor of the dense scan scratch, four 20,480-record
         update chunks against the one made at create, and past the 4,096-packet floor of the host staging

The fresh context of a stateless call (fb_parse_classify, fb_format_zeek_dev, fb_flow_merge_dev) is one that only
ever sees that call; the fresh context of the table calls is created for 131,072-packet batches, so its update and
record scratch are never rebuilt."""
import ctypes as C

import numpy as np
import pytest

from flodbadd_amd import _native as N
from flodbadd_amd import synth
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.sessions import SessionFilter
from test_gpu_parity import rows_sorted

pytestmark = pytest.mark.gpu

CAP = 1 << 15
SMALL, LARGE = 1000, 70000
SIZES = [SMALL, SMALL, LARGE, LARGE, SMALL, SMALL]  # the synchronous cases take batches 0, 2, 4
T0 = 1_700_000_000 * 10 ** 9


@pytest.fixture(scope="module")
def batches():
    out, first = [], 0
    for n in SIZES:
        frames, offs = synth.generate(4, n, first=first, n_flows=6000)
        out.append((frames, offs, T0 + (first + np.arange(n, dtype=np.uint64)) * np.uint64(1000)))
        first += n
    return out


def _capture(max_batch=1024, timed=False):
    return FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=CAP, max_batch_packets=max_batch,
                              timed=timed)


def _destroy(cap):
    """fb_destroy reports FB_OK, and a second context made and destroyed on the device then works."""
    lib = N.gpu_lib()
    ctx, cap.ctx = cap.ctx, None
    assert lib.fb_destroy(ctx) == N.FB_OK
    again = _capture()
    ctx, again.ctx = again.ctx, None
    assert lib.fb_destroy(ctx) == N.FB_OK


def _result(r):
    return r.records.tobytes(), r.dns.tobytes(), r.cls.tobytes(), r.stats


def _keyed_history(cap, n_slots):
    by_slot = {int(r["slot"]): r.tobytes()[:40] for r in cap.export_flows()}
    return {by_slot[s]: h for s, h in cap.flow_history(n_slots).items()}


def test_parse_classify_staging_and_scan_scratch(batches):
    cap = _capture()
    try:
        got = [_result(cap.parse_classify(f, o)) for f, o, _ in batches[0:5:2]]
    finally:
        _destroy(cap)
    for (f, o, _), g in zip(batches[0:5:2], got):
        fresh = _capture()
        try:
            assert _result(fresh.parse_classify(f, o)) == g
        finally:
            fresh.close()


def _sync_run(batches, max_batch, timed):
    """fb_process_seg_dev then fb_flow_history_dev per batch -> per call (records, dns, classes, stats, history by
    key), then the table by key, its count and (timed) its times."""
    cap = _capture(max_batch, timed)
    try:
        calls = []
        for f, o, ts in batches:
            r = cap.process_frames_seg(f, o, ts=ts if timed else None)
            calls.append(_result(r) + (_keyed_history(cap, (len(o) - 1 + 63) // 64 * 64),))
        flows = cap.export_flows()
        by_slot = {int(r["slot"]): r.tobytes()[:40] for r in flows}
        times = None
        if timed:
            t = cap.export_times()
            times = sorted((by_slot[int(x["slot"])], x.tobytes()[:t.dtype.fields["slot"][1]]) for x in t)
        return calls, rows_sorted(flows), cap.flow_count(), times
    finally:
        _destroy(cap) if max_batch == 1024 else cap.close()


@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
def test_process_seg_update_record_and_history_scratch(batches, timed):
    seq = batches[0:5:2]
    calls, table, count, times = _sync_run(seq, 1024, timed)
    ref_calls, ref_table, ref_count, ref_times = _sync_run(seq, 1 << 17, timed)
    for k, (g, r) in enumerate(zip(calls, ref_calls)):
        for field, a, b in zip(("records", "dns", "classes", "stats", "history"), g, r):
            assert a == b, (k, field)
    assert count == ref_count and table == ref_table and times == ref_times
    assert len(calls[1][4]) > 1000  # (the large batch's history is there at all: 6,000 flows)


def _async_run(batches, max_batch):
    """fb_process_seg_async_dev over every batch, two buffer sets rotating (so two batches are in flight around
    each regrowth) -> per-batch stats, the table by key, its count, the last update's history by key."""
    lib = N.gpu_lib()
    cap = _capture(max_batch)
    stream = N.Stream()
    keep = []
    try:
        stats = []
        for f, o, _ in batches:
            n = len(o) - 1
            nseg = (n + 63) // 64
            b = [N.DeviceBuffer(f.nbytes).upload(f), N.DeviceBuffer(o.nbytes).upload(o), N.DeviceBuffer(nseg * N.SEG_BYTES),
                 N.DeviceBuffer(nseg * 4), N.DeviceBuffer(N.STATS_DTYPE.itemsize)]
            keep += b
            N.check(lib.fb_process_seg_async_dev(cap.ctx, b[0].ptr, f.nbytes, b[1].ptr, n, b[2].ptr, b[3].ptr, None, b[4].ptr,
                                                 stream.ptr))
            stats.append(b[4])
        N.check(lib.fb_flow_join(cap.ctx, stream.ptr))
        stream.sync()
        st = [s.download(np.zeros(1, dtype=N.STATS_DTYPE), stream=stream.ptr).tobytes() for s in stats]
        hist = _keyed_history(cap, (len(batches[-1][1]) - 1 + 63) // 64 * 64)
        return st, rows_sorted(cap.export_flows()), cap.flow_count(), hist
    finally:
        for b in keep:
            b.free()
        _destroy(cap) if max_batch == 1024 else cap.close()


def test_process_seg_async_both_scratch_sets(batches):
    got, ref = _async_run(batches, 1024), _async_run(batches, 1 << 17)
    for field, a, b in zip(("stats", "table", "count", "history"), got, ref):
        assert a == b, field
    assert np.frombuffer(got[0][3], dtype=N.STATS_DTYPE)[0]["error"] == 0


def _views(cap):
    """Every flow's fb_flow_view, left on the device -> (buffer, count)."""
    cnt = cap.flow_count()
    q = np.zeros(1, dtype=N.VIEW_QUERY_DTYPE)
    q[0]["set"], q[0]["filter"] = N.FB_VIEW_ALL, int(SessionFilter.All)
    d_views, d_n = N.DeviceBuffer(cnt * N.FLOW_VIEW_DTYPE.itemsize), N.DeviceBuffer(8)
    N.check(N.gpu_lib().fb_flow_export_view_dev(cap.ctx, N.ptr(q), d_views.ptr, cnt, d_n.ptr, None))
    assert int(d_n.download(np.zeros(1, dtype=np.uint64))[0]) == cnt
    return d_views, cnt


def _zeek(cap, d_views, n, stream):
    """fb_format_zeek_dev over the first n views on `stream`, nothing waited for -> a reader to call after a sync."""
    cap_text = n * N.FB_ZEEK_FIXED_MAX
    d_text, d_off, d_st = N.DeviceBuffer(cap_text), N.DeviceBuffer(8 * (n + 1)), N.DeviceBuffer(64)
    N.check(N.gpu_lib().fb_format_zeek_dev(cap.ctx, d_views.ptr, n, None, None, 0, d_text.ptr, cap_text, d_off.ptr, d_st.ptr,
                                           stream.ptr))

    def read():
        st = d_st.download(np.zeros(1, dtype=N.ZEEK_STATS_DTYPE), stream=stream.ptr)
        off = d_off.download(np.zeros(n + 1, dtype=np.uint64), stream=stream.ptr)
        text = d_text.download(np.zeros(int(st[0]["bytes"]), dtype=np.uint8), int(st[0]["bytes"]), stream=stream.ptr)
        return st.tobytes(), off.tobytes(), text.tobytes()
    return read


def test_zeek_scratch_grows_behind_its_event(batches):
    cap = _capture(timed=True)
    sa, sb = N.Stream(), N.Stream()
    try:
        for f, o, ts in batches[0:5:2]:
            cap.process_frames_seg(f, o, ts=ts)
        d_views, cnt = _views(cap)
        assert cnt > 4000
        sizes, streams = [100, cnt, 100], [sa, sb, sa]
        readers = [_zeek(cap, d_views, n, s) for n, s in zip(sizes, streams)]  # (no host synchronise in between)
        got = [r() for r in readers]
        assert int(np.frombuffer(got[1][0], dtype=N.ZEEK_STATS_DTYPE)[0]["lines_written"]) == cnt
        for n, g in zip(sizes, got):
            fresh = _capture(timed=True)
            try:
                assert _zeek(fresh, d_views, n, sa)() == g, n
            finally:
                fresh.close()
    finally:
        _destroy(cap)


def test_merge_scratch_grows_behind_its_event(batches):
    lib = N.gpu_lib()
    cap = _capture()
    sa, sb = N.Stream(), N.Stream()
    try:
        for f, o, _ in batches[0:5:2]:
            cap.process_frames_seg(f, o)
        cnt = cap.flow_count()
        rec = N.FLOW_MREC_DTYPE.itemsize

        def export(stream):
            d_out, d_cnt = N.DeviceBuffer(cnt * rec), N.DeviceBuffer(8)
            N.check(lib.fb_flow_export_merge_dev(cap.ctx, 1, 0, 0, d_out.ptr, cnt, d_cnt.ptr, stream.ptr))
            return d_out, d_cnt

        def merge(ctx, d_in, stream):
            d_out, d_n = N.DeviceBuffer(cnt * N.FLOW_REC_DTYPE.itemsize), N.DeviceBuffer(8)
            N.check(lib.fb_flow_merge_dev(ctx, d_in.ptr, cnt, d_out.ptr, d_n.ptr, stream.ptr))
            return d_out, d_n

        def merged(d_out, d_n, stream):
            m = int(d_n.download(np.zeros(1, dtype=np.uint64), stream=stream.ptr)[0])
            return m, d_out.download(np.zeros(cnt, dtype=N.FLOW_REC_DTYPE), stream=stream.ptr)[:m].tobytes()

        d_m1, d_c1 = export(sa)
        sa.sync()                      # (the merge below reads these records)
        assert int(d_c1.download(np.zeros(1, dtype=np.uint64))[0]) == cnt
        d_m2, d_c2 = export(sa)        # the export on stream A, then the merge on stream B, nothing waited for
        d_o, d_n = merge(cap.ctx, d_m1, sb)
        got = merged(d_o, d_n, sb)
        sa.sync()
        m1 = d_m1.download(np.zeros(cnt, dtype=N.FLOW_MREC_DTYPE))
        m2 = d_m2.download(np.zeros(cnt, dtype=N.FLOW_MREC_DTYPE))
        assert rows_sorted(m1) == rows_sorted(m2) and int(d_c2.download(np.zeros(1, dtype=np.uint64))[0]) == cnt
        assert got[0] == cnt
        fresh = _capture()
        try:
            assert merged(*merge(fresh.ctx, d_m1, sa), sa) == got
        finally:
            fresh.close()
    finally:
        _destroy(cap)
