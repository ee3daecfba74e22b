"""The Zeek conn.log export timed on the C4 table.

The table: flow_capacity 2^21, timed, two 10,485,760-frame C4 batches (about 1.46 M flows; the view records
alone are ~374 MB and the text ~200 MB, past the 256 MB Infinity Cache).  The fused update path keeps no
history strings, so every TCP flow gets a history of its table hist_len made of seeded characters: the blob
has the lengths a capture with track_history would hold, and hist_mismatch stays 0.

  device  fb_format_zeek_dev over view records already in device memory -- all flows, and the ~1 % modified
          most recently -- staged against direct (FB_DEBUG_ZEEK_DIRECT), the two alternating.  A figure is
          the median of --calls calls under device events on the null stream after 3 warm-up calls; a repeat
          is one such median; --repeats repeats per row.  With the view export in front of it too.
  host    wall clock, once each after a warm-up call: cap.export_zeek() whole (view export, history upload,
          format, download of text + offsets + stats) for all flows and for ~1 %, with and without the history
          strings; against format_sessions_zeek(get_sessions()) -- by default on a --sample-flow sample of the
          same table (views_to_sessions + format_sessions_zeek, the per-flow cost scaled to the table; its
          lines are checked to be among the device's), with --full-host on the whole table.

Usage: python tools/experiments/zeek_export_bench.py [--frames N] [--capacity C] [--calls 20] [--repeats 4]
       [--sample 20000] [--full-host] [--out profiles/zeek_export_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

S = 10 ** 9
T0 = 1_700_000_000 * S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10 * (1 << 20))
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--full-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from flodbadd_amd import _native as N
    from flodbadd_amd import synth
    from flodbadd_amd.capture import FlodbaddGpuCapture
    from flodbadd_amd.sessions import SessionFilter, format_sessions_zeek, views_to_sessions

    lib, n = N.gpu_lib(), a.frames
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=a.capacity, max_batch_packets=n,
                             grow=False, timed=True)
    N.check(lib.fb_set_session_records(cap.ctx, 0))
    nseg = (n + 63) // 64
    d_out, d_seg, d_st = N.DeviceBuffer(nseg * N.SEG_BYTES), N.DeviceBuffer(nseg * 4), N.DeviceBuffer(128)
    for k in range(2):
        fr, of = synth.generate(4, n, first=k * n)
        d_fr, d_of = N.DeviceBuffer(fr.nbytes).upload(fr), N.DeviceBuffer(of.nbytes).upload(of)
        d_ts = N.DeviceBuffer(8 * n).upload(T0 + k * S + np.arange(n, dtype=np.uint64) * 50)
        N.check(lib.fb_set_frame_times(cap.ctx, d_ts.ptr))
        N.check(lib.fb_process_seg_dev(cap.ctx, d_fr.ptr, fr.nbytes, d_of.ptr, n, d_out.ptr, d_seg.ptr, None, d_st.ptr, None))
        N.check(lib.fb_stream_sync(None))
        st = d_st.download(np.zeros(1, dtype=N.STATS_DTYPE))
        if int(st[0]["error"]):
            raise RuntimeError("update error word %d" % int(st[0]["error"]))
        del fr, of, d_fr, d_of, d_ts
    del d_out, d_seg
    print("table built", flush=True)

    views = cap.export_view()
    nf, slots = len(views), int(cap.table_info()["capacity"])
    # the history blob: per slot, hist_len seeded characters
    lens = np.zeros(slots + 1, dtype=np.uint64)
    lens[views["rec"]["slot"].astype(np.int64) + 1] = views["rec"]["hist_len"]
    hoff = np.cumsum(lens, dtype=np.uint64)
    alphabet = np.frombuffer(N.FB_HIST_CHARS.encode("ascii"), dtype=np.uint8)
    chars = alphabet[np.random.default_rng(5).integers(0, len(alphabet), int(hoff[-1]))]
    d_hist, d_hoff = N.DeviceBuffer(max(len(chars), 1)).upload(chars), N.DeviceBuffer(hoff.nbytes).upload(hoff)

    la = np.sort(views["time"]["last_activity_ns"])
    since_1pct = int(la[int(0.99 * nf)])
    d_view, d_n = N.DeviceBuffer(nf * 256), N.DeviceBuffer(8)
    text_cap = nf * N.FB_ZEEK_FIXED_MAX + len(chars)
    d_text, d_off, d_stats = N.DeviceBuffer(text_cap), N.DeviceBuffer(8 * (nf + 1)), N.DeviceBuffer(64)
    q = np.zeros(1, dtype=N.VIEW_QUERY_DTYPE)
    q[0]["filter"] = N.FB_FILTER_ALL

    def view(since=None):
        q[0]["flags"], q[0]["since_ns"] = (N.FB_VIEW_MODIFIED_SINCE, since) if since is not None else (0, 0)
        N.check(lib.fb_flow_export_view_dev(cap.ctx, N.ptr(q), d_view.ptr, nf, d_n.ptr, None))

    def count():
        return int(d_n.download(np.zeros(1, dtype=np.uint64))[0])

    def fmt(m):
        N.check(lib.fb_format_zeek_dev(cap.ctx, d_view.ptr, m, d_hist.ptr, d_hoff.ptr, slots, d_text.ptr, text_cap,
                                       d_off.ptr, d_stats.ptr, None))

    def stats():
        st = d_stats.download(np.zeros(1, dtype=N.ZEEK_STATS_DTYPE))
        return {k: int(st[0][k]) for k in N.ZEEK_STATS_FIELDS}

    e0, e1 = N.Event(), N.Event()

    def once(fn):
        e0.record(None)
        fn()
        e1.record(None)
        return e0.elapsed_ms(e1) * 1000.0

    def repeat(fn, warm=3):
        for _ in range(warm):
            fn()
        return round(statistics.median(once(fn) for _ in range(a.calls)), 2)

    res = dict(what=__doc__.split("\n\n")[1].replace("\n", " "), flows=nf, capacity=slots, history_bytes=int(len(chars)),
               calls_per_repeat=a.calls, device_us={}, selected={}, stats={}, host={})
    for name, since in (("all", None), ("1pct", since_1pct)):
        view(since)
        m = min(count(), nf)
        res["selected"][name] = m
        rows = {"format.%s.staged" % name: 0, "format.%s.direct" % name: 1}
        for k in rows:
            res["device_us"][k] = []
        res["device_us"]["view+format.%s.staged" % name] = []
        for r in range(a.repeats):                        # staged and direct alternate
            pair = []
            for k, knob in rows.items():
                N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_ZEEK_DIRECT, knob))
                res["device_us"][k].append(repeat(lambda: fmt(m)))
                st = stats()
                assert st["lines_written"] == m and st["hist_mismatch"] == 0, st
                if r == 0:                                # the same records both times: the same bytes
                    pair.append(d_text.download(np.zeros(st["bytes"], dtype=np.uint8), st["bytes"]).tobytes())
            assert r or pair[0] == pair[1]
            N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_ZEEK_DIRECT, 0))
            res["device_us"]["view+format.%s.staged" % name].append(repeat(lambda: (view(since), fmt(m))))
            view(since)                                   # (the same records for the next repeat's format rows)
        res["stats"][name] = stats()
    res["median_us"] = {k: statistics.median(v) for k, v in res["device_us"].items()}
    res["bytes_moved"] = {name: dict(views_read=res["selected"][name] * 256, text_written=res["stats"][name]["bytes"])
                          for name in ("all", "1pct")}
    print("device rows done", flush=True)

    def wall(fn):
        fn()                                              # warm-up
        t = time.perf_counter()
        out = fn()
        return round(time.perf_counter() - t, 4), out

    host = res["host"]
    host["export_zeek_all_no_history_s"], log = wall(cap.export_zeek)
    host["export_zeek_1pct_no_history_s"], log1 = wall(lambda: cap.export_zeek(since_ns=since_1pct))
    host["lines"], host["text_bytes_no_history"] = len(log), int(len(log.text))
    # the strings a capture with track_history would hold
    raw = chars.tobytes().decode("ascii")
    cap.histories = {int(s): raw[int(hoff[s]):int(hoff[s + 1])] for s in np.flatnonzero(lens[1:]).tolist()}
    cap.track_history = True
    host["export_zeek_all_s"], log = wall(cap.export_zeek)
    host["export_zeek_1pct_s"], log1 = wall(lambda: cap.export_zeek(since_ns=since_1pct))
    host["text_bytes"], host["lines_1pct"] = int(len(log.text)), len(log1)
    device_lines = set(log.lines())
    if a.full_host:
        t = time.perf_counter()
        want = format_sessions_zeek(cap.get_sessions())[1:]
        host["format_sessions_zeek_get_sessions_s"] = round(time.perf_counter() - t, 2)
        assert sorted(want) == sorted(log.lines())
    sample = views[:: max(nf // a.sample, 1)][:a.sample]
    t = time.perf_counter()
    infos = views_to_sessions(sample, cap.histories)
    t_join = time.perf_counter() - t
    t = time.perf_counter()
    want = format_sessions_zeek(infos)[1:]
    t_fmt = time.perf_counter() - t
    assert set(want) <= device_lines and len(set(want)) == len(sample)
    host.update(sample_flows=len(sample), sample_views_to_sessions_s=round(t_join, 3), sample_format_sessions_zeek_s=round(t_fmt, 3),
                host_path_us_per_flow=round((t_join + t_fmt) / len(sample) * 1e6, 2),
                host_path_scaled_to_table_s=round((t_join + t_fmt) / len(sample) * nf, 1))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    cap.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
