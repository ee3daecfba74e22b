"""Session aging (fb_flow_age) timed on the C4 table: flow_capacity 2^21, timed, two 10,485,760-frame C4
batches (the flows the bench's C4 stream leaves behind).  Four calls under device events on the null
stream, medians after warm-ups:

  status      fb_flow_age without FB_AGE_PURGE
  purge_none  FB_AGE_PURGE with a retention span nothing exceeds (no partition is rewritten)
  purge_half  FB_AGE_PURGE with the retention span at the median idle time (every partition rebuilt); the
              table is rebuilt from the two batches (kept on the device) before every repetition
  export      fb_flow_export_times_dev: the existing sweep over the same tag and time-plane lines

fb_flow_age is a synchronous call (counter memset, kernel, 72-B read-back, stream sync); the events
bracket all of it, so the figures are call times, a few launch latencies above the kernel's own.  Bytes
per the model of DESIGN.md §3.9.  Without --fixed the table grows while it is built (the update's growth
projection), so the sweep runs over more, emptier partitions; the output names the capacity it ran on.
Usage: python tools/experiments/age_sweep.py [--fixed] [--frames N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from flodbadd_amd import _native as N  # noqa: E402
from flodbadd_amd import synth  # noqa: E402
from flodbadd_amd.capture import FlodbaddGpuCapture  # noqa: E402
from flodbadd_amd.sessions import SessionFilter  # noqa: E402

BASE_NS = 1_700_000_000 * 10 ** 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10 * (1 << 20))
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--half-reps", type=int, default=5)
    ap.add_argument("--fixed", action="store_true", help="FB_CFG_FIXED_TABLE: the table stays at --capacity")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib, n = N.gpu_lib(), a.frames
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.GlobalOnly, flow_capacity=a.capacity, timed=True,
                             max_batch_packets=n, grow=not a.fixed)
    N.check(lib.fb_set_session_records(cap.ctx, 0))
    nseg = (n + 63) // 64
    batches = []
    for k in range(2):  # frames 2 us apart, the second batch 40 s after the first
        fr, of = synth.generate(4, n, first=k * n)
        ts = (BASE_NS + k * 40 * 10 ** 9 + np.arange(n, dtype=np.uint64) * 2000).astype(np.uint64)
        batches.append((N.DeviceBuffer(fr.nbytes).upload(fr), fr.nbytes, N.DeviceBuffer(of.nbytes).upload(of),
                        N.DeviceBuffer(ts.nbytes).upload(ts)))
        del fr, of, ts
    d_out, d_seg, d_st = N.DeviceBuffer(nseg * N.SEG_BYTES), N.DeviceBuffer(nseg * 4), N.DeviceBuffer(128)

    def rebuild():
        N.check(lib.fb_flow_clear(cap.ctx, None))
        for d_fr, nbytes, d_of, d_ts in batches:
            N.check(lib.fb_set_frame_times(cap.ctx, d_ts.ptr))
            N.check(lib.fb_process_seg_dev(cap.ctx, d_fr.ptr, nbytes, d_of.ptr, n, d_out.ptr, d_seg.ptr, None, d_st.ptr,
                                           None))
        N.check(lib.fb_stream_sync(None))
        st = d_st.download(np.zeros(1, dtype=N.STATS_DTYPE))
        if int(st[0]["error"]):
            raise RuntimeError("update error word %d" % int(st[0]["error"]))

    e0, e1 = N.Event(), N.Event()

    def timed(fn):
        e0.record(None)
        r = fn()
        e1.record(None)
        return e0.elapsed_ms(e1) * 1000.0, r  # us (elapsed_ms synchronises the stop event)

    def med(fn, warm, reps):
        for _ in range(warm):
            fn()
        t = sorted(timed(fn)[0] for _ in range(reps))
        return dict(median_us=statistics.median(t), min_us=t[0], max_us=t[-1], reps=reps)

    rebuild()
    flows = cap.flow_count()
    times = cap.export_times()
    now = int(times["last_activity_ns"].max()) + 10 ** 9
    idle = now - times["last_activity_ns"].astype(np.int64)
    half_s = float(np.median(idle)) / 1e9
    del times, idle
    info = cap.table_info()
    cap_slots = int(info["capacity"])  # (the table may have grown past --capacity while it was built)
    res = dict(frames_per_batch=n, capacity=cap_slots, flows=flows, partitions=int(info["partitions"]),
               max_partition=int(info["max_partition"]))

    res["status"] = med(lambda: cap.update_sessions_status(now, purge=False), 3, a.reps)
    res["purge_none"] = med(lambda: cap.update_sessions_status(now, purge=True, retention_s=10 ** 7), 3, a.reps)
    assert cap.flow_count() == flows and cap.table_info()["generation"] == info["generation"]

    d_t, d_n = N.DeviceBuffer(max(flows, 1) * 64), N.DeviceBuffer(8)
    res["export"] = med(lambda: N.check(lib.fb_flow_export_times_dev(cap.ctx, d_t.ptr, flows, d_n.ptr, None)), 2,
                        a.reps)

    half, purged = [], []
    for r in range(a.half_reps + 1):  # the first is the warm-up
        if r:
            rebuild()
        us, st = timed(lambda: cap.update_sessions_status(now, purge=True, retention_s=half_s))
        if r:
            half.append(us)
            purged.append(st["purged"])
    half.sort()
    res["purge_half"] = dict(median_us=statistics.median(half), min_us=half[0], max_us=half[-1], reps=len(half),
                             purged=purged[0], retention_s=half_s)

    # the byte model of DESIGN.md 3.9: per slot its 128-B tag line, per flow its 64-B plane line and the
    # status byte read and written; a purge writes the 4-B slot map entry of every slot; a rebuilt
    # partition reads and writes (128 + 64 + 16) B per slot more
    status_bytes = cap_slots * 128 + flows * (64 + 2)
    res["model_bytes"] = dict(status=status_bytes, purge_none=status_bytes + 4 * cap_slots,
                              purge_half=status_bytes + 4 * cap_slots + cap_slots * 2 * (128 + 64 + 16),
                              export=cap_slots * 128 + flows * (64 + 64))
    for k in ("status", "purge_none", "purge_half", "export"):
        res[k]["model_GBps"] = res["model_bytes"][k] / res[k]["median_us"] / 1e3
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    cap.close()


if __name__ == "__main__":
    main()
