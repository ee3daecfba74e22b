"""The blacklist pass (fb_flow_blacklist) timed on the C4 table: flow_capacity 2^21, two 10,485,760-frame
C4 batches (the flows the bench's C4 stream leaves behind), with 1,000 and with 50,000 blacklist nets
(eight lists; a fifth of the nets are the /24 or /64 of addresses the table holds, the rest random).
Per list size, under device events on the null stream, medians after warm-ups:

  first       fb_flow_blacklist over a zeroed mask plane: every blacklisted flow's word is written
              (before each repetition the lists are removed, one pass clears the plane, and the lists are
              installed again -- none of that is timed)
  steady      the same call again: nothing changes, nothing is written
  steady_mark the steady call with FB_BL_MARK_WHITELIST (also reads the whitelist byte of every
              blacklisted flow)
  enrich      fb_flow_enrich_dev over all flows with the same lists: the same table scan, four searches
              and a 32-B record per flow
  whitelist   fb_flow_whitelist with a small exact list (1,000 endpoints learned from the table)

fb_flow_blacklist and fb_flow_whitelist are synchronous calls (counter memset, kernel, read-back, stream
sync) and the events bracket all of it; enrich is an asynchronous call bracketed the same way.  No tracing
is active.  Bytes per the model of DESIGN.md §3.11.
Usage: python tools/experiments/blacklist_sweep.py [--frames N] [--capacity C] [--out FILE]
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
from flodbadd_amd.whitelists import rows_from_flows  # noqa: E402


def nets(flows, n, rng):
    """n fb_cidr rows over eight lists: n/5 cover addresses of the table (IPv4 /24, IPv6 /64, either end),
    the rest are random IPv4 /24s and IPv6 /48s."""
    out = np.zeros(n, dtype=N.CIDR_DTYPE)
    own = flows[rng.integers(0, len(flows), n // 5)]
    for i, r in enumerate(own):
        ip = r["dst_ip"] if i & 1 else r["src_ip"]
        v6 = int(r["family"]) == 10
        out[i]["addr"], out[i]["family"], out[i]["prefix"] = ip, (10 if v6 else 2), (64 if v6 else 24)
    k = len(own)
    m = n - k
    out["addr"][k:, 0] = rng.integers(1 << 24, 0xDF000000, m)
    out["family"][k:], out["prefix"][k:] = 2, 24
    six = k + np.arange(0, m, 4)  # every fourth of the random ones is an IPv6 /48
    out["addr"][six, 0] = 0x20010000 | rng.integers(0, 1 << 16, len(six))
    out["addr"][six, 1] = rng.integers(0, 1 << 32, len(six)) & 0xFFFF0000
    out["family"][six], out["prefix"][six] = 10, 48
    out["list"] = np.arange(n) % 8
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10 * (1 << 20))
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib, n = N.gpu_lib(), a.frames
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.GlobalOnly, flow_capacity=a.capacity, max_batch_packets=n,
                             grow=False)
    N.check(lib.fb_set_session_records(cap.ctx, 0))
    nseg = (n + 63) // 64
    d_out, d_seg, d_st = N.DeviceBuffer(nseg * N.SEG_BYTES), N.DeviceBuffer(nseg * 4), N.DeviceBuffer(128)
    for k in range(2):
        fr, of = synth.generate(4, n, first=k * n)
        d_fr, d_of = N.DeviceBuffer(fr.nbytes).upload(fr), N.DeviceBuffer(of.nbytes).upload(of)
        N.check(lib.fb_process_seg_dev(cap.ctx, d_fr.ptr, fr.nbytes, d_of.ptr, n, d_out.ptr, d_seg.ptr, None, d_st.ptr, None))
        N.check(lib.fb_stream_sync(None))
        st = d_st.download(np.zeros(1, dtype=N.STATS_DTYPE))
        if int(st[0]["error"]):
            raise RuntimeError("update error word %d" % int(st[0]["error"]))
        del fr, of, d_fr, d_of
    flows = np.sort(cap.export_flows(), order="slot")  # (the export's block order varies: the same nets every run)
    info = cap.table_info()
    cap_slots = int(info["capacity"])
    res = dict(frames_per_batch=n, capacity=cap_slots, flows=len(flows), partitions=int(info["partitions"]))
    e0, e1 = N.Event(), N.Event()

    def timed(fn):
        e0.record(None)
        r = fn()
        e1.record(None)
        return e0.elapsed_ms(e1) * 1000.0, r

    def med(fn, warm, reps, before=None):
        t = []
        for i in range(warm + reps):
            if before:
                before()
            us = timed(fn)[0]
            if i >= warm:
                t.append(us)
        t.sort()
        return dict(median_us=statistics.median(t), min_us=t[0], max_us=t[-1], reps=reps)

    rows = rows_from_flows(flows[:: max(1, len(flows) // 1000)][:1000])
    cap.install_whitelist(rows)
    res["whitelist"] = med(cap.whitelist_pass, 3, a.reps)
    res["whitelist"].update(endpoints=len(rows), last=cap.whitelist_pass())
    N.check(lib.fb_clear_whitelist(cap.ctx))

    d_e, d_n = N.DeviceBuffer(max(len(flows), 1) * N.FLOW_ENRICH_DTYPE.itemsize), N.DeviceBuffer(8)
    rng = np.random.default_rng(5)
    empty = np.zeros(0, dtype=N.CIDR_DTYPE)
    f4 = int((flows["family"] == 2).sum())
    f6 = len(flows) - f4
    for count in (1000, 50000):
        bl = nets(flows, count, rng)
        r = {}

        def zero_plane():
            cap.set_blacklists(empty)
            cap.update_blacklist(mark_whitelist=False)
            cap.set_blacklists(bl)

        r["first"] = med(lambda: cap.update_blacklist(mark_whitelist=False), 3, a.reps, before=zero_plane)
        r["steady"] = med(lambda: cap.update_blacklist(mark_whitelist=False), 3, a.reps)
        r["last"] = cap.update_blacklist(mark_whitelist=False)
        r["steady_mark"] = med(lambda: cap.update_blacklist(mark_whitelist=True), 3, a.reps)
        N.check(lib.fb_clear_whitelist(cap.ctx))
        r["enrich"] = med(lambda: N.check(lib.fb_flow_enrich_dev(cap.ctx, 0, d_e.ptr, len(flows), d_n.ptr, None)), 3, a.reps)
        # per slot its 128-B tag line; per flow the 8-B mask read, and 8 B written where it
        # changed; two searches of ceil(log2 m) probes per flow (4 B IPv4, 16 B IPv6; L2 / Infinity Cache)
        m4 = int((bl["family"] == 2).sum())
        m6 = count - m4
        scan = cap_slots * 128 + len(flows) * 8
        r["model_bytes"] = dict(first=scan + r["last"]["blacklisted"] * 8, steady=scan, steady_mark=scan + r["last"]["blacklisted"],
                                enrich=cap_slots * 128 + len(flows) * 32,
                                probe_bytes=2 * (f4 * int(np.ceil(np.log2(max(2 * m4, 2)))) * 4 +
                                                 f6 * int(np.ceil(np.log2(max(2 * m6, 2)))) * 16))
        for k in ("first", "steady", "steady_mark", "enrich"):
            r[k]["model_GBps"] = r["model_bytes"][k] / r[k]["median_us"] / 1e3
        r.update(nets=count, nets_v4=m4, nets_v6=m6)
        res["nets_%d" % count] = r
    res["model_bytes_whitelist"] = cap_slots * 128 + len(flows)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    cap.close()


if __name__ == "__main__":
    main()
