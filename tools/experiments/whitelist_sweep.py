"""The whitelist pass (fb_flow_whitelist) timed on the C4 table: flow_capacity 2^21, two 10,485,760-frame
C4 batches (the flows the bench's C4 stream leaves behind), a synthetic ASN table (every IPv4 /12, 2,048
IPv6 first-word ranges) and 1,000 blacklist nets.  Three figures under device events on the null stream,
medians after warm-ups:

  mixed     (a) a list of ~1,000 endpoints: exact addresses, nets, AS-only, domain and process endpoints
  mixed_keyed   the same list with a port on each of its 100 protocol- and port-free nets (no group
            that every flow has to scan)
  learned   (b) the list learned from the table itself (rows_from_flows: one exact endpoint per distinct
            (dst_ip, dst_port, protocol), about one per flow)
  enrich    (c) fb_flow_enrich_dev over all flows: the same table scan plus four binary searches per flow

fb_flow_whitelist is a synchronous call (counter memset, kernel, 40-B read-back, stream sync) and the
events bracket all of it, so (a) and (b) are call times, a few launch latencies above the kernel's own;
(c) is an asynchronous call bracketed the same way.  No tracing is active.  Bytes per the model of
DESIGN.md §3.10.
Usage: python tools/experiments/whitelist_sweep.py [--frames N] [--capacity C] [--out FILE]
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
from flodbadd_amd.sessions import Session, SessionFilter  # noqa: E402
from flodbadd_amd.whitelists import Whitelists, rows_from_flows  # noqa: E402


def asn_tables():
    v4 = np.zeros(4096, dtype=N.ASN_RANGE_DTYPE)
    a = np.arange(4096, dtype=np.uint64) << 20
    v4["start"][:, 0], v4["end"][:, 0] = a, a | 0xFFFFF
    v4["as_number"], v4["record"] = 64000 + np.arange(4096) % 500, np.arange(4096)
    v6 = np.zeros(2048, dtype=N.ASN_RANGE_DTYPE)
    w = 0x20000000 + (np.arange(2048, dtype=np.uint64) << 17)
    v6["start"][:, 0], v6["end"][:, 0] = w, w | 0x1FFFF
    v6["end"][:, 1:] = 0xFFFFFFFF
    v6["as_number"], v6["record"] = 65000 + np.arange(2048) % 300, 4096 + np.arange(2048)
    recs = [(int(x["as_number"]), ("US", "FR", "DE", "JP")[i % 4], "Owner %d" % (i % 700))
            for i, x in enumerate(np.concatenate([v4, v6]))]
    return v4, v6, recs


def mixed_list(sessions, recs, keyed=False):
    """~1,000 endpoints of every kind the index distinguishes.  keyed: the 100 IPv6 nets, which have
    neither protocol nor port and so form one group that every flow scans, get a port each."""
    eps = []
    for s in sessions[:: max(1, len(sessions) // 400)][:400]:
        eps.append({"ip": str(s.dst_ip), "port": s.dst_port, "protocol": s.protocol.name})
    for i in range(300):
        eps.append({"ip": "%d.%d.0.0/%d" % (11 + i % 200, i % 256, 12 + i % 12), "port": (443, 80, 53, 8080)[i % 4],
                    "protocol": ("TCP", "UDP")[i % 2]} if i % 3 else
                   dict({"ip": "2%03x::/%d" % (i, 16 + i % 40)}, **({"port": 3000 + i} if keyed else {})))
    for i in range(200):
        r = recs[(i * 31) % len(recs)]
        eps.append({"as_number": r[0], "port": (443, 80, 53, 123)[i % 4]} if i % 2 else
                   {"as_owner": r[2].upper(), "as_country": r[1].lower(), "protocol": "TCP", "port": 1000 + i})
    for i in range(50):
        eps.append({"domain": "*.svc%d.example.com" % i, "port": 443, "protocol": "TCP"})
        eps.append({"process": "proc%d" % i, "port": 2000 + i})
    return {"date": "", "signature": None, "whitelists": [{"name": "custom_whitelist", "endpoints": eps}]}


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
    flows = cap.export_flows()
    info = cap.table_info()
    cap_slots = int(info["capacity"])
    v4, v6, recs = asn_tables()
    cap.set_asn_tables(v4, v6, recs)
    bl = np.zeros(1000, dtype=N.CIDR_DTYPE)
    bl["addr"][:, 0] = (np.arange(1000, dtype=np.uint64) * 4194301 + (12 << 24)) & 0xFFFFFF00
    bl["family"], bl["prefix"], bl["list"] = 2, 24, np.arange(1000) % 8
    cap.set_blacklists(bl)
    res = dict(frames_per_batch=n, capacity=cap_slots, flows=len(flows), partitions=int(info["partitions"]))

    e0, e1 = N.Event(), N.Event()

    def timed(fn):
        e0.record(None)
        r = fn()
        e1.record(None)
        return e0.elapsed_ms(e1) * 1000.0, r

    def med(fn, warm, reps):
        for _ in range(warm):
            fn()
        t = sorted(timed(fn)[0] for _ in range(reps))
        return dict(median_us=statistics.median(t), min_us=t[0], max_us=t[-1], reps=reps)

    sessions = [Session.from_key(r) for r in flows[:: max(1, len(flows) // 4000)]]
    comp = Whitelists(mixed_list(sessions, recs)).compile("custom_whitelist", recs)
    cap.install_whitelist(comp)
    res["mixed"] = med(cap.whitelist_pass, 3, a.reps)
    res["mixed"].update(endpoints=len(comp.rows), last=cap.whitelist_pass())

    comp = Whitelists(mixed_list(sessions, recs, keyed=True)).compile("custom_whitelist", recs)
    cap.install_whitelist(comp)
    res["mixed_keyed"] = med(cap.whitelist_pass, 3, a.reps)
    res["mixed_keyed"].update(endpoints=len(comp.rows), last=cap.whitelist_pass())

    rows = rows_from_flows(flows)
    cap.install_whitelist(rows)
    res["learned"] = med(cap.whitelist_pass, 3, a.reps)
    st = cap.whitelist_pass()
    assert st["conforming"] == st["flows"] == len(flows), st
    res["learned"].update(endpoints=len(rows), last=st)

    d_e, d_n = N.DeviceBuffer(max(len(flows), 1) * N.FLOW_ENRICH_DTYPE.itemsize), N.DeviceBuffer(8)
    res["enrich"] = med(lambda: N.check(lib.fb_flow_enrich_dev(cap.ctx, 0, d_e.ptr, len(flows), d_n.ptr, None)), 3, a.reps)

    # per slot its 128-B tag line; per flow the state byte read (and written when it
    # changes: not in a repeated pass); the learned list adds the address search, ~2 probes x log2(n) steps
    # of 4 B (IPv4) or 16 B (IPv6) per flow, served by L2 / the Infinity Cache; enrichment writes 32 B per
    # flow and runs four searches of the small ASN / blacklist tables
    n4 = int((rows["family"] == 2).sum())
    n6 = len(rows) - n4
    f4 = int((flows["family"] == 2).sum())
    f6 = len(flows) - f4
    scan = cap_slots * 128 + len(flows)
    probes = f4 * 2 * int(np.ceil(np.log2(max(n4, 2)))) * 4 + f6 * 2 * int(np.ceil(np.log2(max(n6, 2)))) * 16
    res["model_bytes"] = dict(mixed=scan, mixed_keyed=scan, learned=scan, learned_probe_bytes=probes,
                              enrich=cap_slots * 128 + len(flows) * 32)
    for k in ("mixed", "mixed_keyed", "learned", "enrich"):
        res[k]["model_GBps"] = res["model_bytes"][k] / res[k]["median_us"] / 1e3
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    cap.close()


if __name__ == "__main__":
    main()
