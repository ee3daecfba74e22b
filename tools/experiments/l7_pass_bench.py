"""The L7 pass, timed (not product code, and no test asserts any of it).

The C4 table of dns_track_bench.py (flow_capacity 2^21, two C4 batches, about 1.46 M flows) under synthetic socket
snapshots built from the table's own flows.  The builder states what it made (`snapshot` in the result):

  mixed      an exact socket for every third flow (TCP: both sides, the flow's source as the local side; UDP: the
             local side), then a wildcard listener (0.0.0.0) on each of the 64 most frequent destination ports:
             about a third of the flows resolve in the exact phase, the flows to those ports in the fuzzy phase,
             the rest miss after all ten lookups
  hot_port   the same, then 100,000 more TCP sockets that all share the table's most frequent destination port
             (distinct local addresses that match no flow): one busy port.  The reference's bucket scan walks
             them for every flow of that port; the index does not care
  empty      no sockets: every lookup ends at once

Per snapshot, under device events on the null stream, medians after warm-ups:

  first      fb_flow_l7 over a zeroed plane (fb_l7_clear + the snapshot installed again, not timed): every
             current flow is looked up, the resolved ones written and stamped
  retry      the same call again with max_retries 255: only the unresolved flows are looked up, all of them miss
             again, each writes its count
  settled    after a pass with max_retries 0 has failed them: nothing is looked up (the sweep's floor)
  install    fb_set_l7_sockets, wall clock: validate, sort and upload

and beside them, on the same table in the same run:

  domains    fb_flow_domains, steady, resolutions for a tenth of the destinations (dns_track_bench.py's case)
  list_scan  tests/l7space.py's literal restatement (the reference's loops) over --scan-flows flows of the table
             against the first --scan-socks sockets of the snapshot, wall clock, scaled to flows x sockets

Usage: python tools/experiments/l7_pass_bench.py [--frames F] [--capacity C] [--reps R] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import l7space as L  # noqa: E402
from flodbadd_amd import _native as N  # noqa: E402
from flodbadd_amd import synth  # noqa: E402
from flodbadd_amd.capture import FlodbaddGpuCapture  # noqa: E402
from flodbadd_amd.sessions import SessionFilter  # noqa: E402


def med(t):
    t = sorted(t)
    return dict(median_us=statistics.median(t), min_us=t[0], max_us=t[-1], reps=len(t))


def snapshots(flows):
    """{name: fb_l7_socket array} and what each holds."""
    pick = flows[::3]
    ex = np.zeros(len(pick), dtype=N.L7_SOCKET_DTYPE)
    ex["local_ip"], ex["local_port"], ex["local_family"] = pick["src_ip"], pick["src_port"], pick["family"]
    ex["protocol"] = pick["protocol"]
    tcp = pick["protocol"] == 6
    ex["remote_ip"][tcp], ex["remote_port"][tcp] = pick["dst_ip"][tcp], pick["dst_port"][tcp]
    ex["remote_family"][tcp] = pick["family"][tcp]
    ex["process_id"] = 1 + np.arange(len(pick)) % 500
    ports, counts = np.unique(flows["dst_port"][flows["protocol"] == 6], return_counts=True)
    top = ports[np.argsort(-counts)][:64]
    wild = np.zeros(len(top), dtype=N.L7_SOCKET_DTYPE)
    wild["local_port"], wild["protocol"], wild["local_family"], wild["remote_family"] = top, 6, 2, 2
    wild["process_id"] = 501 + np.arange(len(top))
    mixed = np.concatenate([ex, wild])
    rng = np.random.default_rng(11)
    hot = np.zeros(100_000, dtype=N.L7_SOCKET_DTYPE)
    hot["local_ip"][:, 0] = 0xF0000000 + np.arange(len(hot))  # 240.0.0.0/4: no flow's address
    hot["remote_ip"][:, 0] = rng.integers(1 << 24, 0xDF000000, len(hot))
    hot["local_port"], hot["remote_port"] = top[0], rng.integers(1024, 65536, len(hot))
    hot["protocol"], hot["local_family"], hot["remote_family"], hot["process_id"] = 6, 2, 2, 600
    out = {"mixed": mixed, "hot_port": np.concatenate([mixed, hot]), "empty": mixed[:0]}
    what = dict(exact_sockets=len(ex), exact_tcp=int(tcp.sum()), wildcard_listeners=len(wild), hot_port=int(top[0]),
                hot_port_sockets=len(hot), flows_to_the_hot_port=int((flows["dst_port"] == top[0]).sum()),
                sizes={k: len(v) for k, v in out.items()})
    return out, what


def run(a):
    lib, n = N.gpu_lib(), a.frames
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.GlobalOnly, flow_capacity=a.capacity, max_batch_packets=n,
                             grow=False, track_dns=True, dns_name_capacity=1 << 16, dns_addr_capacity=1 << 20)
    N.check(lib.fb_set_session_records(cap.ctx, 0))
    nseg = (n + 63) // 64
    d_out, d_seg, d_st = N.DeviceBuffer(nseg * N.SEG_BYTES), N.DeviceBuffer(nseg * 4), N.DeviceBuffer(128)
    for k in range(2):
        fr, of = synth.generate(4, n, first=k * n)
        d_fr, d_of = N.DeviceBuffer(fr.nbytes).upload(fr), N.DeviceBuffer(of.nbytes).upload(of)
        N.check(lib.fb_process_seg_dev(cap.ctx, d_fr.ptr, fr.nbytes, d_of.ptr, n, d_out.ptr, d_seg.ptr, None, d_st.ptr, None))
        N.check(lib.fb_stream_sync(None))
        del fr, of, d_fr, d_of
    flows = np.sort(cap.export_flows(), order="slot")
    res = dict(frames_per_batch=n, capacity=int(cap.table_info()["capacity"]), flows=len(flows),
               tcp_flows=int((flows["protocol"] == 6).sum()))
    snaps, res["snapshot"] = snapshots(flows)
    e0, e1 = N.Event(), N.Event()
    prm = np.zeros(1, dtype=N.L7_PARAMS_DTYPE)
    st = np.zeros(1, dtype=N.L7_STATS_DTYPE)

    def l7_pass(max_retries):
        prm[0]["max_retries"] = max_retries
        N.check(lib.fb_flow_l7(cap.ctx, N.ptr(prm), N.ptr(st), None))
        return {k: int(st[0][k]) for k in N.L7_STATS_FIELDS}

    def timed(fn, warm, reps, before=None):
        t = []
        for i in range(warm + reps):
            if before:
                before()
            e0.record(None)
            fn()
            e1.record(None)
            if i >= warm:
                t.append(e0.elapsed_ms(e1) * 1000.0)
        return med(t)

    cap.set_pass_time(1)
    for name, socks in snaps.items():
        def install():
            N.check(lib.fb_set_l7_sockets(cap.ctx, N.ptr(socks) if len(socks) else None, len(socks)))

        def fresh():
            N.check(lib.fb_l7_clear(cap.ctx))
            install()

        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            install()
            t.append((time.perf_counter() - t0) * 1e6)
        r = dict(install=med(t))
        r["first"] = timed(lambda: l7_pass(255), 2, a.reps, before=fresh)
        fresh()
        r["first_stats"] = l7_pass(255)
        r["retry"] = timed(lambda: l7_pass(255), 2, a.reps)
        r["retry_stats"] = l7_pass(255)
        l7_pass(0)
        r["settled"] = timed(lambda: l7_pass(0), 2, a.reps)
        r["settled_stats"] = l7_pass(0)
        res[name] = r
    # the list-scan restatement on a sample, scaled up
    socks = snaps["hot_port"]
    step = max(len(socks) // a.scan_socks, 1)
    sample = socks[::step][: a.scan_socks]
    sl = [L.Sock(int(s["protocol"]), L.from_words(int(s["local_family"]), s["local_ip"]), int(s["local_port"]),
                 L.from_words(int(s["remote_family"]) or int(s["local_family"]), s["remote_ip"]), int(s["remote_port"]),
                 int(s["process_id"])) for s in sample]
    fl = [L.flow_of(r) for r in flows[:: max(len(flows) // a.scan_flows, 1)][: a.scan_flows]]
    t0 = time.perf_counter()
    hits = sum(1 for f in fl if L.resolve(sl, f)[0])
    us = (time.perf_counter() - t0) * 1e6
    scale = (len(flows) / len(fl)) * (len(socks) / len(sl))
    res["list_scan"] = dict(flows=len(fl), sockets=len(sl), hits=hits, us=us, scaled_to_table_and_hot_port_snapshot_us=us * scale)
    # the domain pass on the same table (dns_track_bench.py's case): resolutions for every tenth destination
    pick = flows[::10]
    k = len(pick)
    msgs = np.zeros(2 * k, dtype=N.DNS_MSG_DTYPE)
    names = np.zeros((2 * k, N.FB_DNS_MAX_NAME), dtype=np.uint8)
    addrs = np.zeros((2 * k, N.FB_DNS_MAX_ADDRS), dtype=N.FB_IP_DTYPE)
    msgs["pkt_index"] = np.arange(2 * k)
    msgs["id"] = np.repeat(np.arange(k) & 0xFFFF, 2)
    msgs["flags"][0::2] = N.DNS_QUERY | N.DNS_HAS_QUESTION
    msgs["n_addrs"][1::2] = 1
    for i in range(k):
        nm = ("host-%d.example" % (i % 50000)).encode()
        names[2 * i, : len(nm)] = np.frombuffer(nm, dtype=np.uint8)
        msgs[2 * i]["name_len"] = len(nm)
    addrs["addr"][1::2, 0] = pick["dst_ip"]
    addrs["family"][1::2, 0] = pick["family"]
    d_msg, d_names, d_addrs = (N.DeviceBuffer(x.nbytes).upload(x) for x in (msgs, names, addrs))
    cap.track_dns_parsed_dev(d_msg, d_names, d_addrs, 2 * k)
    cap.update_domains()
    res["domains"] = timed(cap.update_domains, 2, a.reps)
    res["domains_stats"] = cap.update_domains()
    cap.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10 * (1 << 20))
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scan-flows", type=int, default=200)
    ap.add_argument("--scan-socks", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = run(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
