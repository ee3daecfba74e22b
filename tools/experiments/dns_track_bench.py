"""The DNS tracker and the domain pass, timed (not product code, and no test asserts any of it).

Tracker.  synth.dns_workload(n) (default 2^20 port-53 payloads) is parsed on the device once; then

  track        fb_dns_track_dev over the parsed arrays where they lie (a synchronous call: classify, the
               insert rounds with their counter read-backs, the sort, take / carry, the resolutions),
               wall clock around the call; before each repetition the state is cleared (fb_dns_track_clear,
               not timed), so every repetition interns the same names
  track_warm   the same call without the clear: every name and address is already stored
  download     what the host loop needs first: the messages, names (256 B each) and answers copied down
  host_loop    DnsResolver.process over the first --host-n messages (the whole batch takes seconds), and
               that time scaled to n

after checking that the device's pending queries and resolutions equal DnsResolver's over the first
--host-n messages.

Domain pass.  The C4 table of blacklist_sweep.py (flow_capacity 2^21, two C4 batches), resolutions for a tenth
of the table's destination addresses, under device events on the null stream, medians after warm-ups:

  first        fb_flow_domains over a zeroed domain plane: every resolved flow's pair is written
  steady       the same call again: nothing changes, nothing is written
  blacklist    fb_flow_blacklist (steady, 1,000 nets) on the same table: the yardstick pass

Usage: python tools/experiments/dns_track_bench.py [--n N] [--host-n M] [--frames F] [--capacity C] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from flodbadd_amd import _native as N  # noqa: E402
from flodbadd_amd import synth  # noqa: E402
from flodbadd_amd.capture import FlodbaddGpuCapture  # noqa: E402
from flodbadd_amd.dns import DnsResolver  # noqa: E402
from flodbadd_amd.sessions import SessionFilter, words_to_ip  # noqa: E402


def med(t):
    t = sorted(t)
    return dict(median_us=statistics.median(t), min_us=t[0], max_us=t[-1], reps=len(t))


def tracker(a):
    lib = N.gpu_lib()
    payload, recs = synth.dns_workload(a.n)
    n = len(recs)
    cap = FlodbaddGpuCapture(0, flow_capacity=0, track_dns=True)
    d_fr = N.DeviceBuffer(payload.nbytes).upload(payload)
    d_dns = N.DeviceBuffer(recs.nbytes).upload(recs)
    d_msg = N.DeviceBuffer(n * N.DNS_MSG_DTYPE.itemsize)
    d_names = N.DeviceBuffer(n * N.FB_DNS_MAX_NAME)
    d_addrs = N.DeviceBuffer(n * N.FB_DNS_MAX_ADDRS * N.FB_IP_DTYPE.itemsize)
    N.check(lib.fb_dns_parse_dev(cap.ctx, d_fr.ptr, payload.nbytes, d_dns.ptr, n, None, d_msg.ptr, d_names.ptr, d_addrs.ptr, None))
    N.check(lib.fb_stream_sync(None))
    res = dict(messages=n)

    def call():
        t0 = time.perf_counter()
        st = cap.track_dns_parsed_dev(d_msg, d_names, d_addrs, n)
        return (time.perf_counter() - t0) * 1e6, st

    cold, warm = [], []
    for i in range(2 + a.reps):
        cap.clear_dns()
        us, st = call()
        if i >= 2:
            cold.append(us)
    res["track"], res["track_stats"] = med(cold), st
    for i in range(2 + a.reps):
        us, st = call()
        if i >= 2:
            warm.append(us)
    res["track_warm"], res["track_warm_stats"] = med(warm), st
    res["info"] = cap.dns_track_info()
    t0 = time.perf_counter()
    msgs = d_msg.download(np.zeros(n, dtype=N.DNS_MSG_DTYPE))
    names = d_names.download(np.zeros((n, N.FB_DNS_MAX_NAME), dtype=np.uint8))
    addrs = d_addrs.download(np.zeros((n, N.FB_DNS_MAX_ADDRS), dtype=N.FB_IP_DTYPE))
    res["download_us"] = (time.perf_counter() - t0) * 1e6
    m = min(a.host_n, n)
    ref = DnsResolver()
    t0 = time.perf_counter()
    ref.process(msgs[:m], names[:m], addrs[:m])
    host = (time.perf_counter() - t0) * 1e6
    res["host_loop"] = dict(messages=m, us=host, scaled_to_n_us=host * n / m)
    cap.clear_dns()
    cap.track_dns_parsed_dev(d_msg, d_names, d_addrs, m)
    res["equal_to_host"] = cap.dns_pending() == ref.pending and cap.dns_resolutions() == ref.resolutions
    cap.close()
    return res


def domains(a):
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
    res = dict(frames_per_batch=n, capacity=int(cap.table_info()["capacity"]), flows=len(flows))
    # resolutions for every tenth flow's destination: parsed arrays built here (query + response per address)
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
    res["track_stats"] = cap.track_dns_parsed_dev(d_msg, d_names, d_addrs, 2 * k)
    e0, e1 = N.Event(), N.Event()

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

    def zero_plane():  # (fb_flow_clear would drop the table: the tracker's clear zeroes the plane, then track again)
        cap.clear_dns()
        cap.track_dns_parsed_dev(d_msg, d_names, d_addrs, 2 * k)

    res["first"] = timed(cap.update_domains, 2, a.reps, before=zero_plane)
    res["steady"] = timed(cap.update_domains, 2, a.reps)
    res["last"] = cap.update_domains()
    rng = np.random.default_rng(5)
    bl = np.zeros(1000, dtype=N.CIDR_DTYPE)
    bl["addr"][:, 0] = rng.integers(1 << 24, 0xDF000000, 1000)
    bl["family"], bl["prefix"], bl["list"] = 2, 24, np.arange(1000) % 8
    cap.set_blacklists(bl)
    res["blacklist"] = timed(lambda: cap.update_blacklist(mark_whitelist=False), 3, a.reps)
    got = cap.dns_resolutions()
    res["resolutions"] = len(got)
    res["lookup_ok"] = all(words_to_ip(r["dst_ip"], int(r["family"])) in got for r in pick[:1000])
    cap.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--host-n", type=int, default=1 << 16)
    ap.add_argument("--frames", type=int, default=10 * (1 << 20))
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-domains", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(tracker=tracker(a))
    if not a.skip_domains:
        res["domains"] = domains(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
