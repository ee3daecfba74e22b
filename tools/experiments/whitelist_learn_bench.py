"""Whitelist learning (fb_flow_learn_endpoints_dev) timed on the C4 table the other pass
benchmarks use: flow_capacity 2^21, two 10,485,760-frame C4 batches (about 1.46 M flows, uniform destinations:
nearly one endpoint per flow), and on a second table with the same flows' sources and Zipf(1.1) destinations
over 65,536 addresses (few endpoints, large groups: the atomic-contention case).  Per table:

  a  device      fb_flow_learn_endpoints_dev into a preallocated buffer: device events on the null stream around
                 the synchronous call, median after warm-ups; its rounds and distinct endpoints
  b  unique      rows_from_flows(export_flows()): the export of every flow plus np.unique on the host -- the
                 fastest way to the same set without the pass; host clock (the export ends in a synchronous copy)
  c  host        create_custom_whitelists() as it was: the export, then Session / SessionInfo objects and a Python
                 set.  The export is timed whole, the Python part on a 20,000-flow sample and scaled per flow
  d  on_device   create_custom_whitelists(on_device=True) end to end, and its parts: the device learning with
                 its download (learn_endpoints) and the JSON building (from_learned + to_json)

(b) and (c) run the code paths the package had before the pass, in the same process.  No tracing is active;
--device-only runs just the calls of (a) for a kernel trace taken in a run of its own, and --fold-db adds that
trace's per-kernel totals (a rocpd database) to the JSON.
Usage: python tools/experiments/whitelist_learn_bench.py [--frames N] [--capacity C] [--out FILE]
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
from flodbadd_amd.sessions import SessionFilter, flows_to_sessions  # noqa: E402
from flodbadd_amd.whitelists import Whitelists, rows_from_flows  # noqa: E402

SAMPLE = 20000


def c4_table(frames, capacity):
    lib = N.gpu_lib()
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.GlobalOnly, flow_capacity=capacity, max_batch_packets=frames,
                             grow=False)
    N.check(lib.fb_set_session_records(cap.ctx, 0))
    nseg = (frames + 63) // 64
    d_out, d_seg, d_st = N.DeviceBuffer(nseg * N.SEG_BYTES), N.DeviceBuffer(nseg * 4), N.DeviceBuffer(128)
    for k in range(2):
        fr, of = synth.generate(4, frames, first=k * frames)
        d_fr, d_of = N.DeviceBuffer(fr.nbytes).upload(fr), N.DeviceBuffer(of.nbytes).upload(of)
        N.check(lib.fb_process_seg_dev(cap.ctx, d_fr.ptr, fr.nbytes, d_of.ptr, frames, d_out.ptr, d_seg.ptr, None, d_st.ptr, None))
        N.check(lib.fb_stream_sync(None))
        st = d_st.download(np.zeros(1, dtype=N.STATS_DTYPE))
        if int(st[0]["error"]):
            raise RuntimeError("update error word %d" % int(st[0]["error"]))
        del fr, of, d_fr, d_of
    return cap


def zipf_table(flows, capacity, batch=1 << 20):
    """The flows' own source addresses towards Zipf(1.1)-distributed destinations (the few keys that then
    coincide fold into one flow)."""
    rng = np.random.default_rng(11)
    p = 1.0 / np.arange(1, 65537, dtype=np.float64) ** 1.1
    rank = rng.choice(65536, size=len(flows), p=p / p.sum()).astype(np.uint32)
    rec = np.zeros(len(flows), dtype=N.PARSED_DTYPE)
    for f in ("src_ip", "protocol", "family"):
        rec[f] = flows[f]
    rec["src_port"] = 50000 + np.arange(len(flows)) % 10000
    v6 = flows["family"] == 10
    rec["dst_ip"][:, 0] = np.where(v6, 0x20010DB8, 0x2D000000 + rank)  # 45.0.0.0/16 or 2001:db8::/96
    rec["dst_ip"][:, 3] = np.where(v6, rank, 0)
    rec["dst_port"] = 443
    rec["packet_length"], rec["ip_packet_length"] = 100, 140
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=capacity, max_batch_packets=batch, grow=False)
    for a in range(0, len(rec), batch):
        part = rec[a:a + batch].copy()
        part["pkt_index"] = np.arange(len(part))
        cap.process_parsed(part)
    return cap


def med(fn, warm, reps):
    for _ in range(warm):
        fn()
    t = sorted(fn() for _ in range(reps))
    return dict(median_us=statistics.median(t), min_us=t[0], max_us=t[-1], reps=reps)


def host_us(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e6, r


def measure(cap, reps, device_only=False):
    lib = N.gpu_lib()
    flows_n = cap.flow_count()
    q = cap._view_query(N.FB_VIEW_ALL, None, None)
    d_out, d_n = N.DeviceBuffer(max(flows_n, 1) * 64), N.DeviceBuffer(8)
    st = np.zeros(1, dtype=N.LEARN_STATS_DTYPE)
    e0, e1 = N.Event(), N.Event()

    def device():
        e0.record(None)
        N.check(lib.fb_flow_learn_endpoints_dev(cap.ctx, N.ptr(q), d_out.ptr, flows_n, d_n.ptr, N.ptr(st), None))
        e1.record(None)
        return e0.elapsed_ms(e1) * 1000.0

    info = cap.table_info()
    res = dict(capacity=int(info["capacity"]), flows=flows_n)
    res["a_device"] = med(device, 3, reps)
    res["a_device"].update({f: int(st[0][f]) for f in N.LEARN_STATS_FIELDS})
    if device_only:
        return res
    res["b_unique"] = med(lambda: host_us(lambda: rows_from_flows(cap.export_flows()))[0], 1, 3)
    res["b_unique"]["rows"] = len(rows_from_flows(cap.export_flows()))
    # (c) the host path: the export whole, the Python objects on a sample
    t_export, flows = host_us(cap.export_flows)
    sample = flows[:: max(1, len(flows) // SAMPLE)][:SAMPLE]
    t_py, _ = host_us(lambda: Whitelists.new_from_sessions(flows_to_sessions(sample)).to_json())
    res["c_host"] = dict(export_us=t_export, sample_flows=len(sample), sample_python_us=t_py,
                         python_us_per_flow=t_py / max(len(sample), 1),
                         scaled_total_us=t_export + t_py / max(len(sample), 1) * len(flows))
    # (d) on the device, end to end, and its two parts
    t_all, text = host_us(lambda: cap.create_custom_whitelists(on_device=True))
    t_learn, (recs, _) = host_us(cap.learn_endpoints)
    t_json, _ = host_us(lambda: Whitelists.from_learned(recs).to_json())
    res["d_on_device"] = dict(total_us=t_all, learn_with_download_us=t_learn, json_us=t_json, endpoints=len(recs),
                              json_bytes=len(text))
    return res


def fold_db(path, out):
    """The per-kernel split of a --device-only run's kernel trace (a rocpd database) into the JSON written
    before: a call starts at its k_learn_select dispatch and ends before the next table kernel that is not the
    pass's; the first half of the calls ran on the uniform table, the second half on the Zipf one.  Per table
    and kernel: dispatches per call and the median over the calls of their summed duration."""
    import sqlite3
    db = sqlite3.connect(path)
    rows = list(db.execute("select name, start, end from kernels order by start"))
    calls = []
    for name, start, end in rows:
        short = next((k for k in ("k_learn_select", "k_learn_round", "k_learn_least", "k_learn_flag", "k_learn_emit",
                                  "rocprim", "fillBuffer", "copyBuffer") if k in name), None)
        if short == "k_learn_select":
            calls.append({})
        elif short is None and calls:
            calls[-1]["_closed"] = True
        if short and calls and not calls[-1].get("_closed"):
            n, t = calls[-1].get(short, (0, 0.0))
            calls[-1][short] = (n + 1, t + (end - start) / 1e3)
    half = len(calls) // 2
    split = {}
    for table, part in (("uniform", calls[:half]), ("zipf_1.1", calls[half:])):
        split[table] = {k: dict(dispatches_per_call=statistics.median(c[k][0] for c in part if k in c),
                                median_us_per_call=statistics.median(c[k][1] for c in part if k in c))
                        for k in sorted({k for c in part for k in c if k != "_closed"})}
        split[table]["calls"] = len(part)
    res = json.load(open(out))
    res["kernel_split"] = split
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10 * (1 << 20))
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--fold-db", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.fold_db:
        return fold_db(a.fold_db, a.out)
    def note(msg):
        print(msg, file=sys.stderr, flush=True)

    cap = c4_table(a.frames, a.capacity)
    note("C4 table built: %d flows" % cap.flow_count())
    res = dict(frames_per_batch=a.frames, uniform=measure(cap, a.reps, a.device_only))
    note("uniform: %s" % json.dumps(res["uniform"]))
    flows = cap.export_flows()
    cap.close()
    zc = zipf_table(flows, a.capacity)
    del flows
    note("Zipf table built: %d flows" % zc.flow_count())
    res["zipf_1.1"] = measure(zc, a.reps, a.device_only)
    zc.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
