"""The process-aware whitelist check and learning, timed (not product code, and no test asserts any of it).

The C4 table of l7_pass_bench.py (flow_capacity 2^21, two C4 batches, about 1.46 M flows) and that tool's `mixed`
socket snapshot (an exact socket for every third flow, wildcard listeners on the 64 busiest ports), its 564
process ids named "proc0" .. "proc49" in turn.  Device events on the null stream for the passes, wall clock for the
calls that read counters between launches; medians after warm-ups, `repeats` medians per figure so the run-to-run
spread stands beside it.

  a  fb_flow_whitelist with the list learned from the table without processes (rows_from_flows: one exact-address
     endpoint per distinct destination, port and protocol).  No process id, no name table: the instances of before.
     This part runs from any tree (--root): the parent commit's and this one's are measured in one session.
  b  the same pass with the list learned WITH processes on the device (a name table installed, every endpoint of a
     resolved flow carries its process id): the process-aware instances.
  c  fb_flow_learn_endpoints_dev without and with the name table.
  d  update_whitelist's work after the list is compiled, for the list of (b): the default mode -- the pass marks
     every flow of a process endpoint's key for the host, which then runs is_session_in_whitelist per marked flow over
     the whole endpoint list; taken from --scan-flows flows against --scan-eps endpoints and scaled to marked flows x
     endpoints -- against processes_on_device: install, pass and the export of the exceptions, nothing left to the host.
     The library refuses a list with more than FB_WL_MAX_OTHER process endpoints without ids, so the default mode
     gets the process-less endpoints and the first --default-eps process endpoints only (the result says so).

Usage: python tools/experiments/whitelist_proc_bench.py [--part a|all] [--root DIR --label NAME] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def med(t):
    t = sorted(t)
    return dict(median_us=statistics.median(t), min_us=t[0], max_us=t[-1], reps=len(t))


def run(a):
    from flodbadd_amd import _native as N
    from flodbadd_amd import synth
    from flodbadd_amd.capture import FlodbaddGpuCapture
    from flodbadd_amd.sessions import SessionFilter
    from flodbadd_amd.whitelists import rows_from_flows
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
        del fr, of, d_fr, d_of
    flows = np.sort(cap.export_flows(), order="slot")
    res = dict(tree=a.label, frames_per_batch=n, capacity=int(cap.table_info()["capacity"]), flows=len(flows))
    e0, e1 = N.Event(), N.Event()

    def events(fn, warm, reps):
        t = []
        for i in range(warm + reps):
            e0.record(None)
            fn()
            e1.record(None)
            if i >= warm:
                t.append(e0.elapsed_ms(e1) * 1000.0)
        return med(t)

    def wall(fn, warm, reps):
        t = []
        for i in range(warm + reps):
            t0 = time.perf_counter()
            fn()
            if i >= warm:
                t.append((time.perf_counter() - t0) * 1e6)
        return med(t)

    # (a) the list without processes
    rows = rows_from_flows(flows)
    cap.install_whitelist(rows)
    res["a_endpoints"] = len(rows)
    res["a_stats"] = cap.whitelist_pass()
    res["a_pass"] = [events(cap.whitelist_pass, 3, a.reps) for _ in range(a.repeats)]
    if a.part == "a":
        cap.close()
        return res

    # the snapshot, one L7 pass, the name table
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))
    import l7_pass_bench as LB
    from flodbadd_amd.whitelists import WhitelistEndpoint, is_session_in_whitelist
    from flodbadd_amd.sessions import Session, words_to_ip
    snaps, res["snapshot"] = LB.snapshots(flows)
    socks = snaps["mixed"]
    N.check(lib.fb_set_l7_sockets(cap.ctx, N.ptr(socks), len(socks)))
    res["l7_stats"] = cap.update_l7()
    n_ids = int(socks["process_id"].max()) + 1
    ids = np.zeros(n_ids, dtype=np.uint32)
    ids[1:] = 1 + np.arange(1, n_ids) % 50  # process p is "proc<p % 50>": lower case, so one id serves both arrays

    def names(on):
        N.check(lib.fb_set_l7_process_names(cap.ctx, N.ptr(ids) if on else None, N.ptr(ids) if on else None, n_ids if on else 0))

    # (c) learning without and with the table
    names(False)
    res["c_learn_without_table"] = [wall(cap.learn_endpoints, 2, a.reps) for _ in range(a.repeats)]
    res["c_without_stats"] = cap.learn_endpoints()[1]
    names(True)
    res["c_learn_with_table"] = [wall(cap.learn_endpoints, 2, a.reps) for _ in range(a.repeats)]
    recs, res["c_with_stats"] = cap.learn_endpoints()

    # (b) the list learned with processes
    pv = recs.view(N.LEARNED_ENDPOINT_PROC_DTYPE)
    prow = np.zeros(len(recs), dtype=N.WL_ENDPOINT_DTYPE)
    prow["addr"], prow["family"], prow["protocol"], prow["port"] = recs["dst_ip"], recs["family"], recs["protocol"], recs["dst_port"]
    prow["prefix"] = np.where(recs["family"] == 2, 32, 128)
    prow["flags"] = N.FB_WL_HAS_PORT | np.where(pv["proc_name_id"] != 0, N.FB_WL_HAS_PROCESS, 0).astype(np.uint8)
    prow["reserved2"] = pv["proc_name_id"]
    res["b_endpoints"], res["b_endpoints_with_process"] = len(prow), int((pv["proc_name_id"] != 0).sum())
    t0 = time.perf_counter()
    cap.install_whitelist(prow)
    res["b_install_us"] = (time.perf_counter() - t0) * 1e6
    res["b_stats"] = cap.whitelist_pass()
    res["b_pass"] = [events(cap.whitelist_pass, 3, a.reps) for _ in range(a.repeats)]

    # (d) what is left after the compile: the device mode ...
    def device_mode():
        cap.install_whitelist(prow)
        cap.whitelist_pass()
        cap.export_whitelist_flows(N.FB_WL_NONCONFORMING)

    res["d_device_mode"] = [wall(device_mode, 1, max(a.reps // 2, 3)) for _ in range(a.repeats)]
    # ... and the default mode: the same list without ids, the marked flows to the host's scan
    zrow = prow.copy()
    zrow["reserved2"] = 0
    try:  # (a process endpoint without an id counts against FB_WL_MAX_OTHER: the whole list is refused)
        cap.install_whitelist(zrow)
        res["d_default_whole_list"] = "installed"
    except N.FbError as e:
        res["d_default_whole_list"] = "refused: %s" % e
        keep = np.flatnonzero(zrow["flags"] & N.FB_WL_HAS_PROCESS)[: a.default_eps]
        zrow = zrow[np.sort(np.concatenate([keep, np.flatnonzero(~(zrow["flags"] & N.FB_WL_HAS_PROCESS).astype(bool))]))]
    res["d_default_endpoints"] = len(zrow)

    def default_pass():
        cap.install_whitelist(zrow)
        st = cap.whitelist_pass()
        cap.export_whitelist_flows(N.FB_WL_HOST_CHECK)
        return st

    res["d_default_stats"] = default_pass()
    res["d_default_device_part"] = [wall(default_pass, 1, max(a.reps // 2, 3)) for _ in range(a.repeats)]
    marked = cap.export_whitelist_flows(N.FB_WL_HOST_CHECK)
    l7 = cap.l7_records()["process_id"]
    step = max(len(recs) // a.scan_eps, 1)
    eps = [WhitelistEndpoint(ip=str(words_to_ip(r["dst_ip"], int(r["family"]))),
                             port=int(r["dst_port"]), protocol={6: "TCP", 17: "UDP"}[int(r["protocol"])],
                             process=("proc%d" % (int(p) - 1)) if int(p) else None)
           for r, p in zip(recs[::step][: a.scan_eps], pv["proc_name_id"][::step][: a.scan_eps])]
    sample = marked[:: max(len(marked) // a.scan_flows, 1)][: a.scan_flows]
    sess = [(Session.from_key(r), int(l7[int(r["slot"])])) for r in sample]
    t0 = time.perf_counter()
    hits = sum(1 for s, p in sess if is_session_in_whitelist(eps, "custom_whitelist", None, str(s.dst_ip), s.dst_port,
                                                              s.protocol.name, None, None, None,
                                                              ("proc%d" % (int(ids[p]) - 1)) if p else None)[0])
    us = (time.perf_counter() - t0) * 1e6
    scale = (len(marked) / max(len(sess), 1)) * (len(zrow) / max(len(eps), 1))
    res["d_host_scan"] = dict(flows=len(sess), endpoints=len(eps), hits=hits, us=us, marked_flows=len(marked),
                              scaled_to_marked_flows_and_the_list_us=us * scale)
    cap.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("a", "all"), default="all")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)),
                    help="the tree flodbadd_amd is imported from (part a: the parent commit's build)")
    ap.add_argument("--label", default="branch", help="what the result calls the tree it ran from")
    ap.add_argument("--frames", type=int, default=10 * (1 << 20))
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scan-flows", type=int, default=200)
    ap.add_argument("--scan-eps", type=int, default=2000)
    ap.add_argument("--default-eps", type=int, default=60000,
                    help="process endpoints the default-mode list keeps when the library refuses the whole one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.root = os.path.abspath(a.root)
    sys.path.insert(0, a.root)
    res = run(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
