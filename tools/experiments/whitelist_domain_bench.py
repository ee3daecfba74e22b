"""Domain endpoints decided on the device, timed (not product code, and no test asserts any of it).

The C4 table of whitelist_proc_bench.py (flow_capacity 2^21, two C4 batches, about 1.46 M flows) on a capture that
tracks DNS: every distinct destination address gets a tracked resolution, eight addresses to a name, and one domain
pass puts the name ids into the plane.  The list is the one learned from that table with its domains
(fb_flow_learn_endpoints_dev): one endpoint per distinct (address, port, protocol), each with its domain as an exact
pattern.  Device events on the null stream for the passes, wall clock for the calls that wait themselves; medians
after warm-ups, `repeats` medians per figure so the run-to-run spread stands beside it.

  free  fb_flow_whitelist with the same list without domains (rows_from_flows): no pattern id, the instances of
        before.  Runs from any tree (--root), so the parent commit's build and this one are measured in one session.
  c     the name-match kernel over every stored name (the mask knob forgets the rows; fb_wl_name_matches_dev of no
        ids then matches them all and waits), and over 1 % more names tracked afterwards.
  d     fb_flow_whitelist with the list learned with domains (every endpoint of a resolved destination carries a
        pattern id): the kDom instances, against `free` in the same process.

The end-to-end update_whitelist comparison is not in this tool: Whitelists.compile of a 1.46 M-endpoint list is a
Python loop of minutes in either mode, and the default mode's fb_set_whitelist refuses a list with more than
FB_WL_MAX_OTHER domain endpoints.

Usage: python tools/experiments/whitelist_domain_bench.py [--part free|all] [--root DIR --label NAME] [--out FILE]
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
                             grow=False, track_dns=a.part != "free")
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

    rows = rows_from_flows(flows)
    cap.install_whitelist(rows)
    res["free_endpoints"] = len(rows)
    res["free_stats"] = cap.whitelist_pass()
    res["free_pass"] = [events(cap.whitelist_pass, 3, a.reps) for _ in range(a.repeats)]
    if a.part == "free":
        cap.close()
        return res

    # a resolution for every distinct destination, eight addresses to a name
    dst = np.unique(np.concatenate([flows["dst_ip"], flows["family"].astype(np.uint32)[:, None]], axis=1), axis=0)
    n_names = (len(dst) + 7) // 8

    def track(first, count, tx0):
        """Names first .. first + count: one query and one response (its eight addresses) each, 16 Ki names a call."""
        for lo in range(first, first + count, 1 << 14):
            m = min(1 << 14, first + count - lo)
            msgs = np.zeros(2 * m, dtype=N.DNS_MSG_DTYPE)
            names = np.zeros((2 * m, N.FB_DNS_MAX_NAME), dtype=np.uint8)
            addrs = np.zeros((2 * m, N.FB_DNS_MAX_ADDRS), dtype=N.FB_IP_DTYPE)
            for j in range(m):
                nm = ("h%07d.zone%03d.example.com" % (lo + j, (lo + j) % 500)).encode()
                names[j, :len(nm)] = np.frombuffer(nm, dtype=np.uint8)
                msgs[j]["name_len"] = len(nm)
                d = dst[(lo + j) * 8:(lo + j) * 8 + 8]
                addrs[m + j, :len(d)]["addr"], addrs[m + j, :len(d)]["family"] = d[:, :4], d[:, 4]
                msgs[m + j]["answers"] = msgs[m + j]["n_addrs"] = len(d)
            msgs["pkt_index"] = np.arange(2 * m)
            msgs["id"] = (tx0 + np.arange(2 * m) % m) & 0xFFFF
            msgs[:m]["flags"], msgs[:m]["questions"] = N.DNS_QUERY | N.DNS_HAS_QUESTION, 1
            bufs = [N.DeviceBuffer(x.nbytes).upload(x) for x in (msgs, names, addrs)]
            cap.track_dns_parsed_dev(bufs[0], bufs[1], bufs[2], 2 * m)

    track(0, n_names, 0)
    res["dns"] = cap.dns_track_info()
    res["domain_pass"] = cap.update_domains()
    recs, res["learn_stats"] = cap.learn_endpoints()
    stored = cap.dns_names(range(1, res["dns"]["names"] + 1))
    blobs = [stored[i].lower().encode() for i in range(1, res["dns"]["names"] + 1)]  # pattern id = name id
    off = np.cumsum([0] + [len(b) for b in blobs], dtype=np.uint64)
    blob = np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()
    prow = np.zeros(len(recs), dtype=N.WL_ENDPOINT_DTYPE)
    prow["addr"], prow["family"], prow["protocol"], prow["port"] = recs["dst_ip"], recs["family"], recs["protocol"], recs["dst_port"]
    prow["prefix"] = np.where(recs["family"] == 2, 32, 128)
    prow["flags"] = N.FB_WL_HAS_PORT | np.where(recs["dst_name_id"] != 0, N.FB_WL_HAS_DOMAIN, 0).astype(np.uint8)
    epp = np.ascontiguousarray(recs["dst_name_id"], dtype=np.uint32)
    res["d_endpoints"], res["d_endpoints_with_domain"], res["patterns"] = len(prow), int((epp != 0).sum()), len(blobs)

    def install():
        N.check(lib.fb_set_whitelist_dom(cap.ctx, N.ptr(prow), len(prow), N.ptr(epp), N.ptr(blob), N.ptr(off), len(blobs),
                                         None, None, 0))

    t0 = time.perf_counter()
    install()
    res["d_install_us"] = (time.perf_counter() - t0) * 1e6

    # (c) every name against the patterns; then 1 % more
    none = N.DeviceBuffer(64)

    def match_all():
        N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_WL_NAME_HASH_MASK, 0))  # forgets the rows
        N.check(lib.fb_stream_sync(None))
        t0 = time.perf_counter()
        N.check(lib.fb_wl_name_matches_dev(cap.ctx, none.ptr, 0, none.ptr, none.ptr, None))
        return (time.perf_counter() - t0) * 1e6

    res["c_match_all_names"] = [med([match_all() for _ in range(a.reps)][2:]) for _ in range(a.repeats)]
    res["c_info"] = cap.whitelist_domain_info()
    # (d) the pass with pattern ids
    res["d_stats"] = cap.whitelist_pass()
    res["d_pass"] = [events(cap.whitelist_pass, 3, a.reps) for _ in range(a.repeats)]
    extra = max(n_names // 100, 1)
    dst = np.concatenate([dst, dst[:extra * 8]])  # (the new names answer addresses that are resolved already)
    track(n_names, extra, 0x4000)
    N.check(lib.fb_stream_sync(None))
    t0 = time.perf_counter()
    N.check(lib.fb_wl_name_matches_dev(cap.ctx, none.ptr, 0, none.ptr, none.ptr, None))
    res["c_match_one_percent_new"] = dict(names=extra, us=(time.perf_counter() - t0) * 1e6)
    res["c_info_after"] = cap.whitelist_domain_info()
    cap.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("free", "all"), default="all")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)),
                    help="the tree flodbadd_amd is imported from (part free: the parent commit's build)")
    ap.add_argument("--label", default="branch", help="what the result calls the tree it ran from")
    ap.add_argument("--frames", type=int, default=10 * (1 << 20))
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.root = os.path.abspath(a.root)
    sys.path.insert(0, a.root)
    res = run(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        prev = json.load(open(a.out)) if os.path.exists(a.out) else []
        with open(a.out, "w") as f:
            json.dump(prev + [res], f, indent=1)


if __name__ == "__main__":
    main()
