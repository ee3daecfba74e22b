"""The view export and the stamped passes timed on the C4 table, and the parent commit's library against this
tree's on everything the change touches.

The table: flow_capacity 2^21, timed, two 10,485,760-frame C4 batches (about 1.46 M flows; table, time plane
and the other planes are ~420 MB, past the 256 MB Infinity Cache), 1,000 blacklist nets, the whitelist
learned from every other flow, a forest trained on 300 of the table's vectors.  Every figure is the median
of 20 calls under device events on the null stream after 3 warm-up calls; a "repeat" is one such median.

The driver starts one child process per side and round, parent and branch alternating, each child building
its own table and taking --repeats repeats of every row:

  1. no regression (pass time 0; both sides): fb_flow_blacklist (steady, steady with the fallback flag),
     fb_flow_whitelist, fb_flow_anomaly, and the device exports fb_flow_export_sessions_dev,
     fb_flow_export_times_dev, fb_flow_export_blacklisted_dev, fb_flow_export_whitelist_dev, plus the four
     plane copies.  limit = the parent's slowest repeat + the spread of the parent's repeats; ok = no
     branch repeat beyond it (the rule of profiles/plane_refactor_ab.json).
  2. view, all flows selected (branch), both copy-out shapes, against the sum of the parent's separate
     device exports it replaces: flow records + time records + the four plane copies.
  3. view with FB_VIEW_MODIFIED_SINCE selecting 0 %, ~1 % and 100 % (branch); and, once (--host, wall clock),
     get_sessions(incremental=True) at ~1 % against what get_sessions() moves to the host before its join --
     the parent's code path -- plus that join's cost on a 20,000-flow sample.
  4. the three passes with a pass time set (steady state: nothing changes, so the cost is the stamped
     instance's, not the stores'), against the same child's unstamped rows.

Usage: python tools/experiments/view_export_ab.py --parent-lib PARENT.so [--rounds 2] [--repeats 4] [--host]
       [--out profiles/view_export_ab.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

S = 10 ** 9
T0 = 1_700_000_000 * S


def child(a):
    from flodbadd_amd import _native as N
    if a.child == "parent":  # the parent's library lacks the new symbols: bind the ones it has
        have = C.CDLL(N.GPU_LIB_PATH)
        N.GPU_SYMBOLS = [s for s in N.GPU_SYMBOLS if hasattr(have, s[0])]
    from flodbadd_amd import analyzer as AN
    from flodbadd_amd import synth
    from flodbadd_amd.capture import FlodbaddGpuCapture
    from flodbadd_amd.sessions import SessionFilter
    from flodbadd_amd.whitelists import rows_from_flows

    lib, n, branch = N.gpu_lib(), a.frames, a.child == "branch"
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
    flows, times = cap.export_flows(), cap.export_times()
    nf, slots = len(flows), int(cap.table_info()["capacity"])
    bl = np.zeros(1000, dtype=N.CIDR_DTYPE)
    bl["addr"][:, 0] = (np.arange(1000, dtype=np.uint64) * 4194301 + (12 << 24)) & 0xFFFFFF00
    bl["family"], bl["prefix"], bl["list"] = 2, 24, np.arange(1000) % 8
    cap.set_blacklists(bl)
    cap.install_whitelist(rows_from_flows(flows[::2]))
    feats, _ = cap.export_features()
    data = feats[np.lexsort(feats.T[::-1])]
    data = data[::max(len(data) // AN.MAX_SAMPLES, 1)][:AN.MAX_SAMPLES]
    forest = AN.train_forest(data, 11)
    sc = np.sort(forest.score(data))
    cap.set_anomaly_model(forest, ([0.0] * 10, [0.0] * 10, False), (float(sc[int(0.7 * len(sc))]), float(sc[int(0.95 * len(sc))])))
    cap.update_sessions_status(T0 + 100 * S, purge=False)

    e0, e1 = N.Event(), N.Event()

    def once(fn):
        e0.record(None)
        fn()
        e1.record(None)
        return e0.elapsed_ms(e1) * 1000.0

    def repeat(fn, calls=20, warm=3):
        for _ in range(warm):
            fn()
        return round(statistics.median(once(fn) for _ in range(calls)), 2)

    d_n = N.DeviceBuffer(8)
    d_rec, d_time = N.DeviceBuffer(nf * 136), N.DeviceBuffer(nf * 64)
    d_mask, d_plane = N.DeviceBuffer(nf * 8), N.DeviceBuffer(slots * 16)
    rows = {
        "bl.steady": lambda: cap.update_blacklist(mark_whitelist=False),
        "bl.steady_mark": lambda: cap.update_blacklist(mark_whitelist=True),
        "wl.learned_half": cap.whitelist_pass,
        "an.pass": cap.anomaly_pass,
        "export.sessions": lambda: N.check(lib.fb_flow_export_sessions_dev(cap.ctx, 2, d_rec.ptr, nf, d_n.ptr, None)),
        "export.times": lambda: N.check(lib.fb_flow_export_times_dev(cap.ctx, d_time.ptr, nf, d_n.ptr, None)),
        "export.blacklisted": lambda: N.check(lib.fb_flow_export_blacklisted_dev(cap.ctx, d_rec.ptr, d_mask.ptr, nf, d_n.ptr, None)),
        "export.whitelist": lambda: N.check(lib.fb_flow_export_whitelist_dev(cap.ctx, N.FB_WL_CONFORMING, d_rec.ptr, nf, d_n.ptr, None)),
        "plane.status": lambda: N.check(lib.fb_flow_status_dev(cap.ctx, d_plane.ptr, slots, None)),
        "plane.whitelist": lambda: N.check(lib.fb_flow_whitelist_dev(cap.ctx, d_plane.ptr, slots, None)),
        "plane.blacklist": lambda: N.check(lib.fb_flow_blacklist_dev(cap.ctx, d_plane.ptr, slots, None)),
        "plane.anomaly": lambda: N.check(lib.fb_flow_anomaly_dev(cap.ctx, d_plane.ptr, slots, None)),
    }
    for fn in list(rows.values())[:4]:   # the first passes (every flow changes) are not the steady rows
        fn()
    res = dict(side=a.child, flows=nf, capacity=slots, rows={k: [] for k in rows})
    for _ in range(a.repeats):
        for k, fn in rows.items():
            res["rows"][k].append(repeat(fn))
    if branch:
        d_view = N.DeviceBuffer(nf * 256)
        q = np.zeros(1, dtype=N.VIEW_QUERY_DTYPE)
        q[0]["filter"] = N.FB_FILTER_ALL

        def view():
            N.check(lib.fb_flow_export_view_dev(cap.ctx, N.ptr(q), d_view.ptr, nf, d_n.ptr, None))

        def count():
            return int(d_n.download(np.zeros(1, dtype=np.uint64))[0])

        la = np.sort(times["last_activity_ns"])
        cuts = {"view.since_0pct": int(la[-1]), "view.since_1pct": int(la[int(0.99 * nf)]), "view.since_100pct": 0}
        extra = {k: [] for k in ("view.all_staged", "view.all_direct", *cuts, "bl.steady.stamped", "bl.steady_mark.stamped",
                                 "wl.learned_half.stamped", "an.pass.stamped")}
        res["selected"] = {}
        for _ in range(a.repeats):
            q[0]["flags"] = 0
            for knob, name in ((0, "view.all_staged"), (1, "view.all_direct")):
                N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_VIEW_DIRECT, knob))
                extra[name].append(repeat(view))
                assert count() == nf
            N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_VIEW_DIRECT, 0))
            q[0]["flags"] = N.FB_VIEW_MODIFIED_SINCE
            for name, since in cuts.items():
                q[0]["since_ns"] = since
                extra[name].append(repeat(view))
                res["selected"][name] = count()
            cap.set_pass_time(T0 + 200 * S)
            for k in ("bl.steady", "bl.steady_mark", "wl.learned_half", "an.pass"):
                extra[k + ".stamped"].append(repeat(rows[k]))
            cap.set_pass_time(0)
        res["rows"].update(extra)
        if a.host:
            # Wall clock.  The incremental call whole; of the full call the stage that moves the table to the
            # host (what get_sessions() exports before it joins), and the Python join on a 20,000-flow sample:
            # the join of all 1.46 M records in Python runs for many minutes and is the same code on both sides.
            from flodbadd_amd.sessions import flows_to_sessions
            cap.set_filter(SessionFilter.All)
            cap._fetch_ts["sessions"] = cuts["view.since_1pct"]
            t = time.perf_counter()
            inc = cap.get_sessions(incremental=True)
            t_inc = time.perf_counter() - t
            t = time.perf_counter()
            views = cap.export_view(N.FB_VIEW_ALL, cuts["view.since_1pct"], cap.filter)
            t_inc_move = time.perf_counter() - t
            t = time.perf_counter()
            fl, tm = cap.export_flows(cap.filter), cap.export_times()
            planes = (cap.status_bytes(), cap.whitelist_bytes(), cap.blacklist_masks(), cap.anomaly_records())
            t_move = time.perf_counter() - t
            t = time.perf_counter()
            sample = flows_to_sessions(fl[:20000], None, times=tm, status=planes[0], whitelist=planes[1],
                                       blacklist=(planes[2], [str(k) for k in range(64)]))
            t_join = time.perf_counter() - t
            res["host"] = dict(incremental_call_s=round(t_inc, 4), incremental_sessions=len(inc),
                               incremental_export_s=round(t_inc_move, 4), incremental_bytes=int(views.nbytes),
                               full_export_s=round(t_move, 4),
                               full_bytes=int(fl.nbytes + tm.nbytes + sum(p.nbytes for p in planes)),
                               full_join_sample_flows=len(sample), full_join_sample_s=round(t_join, 3),
                               full_flows=len(fl))
    print("RESULT " + json.dumps(res))
    cap.close()


def drive(a):
    env = dict(os.environ)
    runs = []
    for r in range(a.rounds):
        for side in ("parent", "branch"):
            e = dict(env)
            if side == "parent":
                e["FLODBADD_GPU_LIB"] = os.path.abspath(a.parent_lib)
            else:
                e.pop("FLODBADD_GPU_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--repeats", str(a.repeats),
                   "--frames", str(a.frames), "--capacity", str(a.capacity)]
            if a.host and side == "branch" and r == a.rounds - 1:
                cmd.append("--host")
            p = subprocess.run(cmd, env=e, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-4000:])
                raise SystemExit("child %s failed (exit %d)" % (side, p.returncode))
            runs.append(json.loads(line[-1][7:]))
            print(side, "round", r, "done", flush=True)
    pooled = {"parent": {}, "branch": {}}
    for run in runs:
        for k, v in run["rows"].items():
            pooled[run["side"]].setdefault(k, []).extend(v)
    out = dict(what=__doc__.split("\n\n")[1].replace("\n", " "), flows=runs[0]["flows"], capacity=runs[0]["capacity"],
               rounds=a.rounds, repeats_per_child=a.repeats, no_regression=[], branch_only={}, selected={}, host=None)
    for k, pv in sorted(pooled["parent"].items()):
        bv = pooled["branch"][k]
        spread = round(max(pv) - min(pv), 2)
        out["no_regression"].append(dict(row=k, parent_us=pv, branch_us=bv, parent_spread_us=spread,
                                         limit_us=round(max(pv) + spread, 2), branch_max_us=max(bv),
                                         ok=max(bv) <= max(pv) + spread))
    for k, bv in sorted(pooled["branch"].items()):
        if k not in pooled["parent"]:
            out["branch_only"][k] = bv
    for run in runs:
        out["selected"].update(run.get("selected", {}))
        out["host"] = run.get("host") or out["host"]
    med = lambda side, k: statistics.median(pooled[side][k])  # noqa: E731
    parts = ("export.sessions", "export.times", "plane.status", "plane.whitelist", "plane.blacklist", "plane.anomaly")
    ssum = round(sum(med("parent", k) for k in parts), 2)
    sspread = round(sum(max(pooled["parent"][k]) - min(pooled["parent"][k]) for k in parts), 2)
    out["view_vs_separate"] = dict(parent_sum_us=ssum, parent_sum_spread_us=sspread, parts=list(parts),
                                   view_all_staged_us=med("branch", "view.all_staged"),
                                   view_all_direct_us=med("branch", "view.all_direct"),
                                   ok=max(pooled["branch"]["view.all_staged"]) <= ssum + sspread)
    out["stamping_cost_us"] = {k: round(med("branch", k + ".stamped") - med("branch", k), 2)
                               for k in ("bl.steady", "bl.steady_mark", "wl.learned_half", "an.pass")}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(r["ok"] for r in out["no_regression"]) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--child", choices=("parent", "branch"))
    ap.add_argument("--frames", type=int, default=10 * (1 << 20))
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    return drive(a)


if __name__ == "__main__":
    sys.exit(main())
