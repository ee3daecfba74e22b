"""Session getters on the view export: what a full getter call costs, against the join of the separate exports.

  host  (no GPU)  flows_to_sessions(flows, times=...) and views_to_sessions(views) on the synthetic records of
        tests/test_sessions_join.py at 2,000 / 8,000 / 32,000 flows: microseconds per flow, --repeats calls each,
        sizes interleaved.  --parent-root DIR times the package of another checkout (the parent commit's) beside
        this tree's, in the same process and on the same records.
  gpu   in one process, tests/joinref.py's list for "sessions" (flow records, time records and the whole-capacity
        planes joined by flows_to_sessions -- the path the getters took before) against cap.get_sessions(),
        alternating, on a timed capture with 20,000 flows in a 2^15-slot and in a 2^21-slot table.  A repeat is the
        median of 5 calls; 4 repeats per side.  limit = the baseline's slowest repeat plus the spread of its
        repeats; ok = the branch's median within it (the rule of profiles/plane_refactor_ab.json).

Usage: python tools/experiments/getter_paths_ab.py host [--parent-root DIR] [--repeats 5] [--out FILE]
       python tools/experiments/getter_paths_ab.py gpu [--flows 20000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
S = 10 ** 9
T0 = 1_700_000_000 * S


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def load_sessions(root, name):
    """The sessions module of the flodbadd_amd package under root, imported under the package name `name` (the
    package's imports are relative), so that two checkouts' joins run side by side in one process."""
    import importlib
    import importlib.util
    init = os.path.join(os.path.abspath(root), "flodbadd_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, init, submodule_search_locations=[os.path.dirname(init)])
    sys.modules[name] = mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return importlib.import_module(name + ".sessions")


def host(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    from test_sessions_join import BL_NAMES, build
    sides = {"branch": load_sessions(ROOT, "flodbadd_amd")}
    if a.parent_root:
        sides["parent"] = load_sessions(a.parent_root, "flodbadd_amd_parent")
    sizes = (2000, 8000, 32000)
    data = {n: build(n, 1 << 16)[0] for n in sizes}
    us = {side: {row: {str(n): [] for n in sizes} for row in ("flows_to_sessions", "flows_to_sessions_untimed",
                                                                "views_to_sessions")} for side in sides}
    for _ in range(a.repeats):          # sizes and sides interleaved: a slow minute of the machine hits them all
        for n in sizes:
            views = data[n]
            flows, times = np.ascontiguousarray(views["rec"]), np.ascontiguousarray(views["time"])
            for side, m in sides.items():
                rows = {"flows_to_sessions": lambda: m.flows_to_sessions(flows, times=times),
                        "flows_to_sessions_untimed": lambda: m.flows_to_sessions(flows),
                        "views_to_sessions": lambda: m.views_to_sessions(views, None, BL_NAMES)}
                for row, fn in rows.items():
                    t, out = wall(fn)
                    assert len(out) == n
                    us[side][row][str(n)].append(round(t / n * 1e6, 2))
    res = dict(what=__doc__.split("\n\n")[1].split("  gpu ")[0].replace("\n", " ").strip(), repeats=a.repeats,
               us_per_flow=us,
               median_us_per_flow={side: {row: {n: statistics.median(v) for n, v in by_n.items()} for row, by_n in rows.items()}
                                   for side, rows in us.items()})
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def gpu(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import joinref
    from flodbadd_amd import _native as N
    from flodbadd_amd.capture import FlodbaddGpuCapture
    from flodbadd_amd.sessions import SessionFilter

    n = a.flows
    pk = np.zeros(n, dtype=N.PARSED_DTYPE)              # one TCP SYN per flow, global IPv4 destinations
    pk["src_ip"][:, 0], pk["dst_ip"][:, 0] = 0xC0A80109, 0x14000001 + np.arange(n, dtype=np.uint32)
    pk["src_port"], pk["dst_port"] = 40000 + np.arange(n) % 20000, 443
    pk["protocol"], pk["family"], pk["has_flags"], pk["tcp_flags"] = 6, 2, 1, 2
    pk["packet_length"], pk["ip_packet_length"], pk["pkt_index"] = 100, 140, np.arange(n)
    out = dict(what=__doc__.split("\n\n")[1].split("  gpu ")[1].replace("\n", " "), flows=n, tables=[])
    for capacity in (1 << 15, 1 << 21):
        cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=capacity, timed=True, grow=False,
                                 max_batch_packets=n)
        cap.process_parsed(pk, ts=T0 + np.arange(n, dtype=np.uint64) * 1000)
        cap.set_custom_blacklists(json.dumps({"date": "d", "signature": "s", "blacklists": [
            {"name": "a", "ip_ranges": ["20.0.0.0/18"]}]}))
        cap.update_sessions(T0 + 10 * S)                # status, masks, stamps: every plane is decoded
        sides = {"joinref": lambda: joinref.sessions(cap, "sessions"), "get_sessions": cap.get_sessions}
        assert [i.session for i in sides["joinref"]()] == [i.session for i in sides["get_sessions"]()] and cap.flow_count() == n
        ms = {k: [] for k in sides}
        for _ in range(4):
            for k, fn in sides.items():
                ms[k].append(round(statistics.median(wall(fn)[0] for _ in range(5)) * 1e3, 1))
        base, got = ms["joinref"], ms["get_sessions"]
        spread = round(max(base) - min(base), 1)
        out["tables"].append(dict(capacity=capacity, joinref_ms=base, get_sessions_ms=got, joinref_spread_ms=spread,
                                  limit_ms=round(max(base) + spread, 1), get_sessions_median_ms=statistics.median(got),
                                  ok=statistics.median(got) <= max(base) + spread))
        cap.close()
        print("capacity", capacity, "done", flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if all(t["ok"] for t in out["tables"]) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("host", "gpu"))
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--flows", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    return host(a) if a.mode == "host" else gpu(a)


if __name__ == "__main__":
    sys.exit(main())
