"""The host join of sessions.py on hand-built records, no GPU: views_to_sessions against flows_to_sessions in
each of the argument shapes it documents (slot-indexed arrays, {slot: value} dicts, positional time records),
and both against tests/golden/sessions_join.json -- the lists the join gave before it was rewritten to work
from per-record columns (recorded by running this file as a script at that commit).  Every value is
an integer or a string: no tolerance."""
import json
import os

import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.sessions import Session, SessionStats, SessionStatus, WhitelistState, flows_to_sessions, views_to_sessions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sessions_join.json")
NREC, CAP = 300, 1 << 12
BL_NAMES = ["zeta", "alpha", "mid"]
DOM_NAMES = {1: "a.example", 2: "b.example", 7: "cdn.example.net"}
NONE = N.FB_SEEN_NONE
T0 = 1_700_000_000 * 10 ** 9


def build(n=NREC, cap=CAP):
    """(views, histories, domain plane): n flows in unsorted, non-contiguous slots of a cap-slot table."""
    rs = np.random.RandomState(20240607)
    v = np.zeros(n, dtype=N.FLOW_VIEW_DTYPE)
    slots = rs.permutation(cap)[:n].astype(np.uint32)
    assert (np.diff(slots.astype(np.int64)) < 0).any() and len(set(slots.tolist())) == n
    r, t = v["rec"], v["time"]
    r["slot"] = t["slot"] = slots
    v6 = np.arange(n) % 3 == 0
    r["family"] = np.where(v6, 10, 2)
    r["protocol"] = np.where(np.arange(n) % 4 == 1, 17, 6)
    for f in ("src_ip", "dst_ip"):
        w = rs.randint(0, 1 << 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
        w[~v6, 1:] = 0
        r[f] = w
    r["src_port"] = rs.randint(1024, 65536, n)
    r["dst_port"] = np.where(np.arange(n) % 5 == 0, rs.randint(1, 65536, n), np.take((443, 53, 22, 80, 8080), np.arange(n) % 5))
    for f in ("outbound_bytes", "inbound_bytes", "orig_pkts", "resp_pkts", "orig_ip_bytes", "resp_ip_bytes"):
        r[f] = rs.randint(0, 1 << 40, n, dtype=np.uint64)
    r["inbound_bytes"][::11] = 0
    r["first_seen"] = rs.randint(0, 1 << 34, n, dtype=np.uint64)
    r["last_seen"] = r["first_seen"] + rs.randint(0, 1 << 20, n, dtype=np.uint64)
    r["end_seen"] = np.where(np.arange(n) % 2 == 0, NONE, r["last_seen"])
    r["hist_len"] = rs.randint(0, 40, n)
    r["conn_state"] = np.arange(n) % len(N.CONN_STATES)
    r["session_flags"] = rs.randint(0, 32, n)
    r["segment_count"] = rs.randint(0, 9, n)
    r["in_segment"] = np.arange(n) % 3 == 1
    t["start_time_ns"] = T0 + rs.randint(0, 10 ** 9, n, dtype=np.uint64)
    t["last_activity_ns"] = t["start_time_ns"] + rs.randint(0, 10 ** 11, n, dtype=np.uint64)
    t["end_time_ns"] = np.where(np.arange(n) % 2 == 0, NONE, t["last_activity_ns"])
    t["current_segment_start_ns"] = t["start_time_ns"] + 5
    t["last_segment_end_ns"] = np.where(np.arange(n) % 3 == 0, NONE, t["last_activity_ns"] - 1)
    t["total_segment_interarrival_ms"] = rs.randint(0, 10 ** 6, n)
    t["segment_interarrival_div"] = rs.randint(0, 8, n)
    t["segment_count"], t["in_segment"] = r["segment_count"], r["in_segment"]
    # stamps: none, older than the last packet, newer than it
    v["stamp_ns"] = np.take((0, T0 - 1, T0 + 10 ** 12), np.arange(n) % 3) + np.where(np.arange(n) % 3, np.arange(n), 0)
    v["last_modified_ns"] = np.maximum(t["last_activity_ns"], v["stamp_ns"])
    v["bl_mask"] = np.take((0, 0, 1, 2, 5, 7, 4), np.arange(n) % 7)
    v["status"] = np.take((0, 1 | 2 | 4, 1 | 16 | 128, 8 | 128, 1 | 2 | 4 | 16 | 128, 128), np.arange(n) % 6)
    v["wl_state"] = np.take((0, N.FB_WL_CONFORMING, N.FB_WL_NONCONFORMING, N.FB_WL_NONCONFORMING | N.FB_WL_BLACKLISTED,
                             N.FB_WL_NONCONFORMING | N.FB_WL_HOST_CHECK, N.FB_WL_MASK_UNKNOWN), np.arange(n) % 6)
    assert (v["status"] == 0).any() and (v["bl_mask"] == 0).any() and (v["wl_state"] & N.FB_WL_BLACKLISTED).any()
    histories = {int(s): "ShAD"[: k % 5] for k, s in enumerate(slots) if k % 4}
    dom = np.zeros((cap, 2), dtype=np.uint32)
    dom[slots, 0] = np.take((0, 1, 2, 7), np.arange(n) % 4)
    dom[slots, 1] = np.take((7, 0, 0, 2, 1), np.arange(n) % 5)
    dom[np.setdiff1d(np.arange(cap), slots)] = 99          # a slot no record names is never read
    return v, histories, dom


def plain(i):
    """A SessionInfo as JSON-ready values, every field: {field: value}, the stats and the status as value lists in
    the order of their dataclass fields (the recorded file stays small)."""
    s = i.session
    return dict(i.__dict__, session=[s.protocol.name, str(s.src_ip), s.src_port, str(s.dst_ip), s.dst_port],
                stats=list(i.stats.__dict__.values()), status=None if i.status is None else list(i.status.__dict__.values()),
                is_whitelisted=i.is_whitelisted.name)


def rows(infos):
    """... as the recorded file holds a list: one value list per session, fields in SessionInfo's order."""
    return [list(plain(i).values()) for i in infos]


def planes(v, as_dict):
    """The per-slot arguments of flows_to_sessions for the views: arrays of CAP slots, or {slot: value}."""
    sl = v["rec"]["slot"]
    if as_dict:
        return {f: dict(zip(sl.tolist(), v[f].tolist())) for f in ("status", "wl_state", "bl_mask", "stamp_ns")}
    out = {}
    for f in ("status", "wl_state", "bl_mask", "stamp_ns"):
        a = np.full(CAP, 0xEE, dtype=v[f].dtype)                  # (what a slot without a record holds is never read)
        a[sl] = v[f]
        out[f] = a
    return out


def all_ways(v, histories, dom):
    """{name: list} of the full join through views_to_sessions and through flows_to_sessions in its three shapes."""
    flows, times = np.ascontiguousarray(v["rec"]), np.ascontiguousarray(v["time"])
    out = {"views": views_to_sessions(v, histories, BL_NAMES, domains=(dom, DOM_NAMES))}
    for name, as_dict in (("arrays", False), ("dicts", True)):
        p = planes(v, as_dict)
        d = {int(s): dom[s] for s in flows["slot"]} if as_dict else dom
        out[name] = flows_to_sessions(flows, histories, times[::-1], status=p["status"], whitelist=p["wl_state"],
                                      blacklist=(p["bl_mask"], BL_NAMES), modified=p["stamp_ns"], domains=(d, DOM_NAMES))
    positional = times.copy()
    positional["slot"] = 0                                        # the kat.py form: one per flow, in `flows` order
    p = planes(v, False)
    out["positional"] = flows_to_sessions(flows, histories, positional, p["status"], p["wl_state"], (p["bl_mask"], BL_NAMES),
                                          p["stamp_ns"], (dom, DOM_NAMES))
    return out


def bare(v):
    return views_to_sessions(v, None, BL_NAMES, timed=False, status=False, whitelist=False, blacklist=False)


def test_every_shape_gives_the_recorded_join():
    v, histories, dom = build()
    with open(GOLDEN) as f:
        gold = json.load(f)
    for name, got in all_ways(v, histories, dom).items():
        assert len(got) == NREC
        assert rows(got) == gold["full"], name
    assert [i.session.sort_key() for i in got] == sorted(i.session.sort_key() for i in got)
    # what the records were built to contain comes out
    assert {i.is_whitelisted for i in got} == set(WhitelistState)
    assert sum(i.whitelist_reason == "Session is blacklisted" for i in got) == NREC // 6
    assert "" in {i.criticality for i in got} and "blacklist:alpha,blacklist:mid,blacklist:zeta" in {i.criticality for i in got}
    assert any(i.stats.end_time_ns is None for i in got) and any(i.stats.last_segment_end_ns is None for i in got)
    assert any(i.src_domain is None and i.dst_domain for i in got) and any(i.src_domain and i.dst_domain is None for i in got)
    assert any(i.last_modified_ns > i.stats.last_activity_ns for i in got)
    assert any(i.last_modified_ns == i.stats.last_activity_ns for i in got)
    assert any(i.status == SessionStatus() for i in got)       # byte 0: the insert status
    # flows only: the same list through both functions
    flows = np.ascontiguousarray(v["rec"])
    assert rows(bare(v)) == rows(flows_to_sessions(flows, modified=planes(v, False)["stamp_ns"])) == gold["bare"]
    assert all(i.last_modified_ns == 0 for i in flows_to_sessions(flows))
    assert flows_to_sessions(flows[:0], times=v["time"][:0]) == [] and views_to_sessions(v[:0]) == []


def test_switches_leave_the_defaults():
    v, histories, dom = build()
    full = views_to_sessions(v, histories, BL_NAMES, domains=(dom, DOM_NAMES))
    time_fields = ("start_time_ns", "last_activity_ns", "end_time_ns", "current_segment_start_ns", "last_segment_end_ns",
                   "total_segment_interarrival_ms", "segment_interarrival_div")
    default = SessionStats()
    stamps = dict(zip(v["rec"]["slot"].tolist(), v["stamp_ns"].tolist()))
    for off in ("timed", "status", "whitelist", "blacklist"):
        got = views_to_sessions(v, histories, BL_NAMES, domains=(dom, DOM_NAMES), **{off: False})
        assert [i.session for i in got] == [i.session for i in full]
        for g, f in zip(got, full):
            want = plain(f)
            if off == "timed":       # no time fields, so no status either, and the stamp alone is last_modified
                assert all(getattr(g.stats, k) == getattr(default, k) for k in time_fields) and g.status is None
                names = list(f.stats.__dict__)
                for k in time_fields:
                    want["stats"][names.index(k)] = getattr(default, k)
                want["status"] = None
                want["last_modified_ns"] = g.last_modified_ns
            elif off == "status":
                assert g.status is None
                want["status"] = None
            elif off == "whitelist":
                assert g.is_whitelisted is WhitelistState.Unknown and g.whitelist_reason is None
                want["is_whitelisted"], want["whitelist_reason"] = "Unknown", None
            else:
                assert g.criticality == ""
                want["criticality"] = ""
            assert plain(g) == want, off
    # untimed: last_modified_ns is the stamp of the session's own slot
    untimed = views_to_sessions(v, timed=False)
    order = sorted(range(NREC), key=lambda k: Session.from_key(v["rec"][k]).sort_key())
    assert [i.last_modified_ns for i in untimed] == [stamps[int(v["rec"]["slot"][k])] for k in order]
    assert all(i.src_domain is None and i.dst_domain is None and i.stats.history == "" for i in untimed)


if __name__ == "__main__":  # record the lists (run at the commit whose join is to be pinned)
    v, histories, dom = build()
    ways = all_ways(v, histories, dom)
    full = rows(ways["arrays"])
    assert all(rows(w) == full for w in ways.values())
    with open(GOLDEN, "w") as f:
        json.dump({"fields": list(plain(ways["arrays"][0])), "full": full, "bare": rows(bare(v))}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
