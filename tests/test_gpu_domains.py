"""The domain pass (fb_flow_domains) against tests/domref.py -- populate_domain_names restated -- run over the
exported flows, the status bytes and dns_resolutions(): the ids each pass writes, its counters, its stamps,
and the plane through growth, purge and the two clears; then end to end from frames."""
import ipaddress
import json
import os
import struct

import numpy as np
import pytest

import dnsgen as G
import dnstrackgen as T
import domref
import framegen as fg
import joinref
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.dns import DnsResolver
from flodbadd_amd.sessions import Protocol, Session, SessionFilter, SessionPacketData, WhitelistState

pytestmark = pytest.mark.gpu

S = 10 ** 9
T0 = 1_700_000_000 * S
HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "domain_kats.json")))["cases"]


def pkt(proto, sip, sport, dip, dport):
    s = Session(Protocol[proto], ipaddress.ip_address(sip), sport, ipaddress.ip_address(dip), dport)
    return SessionPacketData(s, 100, 140, 0x10 if proto == "TCP" else None)


def capture(timed=False, **kw):
    kw.setdefault("flow_capacity", 1 << 9)
    return T.new_capture(timed=timed, **kw)


def resolve(cap, ref, mapping, tx0=0):
    """Track one query + response per {ip: name}, compared with DnsResolver as every tracking call is."""
    b = T.Batch()
    for k, (ip, name) in enumerate(mapping.items()):
        b.query(tx0 + k, name).response(tx0 + k, [ip])
    T.step(cap, ref, b)


def plane_names(cap):
    ids = cap.domain_ids()
    names = cap.dns_names(np.unique(np.concatenate([ids["src_name_id"], ids["dst_name_id"]])))
    return ids, names


def run_pass(cap):
    """One domain pass checked against domref over the capture's own exports; returns (counters, {slot:
    session dict after the pass}, the modified slots)."""
    flows = cap.export_flows(SessionFilter.All)
    status = cap.status_bytes() if cap.timed else None
    ids, names = plane_names(cap)
    sessions, current = {}, []
    for r in flows:
        slot, s = int(r["slot"]), Session.from_key(r)
        a, b = int(ids[slot]["src_name_id"]), int(ids[slot]["dst_name_id"])
        sessions[slot] = {"session": s, "src_ip": s.src_ip, "dst_ip": s.dst_ip, "src_domain": names[a] if a else None,
                          "dst_domain": names[b] if b else None, "last_modified": 0}
        if status is None or domref.is_current(int(status[slot])):
            current.append(slot)
    before = {k: (v["src_domain"], v["dst_domain"]) for k, v in sessions.items()}
    modified = set(domref.populate_domain_names(sessions, current, cap.dns_resolutions(), now=1))
    st = cap.update_domains()
    ids, names = plane_names(cap)
    got = {slot: (names[int(ids[slot]["src_name_id"])] if int(ids[slot]["src_name_id"]) else None,
                  names[int(ids[slot]["dst_name_id"])] if int(ids[slot]["dst_name_id"]) else None) for slot in sessions}
    assert got == {k: (v["src_domain"], v["dst_domain"]) for k, v in sessions.items()}
    occupied = np.zeros(len(ids), dtype=bool)
    occupied[list(sessions)] = True
    assert not ids["src_name_id"][~occupied].any() and not ids["dst_name_id"][~occupied].any()
    assert st == {"flows": len(sessions), "current": len(current), "changed": len(modified),
                  "src_set": sum(1 for k in modified if got[k][0] != before[k][0]),
                  "dst_set": sum(1 for k in modified if got[k][1] != before[k][1]),
                  "with_domain": sum(1 for v in got.values() if v[0] or v[1])}
    return st, sessions, modified


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_fixture_cases_on_the_device(case):
    """domain_kats.json: the sessions' earlier domains come from a first pass over earlier resolutions, the
    sessions the case calls non-current are aged out of current_sessions (180 s) before the pass."""
    cap, ref = capture(timed=True)
    try:
        pk = [pkt(*s[:5]) for s in case["sessions"]]
        ts = np.array([T0 + (150 * S if s[5] else 0) + k for k, s in enumerate(case["sessions"])], dtype=np.uint64)
        cap.process_parsed(pk, ts=ts)
        earlier = {}
        for s in case["sessions"]:
            earlier.update({ip: dom for ip, dom in ((s[1], s[6]), (s[3], s[7])) if dom})
        if earlier:
            resolve(cap, ref, earlier)
            run_pass(cap)
        cap.update_sessions_status(T0 + 200 * S, purge=False)
        resolve(cap, ref, case["resolutions"], tx0=100)
        _, sessions, modified = run_pass(cap)
        by_key = {v["session"]: (k, v) for k, v in sessions.items()}
        for s, p, (sdom, ddom, mod) in zip(case["sessions"], pk, case["expect"]):
            fwd = p.session in by_key
            slot, v = by_key[p.session if fwd else p.session.reversed()]
            want = (sdom, ddom) if fwd else (ddom, sdom)
            assert (v["src_domain"], v["dst_domain"]) == want and (slot in modified) == mod, (s, v)
        infos = {i.session: i for i in cap.get_sessions()}
        for v in sessions.values():
            assert (infos[v["session"]].src_domain, infos[v["session"]].dst_domain) == (v["src_domain"], v["dst_domain"])
    finally:
        cap.close()


def test_pass_behaviour_and_stamps():
    cap, ref = capture()
    try:
        cap.process_parsed([pkt("TCP", "10.1.0.1", 40001, "198.51.100.1", 443),   # dst resolves
                            pkt("TCP", "198.51.100.2", 40002, "10.1.0.2", 8080),   # src resolves
                            pkt("UDP", "198.51.100.3", 40003, "198.51.100.1", 443),  # both
                            pkt("TCP", "10.1.0.4", 40004, "198.51.100.4", 443),    # dst is the literal Unknown
                            pkt("TCP", "198.51.100.5", 40005, "10.1.0.5", 8080),   # src is the literal Resolving
                            pkt("TCP", "10.1.0.6", 40006, "10.1.0.7", 8080)])      # neither
        resolve(cap, ref, {"198.51.100.1": "one.example", "198.51.100.2": "two.example", "198.51.100.3": "three.example",
                           "198.51.100.4": "Unknown", "198.51.100.5": "Resolving"})
        cap.set_pass_time(T0 + 1)
        st, sessions, modified = run_pass(cap)
        assert (st["changed"], st["src_set"], st["dst_set"], st["with_domain"]) == (3, 2, 2, 3)
        stamps = cap.modified_stamps()
        assert {int(i) for i in np.nonzero(stamps)[0]} == modified and set(stamps[list(modified)].tolist()) == {T0 + 1}
        # a second pass with nothing new: nothing changes and no stamp moves
        cap.set_pass_time(T0 + 2)
        st, _, modified2 = run_pass(cap)
        assert st["changed"] == 0 and not modified2 and (cap.modified_stamps() == stamps).all()
        # re-resolving an address to another name updates its flows and stamps them
        resolve(cap, ref, {"198.51.100.1": "uno.example"}, tx0=50)
        cap.set_pass_time(T0 + 3)
        st, sessions, modified3 = run_pass(cap)
        assert st["changed"] == 2 and st["dst_set"] == 2 and st["src_set"] == 0
        now = cap.modified_stamps()
        assert set(now[list(modified3)].tolist()) == {T0 + 3}
        rest = [k for k in sessions if k not in modified3]
        assert (now[rest] == stamps[rest]).all()
        # without a pass time the pass stamps nothing
        resolve(cap, ref, {"198.51.100.2": "dos.example"}, tx0=60)
        cap.set_pass_time(0)
        st, _, _ = run_pass(cap)
        assert st["changed"] == 1 and (cap.modified_stamps() == now).all()
    finally:
        cap.close()


def test_current_only_and_incremental_sessions():
    """A timed capture aged so that half of its sessions are not current: those get no domains; the changed
    ones carry the pass time, and the incremental getter returns exactly them, with their domains."""
    cap, ref = capture(timed=True)
    try:
        pk = [pkt("TCP", "10.2.0.%d" % i, 41000 + i, "203.0.113.%d" % (i % 4), 443) for i in range(40)]
        ts = np.array([T0 + (150 * S if i % 2 else 0) + i for i in range(40)], dtype=np.uint64)
        cap.process_parsed(pk, ts=ts)
        t1 = T0 + 200 * S
        full = cap.get_sessions(now_ns=t1)  # ages the table and moves the getter's fetch timestamp
        assert len(full) == 40 and all(i.dst_domain is None for i in full)
        resolve(cap, ref, {"203.0.113.0": "zero.example", "203.0.113.1": "one.example", "203.0.113.2": "two.example"})
        cap.set_pass_time(t1 + S)
        st, sessions, modified = run_pass(cap)
        assert st["current"] == 20 and st["changed"] == 10 and st["dst_set"] == 10  # odd i: hosts .1 and .3, .3 unresolved
        stamps = cap.modified_stamps()
        assert {int(i) for i in np.nonzero(stamps)[0]} == modified
        inc = cap.get_sessions(incremental=True)
        assert sorted(i.session.sort_key() for i in inc) == sorted(sessions[k]["session"].sort_key() for k in modified)
        assert all(i.dst_domain == "one.example" and i.src_domain is None and i.last_modified_ns == t1 + S for i in inc)
        cur = cap.get_current_sessions(incremental=True)
        assert len(cur) == 20 and sum(1 for i in cur if i.dst_domain) == 10
        # the full fetches against the separate exports joined on the host, domains included
        full = cap.get_sessions()
        joinref.assert_same(full, joinref.sessions(cap, "sessions"), "sessions")
        assert len(full) == 40 and sum(1 for i in full if i.dst_domain) == 10
        full = cap.get_current_sessions()
        joinref.assert_same(full, joinref.sessions(cap, "current"), "current")
        assert [info.__dict__ for info in full] == [info.__dict__ for info in cur]
    finally:
        cap.close()


def test_plane_follows_growth_and_purge_and_the_clears():
    cap, ref = capture(timed=True, flow_capacity=1 << 9)
    try:
        def domains_by_key():
            flows = cap.export_flows(SessionFilter.All)
            ids, names = plane_names(cap)
            return {Session.from_key(r): (names.get(int(ids[int(r["slot"])]["src_name_id"])),
                                          names.get(int(ids[int(r["slot"])]["dst_name_id"]))) for r in flows}

        old = [pkt("TCP", "10.3.0.%d" % i, 42000 + i, "192.0.2.%d" % (i % 8), 443) for i in range(100)]
        new = [pkt("TCP", "10.3.1.%d" % i, 43000 + i, "192.0.2.%d" % (8 + i % 8), 443) for i in range(100)]
        cap.process_parsed(old, ts=np.full(100, T0, dtype=np.uint64))
        cap.process_parsed(new, ts=np.full(100, T0 + 1000 * S, dtype=np.uint64))
        resolve(cap, ref, {"192.0.2.%d" % k: "host%d.example" % k for k in range(16)})
        st, _, _ = run_pass(cap)
        assert st["changed"] == 200
        want = domains_by_key()
        cap0 = cap.table_info()["capacity"]
        # growth: batches of new flows until the table has grown past its first capacity
        k = 0
        while cap.table_info()["capacity"] == cap0:
            more = [pkt("UDP", "10.4.%d.%d" % (k, i), 44000, "10.5.%d.%d" % (k, i), 5000) for i in range(250)]
            cap.process_parsed(more, ts=np.full(250, T0 + 1000 * S, dtype=np.uint64))
            k += 1
            assert k < 8
        got = domains_by_key()
        assert {s: got[s] for s in want} == want and all(v == (None, None) for s, v in got.items() if s not in want)
        # purge: the first hundred flows (idle since T0) go, the others keep their domains at their new slots
        age = cap.update_sessions_status(T0 + 1100 * S, purge=True, retention_s=500)
        assert age["purged"] == 100
        got = domains_by_key()
        keep = {p.session for p in new} | {p.session.reversed() for p in new}
        assert {s: v for s, v in got.items() if v != (None, None)} == {s: v for s, v in want.items() if s in keep}
        assert len([s for s in got if got[s] != (None, None)]) == 100
        run_pass(cap)  # (and the pass still agrees with the restatement on the re-packed table)
        # the tracker's clear zeroes the plane: its ids died with the store
        cap.clear_dns()
        ids = cap.domain_ids()
        assert not ids["src_name_id"].any() and not ids["dst_name_id"].any()
        ref2 = DnsResolver()
        resolve(cap, ref2, {"192.0.2.9": "again.example"})
        st, _, _ = run_pass(cap)
        assert st["changed"] > 0
        cap.clear_all_sessions()
        ids = cap.domain_ids()
        assert not ids["src_name_id"].any() and not ids["dst_name_id"].any()
    finally:
        cap.close()


def test_end_to_end_from_frames():
    """UDP and DNS-over-TCP frames plus session frames to the answered addresses through process_frames on a
    capture that tracks DNS: get_sessions shows the domains, update_sessions returns a "domains" entry, and a
    whitelist with a domain endpoint conforms without the caller passing dns_resolutions."""
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9, track_dns=True,
                             dns_name_capacity=64, dns_addr_capacity=64)
    try:
        q = G.query(0x42, "video.example.com")
        r = G.response(0x42, "video.example.com", [("A", "198.51.100.7"), ("AAAA", "2001:db8::7")])
        q2 = G.query(0x43, "tcp.example.com")
        r2 = G.response(0x43, "tcp.example.com", [("A", "203.0.113.9")])
        frames = [fg.eth(0x0800, fg.ipv4("10.0.0.2", "8.8.8.8", 17, fg.udp(5353, 53, q))),
                  fg.tcp_frame("10.0.0.3", 44000, "1.1.1.1", 443, fg.ACK, 20),
                  fg.eth(0x0800, fg.ipv4("8.8.8.8", "10.0.0.2", 17, fg.udp(53, 5353, r))),
                  fg.eth(0x0800, fg.ipv4("10.0.0.2", "9.9.9.9", 6, fg.tcp(40000, 53, fg.ACK | fg.PSH,
                                                                          struct.pack("!H", len(q2)) + q2))),
                  fg.eth(0x0800, fg.ipv4("9.9.9.9", "10.0.0.2", 6, fg.tcp(53, 40000, fg.ACK | fg.PSH,
                                                                          struct.pack("!H", len(r2)) + r2))),
                  fg.tcp_frame("10.0.0.2", 45000, "198.51.100.7", 443, fg.ACK, 64),
                  fg.tcp_frame("10.0.0.2", 45001, "203.0.113.9", 443, fg.ACK, 64)]
        buf, offs = fg.pack(frames)
        res = cap.process(buf, offs)
        assert len(res.dns) == 4
        assert {str(k): v for k, v in cap.dns_resolutions().items()} == {
            "198.51.100.7": "video.example.com", "2001:db8::7": "video.example.com", "203.0.113.9": "tcp.example.com"}
        assert cap.dns_pending() == {}
        assert all(i.dst_domain is None for i in cap.get_sessions())  # no pass yet
        out = cap.update_sessions()
        assert set(out) == {"status", "blacklist", "whitelist", "domains"}
        assert out["domains"]["changed"] == 2 and out["domains"]["dst_set"] == 2 and out["domains"]["flows"] == 3
        dom = {str(i.session.dst_ip): (i.src_domain, i.dst_domain) for i in cap.get_sessions()}
        assert dom == {"1.1.1.1": (None, None), "198.51.100.7": (None, "video.example.com"),
                       "203.0.113.9": (None, "tcp.example.com")}
        wl = {"date": "today", "signature": None, "whitelists": [
            {"name": "custom_whitelist", "extends": None,
             "endpoints": [{"domain": "*.example.com", "port": 443}, {"ip": "1.1.1.1", "port": 443}]}]}
        cap.set_custom_whitelists(json.dumps(wl))
        out = cap.update_sessions()  # no dns_resolutions from the caller: the tracked ones
        assert out["whitelist"]["conforming"] == 3 and cap.get_whitelist_conformance()
        assert all(i.is_whitelisted is WhitelistState.Conforming for i in cap.get_sessions())
    finally:
        cap.close()


def test_tracking_off_changes_nothing():
    """update_sessions on a capture that does not track DNS: the three passes' counters as the separate calls
    give them, "domains": None the only addition; the tracker's methods refuse, and nothing was allocated."""
    pk = [pkt("TCP", "10.6.0.%d" % i, 46000 + i, "203.0.113.%d" % i, 443) for i in range(20)]
    ts = np.array([T0 + i for i in range(20)], dtype=np.uint64)
    a = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9, timed=True)
    b = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9, timed=True)
    try:
        a.process_parsed(pk, ts=ts)
        b.process_parsed(pk, ts=ts)
        out = a.update_sessions(T0 + 100 * S)
        b.set_pass_time(T0 + 100 * S)
        want = {"status": b.update_sessions_status(T0 + 100 * S), "blacklist": b.update_blacklist(mark_whitelist=True),
                "whitelist": b.update_whitelist(None, None), "domains": None}
        assert out == want
        assert all(i.src_domain is None and i.dst_domain is None for i in a.get_sessions())
        with pytest.raises(ValueError):
            a.update_domains()
        assert N.gpu_lib().fb_flow_domains(a.ctx, 0, None, None) == N.FB_ERR_INVAL
        ids = a.domain_ids()
        assert len(ids) == a.table_info()["capacity"] and not ids["src_name_id"].any()
    finally:
        a.close()
        b.close()
