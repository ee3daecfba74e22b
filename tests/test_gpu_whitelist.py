"""Whitelist conformance on the GPU (fb_set_whitelist / fb_flow_whitelist, flodbadd_amd/csrc/fb_whitelist.hip)
against the restatement of the reference's check in tests/wlref.py (src/whitelists.rs:341-732, 810-1023):
every state byte, every counter and the sorted exception list with its reasons must be equal -- no
tolerance applies.  The table: a C4-mix synthetic batch (IPv4 / IPv6, TCP / UDP, LAN and global
destinations) plus a few hand-made sessions, in a 2^11-slot (4-partition) table."""
import functools
import ipaddress
import json
import os

import numpy as np
import pytest

import wlref
from flodbadd_amd import _native as N
from flodbadd_amd import synth
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.sessions import Protocol, Session, SessionFilter, SessionPacketData, WhitelistState
from flodbadd_amd.whitelists import rows_from_flows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "whitelist_kats.json")))["cases"]
S = 10 ** 9
T0 = 1_700_000_000 * S


@functools.lru_cache(maxsize=None)
def batch(n, first, n_flows):
    fr, of = synth.generate(4, n, first=first, n_flows=n_flows, lan_dst_permille=300)
    fr.setflags(write=False)
    of.setflags(write=False)
    return fr, of


def pkt(proto, src, sport, dst, dport):
    s = Session(Protocol[proto], ipaddress.ip_address(src), sport, ipaddress.ip_address(dst), dport)
    return SessionPacketData(s, 100, 120, 2 if proto == "TCP" else None)


# (source ports the service table does not name, so no key is reversed: src/packets.rs:245-253)
# v6 destinations that differ only in the first word / only in the last, one address under several ports
HAND = [pkt("TCP", "fd00::5", 61001, "2001:db8::1", 443), pkt("TCP", "fd00::5", 61002, "2001:db8::2", 443),
        pkt("TCP", "fd00::5", 61003, "3001:db8::1", 443), pkt("UDP", "fd00::5", 61004, "2001:db8::1", 443),
        pkt("TCP", "192.168.7.7", 61005, "93.184.216.34", 80), pkt("TCP", "192.168.7.7", 61006, "93.184.216.34", 81),
        pkt("TCP", "192.168.7.7", 61007, "93.184.216.34", 8080), pkt("UDP", "192.168.7.7", 61008, "93.184.216.34", 80)]


def keyb(recs):
    a = np.ascontiguousarray(recs)
    return [bytes(r) for r in a.view(np.uint8).reshape(len(a), -1)[:, :40]]


def make_asn(flows):
    """A small synthetic ASN table over the table's own destinations: the /8 of some IPv4 destinations
    (10/8 among them: a LAN destination has no dst_asn whatever the table says) and the first-word /32 of
    some IPv6 ones -> (v4 array, v6 array, records, wlref's sorted range lists)."""
    tops = sorted({int(r["dst_ip"][0]) >> 24 for r in flows if r["family"] == 2})
    tops = sorted(set(tops[::3][:14]) | {10, 93})
    w0 = sorted({int(r["dst_ip"][0]) for r in flows if r["family"] == 10})[::2][:8]
    recs, v4, v6 = [], np.zeros(len(tops), dtype=N.ASN_RANGE_DTYPE), np.zeros(len(w0), dtype=N.ASN_RANGE_DTYPE)
    for i, a in enumerate(tops):
        v4[i]["start"], v4[i]["end"] = (a << 24, 0, 0, 0), (a << 24 | 0xFFFFFF, 0, 0, 0)
        v4[i]["as_number"], v4[i]["record"] = 64500 + i % 5, len(recs)
        recs.append((64500 + i % 5, ("US", "FR", "de")[i % 3], ("Alpha Net", "BETA Corp", "gamma")[i % 3] + " %d" % (i % 2)))
    for i, w in enumerate(w0):
        v6[i]["start"], v6[i]["end"] = (w, 0, 0, 0), (w, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
        v6[i]["as_number"], v6[i]["record"] = 64600 + i % 3, len(recs)
        recs.append((64600 + i % 3, ("US", "jp")[i % 2], "Six Net %d" % (i % 2)))
    r4 = [(int(x["start"][0]), int(x["end"][0]), int(x["record"])) for x in v4]
    r6 = [(int(x["start"][0]) << 96, (int(x["start"][0]) << 96) | ((1 << 96) - 1), int(x["record"])) for x in v6]
    return v4, v6, recs, r4, r6


class World:
    pass


@pytest.fixture(scope="module")
def world():
    w = World()
    w.cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11)
    fr, of = batch(1800, 0, 420)
    w.cap.process_frames(fr, of)
    w.cap.process_parsed(HAND)
    w.flows = w.cap.export_flows()
    assert 500 <= len(w.flows) <= 1500, len(w.flows)
    w.v4, w.v6, w.records, w.r4, w.r6 = make_asn(w.flows)
    w.cap.set_asn_tables(w.v4, w.v6, w.records)
    w.sessions = [Session.from_key(r) for r in w.flows]
    fam = w.flows["family"]
    assert (fam == 2).sum() > 100 and (fam == 10).sum() > 50 and len(set(w.flows["protocol"].tolist())) == 2
    lan = sum(1 for s in w.sessions if wlref.is_lan_ip(s.dst_ip))
    assert 50 < lan < len(w.flows) - 50
    w.d4 = sorted({s.dst_ip for s in w.sessions if s.dst_ip.version == 4})
    w.d6 = sorted({s.dst_ip for s in w.sessions if s.dst_ip.version == 6})
    yield w
    w.cap.close()


def model(eps, name="custom_whitelist", extra=()):
    return {"date": "today", "signature": None,
            "whitelists": [{"name": name, "extends": None, "endpoints": list(eps)}] + list(extra)}


def compare(w, m, name, stats, dns=None, procs=None, asn=True, prev=None):
    """The capture's state after a pass equals the restatement: bytes, counters, exceptions, reasons."""
    want = wlref.session_states(w.flows, m, name, w.r4 if asn else (), w.r6 if asn else (), w.records, dns, procs)
    sb = w.cap.whitelist_bytes()
    got = {k: int(sb[s]) for k, s in zip(keyb(w.flows), w.flows["slot"].tolist())}
    exp = {k: v[0] for k, v in want.items()}
    bad = [(want[k][3], got[k], exp[k]) for k in exp if got[k] != exp[k]]
    assert not bad, (len(bad), bad[:5])
    v = list(exp.values())
    wst = dict(flows=len(v), conforming=sum(1 for b in v if b & 1), nonconforming=sum(1 for b in v if b & 2),
               host_check=sum(1 for b in v if b & 4))
    wst["changed"] = len(v) if prev is None else sum(1 for k in exp if exp[k] != prev[k])
    print("whitelist pass:", stats, "restatement:", wst)
    assert stats == wst
    wexc = sorted((x for x in want.values() if not x[1]), key=lambda x: x[3].sort_key())
    gexc = w.cap.get_whitelist_exceptions()
    assert [i.session for i in gexc] == [x[3] for x in wexc]
    assert [i.whitelist_reason for i in gexc] == [x[2] for x in wexc]
    assert all(i.is_whitelisted is WhitelistState.NonConforming for i in gexc)
    assert w.cap.get_whitelist_conformance() is (not wexc)
    seen = {i.session: i.is_whitelisted for i in w.cap.get_sessions()}  # (the capture's filter is All)
    assert all(seen[x[3]] is (WhitelistState.Conforming if x[1] else WhitelistState.NonConforming) for x in want.values())
    assert int((sb != 0).sum()) == len(v)  # no byte outside the occupied slots
    return exp


def run(w, eps, dns=None, procs=None, asn=True):
    """Install `eps` as the custom list through the public methods, one pass, compare everything."""
    m = model(eps)
    stats = w.cap.set_custom_whitelists(json.dumps(m))
    assert w.cap.get_whitelist_name() == "custom_whitelist"
    exp = compare(w, m, "custom_whitelist", stats, asn=asn)
    if dns or procs:
        stats = w.cap.update_whitelist(dns, procs)
        exp = compare(w, m, "custom_whitelist", stats, dns, procs, asn, prev=exp)
        w.cap.update_whitelist(None, None)
    return exp


def n_conf(exp):
    return sum(1 for b in exp.values() if b & 1)


def port_of(w, ip, proto=None):
    return next(s.dst_port for s in w.sessions if s.dst_ip == ip and (proto is None or s.protocol.name == proto))


# ---- 1. address endpoints ---------------------------------------------------------------------------
def test_exact_addresses_and_wildcards(world):
    w = world
    a, b, c, d = w.d4[0], w.d4[-1], w.d4[len(w.d4) // 2], w.d4[len(w.d4) // 3]
    eps = [{"ip": str(a)},                                                    # smallest of the index: any / any
           {"ip": str(b), "protocol": "tcp"},                                 # largest: protocol / any
           {"ip": str(c), "port": port_of(w, c)},                             # any / port
           {"ip": str(d), "port": port_of(w, d, "UDP") if any(s.dst_ip == d and s.protocol.name == "UDP" for s in w.sessions)
            else port_of(w, d), "protocol": "UDP"},                           # protocol / port
           {"ip": str(w.d6[0]), "protocol": "TCP"}, {"ip": str(w.d6[-1])},
           {"ip": "2001:db8::1", "port": 443, "protocol": "TCP"},            # not ::2 (last word), not 3001:: (first)
           {"ip": "93.184.216.34", "port": 80}, {"ip": "93.184.216.34", "port": 81, "protocol": "TCP"},
           {"ip": "93.184.216.34", "port": 1},                               # the same address under several ports
           {"ip": "203.0.113.77"}, {"ip": "no.such.ip", "port": 443}, {"ip": "93.184.216.34", "protocol": "ICMP"}]
    exp = run(w, eps)
    assert 6 <= n_conf(exp) < 40
    for n in (1, 2):  # exact-address lists of one and two entries (the empty list: test_as_fields)
        exp = run(w, eps[6:6 + n])
        assert n_conf(exp) == (1 if n == 1 else 3)  # 2001:db8::1 TCP 443; + 93.184.216.34:80 TCP and UDP


def test_cidr_prefixes(world):
    w = world
    a, x = w.d4[len(w.d4) // 4], w.d6[len(w.d6) // 2]
    flip4 = ipaddress.ip_address(int(a) ^ 1)
    x64 = ipaddress.ip_address(int(x) ^ 0xFFFF)          # host bits set below /64
    x127 = ipaddress.ip_address(int(x) ^ 1)
    x33 = ipaddress.ip_address(int(x) ^ ((1 << 90) | 5))  # differs below bit 33 only
    lists = [
        [{"ip": "255.255.255.255/1", "protocol": "TCP"}, {"ip": "%s/31" % flip4}, {"ip": "%s/32" % w.d4[1], "port": port_of(w, w.d4[1])},
         {"ip": "%s/33" % x33}, {"ip": "%s/64" % x64, "protocol": "udp"}, {"ip": "%s/127" % x127}, {"ip": "%s/128" % w.d6[1]},
         {"ip": "1.2.3.4/33"}, {"ip": "::/129"}, {"ip": "8000::/1", "port": 1}],
        [{"ip": "9.9.9.9/0", "protocol": "TCP"}],         # every IPv4 TCP flow; no IPv6 flow (a v6 flow against a v4 net)
        [{"ip": "ffff::ffff/0", "port": 443}],            # IPv6 flows to 443 only (a v4 flow against a v6 net)
    ]
    counts = [n_conf(run(w, eps)) for eps in lists]
    v4tcp = sum(1 for s in w.sessions if s.dst_ip.version == 4 and s.protocol.name == "TCP")
    assert counts[1] == v4tcp and counts[2] == sum(1 for s in w.sessions if s.dst_ip.version == 6 and s.dst_port == 443)
    assert counts[0] > 10


# ---- 2. AS fields -----------------------------------------------------------------------------------
def test_as_fields(world):
    w = world
    ip93 = ipaddress.ip_address("93.184.216.34")
    rec = w.records[wlref.asn_lookup(w.r4, int(ip93))]
    wrong = dict(as_number=rec[0], as_owner=rec[2], as_country="zz")
    lists = [
        [{"as_number": 64501}],
        [{"as_owner": "ALPHA net 0"}],                     # owner only, in another case
        [{"as_country": "Fr"}, {"as_country": "JP", "protocol": "UDP"}],
        [wrong], [dict(wrong, as_country=rec[1].lower())],
        [{"ip": "93.184.216.34", "as_number": 1}],          # ip matches, AS does not: conforming
        [{"ip": "203.0.113.1", "as_number": rec[0]}],       # ip does not match, AS does: not conforming
        [{"as_number": 64500, "port": 443}, {"as_owner": "six net 1"}],
        [{}],                                               # nothing specified: everything conforms
        [],                                                 # an empty list: nothing conforms
    ]
    counts = [n_conf(run(w, eps)) for eps in lists]
    assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0 and counts[3] == 0 and counts[4] > 0
    assert counts[5] == 4 and counts[6] == 0 and counts[8] == len(w.flows) and counts[9] == 0
    # a LAN destination has no dst_asn although 10/8 is in the table
    lan10 = [s for s in w.sessions if s.dst_ip.version == 4 and int(s.dst_ip) >> 24 == 10]
    exp = run(w, [{"as_number": w.records[wlref.asn_lookup(w.r4, 10 << 24)][0]}])
    assert lan10 and all(not (exp[k] & 1) for k, s in zip(keyb(w.flows), w.sessions) if s in lan10)
    # no ASN tables installed: dst_asn is None for everyone
    w.cap.set_asn_tables(w.v4[:0], w.v6[:0], w.records)
    try:
        assert n_conf(run(w, [{"as_number": 64501}, {"as_country": "us"}], asn=False)) == 0
        assert n_conf(run(w, [{}], asn=False)) == len(w.flows)
    finally:
        w.cap.set_asn_tables(w.v4, w.v6, w.records)


# ---- 3. domain and process endpoints ----------------------------------------------------------------
def test_domain_and_process_endpoints(world):
    w = world
    tcp = [s for s in w.sessions if s.protocol.name == "TCP" and s.dst_ip.version == 4 and s.dst_ip != ipaddress.ip_address("93.184.216.34")]
    p = tcp[0].dst_port
    eps = [{"process": "curl", "port": p, "protocol": "TCP"}, {"domain": "*.example.com", "port": 443},
           {"domain": "never.test", "protocol": "icmp"}, {"domain": "cdn.example.net", "ip": "93.184.216.34", "port": 80},
           {"process": "dig", "ip": str(w.d4[2]), "port": port_of(w, w.d4[2])}, {"ip": str(w.d4[3])}]
    dns = {str(tcp[1].dst_ip): "www.example.com", "2001:db8::1": "a.b.Example.COM", "2001:db8::2": "example.com",
           "3001:db8::1": "cdn.example.net", str(w.d4[3]): "other.test"}
    procs = {s: "CURL" for s in w.sessions if s.dst_port == p}
    procs.update({s: "dig" for s in w.sessions if s.dst_ip == w.d4[2]})
    procs[tcp[5]] = "wget"
    exp = run(w, eps, dns, procs)
    marked = sum(1 for b in exp.values() if b & 4)
    assert 2 <= marked < len(exp) // 2 and all(b & 2 for b in exp.values() if b & 4)


# ---- 4. index sizes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N.WL_LDS_RULES - 1, N.WL_LDS_RULES, N.WL_LDS_RULES + 1])
def test_rule_count_at_the_staging_threshold(world, n):
    """n nets in one group: the last one is the only one that matches."""
    w = world
    eps = [{"ip": "198.%d.%d.0/25" % (18 + (i >> 8), i & 255)} for i in range(n - 1)] + [{"ip": "128.0.0.0/2", "protocol": "TCP"}]
    assert n_conf(run(w, eps)) > 5


@pytest.mark.parametrize("n", [N.WL_LDS_GROUPS - 1, N.WL_LDS_GROUPS, N.WL_LDS_GROUPS + 1])
def test_group_count_at_the_staging_threshold(world, n):
    """n (protocol | any, port) groups of one net each, the table's own ports first."""
    w = world
    ports = sorted({s.dst_port for s in w.sessions})
    ports = (ports + [q for q in range(1, 70000) if q not in set(ports)])[:n]
    eps = [{"ip": "0.0.0.0/1", "port": q} for q in ports[:-1]] + [{"domain": "x.test", "port": ports[-1], "protocol": "UDP"}]
    assert n_conf(run(w, eps)) > 5


def test_twenty_thousand_exact_addresses(world):
    """The search path: ~20,000 exact endpoints (every other flow's own, random fill).  For endpoints of
    ip + port + protocol only, "some endpoint matches" is membership of (ip, port, protocol) in the list
    (src/whitelists.rs:465-509); the full scan of the restatement confirms it on a sample."""
    w = world
    rng = np.random.default_rng(7)
    eps = [{"ip": str(s.dst_ip), "port": s.dst_port, "protocol": s.protocol.name} for s in w.sessions[::2]]
    for i in range(9700):
        eps.append({"ip": str(ipaddress.ip_address(int(rng.integers(1 << 24, 1 << 32)))), "port": int(rng.integers(1, 65536)),
                    "protocol": ("TCP", "UDP")[i & 1]})
        eps.append({"ip": str(ipaddress.ip_address((0x2001 << 112) | int(rng.integers(0, 1 << 62)))),
                    "port": int(rng.integers(1, 65536)), "protocol": "TCP"})
    m = model(eps)
    stats = w.cap.set_custom_whitelists(m)
    have = {(ipaddress.ip_address(e["ip"]), e["port"], e["protocol"]) for e in eps}
    sb = w.cap.whitelist_bytes()
    want = [1 if (s.dst_ip, s.dst_port, s.protocol.name) in have else 2 for s in w.sessions]
    assert [int(sb[k]) for k in w.flows["slot"].tolist()] == want
    assert stats == dict(flows=len(want), conforming=want.count(1), nonconforming=want.count(2), host_check=0, changed=len(want))
    assert want.count(1) >= len(want) // 2
    sample = wlref.session_states(w.flows[::61], m, "custom_whitelist", w.r4, w.r6, w.records)
    assert [v[0] for v in sample.values()] == want[::61]
    exc = w.cap.get_whitelist_exceptions()
    assert [i.session for i in exc] == sorted((s for s, b in zip(w.sessions, want) if b == 2), key=Session.sort_key)


# ---- 5. round trip ----------------------------------------------------------------------------------
def test_learned_whitelist_round_trip(world):
    w = world
    text = w.cap.create_custom_whitelists()
    m = json.loads(text)
    stats = w.cap.set_custom_whitelists(text)
    assert stats["conforming"] == stats["flows"] == len(w.flows) and stats["nonconforming"] == 0
    assert w.cap.get_whitelist_conformance() is True and w.cap.get_whitelist_exceptions() == []
    eps = m["whitelists"][0]["endpoints"]
    gone = eps.pop(len(eps) // 2)
    compare(w, m, "custom_whitelist", w.cap.set_custom_whitelists(m))
    exc = w.cap.get_whitelist_exceptions()
    assert exc and [i.session for i in exc] == sorted(
        (s for s in w.sessions if (str(s.dst_ip), s.dst_port, s.protocol.name) == (gone["ip"], gone["port"], gone["protocol"])),
        key=Session.sort_key)
    # a list by another name, extending the learned one; then no list at all
    m2 = model([gone], "mine", extra=[dict(m["whitelists"][0], name="learned")])
    m2["whitelists"][0]["extends"] = ["learned"]
    w.cap.set_custom_whitelists(m2)  # (no list is called custom_whitelist: nothing conforms)
    assert w.cap.get_whitelist_conformance() is False
    stats = w.cap.set_whitelist("mine")
    assert w.cap.get_whitelist_name() == "mine" and stats["conforming"] == len(w.flows)
    with pytest.raises(ValueError):
        w.cap.set_whitelist("nope")
    assert w.cap.set_whitelist("") is None
    assert w.cap.get_whitelist_conformance() is True and not w.cap.whitelist_bytes().any()
    assert all(i.is_whitelisted is WhitelistState.Unknown for i in w.cap.get_sessions())


# ---- 6. table lifecycle -----------------------------------------------------------------------------
def states_by_key(cap):
    fl, sb = cap.export_flows(), cap.whitelist_bytes()
    return {k: int(sb[s]) for k, s in zip(keyb(fl), fl["slot"].tolist())}, fl


def test_states_follow_their_flows():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11, timed=True)
    try:
        fa, oa = batch(1800, 0, 420)
        cap.process_frames(fa, oa, ts=(T0 + np.arange(1800, dtype=np.uint64) * 1000))
        first = cap.export_flows()
        rows = rows_from_flows(first[::2])
        cap.install_whitelist(rows)
        st = cap.whitelist_pass()
        s0, _ = states_by_key(cap)
        assert st["changed"] == st["flows"] == len(first) and 0 < st["conforming"] < len(first)
        assert cap.whitelist_pass()["changed"] == 0          # a second identical pass changes nothing
        # a later batch that grows the table: the bytes follow by key, the new flows are Unknown
        cap0 = cap.table_info()["capacity"]
        fb, ob = batch(6000, 200000, 1500)
        cap.process_frames(fb, ob, ts=(T0 + 2 * 86400 * S + np.arange(6000, dtype=np.uint64) * 1000))
        assert cap.table_info()["capacity"] > cap0
        s1, fl1 = states_by_key(cap)
        assert all(s1[k] == v for k, v in s0.items()) and len(s1) > len(s0)
        new = [k for k in s1 if k not in s0]
        assert new and all(s1[k] == 0 for k in new)
        unk = cap.export_whitelist_flows(N.FB_WL_MASK_UNKNOWN)
        assert sorted(keyb(unk)) == sorted(new)
        st = cap.whitelist_pass()
        assert st["changed"] == len(new) and st["flows"] == len(s1)   # only the real changes
        s2, _ = states_by_key(cap)
        assert all(s2[k] == v for k, v in s0.items()) and all(s2[k] in (1, 2) for k in new)
        # a list change without a reset: `changed` counts exactly the bytes that differ
        cap.install_whitelist(rows_from_flows(fl1[::3]))
        st = cap.whitelist_pass()
        s3, _ = states_by_key(cap)
        assert st["changed"] == sum(1 for k in s3 if s3[k] != s2[k]) > 0
        # a purge that removes the flows seen only in the first batch moves others: join by key
        gen = cap.table_info()["generation"]
        ag = cap.update_sessions_status(T0 + 2 * 86400 * S + 10 * S, purge=True)
        assert ag["purged"] > 0 and cap.table_info()["generation"] == gen + 1
        s4, fl4 = states_by_key(cap)
        assert len(s4) == ag["remaining"] and all(s4[k] == s3[k] for k in s4)
        moved = {k: s for k, s in zip(keyb(fl1), fl1["slot"].tolist())}
        assert any(moved[k] != s for k, s in zip(keyb(fl4), fl4["slot"].tolist()))
        assert int((cap.whitelist_bytes() != 0).sum()) == len(s4)
        assert cap.whitelist_pass()["changed"] == 0
        # clear_all_sessions zeroes the plane; flows inserted after it read Unknown until the next pass
        cap.clear_all_sessions()
        assert not cap.whitelist_bytes().any()
        cap.process_frames(fa, oa, ts=(T0 + 3 * 86400 * S + np.arange(1800, dtype=np.uint64) * 1000))
        s5, _ = states_by_key(cap)
        assert len(s5) == len(first) and not any(s5.values())
        assert cap.whitelist_pass()["changed"] == len(first)
    finally:
        cap.close()


# ---- 7. error paths ---------------------------------------------------------------------------------
def test_error_paths():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11)
    lib = N.gpu_lib()
    try:
        fa, oa = batch(1800, 0, 420)
        cap.process_frames(fa, oa)
        flows = cap.export_flows()
        assert lib.fb_flow_whitelist(cap.ctx, 0, None, None) == N.FB_ERR_INVAL     # before fb_set_whitelist
        good = rows_from_flows(flows[:10])
        cap.install_whitelist(good)
        assert lib.fb_flow_whitelist(cap.ctx, 1, None, None) == N.FB_ERR_INVAL     # unknown flags
        base = cap.whitelist_pass()
        before = cap.whitelist_bytes().copy()
        # an over-limit list, and a list with a bad endpoint, are refused whole: the installed list stays
        big = np.zeros(N.FB_WL_MAX_OTHER + 1, dtype=N.WL_ENDPOINT_DTYPE)
        big["flags"], big["port"] = N.FB_WL_HAS_PORT, np.arange(len(big)) & 0xFFFF
        bad = good.copy()
        bad[3]["prefix"] = 33
        for rows in (big, bad):
            assert lib.fb_set_whitelist(cap.ctx, N.ptr(rows), len(rows), None, None, 0) == N.FB_ERR_INVAL
            again = cap.whitelist_pass()
            assert again == dict(base, changed=0) and (cap.whitelist_bytes() == before).all()
        assert base["conforming"] >= 10  # (several flows may share an endpoint)
        assert lib.fb_flow_export_whitelist_dev(cap.ctx, 64, None, 0, N.DeviceBuffer(8).ptr, None) == N.FB_ERR_INVAL
        N.check(lib.fb_clear_whitelist(cap.ctx))
        assert not cap.whitelist_bytes().any()
        assert lib.fb_flow_whitelist(cap.ctx, 0, None, None) == N.FB_ERR_INVAL     # after fb_clear_whitelist
        none = FlodbaddGpuCapture(0, flow_capacity=0)
        try:
            N.check(lib.fb_set_whitelist(none.ctx, N.ptr(good), len(good), None, None, 0))
            assert lib.fb_flow_whitelist(none.ctx, 0, None, None) == N.FB_ERR_INVAL  # no flow table
        finally:
            none.close()
    finally:
        cap.close()


@pytest.mark.parametrize("case", KATS, ids=[c["from"].split()[1] for c in KATS])
def test_reference_kats(case):
    """The reference's own examples (tests/golden/whitelist_kats.json) through the device pass."""
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11)
    try:
        cap.process_parsed([pkt(s["protocol"], s["src_ip"], s["src_port"], s["dst_ip"], s["dst_port"]) for s in case["sessions"]])
        cap.set_custom_whitelists(case["whitelists"])
        if case["name"] != "custom_whitelist":
            cap.set_whitelist(case["name"])
        got = {(str(i.session.dst_ip), i.session.dst_port, i.session.protocol.name): i.is_whitelisted for i in cap.get_sessions()}
        for s in case["sessions"]:
            want = WhitelistState.Conforming if s["conforming"] else WhitelistState.NonConforming
            assert got[(s["dst_ip"], s["dst_port"], s["protocol"])] is want
        assert cap.get_whitelist_conformance() is case["conformance"]
        flows = cap.export_flows()
        ref = wlref.session_states(flows, case["whitelists"], case["name"])
        assert [i.whitelist_reason for i in cap.get_whitelist_exceptions()] == \
            [v[2] for v in sorted((x for x in ref.values() if not x[1]), key=lambda x: x[3].sort_key())]
    finally:
        cap.close()
