"""The blacklist pass on the GPU (fb_flow_blacklist, flodbadd_amd/csrc/fb_blacklist.hip) against the
restatement of the reference in tests/blref.py (src/blacklists.rs:456-731, src/capture.rs:1858-1871):
every mask word, every counter, the export and every criticality string must be equal -- no tolerance
applies.  Tables are 2^9 - 2^14 slots, flows come in through process_parsed."""
import ipaddress
import json
import os

import numpy as np
import pytest

import blref
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.enrich import blacklists_from_json
from flodbadd_amd.sessions import (Protocol, Session, SessionFilter, SessionPacketData, WhitelistState,
                                   flows_to_sessions)
from flodbadd_amd.whitelists import rows_from_flows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = [c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "blacklist_kats.json")))["cases"]
        if c["kind"] == "sessions"]
S = 10 ** 9
T0 = 1_700_000_000 * S
MARKED = N.FB_WL_NONCONFORMING | N.FB_WL_BLACKLISTED


def pkt(proto, src, sport, dst, dport):
    s = Session(Protocol[proto], ipaddress.ip_address(src), sport, ipaddress.ip_address(dst), dport)
    return SessionPacketData(s, 100, 120, 2 if proto == "TCP" else None)  # (SYN: no key is reversed)


def doc(*lists):
    return {"date": "d", "signature": "s", "blacklists": [{"name": n, "ip_ranges": list(r)} for n, r in lists]}


def install(cap, ref, d):
    """The same document into the device (fb_set_blacklists) and into the restatement -> the names."""
    arr, names = blacklists_from_json(d)
    cap.set_blacklists(arr, names)
    ref.set_lists(d)
    return names


def infos_of(cap, known=None):
    """The table's sessions as SessionInfo with the STORED local flags, joined with the restatement's
    state of the sessions it already knows (criticality, whitelist state) -> (list, {Session: slot})."""
    flows = cap.export_flows()
    out = flows_to_sessions(flows)
    slot = {Session.from_key(r): int(r["slot"]) for r in flows}
    if known is not None:
        out = [known.setdefault(i.session, i) for i in out]
        for s in [s for s in known if s not in slot]:
            del known[s]
    return out, slot


def mask_of(names_hit, names):
    return sum(1 << names.index(n) for n in names_hit)


def check_pass(cap, ref, names, known, mark, wl_bytes=None):
    """One device pass and one run of the restatement over the same sessions: the plane, the counters,
    the export, the strings.  wl_bytes: {Session: whitelist byte} expected before the pass (updated)."""
    infos, slot = infos_of(cap, known)
    stats = cap.update_blacklist(mark_whitelist=mark)
    res = ref.run(infos, mark_whitelist=mark)
    print("blacklist pass:", stats, "restatement:", blref.stats_of(res))
    masks = cap.blacklist_masks()
    bad = [(str(s), hex(int(masks[slot[s]])), v) for s, v in res["names"].items()
           if int(masks[slot[s]]) != mask_of(v, names)]
    assert not bad, (len(bad), bad[:5])
    assert stats == blref.stats_of(res)
    assert int((masks != 0).sum()) == res["n_blacklisted"]  # no word outside the blacklisted flows
    recs, ms = cap.export_blacklisted_flows()
    assert len(set(recs["slot"].tolist())) == len(recs) == res["n_blacklisted"]
    assert (ms == masks[recs["slot"]]).all()
    assert sorted((Session.from_key(r) for r in recs), key=Session.sort_key) == res["blacklisted"]
    seen = {i.session: i for i in cap.get_sessions()}  # (the captures here filter All)
    assert {s: seen[s].criticality for s in res["criticality"]} == res["criticality"]
    if wl_bytes is not None:
        for i in infos:
            if mark and res["names"][i.session] and wl_bytes.get(i.session, 0) == 0:
                wl_bytes[i.session] = MARKED
        wb = cap.whitelist_bytes()
        assert {s: int(wb[slot[s]]) for s in slot} == {s: wl_bytes.get(s, 0) for s in slot}
        for s, b in wl_bytes.items():
            if s in seen and b == MARKED:
                assert seen[s].is_whitelisted is WhitelistState.NonConforming
                assert seen[s].whitelist_reason == blref.REASON
    return res, stats


# ---- 1. mixed parity --------------------------------------------------------------------------------
LISTS = doc(("wide", ["64.0.0.0/2", "2000::/4", "0.0.0.0/1"]),
            ("hosts", ["93.184.216.34", "93.184.216.0/24", "2001:db8::1/128", "203.0.113.77/32", "150.1.2.3",
                       "192.168.7.7", "10.0.0.0/8", "fd00::5"]),                     # LAN addresses that are listed
            ("mid", ["93.184.0.0/16", "2001:db8:5::/48", "150.1.2.0/23", "200.0.0.0/7", "2a00::/12"]))


def mixed_packets():
    rng = np.random.default_rng(11)
    lan4 = ["192.168.7.7", "10.1.2.3", "192.168.1.9", "172.16.5.5"]
    pk = []
    for k in range(1900):
        v6, udp = (k % 3) == 0, (k % 4) == 1
        if v6:
            src = "fd00::5" if k % 2 else str(ipaddress.IPv6Address((0x2001 << 112) | int(rng.integers(0, 1 << 62))))
            dst = str(ipaddress.IPv6Address((int(rng.integers(0x1000, 0x4000)) << 112) | int(rng.integers(1, 1 << 62))))
        else:
            src = lan4[k % 4] if k % 5 else str(ipaddress.IPv4Address(int(rng.integers(1 << 24, 0xDF000000))))
            dst = str(ipaddress.IPv4Address(int(rng.integers(1 << 24, 0xDF000000))))
        pk.append(pkt("UDP" if udp else "TCP", src, 40001 + 2 * (k % 9000), dst, (443, 53, 22, 80)[k % 4]))
    edge = ["93.184.215.255", "93.184.216.0", "93.184.216.34", "93.184.216.255", "93.184.217.0",   # below / in / above
            "93.183.255.255", "93.185.0.0", "150.1.1.255", "150.1.2.0", "150.1.3.255", "150.1.4.0", "203.0.113.76",
            "203.0.113.77", "203.0.113.78", "63.255.255.255", "64.0.0.0", "127.255.255.255", "128.0.0.0", "199.255.255.255",
            "200.0.0.0", "201.255.255.255", "202.0.0.0"]
    for k, d in enumerate(edge):
        pk.append(pkt("TCP", "192.168.1.9", 50001 + 2 * k, d, 443))
    edge6 = ["2001:db8::", "2001:db8::1", "2001:db8::2", "2001:db8:4:ffff:ffff:ffff:ffff:ffff", "2001:db8:5::",
             "2001:db8:5:ffff:ffff:ffff:ffff:ffff", "2001:db8:6::", "1fff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "2000::",
             "2fff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "3000::", "2a0f:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "2a10::"]
    for k, d in enumerate(edge6):
        pk.append(pkt("UDP" if k & 1 else "TCP", "fd00::5", 51001 + 2 * k, d, 443))
    pk += [pkt("TCP", "203.0.113.77", 52001, "10.1.2.3", 443),        # source only (the destination is LAN and listed)
           pkt("TCP", "150.1.2.3", 52003, "93.184.216.34", 443),      # both ends in hosts and mid, and in wide
           pkt("TCP", "203.0.113.77", 52005, "201.1.1.1", 443),       # source in hosts, destination in mid only
           pkt("TCP", "2001:db8::1", 52007, "2001:db8:5::9", 443),    # the same over IPv6
           pkt("TCP", "192.168.7.7", 52009, "10.9.9.9", 443),         # both LAN, both listed: nothing
           pkt("UDP", "220.1.1.1", 52011, "221.1.1.1", 53)]           # neither end in any list
    return pk


def test_mixed_parity():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12)
    ref, known = blref.BlRef(), {}
    try:
        cap.process_parsed(mixed_packets())
        names = install(cap, ref, LISTS)
        res, stats = check_pass(cap, ref, names, known, mark=False)
        infos = list(known.values())
        fam = {i.session.src_ip.version for i in infos}
        assert fam == {4, 6} and {i.session.protocol.name for i in infos} == {"TCP", "UDP"} and len(infos) > 1800
        hit = lambda ip: set(ref.ip_lists(ip))  # noqa: E731
        cases = dict(src_only=0, dst_only=0, both_same=0, both_differ=0, lan_listed=0, none=0, multi=0)
        for i in infos:
            a = set() if i.is_local_src else hit(i.session.src_ip)
            b = set() if i.is_local_dst else hit(i.session.dst_ip)
            cases["src_only"] += bool(a and not b)
            cases["dst_only"] += bool(b and not a)
            cases["both_same"] += bool(a & b)
            cases["both_differ"] += bool(a and b and a != b)
            cases["lan_listed"] += bool((i.is_local_src and hit(i.session.src_ip)) or (i.is_local_dst and hit(i.session.dst_ip)))
            cases["none"] += not (a or b)
            cases["multi"] += len(a | b) > 1
        print("mixed parity cases:", cases)
        assert all(v > 0 for v in cases.values()), cases
        assert 100 < stats["blacklisted"] < stats["flows"] - 100
        crit = res["criticality"]
        by_dst = {str(i.session.dst_ip): crit[i.session] for i in infos if i.session.src_port >= 50001}
        assert by_dst["93.184.215.255"] == "blacklist:mid,blacklist:wide" and by_dst["93.184.217.0"] == "blacklist:mid,blacklist:wide"
        assert by_dst["93.184.216.0"] == by_dst["93.184.216.255"] == "blacklist:hosts,blacklist:mid,blacklist:wide"
        assert by_dst["93.183.255.255"] == "blacklist:wide" and by_dst["128.0.0.0"] == "" and by_dst["202.0.0.0"] == ""
        assert by_dst["2001:db8::"] == "blacklist:wide" and by_dst["2001:db8::1"] == "blacklist:hosts,blacklist:wide"
        assert by_dst["3000::"] == "" and by_dst["2a10::"] == "blacklist:wide" and by_dst["1fff:ffff:ffff:ffff:ffff:ffff:ffff:ffff"] == ""
        assert by_dst["10.9.9.9"] == "" and by_dst["10.1.2.3"] == "blacklist:hosts"
    finally:
        cap.close()


# ---- 2. bit 63 --------------------------------------------------------------------------------------
def test_sixty_four_lists_and_bit_63():
    lists = [("l%02d" % k, ["20.0.%d.0/24" % k, "2001:db8:%x::/48" % (k + 1)]) for k in range(64)]
    lists[0][1].append("30.0.0.1")
    lists[63][1].extend(["30.0.0.0/30", "2001:db8:1::/64"])
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12)
    ref, known = blref.BlRef(), {}
    try:
        pk = [pkt("TCP", "192.168.1.9", 40001, "30.0.0.1", 443), pkt("TCP", "192.168.1.9", 40003, "30.0.0.2", 443),
              pkt("UDP", "fd00::5", 40005, "2001:db8:1::7", 53), pkt("UDP", "fd00::5", 40007, "2001:db8:40::7", 53),
              pkt("TCP", "20.0.62.9", 40009, "20.0.63.9", 443), pkt("TCP", "192.168.1.9", 40011, "30.0.0.4", 443)]
        pk += [pkt("TCP", "192.168.1.9", 41001 + 2 * k, "20.0.%d.%d" % (k % 70, k % 250), 443) for k in range(300)]
        cap.process_parsed(pk)
        names = install(cap, ref, doc(*lists))
        res, stats = check_pass(cap, ref, names, known, mark=False)
        masks = cap.blacklist_masks()
        slot = {str(Session.from_key(r).dst_ip): int(r["slot"]) for r in cap.export_flows()}
        assert int(masks[slot["30.0.0.1"]]) == (1 << 63) | 1 and int(masks[slot["30.0.0.2"]]) == 1 << 63
        assert int(masks[slot["2001:db8:1::7"]]) == (1 << 63) | 1 and int(masks[slot["2001:db8:40::7"]]) == 1 << 63
        assert int(masks[slot["20.0.63.9"]]) == (1 << 63) | (1 << 62) and int(masks[slot["30.0.0.4"]]) == 0
        by = {str(i.session.dst_ip): i.criticality for i in cap.get_sessions()}
        assert by["30.0.0.1"] == "blacklist:l00,blacklist:l63" and by["30.0.0.2"] == "blacklist:l63"
    finally:
        cap.close()


# ---- 3. stored, not current, local flags ------------------------------------------------------------
def test_local_flags_are_the_stored_ones():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12, lan_v6=[("2001:db8:aa::", 48)])
    ref, known = blref.BlRef(), {}
    try:
        a = [pkt("TCP", "2001:db8:aa::%x" % (k + 1), 40001 + 2 * k, "2001:db8:bb::%x" % (k + 1), 443) for k in range(40)]
        cap.process_parsed(a)                              # aa:: is LAN while these are inserted
        cap.set_lan_v6([("2001:db8:cc::", 48)])            # ... and no longer; cc:: becomes LAN
        b = [pkt("TCP", "2001:db8:aa::%x" % (k + 1), 42001 + 2 * k, "2001:db8:dd::%x" % (k + 1), 443) for k in range(40)]
        cap.process_parsed(b)                              # the same sources, inserted as global addresses
        cap.set_lan_v6([("2001:db8:dd::", 48)])            # dd:: becomes LAN after its flows exist
        names = install(cap, ref, doc(("v6", ["2001:db8:aa::/48", "2001:db8:dd::/64"])))
        res, stats = check_pass(cap, ref, names, known, mark=False)
        infos = list(known.values())
        first = [i for i in infos if i.session.src_port < 42001]
        second = [i for i in infos if i.session.src_port >= 42001]
        assert len(first) == len(second) == 40
        assert all(i.is_local_src and not i.is_local_dst for i in first)
        assert all(not i.is_local_src and not i.is_local_dst for i in second)
        assert all(res["criticality"][i.session] == "" for i in first)               # listed, but stored as LAN
        assert all(res["criticality"][i.session] == "blacklist:v6" for i in second)  # LAN now, stored as global
        assert stats["blacklisted"] == 40
        # the enrichment call takes the CURRENT configuration: the opposite answer for both groups
        flows = cap.export_flows()
        e = {int(r["slot"]): r for r in cap.enrich()}
        for r in flows:
            x, late = e[int(r["slot"])], int(r["src_port"]) >= 42001
            assert int(x["src_blacklists"]) == 1                                      # aa:: is not LAN now
            assert int(x["dst_blacklists"]) == 0 and bool(int(x["flags"]) & N.ENRICH_LOCAL_DST) is late
        masks = cap.blacklist_masks()
        assert all((int(e[int(r["slot"])]["src_blacklists"]) | int(e[int(r["slot"])]["dst_blacklists"])) != int(masks[int(r["slot"])])
                   for r in flows if int(r["src_port"]) < 42001)
    finally:
        cap.close()


# ---- 4. successive passes ---------------------------------------------------------------------------
def test_successive_passes_and_list_changes():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12)
    ref, known = blref.BlRef(), {}
    try:
        cap.process_parsed(mixed_packets()[::2])
        names = install(cap, ref, LISTS)
        res1, st1 = check_pass(cap, ref, names, known, mark=False)
        assert st1["changed"] == st1["newly_blacklisted"] == st1["blacklisted"] > 100 and st1["cleared"] == 0
        res2, st2 = check_pass(cap, ref, names, known, mark=False)
        assert st2 == dict(st1, changed=0, newly_blacklisted=0)
        # the same names with other ranges, and one more list
        names = install(cap, ref, doc(("wide", ["128.0.0.0/1", "2000::/4"]), ("hosts", ["93.184.216.34", "10.0.0.0/8"]),
                                      ("mid", ["93.184.0.0/16", "200.0.0.0/7"]), ("late", ["64.0.0.0/3", "3000::/4"])))
        res3, st3 = check_pass(cap, ref, names, known, mark=False)
        assert st3["changed"] > st3["newly_blacklisted"] > 0 and st3["cleared"] > 0
        assert st3["blacklisted"] == st2["blacklisted"] + st3["newly_blacklisted"] - st3["cleared"]
        # no list at all: every mask cleared
        names = install(cap, ref, doc())
        res4, st4 = check_pass(cap, ref, names, known, mark=False)
        assert st4 == dict(flows=st1["flows"], blacklisted=0, changed=st3["blacklisted"], newly_blacklisted=0,
                           cleared=st3["blacklisted"], wl_marked=0)
        assert not cap.blacklist_masks().any()
        lib = N.gpu_lib()
        assert lib.fb_flow_blacklist(cap.ctx, 2, None, None) == N.FB_ERR_INVAL          # unknown flag bits
        assert lib.fb_flow_blacklist(cap.ctx, 0, None, None) == N.FB_OK                 # out may be NULL
        none = FlodbaddGpuCapture(0, flow_capacity=0)
        try:
            assert lib.fb_flow_blacklist(none.ctx, 0, None, None) == N.FB_ERR_INVAL     # no flow table
        finally:
            none.close()
    finally:
        cap.close()


# ---- 5. the whitelist fallback ----------------------------------------------------------------------
def test_whitelist_fallback():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12)
    ref, known = blref.BlRef(), {}
    try:
        pk = mixed_packets()
        cap.process_parsed(pk[::4])
        names = install(cap, ref, LISTS)
        # without the flag the whitelist plane stays all zero
        res, st = check_pass(cap, ref, names, known, mark=False, wl_bytes={})
        assert st["wl_marked"] == 0 and st["blacklisted"] > 50 and not cap.whitelist_bytes().any()
        # an earlier whitelist pass: every flow of the first batch Conforming or NonConforming
        first = cap.export_flows()
        cap.install_whitelist(rows_from_flows(first[::2]))
        w0 = cap.whitelist_pass()
        assert w0["conforming"] > 50 and w0["nonconforming"] > 50
        wb = cap.whitelist_bytes()
        wl_bytes = {Session.from_key(r): int(wb[int(r["slot"])]) for r in first}
        for i in known.values():  # the restatement's sessions carry the verdicts too
            i.is_whitelisted = WhitelistState.from_byte(wl_bytes[i.session])
            i.whitelist_reason = None if wl_bytes[i.session] & 1 else "whitelist pass"
        # new flows, Unknown; the pass with the flag marks exactly the blacklisted ones among them
        cap.process_parsed(pk[1::4])
        res, st = check_pass(cap, ref, names, known, mark=True, wl_bytes=wl_bytes)
        new = [i for i in known.values() if i.session not in {Session.from_key(r) for r in first}]
        n_new_bl = sum(1 for i in new if res["names"][i.session])
        assert st["wl_marked"] == n_new_bl > 50 and n_new_bl < len(new)
        assert sum(1 for b in wl_bytes.values() if b == MARKED) == n_new_bl
        assert check_pass(cap, ref, names, known, mark=True, wl_bytes=wl_bytes)[1]["wl_marked"] == 0
        # the whitelist pass overwrites the fallback's bytes and counts them as changed
        w1 = cap.whitelist_pass()
        assert w1["changed"] == len(new) and w1["flows"] == len(known)
        wb = cap.whitelist_bytes()
        assert not (wb & N.FB_WL_BLACKLISTED).any()
        assert all(s.whitelist_reason != blref.REASON for s in cap.get_sessions())
        # fb_clear_whitelist: everything Unknown, so the next pass marks every blacklisted flow
        N.check(N.gpu_lib().fb_clear_whitelist(cap.ctx))
        assert not cap.whitelist_bytes().any()
        for i in known.values():
            i.is_whitelisted, i.whitelist_reason = WhitelistState.Unknown, None
        res, st = check_pass(cap, ref, names, known, mark=True, wl_bytes={})
        assert st["wl_marked"] == st["blacklisted"] > 100 and st["changed"] == 0
    finally:
        cap.close()


# ---- 6. the plane follows its flows -----------------------------------------------------------------
def masks_by_key(cap):
    fl, m = cap.export_flows(), cap.blacklist_masks()
    return {Session.from_key(r): int(m[int(r["slot"])]) for r in fl}, fl


def test_masks_follow_a_purge():
    """A fixed table, so the flows that come back after the purge go into the slots it freed."""
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11, timed=True, grow=False)
    try:
        # 1400 flows in 4 partitions (about 350 of 512 slots each); every other flow was last seen two days
        # before the rest
        pk = mixed_packets()[:1400]
        ts = np.array([T0 + (0 if k & 1 else 2 * 86400 * S) + k * 1000 for k in range(len(pk))], dtype=np.uint64)
        cap.process_parsed(pk, ts=ts)
        assert cap.table_info()["max_partition"] > 300
        arr, names = blacklists_from_json(LISTS)
        cap.set_blacklists(arr, names)
        st = cap.update_blacklist(mark_whitelist=True)
        s0, fl0 = masks_by_key(cap)
        assert st["flows"] == len(s0) and 100 < st["blacklisted"] == sum(1 for v in s0.values() if v) < len(s0)
        assert int((cap.whitelist_bytes() == MARKED).sum()) == st["blacklisted"] == st["wl_marked"]
        # the purge removes every other flow of every partition: survivors keep their words
        gen = cap.table_info()["generation"]
        ag = cap.update_sessions_status(T0 + 2 * 86400 * S + 100 * S, purge=True)
        assert ag["purged"] > 600 and ag["remaining"] > 600 and cap.table_info()["generation"] == gen + 1
        s1, fl1 = masks_by_key(cap)
        old_slot = {Session.from_key(r): int(r["slot"]) for r in fl0}
        assert any(old_slot[Session.from_key(r)] != int(r["slot"]) for r in fl1)      # some survivor moved
        assert len(s1) == ag["remaining"] and all(s0[k] == v for k, v in s1.items())
        n1 = sum(1 for v in s1.values() if v)
        assert int((cap.blacklist_masks() != 0).sum()) == n1                           # the removed flows lost theirs
        assert int((cap.whitelist_bytes() == MARKED).sum()) == n1
        # the removed flows come back into freed slots: they read 0 until the next pass
        gone = [p for p in pk if p.session not in s1]
        cap.process_parsed(gone, ts=np.full(len(gone), T0 + 2 * 86400 * S + 200 * S, dtype=np.uint64))
        assert cap.table_info()["capacity"] == 1 << 11
        s2, fl2 = masks_by_key(cap)
        assert len(s2) == len(s0) and all(s2[k] == v for k, v in s1.items())
        assert all(s2[k] == 0 for k in s2 if k not in s1)
        freed = set(old_slot.values()) - {int(r["slot"]) for r in fl1}
        assert any(int(r["slot"]) in freed for r in fl2 if Session.from_key(r) not in s1)
        st = cap.update_blacklist(mark_whitelist=False)
        s3, _ = masks_by_key(cap)
        assert s3 == s0 and st["changed"] == st["newly_blacklisted"] == sum(1 for k in s0 if s0[k] and k not in s1)
        ref = blref.BlRef()
        ref.set_lists(LISTS)
        res = ref.run(flows_to_sessions(cap.export_flows()), mark_whitelist=False)
        assert {s: mask_of(v, names) for s, v in res["names"].items()} == s3
    finally:
        cap.close()


def test_masks_follow_a_growth_and_clear():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11)
    try:
        pk = mixed_packets()[:1000]
        cap.process_parsed(pk)
        cap0 = cap.table_info()["capacity"]
        arr, names = blacklists_from_json(LISTS)
        cap.set_blacklists(arr, names)
        st = cap.update_blacklist(mark_whitelist=True)
        s0, _ = masks_by_key(cap)
        n0 = sum(1 for v in s0.values() if v)
        assert cap0 == 1 << 11 and st["blacklisted"] == n0 > 100
        # a batch that grows the table: the words follow by key, the new flows read 0
        more = [pkt("UDP", "192.168.1.9", 40001 + 2 * (k % 9000), str(ipaddress.IPv4Address(0x30000000 + 7919 * k)), 53)
                for k in range(3000)]
        cap.process_parsed(more)
        assert cap.table_info()["capacity"] > cap0
        s4, _ = masks_by_key(cap)
        assert len(s4) == len(s0) + 3000 and all(s4[k] == v for k, v in s0.items())
        assert all(s4[k] == 0 for k in s4 if k not in s0)
        assert int((cap.blacklist_masks() != 0).sum()) == n0 == int((cap.whitelist_bytes() == MARKED).sum())
        st = cap.update_blacklist(mark_whitelist=False)
        assert st["changed"] == st["newly_blacklisted"] == 3000 and st["flows"] == len(s4)  # 48.0.0.0 ..: all in 0.0.0.0/1
        ref = blref.BlRef()
        ref.set_lists(LISTS)
        res = ref.run(flows_to_sessions(cap.export_flows()), mark_whitelist=False)
        assert {s: mask_of(v, names) for s, v in res["names"].items()} == masks_by_key(cap)[0]
        # fb_flow_clear zeroes the plane
        cap.clear_all_sessions()
        assert not cap.blacklist_masks().any() and not cap.whitelist_bytes().any()
        cap.process_parsed(pk[:200])
        s6, _ = masks_by_key(cap)
        assert len(s6) == 200 and not any(s6.values())
    finally:
        cap.close()


# ---- 7. edges of the sweep and of the compaction ----------------------------------------------------
def export_raw(cap, cap_recs, with_masks=True, guard=64):
    """fb_flow_export_blacklisted_dev into buffers with `guard` bytes of 0xA5 behind the first cap_recs
    records / words -> (n, records, masks or None, the guards intact)."""
    rb, mb = cap_recs * N.FLOW_REC_DTYPE.itemsize, cap_recs * 8
    d_out, d_m, d_n = N.DeviceBuffer(rb + guard), N.DeviceBuffer(mb + guard), N.DeviceBuffer(8)
    fill = np.full(rb + guard, 0xA5, dtype=np.uint8)
    d_out.upload(fill)
    d_m.upload(fill[: mb + guard])
    N.check(N.gpu_lib().fb_flow_export_blacklisted_dev(cap.ctx, d_out.ptr, d_m.ptr if with_masks else None, cap_recs, d_n.ptr, None))
    n = int(d_n.download(np.zeros(1, dtype=np.uint64))[0])
    raw = d_out.download(np.zeros(rb + guard, dtype=np.uint8))
    rawm = d_m.download(np.zeros(mb + guard, dtype=np.uint8))
    ok = bool((raw[rb:] == 0xA5).all() and (rawm[mb:] == 0xA5).all())
    if not with_masks:
        ok = ok and bool((rawm == 0xA5).all())
    return n, raw[:rb].view(N.FLOW_REC_DTYPE), rawm[:mb].view(np.uint64) if with_masks else None, ok


def test_sweep_and_compaction_edges():
    ref = blref.BlRef()
    # an empty table
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 14)
    try:
        names = install(cap, ref, LISTS)
        assert cap.update_blacklist() == dict(flows=0, blacklisted=0, changed=0, newly_blacklisted=0, cleared=0, wl_marked=0)
        n, _, _, ok = export_raw(cap, 4)
        assert n == 0 and ok
        assert cap.get_blacklisted_sessions() == [] and cap.get_blacklisted_status() is False
        # before any pass on a fresh context the export and the plane read nothing / zeros
        # (about) one occupied slot per 64: 256 flows in 2^14 slots
        pk = mixed_packets()
        cap.process_parsed(pk[:256])
        check_pass(cap, ref, names, {}, mark=False)
    finally:
        cap.close()
    # a completely full partition: 512 flows in a fixed one-partition table
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=512, grow=False)
    try:
        fresh = N.DeviceBuffer(512 * 8)
        fresh.upload(np.full(512, 7, dtype=np.uint64))
        N.check(N.gpu_lib().fb_flow_blacklist_dev(cap.ctx, fresh.ptr, 1 << 20, None))   # min(cap, capacity) zeros
        assert not fresh.download(np.zeros(512, dtype=np.uint64)).any()
        cap.process_parsed(pk[:512])
        assert cap.flow_count() == 512
        names = install(cap, ref, LISTS)
        res, st = check_pass(cap, ref, names, {}, mark=True)
        assert st["flows"] == 512 and st["blacklisted"] > 64
        # cap smaller than the count: *d_n is the total, exactly cap records, the guards intact
        full_recs, full_masks = cap.export_blacklisted_flows()
        for c in (0, 1, 63, 64, 65):
            n, recs, ms, ok = export_raw(cap, c)
            assert n == st["blacklisted"] and ok
            got = sorted(zip(recs["slot"].tolist(), ms.tolist()))
            allowed = set(zip(full_recs["slot"].tolist(), full_masks.tolist()))
            assert len(set(got)) == c and set(got) <= allowed
        n, recs, ms, ok = export_raw(cap, st["blacklisted"], with_masks=False)     # d_masks == NULL
        assert n == st["blacklisted"] and ok and ms is None
        assert np.sort(recs, order="slot").tobytes() == np.sort(full_recs, order="slot").tobytes()
    finally:
        cap.close()


# The other compacting exports -> (record dtype, the _dev call into (d_out, cap, d_n)).  The whitelist
# export selects the conforming flows only, so its total is below the occupancy.
OTHER_EXPORTS = {
    "sessions": (N.FLOW_REC_DTYPE, lambda lib, ctx, out, c, n: lib.fb_flow_export_sessions_dev(ctx, N.FB_FILTER_ALL, out, c, n, None)),
    "whitelist": (N.FLOW_REC_DTYPE, lambda lib, ctx, out, c, n: lib.fb_flow_export_whitelist_dev(ctx, N.FB_WL_CONFORMING, out, c, n, None)),
    "times": (N.FLOW_TIME_DTYPE, lambda lib, ctx, out, c, n: lib.fb_flow_export_times_dev(ctx, out, c, n, None)),
}


@pytest.mark.parametrize("which", sorted(OTHER_EXPORTS))
def test_compaction_edges_of_the_other_exports(which):
    """The output-capacity edge of test_sweep_and_compaction_edges for the session, whitelist and time
    exports, against a completely full 512-slot partition: *d_n is the total whatever the capacity, exactly
    `cap` distinct records arrive, each one of the full export's, and nothing is written behind them."""
    dtype, call = OTHER_EXPORTS[which]
    guard, rec = 64, dtype.itemsize

    def raw(cap, c):
        d_out, d_n = N.DeviceBuffer(c * rec + guard), N.DeviceBuffer(8)
        d_out.upload(np.full(c * rec + guard, 0xA5, dtype=np.uint8))
        N.check(call(N.gpu_lib(), cap.ctx, d_out.ptr, c, d_n.ptr))
        n = int(d_n.download(np.zeros(1, dtype=np.uint64))[0])
        b = d_out.download(np.zeros(c * rec + guard, dtype=np.uint8))
        return n, b[: c * rec].view(dtype), bool((b[c * rec:] == 0xA5).all())

    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=512, grow=False, timed=True)
    try:
        pk = mixed_packets()[:512]
        cap.process_parsed(pk, ts=(T0 + np.arange(512, dtype=np.uint64) * 1000))
        assert cap.flow_count() == 512
        cap.install_whitelist(rows_from_flows(cap.export_flows()[::2]))
        cap.whitelist_pass()
        total = int((cap.whitelist_bytes() == N.FB_WL_CONFORMING).sum()) if which == "whitelist" else 512
        assert 65 < total <= 512
        n, full, ok = raw(cap, total)
        assert n == total and ok and len(set(full["slot"].tolist())) == total
        allowed = {r.tobytes() for r in full}
        for c in (0, 1, 63, 64, 65):
            n, recs, ok = raw(cap, c)
            print("%s export, cap %d: d_n %d, %d distinct slots" % (which, c, n, len(set(recs["slot"].tolist()))))
            assert n == total and ok
            assert len(set(recs["slot"].tolist())) == c and {r.tobytes() for r in recs} <= allowed
    finally:
        cap.close()


def test_table_larger_than_the_grid():
    """2^19 slots: the pass's and the export's grids stop at 1024 workgroups (2^18 slots), so every thread
    takes more than one step of the sweep."""
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 19, grow=False, timed=True)
    ref = blref.BlRef()
    try:
        pk = mixed_packets()
        cap.process_parsed(pk, ts=(T0 + np.arange(len(pk), dtype=np.uint64) * 1000))
        flows, times = cap.export_flows(), cap.export_times()
        slots = flows["slot"]
        assert cap.table_info()["capacity"] == 1 << 19 and int(slots.min()) < 1 << 18 <= int(slots.max())
        # the session and the time export: every flow put in, once, and the same slots from both
        assert len(flows) == len(times) == cap.flow_count() == len(pk) == len({p.session for p in pk})
        assert sorted(slots.tolist()) == sorted(times["slot"].tolist()) and len(set(slots.tolist())) == len(flows)
        assert sorted(times["last_activity_ns"].tolist()) == (T0 + np.arange(len(pk), dtype=np.uint64) * 1000).tolist()
        names = install(cap, ref, LISTS)
        known = {}
        check_pass(cap, ref, names, known, mark=True, wl_bytes={})
        st = check_pass(cap, ref, names, known, mark=True, wl_bytes={s: MARKED for s, i in known.items() if i.criticality})[1]
        assert st["changed"] == 0 and st["wl_marked"] == 0
    finally:
        cap.close()


# ---- 8. the Python surface ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", KATS, ids=[c["from"].split()[1] for c in KATS])
def test_reference_kats_end_to_end(case):
    """The reference's capture tests through FlodbaddGpuCapture.  Sessions come in through
    process_parsed, so their local flags are is_lan_ip of their addresses -- what the reference stores
    for a session made from a packet; where a reference test wrote other flags into a hand-made
    SessionInfo, the restatement run over the capture's own sessions is the expectation, and the
    recorded strings are checked where the flags agree."""
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11)
    ref = blref.BlRef()
    try:
        for step in case["steps"]:
            cap.clear_all_sessions()  # (a step lists the sessions present; the reference's tests clear the map too)
            ref.blacklisted = []
            cap.process_parsed([pkt(s["protocol"], s["src_ip"], s["src_port"], s["dst_ip"], s["dst_port"]) for s in step["sessions"]])
            if "blacklists" in step:
                out = cap.set_custom_blacklists(json.dumps(step["blacklists"]))
                assert out["status"] is None and out["whitelist"] is None and out["blacklist"]["flows"] == len(step["sessions"])
                ref.set_lists(step["blacklists"])
                assert {i["name"] for i in json.loads(cap.get_blacklists())["blacklists"]} == set(ref.lists)
            infos = flows_to_sessions(cap.export_flows())
            res = ref.run(infos)
            got = cap.get_blacklisted_sessions()
            assert [i.session for i in got] == res["blacklisted"]
            assert [i.criticality for i in got] == [res["criticality"][i.session] for i in got]
            assert all(i.is_whitelisted is WhitelistState.NonConforming and i.whitelist_reason == blref.REASON for i in got)
            assert cap.get_blacklisted_status() is bool(res["blacklisted"])
            every = {i.session: i for i in cap.get_sessions()}
            assert {s: i.criticality for s, i in every.items()} == res["criticality"]
            want = {i.session: i for i in infos}
            assert all(every[s].is_whitelisted is want[s].is_whitelisted and every[s].whitelist_reason == want[s].whitelist_reason
                       for s in every)
            by_key = {(str(i.session.src_ip), i.session.src_port, str(i.session.dst_ip), i.session.dst_port): i for i in every.values()}
            agree = True
            for s in step["sessions"]:
                i = by_key[(s["src_ip"], s["src_port"], s["dst_ip"], s["dst_port"])]
                if (i.is_local_src, i.is_local_dst) != (s["is_local_src"], s["is_local_dst"]):
                    agree = False
                    continue
                if "criticality" in s:
                    assert i.criticality == s["criticality"]
                if "contains" in s:
                    assert s["contains"] in i.criticality
                if s.get("not_unknown"):
                    assert i.is_whitelisted is not WhitelistState.Unknown
            if case["from_packets"]:
                assert agree
            if agree:
                assert [i.session for i in got] == sorted((by_key[(s["src_ip"], s["src_port"], s["dst_ip"], s["dst_port"])].session
                                                           for s in (step["sessions"][k] for k in step["blacklisted"])),
                                                          key=Session.sort_key)
                assert cap.get_blacklisted_status() is step["status"]
    finally:
        cap.close()


def test_python_surface_and_update_order():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11, timed=True)
    try:
        pk = [pkt("TCP", "192.168.1.9", 40001, "93.184.216.34", 443), pkt("TCP", "192.168.1.9", 40003, "8.8.8.8", 443),
              pkt("UDP", "192.168.1.9", 40005, "9.9.9.9", 53), pkt("TCP", "192.168.1.9", 40007, "1.1.1.1", 443)]
        ts = np.array([T0, T0, T0 + 2 * 86400 * S, T0 + 2 * 86400 * S], dtype=np.uint64)
        cap.process_parsed(pk, ts=ts)
        assert all(i.criticality == "" and i.whitelist_reason is None for i in cap.get_sessions())   # before any pass
        assert not cap.blacklist_masks().any()
        text = json.dumps(doc(("zz", ["93.184.216.34", "9.9.9.9"]), ("aa", ["9.0.0.0/8", "8.8.8.8"])))
        out = cap.set_custom_blacklists(text)
        assert out["blacklist"] == dict(flows=4, blacklisted=3, changed=3, newly_blacklisted=3, cleared=0, wl_marked=3)
        assert json.loads(cap.get_blacklists())["blacklists"][1] == {"name": "aa", "description": None, "last_updated": None,
                                                                      "source_url": None, "ip_ranges": ["9.0.0.0/8", "8.8.8.8"]}
        by = {str(i.session.dst_ip): i for i in cap.get_sessions()}
        assert by["9.9.9.9"].criticality == "blacklist:aa,blacklist:zz" and by["8.8.8.8"].criticality == "blacklist:aa"
        assert by["93.184.216.34"].criticality == "blacklist:zz" and by["1.1.1.1"].criticality == ""
        assert by["9.9.9.9"].whitelist_reason == blref.REASON and by["9.9.9.9"].is_whitelisted is WhitelistState.NonConforming
        assert by["1.1.1.1"].is_whitelisted is WhitelistState.Unknown and by["1.1.1.1"].whitelist_reason is None
        assert [str(i.session.dst_ip) for i in cap.get_blacklisted_sessions()] == \
            [str(s.dst_ip) for s in sorted((i.session for i in by.values() if i.criticality), key=Session.sort_key)]
        # exceptions and conformance stay the whitelist pass's products: no list is active
        assert cap.get_whitelist_exceptions() == [] and cap.get_whitelist_conformance() is True
        # invalid text raises and leaves the installed lists as they were
        for bad in ("{", json.dumps({"blacklists": []}), json.dumps(dict(json.loads(text), more=1))):
            with pytest.raises(ValueError):
                cap.set_custom_blacklists(bad)
        assert cap.get_blacklists() == json.dumps(json.loads(cap.get_blacklists())) and len(json.loads(cap.get_blacklists())["blacklists"]) == 2
        assert cap.update_blacklist()["blacklisted"] == 3
        # update_sessions: status (and purge) first, then the blacklist pass with the fallback, then the
        # whitelist pass, which replaces the fallback's verdicts
        wl = {"date": "d", "signature": None, "whitelists": [{"name": "custom_whitelist", "extends": None,
                                                               "endpoints": [{"ip": "9.9.9.9", "port": 53, "protocol": "UDP"}]}]}
        cap.set_custom_whitelists(json.dumps(wl))
        cap.reset_whitelist()
        out = cap.update_sessions(T0 + 2 * 86400 * S + 100 * S)
        assert out["status"]["purged"] == 2 and out["status"]["remaining"] == 2       # the two old flows are gone first
        assert out["blacklist"] == dict(flows=2, blacklisted=1, changed=0, newly_blacklisted=0, cleared=0, wl_marked=1)
        assert out["whitelist"]["flows"] == 2 and out["whitelist"]["conforming"] == 1 and out["whitelist"]["changed"] == 2
        by = {str(i.session.dst_ip): i for i in cap.get_sessions()}
        assert set(by) == {"9.9.9.9", "1.1.1.1"}
        assert by["9.9.9.9"].is_whitelisted is WhitelistState.Conforming and by["9.9.9.9"].whitelist_reason is None
        assert by["9.9.9.9"].criticality == "blacklist:aa,blacklist:zz" and by["1.1.1.1"].is_whitelisted is WhitelistState.NonConforming
        assert [str(i.session.dst_ip) for i in cap.get_whitelist_exceptions()] == ["1.1.1.1"]
        assert [str(i.session.dst_ip) for i in cap.get_current_sessions()] == ["1.1.1.1", "9.9.9.9"] or \
            {i.criticality for i in cap.get_current_sessions()} == {"", "blacklist:aa,blacklist:zz"}
        # "" resets to no lists
        out = cap.set_custom_blacklists("")
        assert out["blacklist"]["cleared"] == 1 and out["blacklist"]["blacklisted"] == 0
        assert cap.get_blacklisted_sessions() == [] and cap.get_blacklisted_status() is False
        assert json.loads(cap.get_blacklists())["blacklists"] == []
        assert all(i.criticality == "" for i in cap.get_sessions())
    finally:
        cap.close()
