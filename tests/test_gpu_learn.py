"""Endpoint learning on the device (fb_flow_learn_endpoints_dev, flodbadd_amd/csrc/fb_learn.hip) against
tests/learnref.py run over the capture's own exports -- the flow records, the domain-id plane and the selection
computed from the planes --: the records must be equal byte for byte, so no tolerance applies.
tests/test_learn_oracle.py ties learnref to Whitelists.new_from_sessions without a GPU.  Tables of 2^9 slots and at
most a few hundred flows, injected with process_parsed."""
import ctypes as C
import ipaddress
import json

import numpy as np
import pytest

import dnstrackgen as T
import learncorpus as LC
import learnref
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.sessions import Protocol, Session, SessionFilter, SessionPacketData
from flodbadd_amd.whitelists import Whitelists

pytestmark = pytest.mark.gpu

S = 10 ** 9
T0 = 1_700_000_000 * S
ONE_CHAIN = 1 << 63  # FB_DEBUG_LEARN_HASH_MASK: the tag's "used" bit alone -- no hash bit is left, so every tag and
                     # every home are equal, as an AND with 0 would leave them (the value 0 itself restores all bits)


def pkts(corpus):
    return [SessionPacketData(Session(Protocol[p], ipaddress.ip_address(s), sp, ipaddress.ip_address(d), dp), 100, 140,
                              0x10 if p == "TCP" else None) for p, s, sp, d, dp in corpus]


def capture(**kw):
    kw.setdefault("flow_capacity", 1 << 9)
    return FlodbaddGpuCapture(0, session_filter=SessionFilter.All, **kw)


def inject(cap, corpus, t=None):
    cap.process_parsed(pkts(corpus), ts=None if t is None else np.full(len(corpus), t, dtype=np.uint64))


def round_bound(selected):
    """The hard cap of the insert rounds: the index's slots + 2 (fb_learn.hip: at least 64, at least 2 x selected)."""
    slots = 64
    while slots < 2 * selected:
        slots *= 2
    return slots + 2


def check(cap, view_set=N.FB_VIEW_ALL, since=None, flt=None, slots=None):
    """One learning call equals learnref over the capture's exports (slots: the table slots of the selected flows;
    None: every flow -- by slot, not by position: two exports need not list the flows in the same order) ->
    (records, counters)."""
    recs, st = cap.learn_endpoints(view_set, since, flt)
    flows = cap.export_flows(SessionFilter.All)
    mask = None if slots is None else np.isin(flows["slot"], np.asarray(slots, dtype=np.uint32))
    want = learnref.records(flows, cap.domain_ids()["dst_name_id"], mask)
    assert len(recs) == len(want), (len(recs), len(want))
    assert recs.tobytes() == want.tobytes()
    selected = len(flows) if mask is None else int(np.count_nonzero(mask))
    print("learn:", st, "hard cap", round_bound(selected))
    assert (st["flows"], st["selected"], st["endpoints"], st["written"]) == (len(flows), selected, len(want), len(want))
    assert int(recs["sessions"].sum()) == st["selected"]
    assert (st["rounds"] >= 1) == (selected > 0) and st["rounds"] < round_bound(selected)
    assert (np.diff(recs["rep_slot"].astype(np.int64)) > 0).all()
    return recs, st


def core(recs, dsts=None):
    """The records without their slots (what a slot move must leave alone), of the given destinations."""
    out = []
    for r in recs:
        dst = str(ipaddress.ip_address(bytes(r["dst_ip"].astype(">u4").tobytes()) if r["family"] == 10
                                       else int(r["dst_ip"][0])))
        if dsts is None or dst in dsts:
            out.append((dst, int(r["dst_port"]), int(r["protocol"]), int(r["dst_name_id"]), tuple(r["rep_src_ip"].tolist()),
                        int(r["rep_src_port"]), int(r["sessions"])))
    return sorted(out)


def resolve(cap, ref, mapping, tx0=0):
    b = T.Batch()
    for k, (ip, name) in enumerate(mapping.items()):
        b.query(tx0 + k, name).response(tx0 + k, [ip])
    T.step(cap, ref, b)


def test_group_sizes():
    """One fingerprint of 1 .. 257 sessions: duplicates inside a wave, across waves and across the workgroups of
    the round kernel (one lane per table slot; the flows sit all over the table)."""
    cap = capture()
    try:
        for n in LC.GROUP_SIZES:
            cap.clear_all_sessions()
            inject(cap, LC.group(n))
            recs, st = check(cap)
            assert len(recs) == 1 and int(recs[0]["sessions"]) == n and st["selected"] == n
            assert (int(recs[0]["rep_src_ip"][0]), int(recs[0]["rep_src_port"])) == (int(ipaddress.ip_address("10.7.0.0")), 61000)
        # and several groups at once, next to single sessions
        cap.clear_all_sessions()
        inject(cap, LC.group(65) + LC.group(64, dst="203.0.113.78", base=300) + LC.group(2, dport=444, base=600) +
               LC.distinct(20))
        recs, st = check(cap)
        assert sorted(recs["sessions"].tolist()) == [1] * 20 + [2, 64, 65]
    finally:
        cap.close()


def test_one_field_apart():
    corpus = LC.one_field_apart()
    cap = capture()
    try:
        inject(cap, corpus)
        recs, _ = check(cap)
        assert len(recs) == len(corpus) and (recs["sessions"] == 1).all()  # none may merge
    finally:
        cap.close()


def test_name_id_alone_tells_two_endpoints_apart():
    """The same address, port and protocol once resolved and once not: the first flow has left current_sessions
    (idle for more than 180 s) when the domain pass sees the resolution, so only the second gets the name."""
    cap, ref = T.new_capture(timed=True, flow_capacity=1 << 9)
    try:
        cap.process_parsed(pkts([("TCP", "10.8.1.1", 61020, "198.51.100.30", 443), ("TCP", "10.8.1.2", 61021, "198.51.100.30", 443),
                                 ("TCP", "10.8.1.3", 61022, "198.51.100.30", 443)]),
                           ts=np.array([T0, T0 + 150 * S, T0 + 151 * S], dtype=np.uint64))
        recs, _ = check(cap)  # before any domain pass: one endpoint, id 0
        assert len(recs) == 1 and int(recs[0]["dst_name_id"]) == 0 and int(recs[0]["sessions"]) == 3
        resolve(cap, ref, {"198.51.100.30": "one.example"})
        cap.update_sessions_status(T0 + 200 * S, purge=False)
        assert cap.update_domains()["dst_set"] == 2
        recs, _ = check(cap)
        assert len(recs) == 2 and (recs["dst_ip"][0] == recs["dst_ip"][1]).all()
        by_id = {int(r["dst_name_id"]): r for r in recs}
        named = [i for i in by_id if i]
        assert set(by_id) == {0, named[0]} and cap.dns_names(named) == {named[0]: "one.example"}
        assert int(by_id[0]["sessions"]) == 1 and int(by_id[named[0]]["sessions"]) == 2
        assert int(by_id[named[0]]["rep_src_port"]) == 61021
    finally:
        cap.close()


def test_representative_through_growth_and_purge():
    rep = LC.representatives()
    dsts = {c[3] for c in rep}
    cap = capture(timed=True)
    try:
        inject(cap, LC.group(100, dst="192.0.2.200", dport=9000, base=1000), T0)  # idle since T0: the purge takes them
        inject(cap, rep, T0 + 1000 * S)
        recs, _ = check(cap)
        first = core(recs, dsts)
        got = {(d, proto): (str(ipaddress.ip_address(bytes(np.array(src, dtype=">u4").tobytes()) if ":" in d else src[0])), port, n)
               for d, _, proto, _, src, port, n in first}
        assert got[("2001:db8::50", 6)] == ("fd00::1:1", 61100, 5)         # the last word alone
        assert got[("2001:db8::51", 6)] == ("fd00::2", 61201, 4)           # the port alone (IPv6)
        assert got[("198.51.100.51", 17)] == ("10.9.0.1", 61201, 4)        # the port alone (IPv4)
        assert got[("2001:db8::52", 6)] == ("fd00::1:0:1", 61299, 2)       # words 2-3 before the port
        # some group's least session sits in a higher slot than another of its members
        flows = cap.export_flows(SessionFilter.All)
        low = {}
        for r in flows:
            k = (bytes(r["dst_ip"]), int(r["dst_port"]), int(r["protocol"]))
            low[k] = min(low.get(k, 1 << 32), int(r["slot"]))
        assert any(int(r["rep_slot"]) > low[(bytes(r["dst_ip"]), int(r["dst_port"]), int(r["protocol"]))] for r in recs)
        # a growth moves every flow
        info = cap.table_info()
        k = 0
        while cap.table_info()["capacity"] == info["capacity"]:
            inject(cap, [("UDP", "10.4.%d.%d" % (k, i), 44000, "10.5.%d.%d" % (k, i), 5000) for i in range(250)], T0 + 1000 * S)
            k += 1
            assert k < 8
        assert cap.table_info()["generation"] > info["generation"]
        recs, _ = check(cap)
        assert core(recs, dsts) == first
        # a purge that removes the idle group re-packs the partitions
        gen = cap.table_info()["generation"]
        assert cap.update_sessions_status(T0 + 1100 * S, purge=True, retention_s=500)["purged"] == 100
        assert cap.table_info()["generation"] > gen
        recs, _ = check(cap)
        assert core(recs, dsts) == first and "192.0.2.200" not in {c[0] for c in core(recs)}
    finally:
        cap.close()


def test_forced_collisions():
    lib = N.gpu_lib()
    cap = capture()
    try:
        inject(cap, LC.distinct(40))
        base, st = check(cap)
        assert len(base) == 40 and st["rounds"] <= 3  # 64-bit tags: one round, two with a shared home
        N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_LEARN_HASH_MASK, ONE_CHAIN))
        recs, st = check(cap)
        assert recs.tobytes() == base.tobytes()
        # one tag, one home, one chain: a round publishes one slot, every other flow waits at it and compares in
        # the next round -- forty endpoints take forty rounds
        print("one chain of 40: rounds", st["rounds"], "hard cap", round_bound(40))
        assert st["rounds"] == 40
        N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_LEARN_HASH_MASK, 0))  # all bits again
        recs, st = check(cap)
        assert recs.tobytes() == base.tobytes() and st["rounds"] <= 3
        # sixteen tags for a few hundred endpoints, several sessions for some
        cap.clear_all_sessions()
        inject(cap, LC.distinct(300) + LC.group(30, dst="192.0.2.7", dport=7000, proto="TCP"))
        base, _ = check(cap)
        N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_LEARN_HASH_MASK, 0xF))
        recs, st = check(cap)
        print("16 tags, %d endpoints: rounds" % len(recs), st["rounds"], "hard cap", round_bound(st["selected"]))
        assert recs.tobytes() == base.tobytes() and len(recs) >= 300 and st["rounds"] > 3
        assert lib.fb_debug_set(cap.ctx, 99, 0) == N.FB_ERR_INVAL
    finally:
        cap.close()


def test_selection():
    corpus = LC.mixed_local()
    cap = capture(timed=True)
    try:
        inject(cap, corpus[:60], T0)
        inject(cap, corpus[60:], T0 + 100 * S)
        every, _ = check(cap)
        assert len(every) == 16
        # half the endpoints whitelisted: the exceptions are the flows of the other half
        eps = Whitelists.from_learned(every).whitelists["custom_whitelist"].endpoints
        w = Whitelists()
        w.as_custom(eps[::2])
        st = cap.set_custom_whitelists(w.to_json())
        assert 0 < st["nonconforming"] < st["flows"]
        occupied = cap.export_flows(SessionFilter.All)["slot"]  # (selections below are sets of table slots)
        nonconf = np.intersect1d(np.nonzero(cap.whitelist_bytes() & N.FB_WL_NONCONFORMING)[0], occupied)
        assert len(nonconf) == st["nonconforming"]
        exc, _ = check(cap, N.FB_VIEW_WL_EXCEPTIONS, slots=nonconf)
        assert [c[:3] for c in core(exc)] == sorted(c[:3] for c in core(every[1::2]))
        # (the selection is the view export's: the same flows, and every representative is one of them)
        viewed = set(cap.export_view(N.FB_VIEW_WL_EXCEPTIONS)["rec"]["slot"].tolist())
        assert viewed == set(nonconf.tolist()) and set(exc["rep_slot"].tolist()) <= viewed
        # a LocalOnly filter, evaluated now
        local = cap.export_flows(SessionFilter.LocalOnly)["slot"]
        loc, _ = check(cap, flt=SessionFilter.LocalOnly, slots=local)
        assert len(loc) == 6 and len(local) == 60
        # MODIFIED_SINCE: last_modified = max(last activity, stamp) later than since
        times = cap.export_times()
        last = np.zeros(cap.table_info()["capacity"], dtype=np.uint64)
        last[times["slot"]] = times["last_activity_ns"]
        last = np.maximum(last, cap.modified_stamps())
        since = T0 + 50 * S
        recent = np.intersect1d(np.nonzero(last > since)[0], occupied)
        assert 0 < len(recent) < len(occupied)
        inc, _ = check(cap, since=since, slots=recent)
        assert int(inc["sessions"].sum()) == 60 and core(inc) != core(every)  # the later batch's flows alone
        both, _ = check(cap, N.FB_VIEW_WL_EXCEPTIONS, since=since, flt=SessionFilter.GlobalOnly,
                        slots=np.setdiff1d(np.intersect1d(recent, nonconf), local))
        assert 0 < len(both) <= len(exc)
        none, st = check(cap, since=T0 + 1000 * S, slots=[])
        assert len(none) == 0 and st["rounds"] == 0
    finally:
        cap.close()


def test_invalid_queries_are_refused_like_the_view_exports():
    lib = N.gpu_lib()
    cap, untimed, bare = capture(timed=True), capture(), FlodbaddGpuCapture(0, flow_capacity=0)
    try:
        inject(cap, LC.distinct(8), T0)
        inject(untimed, LC.distinct(8))
        d_out, d_n = N.DeviceBuffer(64 * 16), N.DeviceBuffer(8)

        def call(c, **kw):
            q = np.zeros(1, dtype=N.VIEW_QUERY_DTYPE)
            for k, v in kw.items():
                q[0][k] = v
            return lib.fb_flow_learn_endpoints_dev(c.ctx, N.ptr(q), d_out.ptr, 16, d_n.ptr, None, None)

        assert call(cap) == 0 and call(cap, set=4, filter=2, flags=1, since_ns=5) == 0
        assert call(cap, set=5) == N.FB_ERR_INVAL and call(cap, set=0xFFFFFFFF) == N.FB_ERR_INVAL
        assert call(cap, filter=3) == N.FB_ERR_INVAL
        assert call(cap, flags=2) == N.FB_ERR_INVAL and call(cap, flags=3) == N.FB_ERR_INVAL
        assert call(cap, reserved=1) == N.FB_ERR_INVAL
        assert call(untimed) == 0 and call(untimed, flags=1) == N.FB_ERR_INVAL
        assert call(bare) == N.FB_ERR_INVAL
        q = np.zeros(1, dtype=N.VIEW_QUERY_DTYPE)
        assert lib.fb_flow_learn_endpoints_dev(cap.ctx, None, d_out.ptr, 16, d_n.ptr, None, None) == N.FB_ERR_INVAL
        assert lib.fb_flow_learn_endpoints_dev(cap.ctx, N.ptr(q), d_out.ptr, 16, None, None, None) == N.FB_ERR_INVAL
        assert lib.fb_flow_learn_endpoints_dev(cap.ctx, N.ptr(q), None, 16, d_n.ptr, None, None) == N.FB_ERR_INVAL
        assert lib.fb_flow_learn_endpoints_dev(cap.ctx, N.ptr(q), C.c_void_p(d_out.ptr.value + 8), 8, d_n.ptr, None,
                                               None) == N.FB_ERR_INVAL
        assert lib.fb_flow_learn_endpoints_dev(None, N.ptr(q), d_out.ptr, 16, d_n.ptr, None, None) == N.FB_ERR_INVAL
        check(cap)  # (and the refusals left the context usable)
    finally:
        cap.close()
        untimed.close()
        bare.close()


def test_edges():
    lib = N.gpu_lib()
    cap = capture()
    try:
        recs, st = check(cap)  # an empty table
        assert len(recs) == 0 and st == {"flows": 0, "selected": 0, "endpoints": 0, "written": 0, "rounds": 0}
        inject(cap, LC.distinct(40) + LC.group(9))
        base, _ = check(cap)
        n = len(base)
        assert n == 41
        q = np.zeros(1, dtype=N.VIEW_QUERY_DTYPE)
        q[0]["set"], q[0]["filter"] = N.FB_VIEW_ALL, N.FB_FILTER_ALL

        def call(cap_records):
            """(the whole 64-record buffer, pre-filled with 0xAB; *d_n; the counters)"""
            d_out, d_n = N.DeviceBuffer(64 * 64), N.DeviceBuffer(8)
            d_out.upload(np.full(64 * 64, 0xAB, dtype=np.uint8))
            d_n.upload(np.full(1, 77, dtype=np.uint64))
            st = np.zeros(1, dtype=N.LEARN_STATS_DTYPE)
            N.check(lib.fb_flow_learn_endpoints_dev(cap.ctx, N.ptr(q), d_out.ptr if cap_records else None, cap_records,
                                                    d_n.ptr, N.ptr(st), None))
            return (d_out.download(np.zeros(64 * 64, dtype=np.uint8)), int(d_n.download(np.zeros(1, dtype=np.uint64))[0]),
                    {f: int(st[0][f]) for f in N.LEARN_STATS_FIELDS})

        buf, cnt, st = call(0)  # the count only
        assert cnt == n and (buf == 0xAB).all() and (st["endpoints"], st["written"]) == (n, 0)
        buf, cnt, st = call(10)  # the first ten, the full count
        assert cnt == n and buf[:640].tobytes() == base[:10].tobytes() and (buf[640:] == 0xAB).all()
        assert (st["endpoints"], st["written"]) == (n, 10)
        buf, cnt, st = call(64)
        assert cnt == n and buf[:64 * n].tobytes() == base.tobytes() and (buf[64 * n:] == 0xAB).all()
        again, cnt2, st2 = call(64)  # an unchanged table: identical bytes
        assert cnt2 == n and again.tobytes() == buf.tobytes() and st2 == st
        assert not base["reserved"].any() and not base["reserved2"].any()
    finally:
        cap.close()


def by_fingerprint(eps):
    return sorted(eps, key=lambda e: json.dumps([e[f] for f in sorted(e) if f != "description"]))


def test_python_create_install_augment():
    corpus = LC.representatives() + LC.one_field_apart() + LC.mixed_local()
    cap = capture()
    try:
        inject(cap, corpus)
        text = cap.create_custom_whitelists(on_device=True)
        host = cap.create_custom_whitelists()  # (flows_to_sessions sorts by Session's Ord: the first is the least)
        assert "\n" in text  # pretty
        dev, ref = json.loads(text), json.loads(host)
        assert [w["name"] for w in dev["whitelists"]] == ["custom_whitelist"] and dev["whitelists"][0]["extends"] is None
        assert (dev["date"], dev["signature"]) == (ref["date"], None)
        eps = dev["whitelists"][0]["endpoints"]
        assert by_fingerprint(eps) == by_fingerprint(ref["whitelists"][0]["endpoints"]) and len(eps) == 38
        # process names: the host path, whatever on_device says
        procs = {p.session: "curl" for p in pkts(corpus[:5])}
        assert cap.create_custom_whitelists(process_names=procs, on_device=True) == cap.create_custom_whitelists(process_names=procs)
        assert '"curl"' in cap.create_custom_whitelists(process_names=procs, on_device=True)
        # a dictionary stands for dst_domain on both paths
        dns = LC.dns_for(corpus)
        dev_d = json.loads(cap.create_custom_whitelists(dns_resolutions=dns, on_device=True))["whitelists"][0]["endpoints"]
        ref_d = json.loads(cap.create_custom_whitelists(dns_resolutions=dns))["whitelists"][0]["endpoints"]
        assert by_fingerprint(dev_d) == by_fingerprint(ref_d) and any(e["domain"] for e in dev_d)
        # installing the learned list makes every flow Conforming
        st = cap.set_custom_whitelists(text)
        assert st["conforming"] == st["flows"] == len(cap.export_flows()) and cap.get_whitelist_conformance()
        # the learn / check / augment loop: one endpoint missing, a parent list named
        doc = json.loads(text)
        popped = doc["whitelists"][0]["endpoints"].pop(7)
        doc["whitelists"][0]["extends"] = ["base"]
        base = {"name": "base", "extends": None, "endpoints": []}
        doc["whitelists"].append(base)
        st = cap.set_custom_whitelists(json.dumps(doc))
        assert st["nonconforming"] > 0 and not cap.get_whitelist_conformance()
        aug = cap.augment_custom_whitelists()
        assert "\n" not in aug and aug == json.dumps(json.loads(aug), separators=(",", ":"))  # compact
        got = json.loads(aug)
        assert len(got["whitelists"]) == 1 and got["signature"] is None and got["date"] == dev["date"]
        info = got["whitelists"][0]
        assert (info["name"], info["extends"]) == ("custom_whitelist", ["base"])
        assert info["endpoints"] == doc["whitelists"][0]["endpoints"] + [popped]  # existing first, the popped one back
        full = FlodbaddGpuCapture.merge_custom_whitelists(aug, json.dumps({"date": "", "signature": None, "whitelists": [base]}))
        st = cap.set_custom_whitelists(full)
        assert st["conforming"] == st["flows"] and cap.get_whitelist_conformance()
        again = json.loads(cap.augment_custom_whitelists())  # nothing to add
        assert again["whitelists"][0]["endpoints"] == info["endpoints"]
        # no active list: no exceptions -- the current custom list, re-dated
        cap.set_whitelist("")
        plain = json.loads(cap.augment_custom_whitelists())
        assert plain["whitelists"][0]["endpoints"] == info["endpoints"] and plain["whitelists"][0]["extends"] == ["base"]
    finally:
        cap.close()


def test_python_learns_domains_from_the_tracked_resolutions():
    cap, ref = T.new_capture(flow_capacity=1 << 9)
    try:
        inject(cap, [("TCP", "10.12.0.1", 61800, "198.51.100.7", 443), ("TCP", "10.12.0.2", 61801, "198.51.100.7", 443),
                     ("TCP", "10.12.0.1", 61802, "203.0.113.9", 443), ("UDP", "10.12.0.1", 61803, "192.0.2.55", 4000)])
        resolve(cap, ref, {"198.51.100.7": "video.example.com", "203.0.113.9": "tcp.example.com"})
        eps = json.loads(cap.create_custom_whitelists(on_device=True))["whitelists"][0]["endpoints"]  # no dictionary
        assert {(e["ip"], e["domain"]) for e in eps} == {("198.51.100.7", "video.example.com"), ("203.0.113.9", "tcp.example.com"),
                                                         ("192.0.2.55", None)}
        tracked = {str(ip): name for ip, name in cap.dns_resolutions().items()}
        want = json.loads(cap.create_custom_whitelists(dns_resolutions=tracked))["whitelists"][0]["endpoints"]
        assert by_fingerprint(eps) == by_fingerprint(want)
        st = cap.set_custom_whitelists(json.dumps({"date": "d", "signature": None, "whitelists": [
            {"name": "custom_whitelist", "extends": None, "endpoints": [{"domain": "video.example.com", "port": 443}]}]}))
        assert st["nonconforming"] == 2
        aug = json.loads(cap.augment_custom_whitelists())["whitelists"][0]["endpoints"]
        assert [(e["ip"], e["domain"]) for e in aug[:1]] == [(None, "video.example.com")]
        assert {(e["ip"], e["domain"]) for e in aug[1:]} == {("203.0.113.9", "tcp.example.com"), ("192.0.2.55", None)}
        st = cap.set_custom_whitelists(json.dumps({"date": "d", "signature": None, "whitelists": [
            {"name": "custom_whitelist", "extends": None, "endpoints": aug}]}))
        assert st["conforming"] == st["flows"] == 4
    finally:
        cap.close()
