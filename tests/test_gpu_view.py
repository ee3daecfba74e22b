"""The view export and the stamp plane on the GPU (fb_flow_export_view, fb_set_pass_time, fb_flow_modified_dev;
flodbadd_amd/csrc/fb_view.hip and the stamped instances of the three pass kernels).

The view is compared, byte for byte and for every flow, with the join by slot of the exports that existed
before it (flow records, time records, the status / whitelist / blacklist / anomaly planes) plus the raw
stamps; the stamps with what the passes report as changed; the Python getters with tests/modref.py and, field
for field, with tests/joinref.py -- the same join done on the host from the separate exports.  No
tolerance applies anywhere: every value is an integer or a copied record.  Tables are 2^12 slots with about
700 flows, so the sweep's 256-slot steps are partly selected."""
import ctypes as C
import functools
import ipaddress
import json

import numpy as np
import pytest

import joinref
import modref
from flodbadd_amd import _native as N
from flodbadd_amd import analyzer as AN
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.enrich import blacklists_from_json
from flodbadd_amd.sessions import Protocol, Session, SessionFilter, SessionPacketData
from flodbadd_amd.whitelists import rows_from_flows

pytestmark = pytest.mark.gpu

S = 10 ** 9
T0 = 1_700_000_000 * S
NFLOWS = 700
SETS = (N.FB_VIEW_ALL, N.FB_VIEW_CURRENT, N.FB_VIEW_BLACKLISTED, N.FB_VIEW_WL_EXCEPTIONS, N.FB_VIEW_ANOMALOUS)
FILTERS = (SessionFilter.LocalOnly, SessionFilter.GlobalOnly, SessionFilter.All)
NO_STATS = ([0.0] * 10, [0.0] * 10, False)


def doc(*lists):
    return {"date": "d", "signature": "s", "blacklists": [{"name": n, "ip_ranges": list(r)} for n, r in lists]}


L1 = doc(("a", ["20.0.0.0/18", "2001:db8:3::/48"]))
L2 = doc(("a", ["20.0.16.0/20", "2001:db8:3::/48"]), ("b", ["20.0.24.0/21", "20.0.128.0/18"]))


@functools.lru_cache(maxsize=None)
def flow_packets(n):
    """n flows, one packet each (so the slot order of a table is not the flow order): IPv4 / IPv6, TCP / UDP,
    LAN and global destinations.  Flow k's packet has capture time T0 + 1000 k ns; flow 5's is 1 ns after
    flow 4's, for the strict comparison."""
    pk = []
    for k in range(n):
        udp = (k % 4) == 1
        if k % 3 == 0:
            src = "fd00::5"
            dst = "fd00::%x" % (k + 16) if k % 7 == 0 else "2001:db8:%x::%x" % ((k // 3) % 5, k + 1)
        else:
            src = ("192.168.1.9", "10.1.2.3", "172.16.5.5")[k % 3]
            dst = "192.168.7.%d" % (k % 250 + 1) if k % 7 == 0 else "20.0.%d.%d" % (k % 250, k // 250 + 1)
        s = Session(Protocol.UDP if udp else Protocol.TCP, ipaddress.ip_address(src), 40001 + 2 * k,
                    ipaddress.ip_address(dst), (443, 53, 22, 80)[k % 4])
        pk.append(SessionPacketData(s, 100 + k % 50, 140 + k % 50, None if udp else 2))
    ts = T0 + np.arange(n, dtype=np.uint64) * 1000
    if n > 5:
        ts[5] = ts[4] + 1
    return pk, ts


def make_cap(timed=True, flow_capacity=1 << 12, grow=False, n=NFLOWS):
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=flow_capacity, timed=timed, grow=grow)
    pk, ts = flow_packets(n)
    cap.process_parsed(list(pk), ts=ts if timed else None)
    assert cap.flow_count() == n
    return cap


def quiet_model(cap, seed):
    """A forest trained on the table's own vectors, with score thresholds no flow reaches and no statistics:
    every level is 1 (normal) and every diagnostic mask 0, whatever the path sums."""
    feats, _ = cap.export_features()
    data = feats[np.lexsort(feats.T[::-1])]
    data = data[::max(len(data) // AN.MAX_SAMPLES, 1)][:AN.MAX_SAMPLES]
    return AN.train_forest(data, seed), NO_STATS, (0.99, 0.995)


def loud_model(cap, seed):
    """... with thresholds at the 70th / 95th percentile of the host's scores: all three levels occur."""
    forest, stats, _ = quiet_model(cap, seed)
    sc = np.sort(forest.score(cap.export_features()[0]))
    return forest, stats, (float(sc[int(0.70 * len(sc))]), float(sc[int(0.95 * len(sc))]))


def install_lists(cap, d):
    arr, names = blacklists_from_json(d)
    cap.set_blacklists(arr, names)


def by_slot(a, field="slot"):
    return a[np.argsort(a[field], kind="stable")]


def expected_views(cap, vset=N.FB_VIEW_ALL, flt=SessionFilter.All, since=None):
    """The join by slot of the separate exports, restricted by the set's rule, slot order."""
    flows = by_slot(cap.export_flows(flt))
    sl = flows["slot"]
    v = np.zeros(len(flows), dtype=N.FLOW_VIEW_DTYPE)
    v["rec"] = flows
    if cap.timed:
        times = by_slot(cap.export_times())
        t = times[np.searchsorted(times["slot"], sl)]
        assert (t["slot"] == sl).all()
        v["time"] = t
    else:
        v["time"]["slot"] = sl
    v["stamp_ns"] = cap.modified_stamps()[sl]
    v["last_modified_ns"] = np.maximum(v["time"]["last_activity_ns"], v["stamp_ns"])
    v["bl_mask"] = cap.blacklist_masks()[sl]
    v["an"] = cap.anomaly_records()[sl]
    v["status"] = cap.status_bytes()[sl]
    v["wl_state"] = cap.whitelist_bytes()[sl]
    keep = {N.FB_VIEW_ALL: np.ones(len(v), dtype=bool),
            N.FB_VIEW_CURRENT: (v["status"] == 0) | ((v["status"] & N.STATUS_CURRENT) != 0),
            N.FB_VIEW_BLACKLISTED: v["bl_mask"] != 0,
            N.FB_VIEW_WL_EXCEPTIONS: (v["wl_state"] & N.FB_WL_NONCONFORMING) != 0,
            N.FB_VIEW_ANOMALOUS: v["an"]["level"] >= 2}[vset]
    if since is not None:
        keep = keep & (v["last_modified_ns"] > np.uint64(since))
    return v[keep]


def got_views(cap, vset=N.FB_VIEW_ALL, flt=SessionFilter.All, since=None):
    v = cap.export_view(vset, since, flt)
    assert len(set(v["rec"]["slot"].tolist())) == len(v)
    return v[np.argsort(v["rec"]["slot"], kind="stable")]


def check_join(cap, sizes=None):
    """Every set x every filter: the view equals the join, byte for byte; returns {(set, filter): flows}."""
    out = {}
    for vset in SETS:
        for flt in FILTERS:
            want, got = expected_views(cap, vset, flt), got_views(cap, vset, flt)
            assert len(got) == len(want), (vset, flt, len(got), len(want))
            assert got.tobytes() == want.tobytes(), (vset, flt)
            assert (got["rec"]["slot"] == got["time"]["slot"]).all() and not got["reserved"].any()
            out[(vset, int(flt))] = len(got)
    print("view sizes:", out)
    return out


def view_dev(cap, vset=N.FB_VIEW_ALL, since=None, flt=SessionFilter.All, room=0, guard=2, flags=None):
    """fb_flow_export_view_dev into a buffer of room + guard records pre-filled with 0xA5 ->
    (the return code, *d_n, the first `room` records, whether everything past them is untouched)."""
    q = np.zeros(1, dtype=N.VIEW_QUERY_DTYPE)
    q[0]["set"], q[0]["filter"] = int(vset), int(flt)
    if since is not None:
        q[0]["flags"], q[0]["since_ns"] = N.FB_VIEW_MODIFIED_SINCE, int(since)
    if flags is not None:
        q[0]["flags"] = flags
    raw = np.full((room + guard) * 256, 0xA5, dtype=np.uint8)
    d_out, d_n = N.DeviceBuffer(max(raw.nbytes, 256)), N.DeviceBuffer(8).upload(np.full(1, 77, dtype=np.uint64))
    if raw.size:
        d_out.upload(raw)
    rc = N.gpu_lib().fb_flow_export_view_dev(cap.ctx, N.ptr(q), d_out.ptr if raw.size else None, room, d_n.ptr, None)
    if rc:
        return rc, None, None, None
    n = int(d_n.download(np.zeros(1, dtype=np.uint64))[0])
    if raw.size:
        d_out.download(raw)
    return rc, n, raw[: room * 256].view(N.FLOW_VIEW_DTYPE), bool((raw[room * 256:] == 0xA5).all())


def dressed_cap(timed=True):
    """700 flows after an aging call that leaves some outside current_sessions (timed), a blacklist pass with
    the fallback, a whitelist pass, an anomaly pass on all three levels and -- under a pass time -- a list
    change, so that some flows carry a stamp and others none."""
    cap = make_cap(timed)
    if timed:
        pk, ts = flow_packets(NFLOWS)
        late = list(pk[::3])
        cap.process_parsed(late, ts=T0 + 400 * S + np.arange(len(late), dtype=np.uint64) * 1000)
        st = cap.update_sessions_status(T0 + 500 * S, purge=False)
        assert 0 < st["current"] < st["flows"]
    install_lists(cap, L1)
    cap.update_blacklist(mark_whitelist=True)             # pass time 0: no stamps yet
    cap.install_whitelist(rows_from_flows(cap.export_flows()[::2]))
    cap.whitelist_pass()
    cap.set_anomaly_model(*loud_model(cap, 11))
    a = cap.anomaly_pass()
    assert min(a["normal"], a["suspicious"], a["abnormal"]) > 5
    cap.set_pass_time(T0 + 600 * S)
    install_lists(cap, L2)
    assert 20 < cap.update_blacklist(mark_whitelist=True)["changed"] < NFLOWS // 2
    return cap


# ---- 1. the join ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [False, True], ids=["staged", "direct"])
def test_view_equals_the_join_of_the_separate_exports(direct):
    cap = dressed_cap(timed=True)
    try:
        N.check(N.gpu_lib().fb_debug_set(cap.ctx, N.FB_DEBUG_VIEW_DIRECT, 1 if direct else 0))
        sizes = check_join(cap)
        n = sizes[(N.FB_VIEW_ALL, int(SessionFilter.All))]
        assert n == NFLOWS and all(0 < sizes[(s, int(SessionFilter.All))] < n for s in SETS[1:])
        assert all(0 < sizes[(N.FB_VIEW_ALL, int(f))] < n for f in FILTERS[:2])
        v = got_views(cap)
        assert v["stamp_ns"].any() and (v["stamp_ns"] == 0).any()
    finally:
        cap.close()


def test_view_on_an_untimed_context():
    cap = dressed_cap(timed=False)
    try:
        sizes = check_join(cap)
        assert sizes[(N.FB_VIEW_CURRENT, int(SessionFilter.All))] == NFLOWS     # no status plane: every flow is current
        v = got_views(cap)
        t = v["time"].copy()
        t["slot"] = 0
        assert not t.view(np.uint8).any()                                       # zeros except the slot
        assert (v["last_modified_ns"] == v["stamp_ns"]).all() and v["stamp_ns"].any()
    finally:
        cap.close()


def test_view_before_any_pass():
    cap = make_cap(timed=True)
    try:
        sizes = check_join(cap)
        for flt in FILTERS:
            assert sizes[(N.FB_VIEW_CURRENT, int(flt))] == sizes[(N.FB_VIEW_ALL, int(flt))]   # a zero byte is current
            for s in (N.FB_VIEW_BLACKLISTED, N.FB_VIEW_WL_EXCEPTIONS, N.FB_VIEW_ANOMALOUS):
                assert sizes[(s, int(flt))] == 0                                             # no plane: nothing
        v = got_views(cap)
        assert not (v["stamp_ns"].any() or v["bl_mask"].any() or v["status"].any() or v["wl_state"].any())
        assert not np.ascontiguousarray(v["an"]).view(np.uint8).any()
        assert (v["last_modified_ns"] == v["time"]["last_activity_ns"]).all()
    finally:
        cap.close()


# ---- 2. selection sizes ----------------------------------------------------------------------------------
def test_selection_sizes_and_the_strict_comparison():
    cap = make_cap(timed=True)
    try:
        allv = expected_views(cap)
        lm = np.sort(allv["last_modified_ns"])
        assert len(set(lm.tolist())) == NFLOWS                       # distinct: a threshold selects an exact count
        for want_n in (0, 1, 63, 64, 65, 255, 256, 257, NFLOWS):
            since = int(lm[NFLOWS - want_n - 1]) if want_n < NFLOWS else int(lm[0]) - 1
            got, want = got_views(cap, since=since), expected_views(cap, since=since)
            assert len(want) == want_n and got.tobytes() == want.tobytes(), want_n
        # flow 4's packet at t, flow 5's at t + 1 ns: since = t excludes the first and includes the second
        t = T0 + 4000
        got = got_views(cap, since=t)
        assert t not in got["last_modified_ns"].tolist() and t + 1 in got["last_modified_ns"].tolist()
        assert len(got) == NFLOWS - 5
        assert t in got_views(cap, since=t - 1)["last_modified_ns"].tolist()
        # cap below the matches: *d_n is the full count, nothing past cap is written; cap = 0 works
        want = {r.tobytes() for r in allv}
        for room in (0, 1, 64, 100, 129, 300, NFLOWS, NFLOWS + 3):
            rc, n, recs, clean = view_dev(cap, room=room)
            assert rc == 0 and n == NFLOWS and clean, room
            m = min(room, NFLOWS)
            assert len({r.tobytes() for r in recs[:m]} & want) == m, room
            assert (recs[m:].view(np.uint8) == 0xA5).all()
        rc, n, _, _ = view_dev(cap, room=0, guard=0)                 # d_out NULL with cap 0
        assert rc == 0 and n == NFLOWS
        rc, n, recs, clean = view_dev(cap, since=int(lm[NFLOWS - 258]), room=130)
        assert rc == 0 and n == 257 and clean and len({r.tobytes() for r in recs} & want) == 130
    finally:
        cap.close()


# ---- 3. stamps -------------------------------------------------------------------------------------------
def stamps_by_key(cap):
    fl, st = cap.export_flows(), cap.modified_stamps()
    return {Session.from_key(r): int(st[int(r["slot"])]) for r in fl}


def plane_by_key(cap, plane):
    fl = cap.export_flows()
    return {Session.from_key(r): plane[int(r["slot"])] for r in fl}


def test_what_the_passes_stamp():
    cap = make_cap(timed=True)
    t1, t2, t3, t4, t5, t6 = (T0 + k * S for k in (10, 20, 30, 40, 50, 60))
    try:
        # pass time 0: nothing is stamped, last_modified is the last packet's time
        install_lists(cap, L1)
        st = cap.update_blacklist(mark_whitelist=True)
        assert st["changed"] > 50 and st["wl_marked"] == st["changed"]
        cap.install_whitelist(rows_from_flows(cap.export_flows()[::2]))
        assert cap.whitelist_pass()["changed"] == NFLOWS
        v = got_views(cap)
        assert not v["stamp_ns"].any() and not cap.modified_stamps().any()
        assert (v["last_modified_ns"] == v["time"]["last_activity_ns"]).all()
        N.check(N.gpu_lib().fb_clear_whitelist(cap.ctx))
        install_lists(cap, doc())
        assert cap.update_blacklist(mark_whitelist=False)["blacklisted"] == 0
        # a list change under a pass time stamps exactly the flows whose mask changed
        cap.set_pass_time(t1)
        install_lists(cap, L1)
        st = cap.update_blacklist(mark_whitelist=False)
        m1, s1 = plane_by_key(cap, cap.blacklist_masks()), stamps_by_key(cap)
        assert {k for k, v in s1.items() if v} == {k for k, m in m1.items() if m} and set(s1.values()) == {0, t1}
        assert st["changed"] == sum(1 for v in s1.values() if v) > 50
        # a second change, with the fallback: the flows whose mask flips and the flows it marks, and no other
        cap.set_pass_time(t2)
        install_lists(cap, L2)
        st = cap.update_blacklist(mark_whitelist=True)
        m2, s2 = plane_by_key(cap, cap.blacklist_masks()), stamps_by_key(cap)
        flipped = {k for k in m1 if int(m1[k]) != int(m2[k])}
        marked = {k for k, m in m2.items() if m}                      # (every whitelist byte was 0)
        assert st["changed"] == len(flipped) > 20 and st["wl_marked"] == len(marked) > 20
        assert flipped - marked and marked - flipped                  # cleared flows, and marked ones whose mask stayed
        assert {k for k, v in s2.items() if v == t2} == flipped | marked
        assert all(s2[k] == s1[k] for k in s2 if k not in flipped | marked)
        # the same lists again: nothing changes, nothing is stamped
        cap.set_pass_time(t3)
        st = cap.update_blacklist(mark_whitelist=True)
        assert st["changed"] == st["wl_marked"] == 0 and stamps_by_key(cap) == s2
        # a whitelist change does the same
        flows = cap.export_flows()
        cap.install_whitelist(rows_from_flows(flows[::2]))
        w0, st = plane_by_key(cap, cap.whitelist_bytes()), cap.whitelist_pass()
        w1, s3 = plane_by_key(cap, cap.whitelist_bytes()), stamps_by_key(cap)
        changed = {k for k in w0 if int(w0[k]) != int(w1[k])}
        assert st["changed"] == len(changed) and {k for k, v in s3.items() if v == t3} == changed
        assert len(changed) > NFLOWS - 60 and all(s3[k] == s2[k] for k in s3 if k not in changed)
        cap.set_pass_time(t4)
        cap.install_whitelist(rows_from_flows(flows[::3]))
        st = cap.whitelist_pass()
        w2, s4 = plane_by_key(cap, cap.whitelist_bytes()), stamps_by_key(cap)
        changed = {k for k in w1 if int(w1[k]) != int(w2[k])}
        assert 50 < st["changed"] == len(changed) < NFLOWS - 50
        assert {k for k, v in s4.items() if v == t4} == changed and all(s4[k] == s3[k] for k in s4 if k not in changed)
        # the anomaly pass stamps a new level or new diagnostic codes, not a new path sum
        cap.set_pass_time(t5)
        cap.set_anomaly_model(*quiet_model(cap, 11))
        st = cap.anomaly_pass()
        a1 = plane_by_key(cap, cap.anomaly_records())
        assert st["changed"] == st["normal"] == NFLOWS and set(stamps_by_key(cap).values()) == {t5}   # level 0 -> 1
        cap.set_pass_time(t6)
        cap.set_anomaly_model(*quiet_model(cap, 12))
        st = cap.anomaly_pass()
        a2 = plane_by_key(cap, cap.anomaly_records())
        moved = sum(1 for k in a1 if a1[k]["path_sum"] != a2[k]["path_sum"])
        assert st["changed"] == moved > NFLOWS // 2 and st["normal"] == NFLOWS
        assert set(stamps_by_key(cap).values()) == {t5}                                               # nothing stamped
        cap.set_anomaly_model(*loud_model(cap, 12))
        st = cap.anomaly_pass()
        a3, s6 = plane_by_key(cap, cap.anomaly_records()), stamps_by_key(cap)
        shown = {k for k in a2 if (int(a2[k]["level"]), int(a2[k]["diag"])) != (int(a3[k]["level"]), int(a3[k]["diag"]))}
        assert shown and {k for k, v in s6.items() if v == t6} == shown == {k for k in a3 if a3[k]["level"] >= 2}
        # aging never stamps
        cap.set_pass_time(T0 + 70 * S)
        ag = cap.update_sessions_status(T0 + 500 * S, purge=False)
        assert ag["deactivated"] == NFLOWS and stamps_by_key(cap) == s6
        # a stamp older than the last packet loses the max, a newer one wins
        v = got_views(cap)
        assert (v["last_modified_ns"] == np.maximum(v["time"]["last_activity_ns"], v["stamp_ns"])).all()
        assert (v["stamp_ns"] > v["time"]["last_activity_ns"]).all()
        pk, _ = flow_packets(NFLOWS)
        cap.process_parsed(list(pk[:100]), ts=T0 + 1000 * S + np.arange(100, dtype=np.uint64))
        v = got_views(cap)
        newer = v["time"]["last_activity_ns"] > v["stamp_ns"]
        assert int(newer.sum()) == 100 and (v["last_modified_ns"][newer] == v["time"]["last_activity_ns"][newer]).all()
        assert (v["last_modified_ns"][~newer] == v["stamp_ns"][~newer]).all()
        assert len(got_views(cap, since=T0 + 999 * S)) == 100
    finally:
        cap.close()


# ---- 4. the stamps follow their flows ----------------------------------------------------------------------
def test_stamps_follow_a_growth_and_clear():
    cuts = (700, 1500, 3000, 4500)      # each batch brings at most twice the new flows of the one before
    pk, ts = flow_packets(cuts[-1])
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12, timed=True, grow=True)
    try:
        cap.process_parsed(list(pk[:cuts[0]]), ts=ts[:cuts[0]])
        assert cap.table_info()["capacity"] == 1 << 12
        cap.set_pass_time(T0 + 10 * S)
        install_lists(cap, L1)
        assert cap.update_blacklist(mark_whitelist=False)["changed"] > 50
        s0 = stamps_by_key(cap)
        gen = cap.table_info()["generation"]
        for a, b in zip(cuts, cuts[1:]):
            cap.process_parsed(list(pk[a:b]), ts=ts[a:b])
        assert cap.table_info()["capacity"] > 1 << 12 and cap.table_info()["generation"] > gen
        assert cap.flow_count() == cuts[-1]
        s1 = stamps_by_key(cap)
        assert all(s1[k] == s0[k] for k in s0) and not any(s1[k] for k in s1 if k not in s0)
        assert int((cap.modified_stamps() != 0).sum()) == sum(1 for v in s0.values() if v)
        v = got_views(cap)
        assert len(v) == cuts[-1] and v.tobytes() == expected_views(cap).tobytes()
        cap.clear_all_sessions()
        assert not cap.modified_stamps().any()
        cap.process_parsed(list(pk[:cuts[0]]), ts=ts[:cuts[0]])
        assert not cap.modified_stamps().any() and not got_views(cap)["stamp_ns"].any()
    finally:
        cap.close()


def test_stamps_follow_a_purge():
    n = 1400
    pk, ts = flow_packets(n)
    late = np.where(np.arange(n) & 1, 2 * 86400 * S, 0).astype(np.uint64)   # every other flow two days later
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12, timed=True, grow=False)
    try:
        cap.process_parsed(list(pk), ts=ts + late)
        cap.set_pass_time(T0 + 10 * S)
        install_lists(cap, L1)
        assert cap.update_blacklist(mark_whitelist=False)["changed"] > 100
        s0 = stamps_by_key(cap)
        old = cap.export_flows()
        old_stamps = cap.modified_stamps()
        ag = cap.update_sessions_status(T0 + 2 * 86400 * S + 100 * S, purge=True)
        assert ag["purged"] == n // 2 and ag["remaining"] == n // 2
        m = np.zeros(1 << 12, dtype=np.uint32)
        cnt = C.c_uint64(0)
        N.check(N.gpu_lib().fb_flow_slot_remap(cap.ctx, N.ptr(m), 1 << 12, C.byref(cnt)))
        new_stamps = cap.modified_stamps()
        moved = 0
        for r in old:                                       # through the purge's own slot map
            d = int(m[int(r["slot"])])
            if d != 0xFFFFFFFF:
                assert int(new_stamps[d]) == int(old_stamps[int(r["slot"])])
                moved += d != int(r["slot"])
        assert moved > 0
        s1 = stamps_by_key(cap)
        assert len(s1) == n // 2 and all(s0[k] == v for k, v in s1.items())
        assert int((new_stamps != 0).sum()) == sum(1 for v in s1.values() if v) > 20
        # a purged flow that returns starts with no stamp
        gone = next(i for i in range(n) if not i & 1 and s0[pk[i].session])
        cap.process_parsed([pk[gone]], ts=np.array([T0 + 2 * 86400 * S + 200 * S], dtype=np.uint64))
        s2 = stamps_by_key(cap)
        assert len(s2) == n // 2 + 1 and s2[pk[gone].session] == 0
        assert got_views(cap).tobytes() == expected_views(cap).tobytes()
    finally:
        cap.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------
def test_refusals():
    lib = N.gpu_lib()
    cap = make_cap(timed=True, n=8)
    untimed = make_cap(timed=False, n=8)
    bare = FlodbaddGpuCapture(0, flow_capacity=0)
    try:
        d_out, d_n = N.DeviceBuffer(256 * 16), N.DeviceBuffer(8)

        def call(c, **kw):
            q = np.zeros(1, dtype=N.VIEW_QUERY_DTYPE)
            for k, v in kw.items():
                q[0][k] = v
            return lib.fb_flow_export_view_dev(c.ctx, N.ptr(q), d_out.ptr, 16, d_n.ptr, None)

        assert call(cap) == 0 and call(cap, set=4, filter=2, flags=1, since_ns=5) == 0
        assert call(cap, set=5) == N.FB_ERR_INVAL and call(cap, set=0xFFFFFFFF) == N.FB_ERR_INVAL
        assert call(cap, filter=3) == N.FB_ERR_INVAL
        assert call(cap, flags=2) == N.FB_ERR_INVAL and call(cap, flags=3) == N.FB_ERR_INVAL
        assert call(cap, reserved=1) == N.FB_ERR_INVAL
        assert call(untimed) == 0 and call(untimed, flags=1) == N.FB_ERR_INVAL
        assert call(bare) == N.FB_ERR_INVAL
        assert lib.fb_flow_export_view_dev(cap.ctx, None, d_out.ptr, 16, d_n.ptr, None) == N.FB_ERR_INVAL
        q = np.zeros(1, dtype=N.VIEW_QUERY_DTYPE)
        assert lib.fb_flow_export_view_dev(cap.ctx, N.ptr(q), C.c_void_p(d_out.ptr.value + 8), 8, d_n.ptr, None) == N.FB_ERR_INVAL
        out, n = np.zeros(16, dtype=N.FLOW_VIEW_DTYPE), C.c_uint64(9)
        q[0]["set"] = 9
        assert lib.fb_flow_export_view(cap.ctx, N.ptr(q), N.ptr(out), 16, C.byref(n), None) == N.FB_ERR_INVAL and n.value == 0
        with pytest.raises(ValueError):
            untimed.get_sessions(incremental=True)
        with pytest.raises(ValueError):
            untimed.get_blacklisted_sessions(incremental=True)
        with pytest.raises(ValueError):
            untimed.get_whitelist_exceptions(incremental=True)
    finally:
        for c in (cap, untimed, bare):
            c.close()


# ---- 6. the Python getters -----------------------------------------------------------------------------------
def sess_of(t):
    return Session(Protocol[t[0]], ipaddress.ip_address(t[1]), t[2], ipaddress.ip_address(t[3]), t[4])


def tuple_of(s):
    return (s.protocol.name, str(s.src_ip), s.src_port, str(s.dst_ip), s.dst_port)


class GpuWorld:
    """modref's world interface over a FlodbaddGpuCapture, with a ModRefWorld run beside it: every getter call
    must return the restatement's sessions, each with the restatement's last_modified."""

    def __init__(self):
        self.cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12, timed=True, grow=False)
        self.ref = modref.ModRefWorld()

    def packet(self, sess, t):
        self.cap.process_parsed([SessionPacketData(sess_of(sess), 100, 140, 2)], ts=np.array([t], dtype=np.uint64))
        self.ref.packet(sess, t)

    def set_pass_time(self, now):
        self.cap.set_pass_time(now)
        self.ref.set_pass_time(now)

    def set_blacklists(self, lists):
        self.cap.set_custom_blacklists(json.dumps(doc(*lists)))
        self.ref.set_blacklists(lists)

    def set_whitelist(self, endpoints):
        eps = [{"ip": ip, "port": port, "protocol": proto} for ip, port, proto in endpoints]
        self.cap.set_custom_whitelists(json.dumps({"date": "today", "signature": None, "whitelists": [
            {"name": "custom_whitelist", "extends": None, "endpoints": eps}]}))
        self.ref.set_whitelist(endpoints)

    def get(self, getter, now=None, incremental=False):
        fn = {"sessions": self.cap.get_sessions, "current": self.cap.get_current_sessions,
              "blacklisted": self.cap.get_blacklisted_sessions, "exceptions": self.cap.get_whitelist_exceptions}[getter]
        infos = fn(now_ns=now, incremental=incremental)
        got = [tuple_of(i.session) for i in infos]
        assert sorted(got) == self.ref.get(getter, now, incremental), (getter, now, incremental)
        for i in infos:
            assert i.last_modified_ns == self.ref.last_modified(tuple_of(i.session)), (getter, i.session)
        if getter == "exceptions":
            assert all(i.is_whitelisted.name == "NonConforming" and i.whitelist_reason for i in infos)
        assert self.cap._fetch_ts == self.ref.m.fetch_ts
        return got

    def last_modified(self, sess):
        got = {tuple_of(i.session): i.last_modified_ns for i in self.cap.get_sessions()}[sess]
        assert got == self.ref.last_modified(sess)
        return got


@pytest.mark.parametrize("getter", modref.SCENARIOS)
def test_reference_incremental_scenarios(getter):
    w = GpuWorld()
    try:
        assert modref.incremental_scenario(w, getter) == modref.T0 + 50 * modref.MS
        w.cap.reset_fetch_timestamps()
        assert set(w.cap._fetch_ts.values()) == {0}
    finally:
        w.cap.close()


info_fields = joinref.info_fields


def wl_doc(eps):
    return json.dumps({"date": "today", "signature": None, "whitelists": [
        {"name": "custom_whitelist", "extends": None, "endpoints": eps}]})


def exact_endpoints(rows):
    return [{"ip": str(Session.from_key(r).dst_ip), "port": int(r["dst_port"]), "protocol": Protocol(int(r["protocol"])).name}
            for r in rows]


def test_incremental_before_any_full_fetch_equals_the_full_fetch():
    cap = make_cap(timed=True)
    ref = modref.ModRef()
    try:
        fl, tm = cap.export_flows(), {int(t["slot"]): int(t["last_activity_ns"]) for t in cap.export_times()}
        for r in fl:
            ref.packet(tuple_of(Session.from_key(r)), tm[int(r["slot"])])
        now = T0 + 100 * S
        cap.set_custom_whitelists(wl_doc(exact_endpoints(cap.export_flows()[::2])))   # pass time 0: no stamps
        cap.set_pass_time(now)
        cap.set_custom_blacklists(json.dumps(L1))                # stamps the flows whose mask it sets
        cap.set_filter(SessionFilter.GlobalOnly)
        for name, fn in (("sessions", cap.get_sessions), ("current", cap.get_current_sessions),
                         ("blacklisted", cap.get_blacklisted_sessions), ("exceptions", cap.get_whitelist_exceptions)):
            inc = fn(now_ns=now, incremental=True)
            assert cap._fetch_ts[name] == 0                      # an incremental fetch never moves the timestamp
            full = fn()                                          # no now_ns: the timestamp stays too
            assert cap._fetch_ts[name] == 0
            assert len(inc) == len(full) > 20, name
            assert [info_fields(i) for i in inc] == [info_fields(i) for i in full], name
            want = joinref.sessions(cap, name)                   # the separate exports, joined on the host
            assert len(want) == len(full)
            joinref.assert_same(inc, want, (name, "incremental"))
            joinref.assert_same(full, want, (name, "full"))
        cap.set_filter(SessionFilter.All)
        # last_modified_ns against the restatement: the list change above ran under `now`
        ref.set_pass_time(now)
        masks = {tuple_of(i.session): 1 for i in cap.get_blacklisted_sessions()}
        assert len(ref.blacklist_pass(lambda k: masks.get(k, 0), mark=False)[0]) == len(masks) > 20
        got = {tuple_of(i.session): i.last_modified_ns for i in cap.get_sessions()}
        assert got == {k: ref.last_modified(k) for k in ref.s} and now in got.values() and len(set(got.values())) > 100
        # a full fetch with a now moves that getter's timestamp only, and empties its next incremental fetch
        cap.get_sessions(now_ns=now + S)
        assert cap._fetch_ts == {"sessions": now + S, "current": 0, "blacklisted": 0, "exceptions": 0}
        assert cap.get_sessions(incremental=True) == [] and len(cap.get_current_sessions(incremental=True)) == NFLOWS
    finally:
        cap.close()


@pytest.mark.parametrize("timed", [True, False], ids=["timed", "untimed"])
def test_getters_equal_the_join_of_the_separate_exports(timed):
    """Every getter's full fetch (timed: its first incremental fetch too) against tests/joinref.py, field for
    field, under both filters, before and after an analysis, and with host verdicts (process names)."""
    cap = dressed_cap(timed)
    try:
        flows = cap.export_flows()
        # exact endpoints for every other flow, and a process endpoint that leaves the other port-22 flows to the host
        cap.set_custom_whitelists(wl_doc(exact_endpoints(flows[::2]) + [{"process": "curl", "port": 22, "protocol": "TCP"}]))
        fns = {"sessions": cap.get_sessions, "current": cap.get_current_sessions, "blacklisted": cap.get_blacklisted_sessions,
               "exceptions": cap.get_whitelist_exceptions, "anomalous": cap.get_anomalous_sessions}
        if not timed:
            with pytest.raises(ValueError):
                cap.get_current_sessions()
            del fns["current"]

        def compare(names, incremental=False):
            sizes = {}
            for name in names:
                got = fns[name](incremental=True) if incremental else fns[name]()
                want = joinref.sessions(cap, name)               # (after the getter: it reads what its passes left)
                joinref.assert_same(got, want, (name, timed, cap._an_mode, int(cap.filter), incremental))
                sizes[name] = len(got)
            print("getter sizes:", timed, cap._an_mode, cap.filter.name, sizes)
            assert all(n > 0 for n in sizes.values()), sizes
            return sizes

        assert cap._an_mode is None and cap.get_anomalous_sessions() == []      # a model on the device, no analysis yet
        for flt in (SessionFilter.GlobalOnly, SessionFilter.All):
            cap.set_filter(flt)
            compare([n for n in fns if n != "anomalous"])
            assert not any("anomaly:" in i.criticality for i in cap.get_sessions())
        cap._an_mode = "model"                                   # what analyze_sessions leaves after its device pass
        for flt in (SessionFilter.GlobalOnly, SessionFilter.All):
            cap.set_filter(flt)
            sizes = compare(fns)
            assert 0 < sizes["anomalous"] < NFLOWS and 0 < sizes["exceptions"] < NFLOWS and 0 < sizes["blacklisted"] < NFLOWS
            assert (sizes["sessions"] == NFLOWS) == (flt == SessionFilter.All)
            if timed:
                assert 0 < sizes["current"] < sizes["sessions"]
                assert compare([n for n in fns if n != "anomalous"], incremental=True) == {k: v for k, v in sizes.items() if k != "anomalous"}
        got = cap.get_sessions()
        assert all("anomaly:" in i.criticality for i in got) and any("blacklist:" in i.criticality for i in got)
        # host verdicts: curl owns some of the flows the pass left to the host; they stop being exceptions
        before = {i.session for i in cap.get_whitelist_exceptions()}
        left = sorted(s for s in before if s.dst_port == 22)
        assert len(left) > 20
        cap.update_whitelist(None, {s: "curl" for s in left[::2]})
        assert cap._wl_host_ok == set(left[::2])
        sizes = compare(["sessions", "exceptions"])
        assert sizes["exceptions"] == len(before) - len(cap._wl_host_ok) > 0
        assert not {i.session for i in cap.get_whitelist_exceptions()} & cap._wl_host_ok
        by_key = {i.session: i for i in cap.get_sessions()}
        assert all(by_key[s].is_whitelisted.name == "Conforming" for s in cap._wl_host_ok)
        assert cap.get_whitelist_conformance() is False
    finally:
        cap.close()


def test_a_capture_without_a_table_has_no_sessions():
    bare = FlodbaddGpuCapture(0, flow_capacity=0)
    try:
        assert bare.get_sessions() == []
    finally:
        bare.close()
