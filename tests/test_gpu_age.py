"""Session aging (fb_flow_age, flodbadd_amd/csrc/fb_age.hip) against the reference's
update_sessions_status (src/capture.rs:1497-1551): the per-flow status byte and the call's counters
against a restatement of that function written here (StatusModel, fed from the oracle's time records),
and the table after a purge against a "subset replay" of the oracle: a fresh oracle table fed the earlier
batches' records restricted to the surviving keys (pkt_index and timestamps unchanged), then the later
batches whole -- which is the full table restricted to the survivors, byte for byte."""
import ctypes as C
import functools

import numpy as np
import pytest

from flodbadd_amd import _native as N
from flodbadd_amd import synth
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.distributed import sort_by_ord
from flodbadd_amd.sessions import Protocol, Session, SessionFilter, SessionPacketData, packets_to_parsed
from oracle import coracle

pytestmark = pytest.mark.gpu

S = 10 ** 9
T0 = 1_700_000_000 * S
ACTIVE, ADDED, ACTIVATED, DEACTIVATED, CURRENT, AGED = 1, 2, 4, 8, 16, 128
GONE = 0xFFFFFFFF


class StatusModel:
    """update_sessions_status per flow key, in exact (Python) integers.  `prev` holds status.active as the
    last call left it; a key it does not hold has the insert status (src/packets.rs:497-502: active)."""

    def __init__(self):
        self.prev = {}

    def age(self, keys, times, now, purge, act=60 * S, cur=180 * S, ret=86400 * S):
        out, removed = {}, set()
        for k, start, last in zip(keys, times["start_time_ns"].tolist(), times["last_activity_ns"].tolist()):
            prev = self.prev.get(k, True)                     # capture.rs:1510
            active = last >= now - act                        # capture.rs:1514
            added = start >= now - act                        # capture.rs:1515
            b = AGED | (ACTIVE if active else 0) | (ADDED if added else 0)
            b |= ACTIVATED if (not prev and active) else 0    # capture.rs:1517
            b |= DEACTIVATED if (prev and not active) else 0  # capture.rs:1519
            b |= CURRENT if now < last + cur else 0           # capture.rs:1531
            out[k] = b
            self.prev[k] = active                             # capture.rs:1528
            if purge and now > last + ret:                    # capture.rs:1536, 1548-1550
                removed.add(k)
        for k in removed:
            del self.prev[k]
        v = list(out.values())
        stats = dict(flows=len(v), active=sum(1 for b in v if b & ACTIVE), added=sum(1 for b in v if b & ADDED),
                     activated=sum(1 for b in v if b & ACTIVATED), deactivated=sum(1 for b in v if b & DEACTIVATED),
                     current=sum(1 for b in v if b & CURRENT), purged=len(removed), remaining=len(v) - len(removed))
        return out, removed, stats


def keyb(recs):
    """The 40-B keys of records (fb_pkt_out / fb_flow_rec) as bytes objects."""
    a = np.ascontiguousarray(recs)
    return [bytes(r) for r in a.view(np.uint8).reshape(len(a), -1)[:, :40]]


def ts_at(n, at_s):
    """Capture timestamps of a batch that starts at T0 + at_s seconds: 1 us apart."""
    return (T0 + at_s * S + np.arange(n, dtype=np.uint64) * 1000).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def batch(n, first, n_flows):
    """(frames, offsets, the oracle's SESSION records) of a C4-mix batch, computed once."""
    fr, of = synth.generate(4, n, first=first, n_flows=n_flows)
    recs = coracle.parse_classify(coracle.make_cfg(2), fr, of)[0]
    for a in (fr, of, recs):
        a.setflags(write=False)
    return fr, of, recs


# generate(4, 6000, first=0, n_flows=1400): 5,992 records, 1,835 flows; generate(4, 4000, first=100000,
# n_flows=700): 961 flows -- 886 in both, 949 only in A, 75 only in B
BATCH_A, BATCH_B = (6000, 0, 1400), (4000, 100000, 700)


def gpu_status(cap):
    fl, sb = cap.export_flows(), cap.status_bytes()
    return {k: int(sb[s]) for k, s in zip(keyb(fl), fl["slot"].tolist())}


def model_age(model, ref, now, purge=False):
    return model.age(keyb(ref.export_sorted()), ref.export_times(), now, purge)


def check_age(cap, model, ref, now, purge=False):
    """One aging call on the GPU and in the model: every flow's byte and the counters agree."""
    want, removed, wst = model_age(model, ref, now, purge)
    got_stats = cap.update_sessions_status(now, purge=purge)
    got = gpu_status(cap)
    print("age at +%.3f s: model %s gpu %s" % ((now - T0) / S, wst, got_stats))
    assert {k: got_stats[k] for k in wst} == wst
    live = {k: b for k, b in want.items() if k not in removed}
    assert got == live
    return want, removed, got_stats


def check_table(cap, ref, tag=""):
    """The GPU table equals the oracle's: every fb_flow_rec field but the slot, and every time record."""
    recs, times = cap.export_flows(), cap.export_times()
    er, et = ref.export_sorted(), ref.export_times()
    assert len(recs) == len(er) == len(times), (tag, len(recs), len(er), len(times))
    recs = sort_by_ord(recs)
    tsl = times[np.argsort(times["slot"], kind="stable")]
    tg = tsl[np.searchsorted(tsl["slot"], recs["slot"])].copy()
    assert (tg["slot"] == recs["slot"]).all(), tag
    assert keyb(recs) == keyb(er), tag
    for f in N.FLOW_REC_DTYPE.names:
        if f != "slot":
            assert (recs[f] == er[f]).all(), (tag, f)
    for f in N.FLOW_TIME_DTYPE.names:
        if f != "slot":
            assert (tg[f] == et[f]).all(), (tag, f)
    return len(er)


def slot_remap(cap):
    capacity = int(cap.table_info()["capacity"])
    m = np.full(capacity, 0x55555555, dtype=np.uint32)
    n = C.c_uint64(0)
    N.check(N.gpu_lib().fb_flow_slot_remap(cap.ctx, N.ptr(m), capacity, C.byref(n)))
    return m[: n.value]


def max_partition(keys, partitions):
    """Fullest partition of a key set: a key's partition is the top bits of fb_flow_hash."""
    lib, cnt = N.gpu_lib(), np.zeros(partitions, dtype=np.int64)
    shift = 64 - (partitions.bit_length() - 1)
    for k in keys:
        a = np.frombuffer(k, dtype=np.uint8).copy()
        cnt[(lib.fb_flow_hash(N.ptr(a)) >> shift) if partitions > 1 else 0] += 1
    return int(cnt.max())


def test_status_transitions_defaults():
    """A at t0; aged at +5 s, +100 s, +100 s again; B at +150 s; aged at +151 s and +200 s (no purge).
    After each call every flow's byte and the counters equal the model's, and over the sequence the model
    shows each flag and `current` both set and clear.  Then the Python surface: get_sessions(now_ns) decodes
    the bytes, get_current_sessions returns the current set."""
    frA, ofA, recA = batch(*BATCH_A)
    frB, ofB, recB = batch(*BATCH_B)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12, timed=True)
    ref, model, seen = coracle.Flows(), StatusModel(), []
    try:
        assert not cap.status_bytes().any()  # no aging call yet: zeros
        tsA = ts_at(6000, 0)
        cap.process_frames(frA, ofA, ts=tsA)
        ref.update(recA, ts=tsA)
        assert not cap.status_bytes().any()
        for at in (5, 100, 100):
            seen.append(check_age(cap, model, ref, T0 + at * S)[0])
        tsB = ts_at(4000, 150)
        cap.process_frames_seg(frB, ofB, ts=tsB)
        ref.update(recB, ts=tsB)
        fresh = set(keyb(recB)) - set(keyb(recA))
        assert len(fresh) == 75 and all(gpu_status(cap)[k] == 0 for k in fresh)  # inserted since: never aged
        for at in (151, 200):
            seen.append(check_age(cap, model, ref, T0 + at * S)[0])
        allb = [b for s in seen for b in s.values()]
        for bit in (ACTIVE, ADDED, ACTIVATED, DEACTIVATED, CURRENT):
            assert any(b & bit for b in allb) and any(not b & bit for b in allb), bit
        check_table(cap, ref, "aging changes no flow")
        # the Python surface at +230 s
        now = T0 + 230 * S
        want, _, _ = model_age(model, ref, now)
        infos = cap.get_sessions(now_ns=now)
        assert len(infos) == len(want) == 1910
        er = ref.export_sorted()
        by_session = {Session.from_key(r): want[k] for r, k in zip(er, keyb(er))}
        for i in infos:
            b = by_session[i.session]
            assert (i.status.active, i.status.added, i.status.activated, i.status.deactivated) == \
                (bool(b & ACTIVE), bool(b & ADDED), bool(b & ACTIVATED), bool(b & DEACTIVATED))
        cur = cap.get_current_sessions()
        assert sorted(i.session.sort_key() for i in cur) == \
            sorted(s.sort_key() for s, b in by_session.items() if b & CURRENT)
        assert 0 < len(cur) < len(infos)
    finally:
        cap.close()


def test_boundaries_exact():
    """Hand-made flows on the boundaries of every comparison (capture.rs:1514-1536); custom spans are not
    used: the reference's 60 s / 180 s / 86400 s.  Exact per flow; the flow idle for exactly the retention
    span is kept, the one 1 ns older removed."""
    now = T0 + 90000 * S
    last = [now - 60 * S,            # 0: active (>=)
            now - 60 * S - 1,        # 1: not active
            now - 180 * S,           # 2: last + 180 s == now: not current (strict)
            now - 180 * S + 1,       # 3: last + 180 s == now + 1 ns: current
            now - 86400 * S,         # 4: last + 86400 s == now: kept (strict)
            now - 86400 * S - 1,     # 5: last + 86400 s == now - 1 ns: removed
            now + 5 * S,             # 6: captured after `now`
            now - 10 * S]            # 7: two packets, the first 100 s before now: active, not added
    pk, ts = [], []
    for f, t in enumerate(last):
        s = Session(Protocol.TCP, "10.0.0.%d" % (f + 1), 40000 + f, "93.184.216.34", 443)
        if f == 7:
            pk.append(SessionPacketData(s, 0, 40, 0x02))
            ts.append(now - 100 * S)
        pk.append(SessionPacketData(s, 100, 140, 0x18))
        ts.append(t)
    ts = np.array(ts, dtype=np.uint64)
    A, D = AGED | ACTIVE, AGED | DEACTIVATED
    want = [A | ADDED | CURRENT, D | CURRENT, D, D | CURRENT, D, D, A | ADDED | CURRENT, A | CURRENT]
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 10, timed=True, grow=False)
    ref, model = coracle.Flows(), StatusModel()
    try:
        res = cap.process_parsed(pk, ts=ts)
        assert res.stats["new_sessions"] == 8
        ref.update(coracle.process_parsed(coracle.make_cfg(2), packets_to_parsed(pk))[0], ts=ts)
        fl = cap.export_flows()
        key_of = {max(int(r["src_port"]), int(r["dst_port"])) - 40000: k for r, k in zip(fl, keyb(fl))}
        mwant, removed, mst = model_age(model, ref, now, purge=True)
        assert [mwant[key_of[f]] for f in range(8)] == want  # the model and the literal table agree
        assert removed == {key_of[5]}
        st = cap.update_sessions_status(now, purge=True)
        got = gpu_status(cap)
        print("boundaries: gpu", {f: got.get(key_of[f]) for f in range(8)}, st)
        assert {f: got.get(key_of[f]) for f in range(8)} == {f: (None if f == 5 else want[f]) for f in range(8)}
        assert {k: st[k] for k in mst} == mst and st["purged"] == 1 and st["remaining"] == 7
        assert cap.flow_count() == 7
    finally:
        cap.close()


def _purge_and_reinsert(flow_capacity, spec_a, spec_b, before=None, track_history=False):
    """A at t0, B at +150 s, a purge at +86500 s (removes exactly the flows only A has), then A's frames
    again at +86600 s."""
    frA, ofA, recA = batch(*spec_a)
    frB, ofB, recB = batch(*spec_b)
    ka, kb = set(keyb(recA)), set(keyb(recB))
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=flow_capacity, timed=True, grow=False,
                             track_history=track_history)
    full, model = coracle.Flows(), StatusModel()
    try:
        tsA, tsB = ts_at(spec_a[0], 0), ts_at(spec_b[0], 150)
        cap.process_frames(frA, ofA, ts=tsA)
        cap.process_frames_seg(frB, ofB, ts=tsB)
        full.update(recA, ts=tsA)
        full.update(recB, ts=tsB)
        if before:
            before(cap, full, ka, kb)
        fl0 = cap.export_flows()
        old_slot = dict(zip(keyb(fl0), fl0["slot"].tolist()))
        hist0 = {k: cap.histories.get(s, "") for k, s in old_slot.items()} if track_history else None
        gen0 = cap.table_info()["generation"]
        now = T0 + 86500 * S
        want, removed, st = check_age(cap, model, full, now, purge=True)
        assert removed == ka - kb and st["purged"] == len(ka - kb)
        # the subset replay
        sub = coracle.Flows()
        sub.update(recA[np.array([k in kb for k in keyb(recA)])], ts=tsA)
        sub.update(recB, ts=tsB)
        assert check_table(cap, sub, "after the purge") == len(kb) == st["remaining"]
        info = cap.table_info()
        assert cap.flow_count() == len(kb) and info["flows"] == len(kb)
        assert info["generation"] == gen0 + 1
        assert info["max_partition"] == st["max_partition"] == max_partition(kb, int(info["partitions"]))
        # the slot map, through the keys
        fl1 = cap.export_flows()
        new_slot = dict(zip(keyb(fl1), fl1["slot"].tolist()))
        m = slot_remap(cap)
        assert len(m) == flow_capacity
        assert all(int(m[old_slot[k]]) == new_slot[k] for k in kb)
        assert all(int(m[old_slot[k]]) == GONE for k in ka - kb)
        assert int((m != GONE).sum()) == len(kb)
        if track_history:  # every survivor's string unchanged (and the oracle's), removed flows have no entry
            assert set(cap.histories) <= set(new_slot.values())
            for r, k in zip(fl1, keyb(fl1)):
                h = cap.histories.get(int(r["slot"]), "")
                assert h == hist0[k] and h == (full.history(r)[0] or ""), k
            assert any(hist0[k] for k in ka - kb) and any(hist0[k] for k in kb)
        # A's frames again: every survivor found, every purged key inserted afresh
        ts3 = ts_at(spec_a[0], 86600)
        res = cap.process_frames(frA, ofA, ts=ts3)
        ost = np.zeros(1, dtype=N.STATS_DTYPE)
        sub.update(recA, ost, ts=ts3)
        print("third batch: gpu new %d updated %d, oracle new %d updated %d" % (
            res.stats["new_sessions"], res.stats["updated_sessions"], int(ost[0]["new_sessions"]),
            int(ost[0]["updated_sessions"])))
        assert int(ost[0]["new_sessions"]) == len(ka - kb)
        assert res.stats["new_sessions"] == int(ost[0]["new_sessions"])
        assert res.stats["updated_sessions"] == int(ost[0]["updated_sessions"])
        check_table(cap, sub, "after the re-insert")
        got = gpu_status(cap)
        assert all(got[k] == 0 for k in ka - kb)
        assert all(got[k] == want[k] for k in kb)
        return st
    finally:
        cap.close()


def test_purge_and_reinsert():
    st = _purge_and_reinsert(1 << 12, BATCH_A, BATCH_B)
    assert st["purged"] == 949 and st["remaining"] == 961


def test_purge_dense_partitions():
    """The same purge on 4 partitions of 512 slots holding 1,523 flows (generate(4, 6000, first=0,
    n_flows=1100): 1,445 flows; generate(4, 4000, first=100000, n_flows=550): 773 flows, 695 in both), the
    fullest 407 slots = 79 % full: probe chains run through the removed flows, so the survivors are only
    found again if their partitions are re-packed.  750 flows (49 %) expire."""
    def before(cap, full, ka, kb):
        mp = cap.table_info()["max_partition"]
        print("dense: %d flows, fullest partition %d, %d expire" % (len(ka | kb), mp, len(ka - kb)))
        assert 0.75 * 512 <= mp <= 0.87 * 512
        assert 0.30 <= len(ka - kb) / len(ka | kb) <= 0.70
    st = _purge_and_reinsert(1 << 11, (6000, 0, 1100), (4000, 100000, 550), before=before)
    assert st["flows"] == 1523 and st["purged"] == 750


def test_history_follows_a_purge():
    _purge_and_reinsert(1 << 12, BATCH_A, BATCH_B, track_history=True)


def test_nothing_expired_changes_nothing():
    frA, ofA, _ = batch(*BATCH_A)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12, timed=True, grow=False)
    try:
        cap.process_frames(frA, ofA, ts=ts_at(6000, 0))
        cap.update_sessions_status(T0 + 5 * S, purge=False)  # (the same status at +5 s and +10 s: comparable too)
        by_slot = lambda a: a[np.argsort(a["slot"], kind="stable")].tobytes()  # noqa: E731 (export order is not fixed)
        snap = lambda: (by_slot(cap.export_flows()), by_slot(cap.export_times()), slot_remap(cap).tobytes(),  # noqa: E731
                        cap.status_bytes().tobytes(), cap.table_info())
        s0 = snap()
        st = cap.update_sessions_status(T0 + 10 * S, purge=True)
        assert st["purged"] == 0 and st["remaining"] == st["flows"] == 1835
        assert snap() == s0
        assert len(slot_remap(cap)) == 0  # no slot map: nothing has moved
    finally:
        cap.close()


def test_growth_carries_status():
    """846 flows (generate(4, 6000, first=0, n_flows=600)) aged inactive at +100 s; a batch at +150 s
    (n_flows=1500: 1,962 flows, 775 of them returning) makes the 2^11-slot table grow; aged at +151 s,
    `activated` is set exactly for the returning flows."""
    spec_a, spec_g = (6000, 0, 600), (6000, 200000, 1500)
    frA, ofA, recA = batch(*spec_a)
    frG, ofG, recG = batch(*spec_g)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11, timed=True)
    ref, model = coracle.Flows(), StatusModel()
    try:
        tsA, tsG = ts_at(6000, 0), ts_at(6000, 150)
        cap.process_frames(frA, ofA, ts=tsA)
        ref.update(recA, ts=tsA)
        want, _, st = check_age(cap, model, ref, T0 + 100 * S)
        assert st["active"] == 0 and st["deactivated"] == 846
        gen0 = cap.table_info()["generation"]
        cap.process_frames(frG, ofG, ts=tsG)
        ref.update(recG, ts=tsG)
        assert cap.table_info()["generation"] > gen0
        want, _, st = check_age(cap, model, ref, T0 + 151 * S)
        ka, kg = set(keyb(recA)), set(keyb(recG))
        assert {k for k, b in want.items() if b & ACTIVATED} == ka & kg
        assert st["activated"] == len(ka & kg) == 775 and len(ka - kg) == 71
        check_table(cap, ref, "after the growth")
    finally:
        cap.close()


def planes_by_key(cap):
    """Per flow key: (status byte, whitelist byte, blacklist mask, time record without its slot); the slot
    of every key; and the three lazily made planes whole."""
    fl, tm = cap.export_flows(), cap.export_times()
    planes = (cap.status_bytes(), cap.whitelist_bytes(), cap.blacklist_masks())
    tms = tm[np.argsort(tm["slot"], kind="stable")]
    tt = tms[np.searchsorted(tms["slot"], fl["slot"])].copy()
    assert len(tm) == len(fl) and (tt["slot"] == fl["slot"]).all()
    tt["slot"] = 0
    slots = fl["slot"].tolist()
    by_key = {k: (int(planes[0][s]), int(planes[1][s]), int(planes[2][s]), t.tobytes())
              for k, s, t in zip(keyb(fl), slots, tt)}
    return by_key, dict(zip(keyb(fl), slots)), planes


def test_all_planes_follow_every_slot_move():
    """All four per-slot planes (time, status, whitelist, blacklist) alive through one purge, one growth and
    one clear: 1,400 flows in 4 partitions of 512 slots (about 350 each), every other one last seen two days
    before the rest; aged without purge, one whitelist pass, one blacklist pass with the fallback."""
    from flodbadd_amd.enrich import blacklists_from_json
    from flodbadd_amd.whitelists import rows_from_flows
    from test_gpu_blacklist import LISTS, mixed_packets, pkt
    day2 = 2 * 86400 * S
    pk = mixed_packets()[:1400]
    ts = np.array([T0 + (0 if k & 1 else day2) + k * 1000 for k in range(len(pk))], dtype=np.uint64)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11, timed=True)
    ref, model = coracle.Flows(), StatusModel()
    try:
        cap.process_parsed(pk, ts=ts)
        ref.update(coracle.process_parsed(coracle.make_cfg(2), packets_to_parsed(pk))[0], ts=ts)
        info = cap.table_info()
        assert info["capacity"] == 1 << 11 and info["max_partition"] > 300
        check_table(cap, ref, "before the passes")
        check_age(cap, model, ref, T0 + day2 + 100 * S, purge=False)
        cap.install_whitelist(rows_from_flows(cap.export_flows()[::2]))
        wst = cap.whitelist_pass()
        cap.set_blacklists(*blacklists_from_json(LISTS))
        bst = cap.update_blacklist(mark_whitelist=True)
        snap, slot0, _ = planes_by_key(cap)
        assert len(snap) == 1400 == wst["flows"] == bst["flows"] and 0 < wst["conforming"] < 1400
        assert 100 < bst["blacklisted"] < 1400
        for j in range(3):  # every plane holds more than one value: a mix-up between flows would show
            assert len({v[j] for v in snap.values()}) > 1, j

        def unoccupied_read_zero(slot, planes):
            free = np.ones(len(planes[0]), dtype=bool)
            free[list(slot.values())] = False
            assert free.sum() == len(free) - len(slot) and not any(p[free].any() for p in planes)

        # 1. a purge that removes half: the survivors keep everything but take the status this call computes
        now = T0 + day2 + 150 * S
        want, removed, wstats = model_age(model, ref, now, purge=True)
        ag = cap.update_sessions_status(now, purge=True)
        assert {k: ag[k] for k in wstats} == wstats and ag["purged"] == len(removed) == 700
        s1, slot1, planes1 = planes_by_key(cap)
        assert set(s1) == set(snap) - removed
        assert all(s1[k] == (want[k],) + snap[k][1:] for k in s1)
        assert any(slot1[k] != slot0[k] for k in s1)
        unoccupied_read_zero(slot1, planes1)
        # 2. 3,000 new flows grow the table: every old flow keeps all four, the new ones read zero
        more = [pkt("UDP", "192.168.1.9", 40001 + 2 * (k % 9000), "48.%d.%d.%d" % (k >> 16, (k >> 8) & 255, k & 255), 53)
                for k in range(3000)]
        cap.process_parsed(more, ts=np.full(3000, now + 100 * S, dtype=np.uint64))
        assert cap.table_info()["capacity"] > 1 << 11
        s2, slot2, planes2 = planes_by_key(cap)
        assert len(s2) == len(s1) + 3000 and all(s2[k] == s1[k] for k in s1)
        assert all(s2[k][:3] == (0, 0, 0) for k in s2 if k not in s1)
        unoccupied_read_zero(slot2, planes2)
        # 3. clear_all_sessions: the three lazily made planes read zero over the whole capacity
        cap.clear_all_sessions()
        planes3 = (cap.status_bytes(), cap.whitelist_bytes(), cap.blacklist_masks())
        assert all(len(p) == cap.table_info()["capacity"] and not p.any() for p in planes3)
    finally:
        cap.close()


def test_refusals():
    lib = N.gpu_lib()
    plain = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 10)
    bare = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=0)
    try:
        st = np.zeros(1, dtype=N.AGE_STATS_DTYPE)
        assert lib.fb_flow_age(plain.ctx, T0, None, 0, N.ptr(st), None) == N.FB_ERR_INVAL  # no clock
        assert b"FB_CFG_TIMED" in lib.fb_last_error()
        assert lib.fb_flow_age(bare.ctx, T0, None, N.FB_AGE_PURGE, None, None) == N.FB_ERR_INVAL  # no table
        with pytest.raises(N.FbError):
            plain.update_sessions_status(T0)
    finally:
        plain.close()
        bare.close()
