"""The anomaly pass on the GPU (fb_flow_anomaly, flodbadd_amd/csrc/fb_anomaly.hip) against the restatement
in tests/anref.py: every feature, every path sum, every record, counter, export and criticality string
must be equal -- doubles are compared by their bits, no tolerance applies.  Tables are 2^9 - 2^12 slots,
flows come in through process_parsed."""
import functools
import ipaddress
import struct

import numpy as np
import pytest

import anforests as F
import anref
import joinref
from flodbadd_amd import _native as N
from flodbadd_amd import analyzer as A
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.enrich import blacklists_from_json
from flodbadd_amd.sessions import Protocol, Session, SessionFilter, SessionPacketData, flows_to_sessions

pytestmark = pytest.mark.gpu

S = 10 ** 9
T0 = 1_700_000_000 * S
OWN = ["93.184.216.34", "2001:db8::34"]
SYN, SYNACK, ACK, PSHACK, FINACK = 0x02, 0x12, 0x10, 0x18, 0x11
CODES = anref.service_codes()
NO_STATS = ([0.0] * 10, [0.0] * 10, False)


def bits(values):
    return [struct.pack("<d", float(v)) for v in values]


def install(cap, forest, stats=NO_STATS, thresholds=(0.75, 0.80)):
    cap.set_anomaly_model(forest, stats, thresholds)


# ---- 1. the walk -------------------------------------------------------------------------------------
@functools.lru_cache(None)
def ref_sums(name):
    forest = F.ALL[name]()
    trees = anref.trees_of(forest.nodes, forest.first)
    return [anref.path_sum(trees, [float(v) for v in x]) for x in F.inputs(1000)]


def device_path_sums(cap, X, guard=64):
    n = len(X)
    d_x, d_o = N.DeviceBuffer(X.nbytes), N.DeviceBuffer(8 * n + guard)
    d_x.upload(X)
    d_o.upload(np.full(8 * n + guard, 0xA5, dtype=np.uint8))
    N.check(N.gpu_lib().fb_if_score_dev(cap.ctx, d_x.ptr, n, d_o.ptr, None))
    raw = d_o.download(np.zeros(8 * n + guard, dtype=np.uint8))
    assert (raw[8 * n:] == 0xA5).all()
    return raw[: 8 * n].view(np.float64)


@pytest.fixture(scope="module")
def score_cap():
    cap = FlodbaddGpuCapture(0, flow_capacity=0)
    yield cap
    cap.close()


@pytest.mark.parametrize("name", sorted(F.ALL))
def test_score_dev_equals_the_restatement(score_cap, name):
    install(score_cap, F.ALL[name]())
    want = ref_sums(name)
    assert len({w for w in want if w == w}) > (1 if name != "leaf_only" else 0)
    for n in (1, 63, 64, 65, 257, 1000):
        got = device_path_sums(score_cap, F.inputs(n))
        bad = [(k, float(got[k]), want[k]) for k in range(n) if bits([got[k]]) != bits([want[k]])]
        print("fb_if_score_dev %s n=%d: %d differ" % (name, n, len(bad)))
        assert not bad, bad[:5]
    if name == "three_nodes":  # the NaN vector goes right, a zero vector left
        x = np.concatenate([F.special_vectors()[4:5], np.zeros((1, 10))])
        assert device_path_sums(score_cap, x).tolist() == [2.5, 1.25]


# ---- 2. no fused multiply-add ------------------------------------------------------------------------
def test_contraction_probe(score_cap):
    probe, x = F.contraction_probe()
    install(score_cap, probe)
    got = device_path_sums(score_cap, x)
    print("contraction probe: path_sum", got[0], "(1.0 = unfused, 2.0 = fused)")
    assert got[0] == 1.0 == anref.path_sum(anref.trees_of(probe.nodes, probe.first), x[0].tolist())


# ---- 3. features -------------------------------------------------------------------------------------
def flow_packets(n_flows):
    """(packets, timestamps): n_flows flows of one to five packets over IPv4 / IPv6, TCP / UDP, towards
    service ports and towards a port without a name, some only ever answered (outbound == 0), some with a
    FIN (end_time), some with PSH segments, some whose later packets carry EARLIER timestamps."""
    pk, ts = [], []
    for k in range(n_flows):
        v6, udp = (k % 3) == 0, (k % 4) == 1
        if v6:
            a = ipaddress.ip_address("fd00::%x" % (k + 1))
            b = ipaddress.ip_address("2001:db8::34" if k % 7 == 0 else "2001:db8:1::%x" % (k + 2))
        else:
            a = ipaddress.ip_address("192.168.%d.%d" % (1 + k // 250, 1 + k % 250))
            b = ipaddress.ip_address("93.184.216.34" if k % 7 == 1 else int(ipaddress.ip_address("20.0.0.0")) + 7919 * k)
        dport = (443, 53, 22, 80, 40002)[k % 5]
        sport = 40001 + 2 * (k % 9000)
        s = Session(Protocol.UDP if udp else Protocol.TCP, a, sport, b, dport)
        back = s.reversed() if dport != 40002 else s   # (between two ports without a name a reply is a session of its own)
        t = T0 + k * 1_000_003
        kind = k % 6
        fl = (lambda f: None) if udp else (lambda f: f)
        seq = []
        if kind == 0:     # one packet: div == 0, duration 0
            seq = [(s, 60 + k % 900, fl(SYN), 0)]
        elif kind == 1:   # answered only: a packet FROM the service port first, so outbound stays 0
            if dport == 40002:
                seq = [(s, 100, fl(SYN), 0), (back, 200 + k % 1000, fl(SYNACK), 1_700_000)]
            else:
                seq = [(back, 200 + k % 1000, fl(ACK), 0), (back, 77, fl(ACK), 2_500_000_000)]
        elif kind == 2:   # PSH segments, seconds apart (below and above the 5-s timeout)
            gaps = [0, 1_234_567_890, 3_000_000_000 + (k % 5) * S, 9_999_999_999 if k % 36 != 2 else 900 * S]
            seq = [(s, 100, fl(SYN), gaps[0]), (s, 500 + k % 700, fl(PSHACK), gaps[1]),
                   (back, 1400, fl(PSHACK), gaps[2]), (s, 90, fl(PSHACK), gaps[3])]
        elif kind == 3:   # ended by a FIN, then one more packet
            seq = [(s, 100, fl(SYN), 0), (back, 60, fl(SYNACK), 900_000), (s, 1000, fl(PSHACK), 2_600_000),
                   (back, 40, fl(FINACK), 3_499_999), (s, 40, fl(ACK), 8_000_000)]
        elif kind == 4:   # clock steps back: the last packet (and the FIN) are earlier than the first
            seq = [(s, 100, fl(SYN), 0), (s, 300, fl(PSHACK), -1_500_000), (back, 50, fl(FINACK if k % 12 == 4 else ACK), -7_123_456_789)]
        else:             # many small packets
            big = 30000 if k % 48 == 5 else 0   # a few bulk transfers
            seq = [(s, 40 + j + big, fl(SYN if j == 0 else ACK), j * 10_000_000) for j in range(5)]
        for sess, plen, flags, dt in seq:
            pk.append(SessionPacketData(sess, plen, plen + 40, flags))
            ts.append(t + dt)
    return pk, np.array(ts, dtype=np.uint64)


def infos_of(cap):
    """The table's sessions as SessionInfo (with capture times on a timed capture) and {Session: slot}."""
    flows = cap.export_flows()
    infos = flows_to_sessions(flows, times=cap.export_times() if cap.timed else None)
    return infos, {Session.from_key(r): int(r["slot"]) for r in flows}


def check_features(cap, infos, slot):
    feats, slots = cap.export_features()
    assert sorted(slots.tolist()) == sorted(slot.values()) and len(feats) == len(infos)
    row = {int(s): feats[k] for k, s in enumerate(slots)}
    bad = []
    for i in infos:
        want = anref.features(i, CODES)
        got = row[slot[i.session]]
        if bits(got) != bits(want):
            bad.append((str(i.session), got.tolist(), want))
        assert A.compute_features(i) == want
    print("features: %d flows, %d differ" % (len(infos), len(bad)))
    assert not bad, bad[:3]
    return row


@pytest.mark.parametrize("slots,n_flows", [(1 << 9, 240), (1 << 12, 3000)], ids=["2^9", "2^12"])
def test_features_equal_the_restatement(slots, n_flows):
    pk, ts = flow_packets(n_flows)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=slots, timed=True, own_ips=OWN, grow=False)
    try:
        cap.process_parsed(pk, ts=ts)     # (no model: export_features installs the default service codes)
        infos, slot = infos_of(cap)
        assert len(infos) == n_flows and cap.table_info()["capacity"] == slots
        row = check_features(cap, infos, slot)
        x = np.array([row[slot[i.session]] for i in infos])
        cover = dict(v4=sum(i.session.src_ip.version == 4 for i in infos), v6=sum(i.session.src_ip.version == 6 for i in infos),
                     tcp=sum(i.session.protocol is Protocol.TCP for i in infos), udp=sum(i.session.protocol is Protocol.UDP for i in infos),
                     no_outbound=sum(i.stats.outbound_bytes == 0 for i in infos), ended=sum(i.stats.end_time_ns is not None for i in infos),
                     not_ended=sum(i.stats.end_time_ns is None for i in infos), no_div=sum(i.stats.segment_interarrival_div == 0 for i in infos),
                     div=sum(i.stats.segment_interarrival_div > 0 for i in infos), negative=int((x[:, 1] < 0).sum()),
                     service=sum(i.dst_service is not None for i in infos), no_service=sum(i.dst_service is None for i in infos),
                     self_dst=sum(i.is_self_dst for i in infos), interarrival=int((x[:, 4] > 0).sum()), ratio=int((x[:, 5] > 0).sum()))
        print("feature cases:", cover)
        assert all(v > 0 for v in cover.values()), cover
        assert int((x[:, 8] == 1.0).sum()) == cover["self_dst"]
        assert int((x[:, 7] > 0).sum()) == cover["service"] and not x[:, 0].any() and not x[:, 9].any()
    finally:
        cap.close()
    # the same flows without a clock: features 1 and 4 are exactly 0.0, the others as before
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=slots, own_ips=OWN, grow=False)
    try:
        install(cap, F.three_nodes())     # (here the codes come with a model)
        cap.process_parsed(pk)
        infos, slot = infos_of(cap)
        row_u = check_features(cap, infos, slot)
        xu = np.array([row_u[slot[i.session]] for i in infos])
        assert len(infos) == n_flows and not xu[:, 1].any() and not xu[:, 4].any()
        assert bits(np.signbit(xu[:, 1]).astype(float)) == bits(np.zeros(n_flows))   # +0.0, not -0.0
        keep = [0, 2, 3, 5, 6, 7, 8, 9]
        assert xu[:, keep].tobytes() == x[:, keep].tobytes()
    finally:
        cap.close()


# ---- 4. the full pass --------------------------------------------------------------------------------
def check_pass(cap, model, known, before):
    """One device pass and one run of the restatement over the same sessions: the plane, the counters, the
    export, the strings.  model: (forest, stats, thresholds); before: the restatement's previous records."""
    forest, stats, thr = model
    infos, slot = infos_of(cap)
    infos = [known.setdefault(i.session, i) for i in infos]
    got_stats = cap.anomaly_pass()
    res = anref.run(infos, anref.trees_of(forest.nodes, forest.first), forest.sample_size, stats[0], stats[1], stats[2], thr,
                    CODES, before)
    print("anomaly pass:", got_stats, "restatement:", res["stats"])
    recs = cap.anomaly_records()
    bad = []
    for s, (total, mask, lvl) in res["records"].items():
        r = recs[slot[s]]
        if bits([r["path_sum"]]) != bits([total]) or int(r["diag"]) != mask or int(r["level"]) != lvl or r["reserved"].any():
            bad.append((str(s), r, (total, mask, lvl)))
    assert not bad, (len(bad), bad[:3])
    assert got_stats == res["stats"]
    assert int((recs["level"] != 0).sum()) == len(infos)          # no record outside the flows
    for min_level in (1, 2, 3):
        fl, rr = cap.export_anomalous_flows(min_level)
        want = {s for s, r in res["records"].items() if r[2] >= min_level}
        assert len(fl) == len(want) and {Session.from_key(r) for r in fl} == want
        assert rr.tobytes() == recs[fl["slot"]].tobytes()
    return res


def quantile_thresholds(forest, feats, lo=0.70, hi=0.95):
    """Score thresholds at two quantiles of the HOST scorer's scores of `feats`: some flows on every level."""
    sc = np.sort(forest.score(feats))
    return float(sc[int(lo * len(sc))]), float(sc[int(hi * len(sc))])


def trained_model(cap, seed, thresholds):
    feats, _ = cap.export_features()
    data = feats[np.lexsort(feats.T[::-1])]                   # (the export's order is not fixed)
    data = data[::max(len(data) // A.MAX_SAMPLES, 1)][:A.MAX_SAMPLES]   # a deterministic choice of 300 vectors
    forest = A.train_forest(data, seed)
    return forest, A.feature_stats(data), thresholds


def test_full_pass_against_the_restatement():
    pk, ts = flow_packets(3000)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12, timed=True, own_ips=OWN, grow=False)
    try:
        cap.process_parsed(pk, ts=ts)
        known = {}
        # the reference's test thresholds
        m1 = trained_model(cap, 11, (0.60, 0.72))
        assert m1[0].n_trees == 25 and m1[0].sample_size == 128
        cap.set_anomaly_model(*m1)
        r1 = check_pass(cap, m1, known, None)
        assert r1["stats"]["flows"] == r1["stats"]["changed"] == 3000 and r1["stats"]["cleared"] == 0
        assert r1["stats"]["newly_anomalous"] == r1["stats"]["suspicious"] + r1["stats"]["abnormal"]
        # the same model again: nothing changes
        r2 = check_pass(cap, m1, known, r1["records"])
        assert r2["stats"] == dict(r1["stats"], changed=0, newly_anomalous=0) and r2["records"] == r1["records"]
        # thresholds at the 70th and 95th percentile of the host's own scores: all three levels occur
        thr = quantile_thresholds(m1[0], cap.export_features()[0])
        assert thr[0] < thr[1]
        m2 = (m1[0], m1[1], thr)
        cap.set_anomaly_model(*m2)
        r3 = check_pass(cap, m2, known, r2["records"])
        st = r3["stats"]
        assert min(st["normal"], st["suspicious"], st["abnormal"]) > 50, st
        diags = {r[1] for r in r3["records"].values() if r[2] >= 2}
        assert 0 in diags and len(diags) >= 3                                       # OverallScoreHigh and named features
        # another forest: the counters stay consistent with the levels before and after
        m3 = trained_model(cap, 12, thr)
        cap.set_anomaly_model(*m3)
        r4 = check_pass(cap, m3, known, r3["records"])
        s4 = r4["stats"]
        assert s4["changed"] == 3000 and s4["newly_anomalous"] > 0 and s4["cleared"] > 0
        assert s4["suspicious"] + s4["abnormal"] == st["suspicious"] + st["abnormal"] + s4["newly_anomalous"] - s4["cleared"]
        # no statistics: the levels stay, every diagnostic mask is zero
        m4 = (m3[0], (m3[1][0], m3[1][1], False), thr)
        cap.set_anomaly_model(*m4)
        r5 = check_pass(cap, m4, known, r4["records"])
        assert not cap.anomaly_records()["diag"].any() and r5["stats"]["changed"] == sum(1 for r in r4["records"].values() if r[1])
        assert {s: r[2] for s, r in r5["records"].items()} == {s: r[2] for s, r in r4["records"].items()}
    finally:
        cap.close()


# ---- 5. the plane follows its flows ------------------------------------------------------------------
def recs_by_key(cap):
    fl, rr = cap.export_flows(), cap.anomaly_records()
    return {Session.from_key(r): rr[int(r["slot"])].tobytes() for r in fl}


ZERO = bytes(16)


def test_records_follow_a_growth_and_clear():
    pk, _ = flow_packets(3000)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9, own_ips=OWN)
    try:
        # the packets of the first 180, 480, 1000, 1900 and 3000 flows: each batch brings at most twice the new
        # flows of the one before, which is what the table's growth projects from
        cuts = [len(flow_packets(n)[0]) for n in (180, 480, 1000, 1900, 3000)]
        first = pk[:cuts[0]]
        cap.process_parsed(first)
        assert cap.table_info()["capacity"] == 1 << 9
        forest = trained_model(cap, 11, None)[0]
        install(cap, forest, thresholds=quantile_thresholds(forest, cap.export_features()[0]))
        st = cap.anomaly_pass()
        r0 = recs_by_key(cap)
        assert st["flows"] == len(r0) == 180 and all(v != ZERO for v in r0.values()) and st["suspicious"] + st["abnormal"] > 0
        # batches that grow the table several times: the records follow by key, the new flows read all zero
        gen = cap.table_info()["generation"]
        for a, b in zip(cuts, cuts[1:]):
            cap.process_parsed(pk[a:b])
        assert cap.table_info()["capacity"] > 1 << 9 and cap.flow_count() == 3000 and cap.table_info()["generation"] > gen + 1
        r1 = recs_by_key(cap)
        assert all(r1[k] == r0[k] for k in r0) and all(r1[k] == ZERO for k in r1 if k not in r0)
        assert int((cap.anomaly_records()["level"] != 0).sum()) == len(r0)
        st = cap.anomaly_pass()
        assert st["flows"] == 3000 and st["changed"] >= 3000 - len(r0)
        assert all(v != ZERO for v in recs_by_key(cap).values())
        # fb_flow_clear zeroes the plane; flows inserted afterwards read all zero
        cap.clear_all_sessions()
        assert not cap.anomaly_records().view(np.uint8).any()
        cap.process_parsed(first)
        assert set(recs_by_key(cap).values()) == {ZERO}
        assert cap.anomaly_pass()["changed"] == len(r0)
        # fb_clear_anomaly_model zeroes it too, and leaves no model
        cap.clear_anomaly_model()
        assert not cap.anomaly_records().view(np.uint8).any()
        assert N.gpu_lib().fb_flow_anomaly(cap.ctx, 0, None, None) == N.FB_ERR_INVAL
    finally:
        cap.close()


def test_records_follow_a_purge():
    pk, ts = flow_packets(1400)
    # every other flow was last seen two days before the rest
    flow_of = {}
    for p in pk:
        key = min(p.session, p.session.reversed(), key=Session.sort_key)
        flow_of.setdefault(key, len(flow_of))
    late = np.array([2 * 86400 * S if flow_of[min(p.session, p.session.reversed(), key=Session.sort_key)] & 1 else 0 for p in pk],
                    dtype=np.uint64)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11, timed=True, grow=False, own_ips=OWN)
    try:
        cap.process_parsed(pk, ts=ts + late)
        forest = trained_model(cap, 11, None)[0]
        install(cap, forest, thresholds=quantile_thresholds(forest, cap.export_features()[0]))
        st = cap.anomaly_pass()
        r0 = recs_by_key(cap)
        assert st["suspicious"] + st["abnormal"] > 0 and st["normal"] > 0
        old_slot = {Session.from_key(r): int(r["slot"]) for r in cap.export_flows()}
        assert st["flows"] == len(r0) == 1400 and all(v != ZERO for v in r0.values())
        gen = cap.table_info()["generation"]
        ag = cap.update_sessions_status(T0 + 2 * 86400 * S + 100 * S, purge=True)
        assert ag["purged"] > 600 and ag["remaining"] > 600 and cap.table_info()["generation"] == gen + 1
        r1 = recs_by_key(cap)
        new_slot = {Session.from_key(r): int(r["slot"]) for r in cap.export_flows()}
        assert any(old_slot[k] != v for k, v in new_slot.items())                      # some survivor moved
        assert len(r1) == ag["remaining"] and all(r0[k] == v for k, v in r1.items())
        assert int((cap.anomaly_records()["level"] != 0).sum()) == len(r1)              # the removed flows lost theirs
        # a flow inserted after the pass reads all zero
        cap.process_parsed([SessionPacketData(Session(Protocol.UDP, ipaddress.ip_address("192.168.9.9"), 40001,
                                                      ipaddress.ip_address("9.9.9.9"), 53), 80, 120, None)],
                           ts=np.array([T0 + 2 * 86400 * S + 200 * S], dtype=np.uint64))
        r2 = recs_by_key(cap)
        assert len(r2) == len(r1) + 1 and sum(1 for v in r2.values() if v == ZERO) == 1
        assert cap.anomaly_pass()["changed"] >= 1
    finally:
        cap.close()


# ---- 6. analyze_sessions end to end ------------------------------------------------------------------
def test_analyze_sessions_end_to_end():
    pk, ts = flow_packets(400)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 10, timed=True, own_ips=OWN)
    try:
        cap.process_parsed(pk, ts=ts)
        lists = {"date": "d", "signature": "s", "blacklists": [{"name": "zz", "ip_ranges": ["20.0.0.0/8"]},
                                                               {"name": "aa", "ip_ranges": ["20.0.0.0/12", "2001:db8:1::/64"]}]}
        arr, names = blacklists_from_json(lists)
        cap.set_blacklists(arr, names)
        cap.update_blacklist(mark_whitelist=False)
        before = {i.session: i.criticality for i in cap.get_sessions()}
        assert set(before.values()) == {"", "blacklist:aa", "blacklist:aa,blacklist:zz", "blacklist:zz"}   # exactly as today
        assert cap.get_anomalous_sessions() == [] and cap.get_anomalous_status() is False
        now = T0 + 100 * S
        # warm-up: 30 s from the first call; only sessions without a tag get one
        assert cap.analyze_sessions(now) is None
        warm = {i.session: i.criticality for i in cap.get_sessions()}
        assert warm == {s: (c or "anomaly:normal/warming_up") for s, c in before.items()}
        assert cap.analyze_sessions(now + 29 * S) is None and len(cap.analyzer.recent_data) == A.MAX_SAMPLES
        # after it: the trained model scores every flow
        cap.analyzer.set_test_thresholds(0.60, 0.72)
        st = cap.analyze_sessions(now + 30 * S)
        assert st["flows"] == 400 == st["changed"]
        a = cap.analyzer
        infos, slot = infos_of(cap)
        # recent_data: the last 300 of (400 + 400 + 400) vectors appended in Session order
        want_recent = [anref.features(i, CODES) for i in infos][-A.MAX_SAMPLES:]
        assert [bits(r) for r in a.recent_data] == [bits(r) for r in want_recent]
        for i in infos:
            i.criticality = before[i.session]
        res = anref.run(infos, anref.trees_of(a.forest.nodes, a.forest.first), a.forest.sample_size, a.stats[0], a.stats[1],
                        a.stats[2], (0.60, 0.72), CODES)
        assert st == res["stats"]
        got = cap.get_sessions()
        assert {i.session: i.criticality for i in got} == res["criticality"]
        assert all(i.criticality.split(",") == sorted(i.criticality.split(",")) and "anomaly:" in i.criticality for i in got)
        assert any(c.startswith("anomaly:") and ",blacklist:aa,blacklist:zz" in c for c in res["criticality"].values())
        # thresholds that leave some flows on every level
        thr = quantile_thresholds(a.forest, [anref.features(i, CODES) for i in infos])
        cap.analyzer.set_test_thresholds(*thr)
        st = cap.analyze_sessions(now + 31 * S)
        res = anref.run(infos, anref.trees_of(a.forest.nodes, a.forest.first), a.forest.sample_size, a.stats[0], a.stats[1],
                        a.stats[2], thr, CODES, res["records"])
        assert st == res["stats"] and min(st["normal"], st["suspicious"], st["abnormal"]) > 0
        anomalous = cap.get_anomalous_sessions()
        assert [i.session for i in anomalous] == res["anomalous"] and cap.get_anomalous_status() is True
        # each one as get_sessions reports it, field for field; every flow's tag changed in the pass at now + 30 s
        # (the packets are near T0), so that pass's stamp -- or a later one's -- is its last_modified
        everyone = {i.session: i for i in cap.get_sessions()}
        assert anomalous and all(joinref.info_fields(i) == joinref.info_fields(everyone[i.session]) for i in anomalous)
        assert all(i.last_modified_ns >= now + 30 * S for i in anomalous)
        assert [i.criticality for i in anomalous] == [res["criticality"][s] for s in res["anomalous"]]
        assert all(("anomaly:suspicious/" in i.criticality) or ("anomaly:abnormal/" in i.criticality) for i in anomalous)
        assert {i.session: i.criticality for i in cap.get_current_sessions()} == res["criticality"]
        # update_sessions leaves the tags alone
        cap.update_sessions(now + 32 * S)
        assert {i.session: i.criticality for i in cap.get_sessions()} == res["criticality"]
    finally:
        cap.close()
    # no model: fewer than two distinct vectors
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9)
    try:
        one = SessionPacketData(Session(Protocol.UDP, ipaddress.ip_address("192.168.1.9"), 40001, ipaddress.ip_address("20.1.1.1"), 53), 80, 120, None)
        two = SessionPacketData(Session(Protocol.UDP, ipaddress.ip_address("192.168.1.9"), 40003, ipaddress.ip_address("30.1.1.1"), 53), 80, 120, None)
        cap.process_parsed([one, two])
        arr, names = blacklists_from_json({"blacklists": [{"name": "zz", "ip_ranges": ["20.0.0.0/8"]}]})
        cap.set_blacklists(arr, names)
        cap.update_blacklist(mark_whitelist=False)
        assert cap.analyze_sessions() is None                       # no clock: no warm-up; identical vectors: no model
        assert sorted(i.criticality for i in cap.get_sessions()) == ["anomaly:normal/no_model", "blacklist:zz"]
        assert cap.get_anomalous_sessions() == []
    finally:
        cap.close()


# ---- 7. errors ---------------------------------------------------------------------------------------
def test_errors_leave_the_installed_model():
    lib = N.gpu_lib()
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9)
    none = FlodbaddGpuCapture(0, flow_capacity=0)
    try:
        pk, _ = flow_packets(100)
        cap.process_parsed(pk)
        assert lib.fb_flow_anomaly(cap.ctx, 0, None, None) == N.FB_ERR_INVAL             # no model
        assert b"model" in lib.fb_last_error()
        x = N.DeviceBuffer(80)
        assert lib.fb_if_score_dev(cap.ctx, x.ptr, 1, x.ptr, None) == N.FB_ERR_INVAL     # no model
        assert not cap.anomaly_records().view(np.uint8).any()                            # zeros before any pass
        assert len(cap.export_anomalous_flows(1)[0]) == 0
        good = F.trained()
        install(cap, good, thresholds=(0.45, 0.55))
        install(none, good)
        assert lib.fb_flow_anomaly(none.ctx, 0, None, None) == N.FB_ERR_INVAL            # no flow table
        assert lib.fb_flow_anomaly(cap.ctx, 1, None, None) == N.FB_ERR_INVAL             # flags must be 0
        assert lib.fb_flow_anomaly(cap.ctx, 0, None, None) == N.FB_OK                    # out may be NULL
        st = cap.anomaly_pass()
        assert st["flows"] == 100 and st["changed"] == 0
        ref = cap.anomaly_records().tobytes()
        n = [0.0] * 10
        bad = [F.make([[(n, 0.0, 0, 2), F.leaf(1), F.leaf(1)]]),                          # child == parent
               F.make([[(n, 0.0, 1, 3), F.leaf(1), F.leaf(1)]]),                          # child outside the tree
               F.make([[(n, float("nan"), 1, 2), F.leaf(1), F.leaf(1)]]),                 # non-finite value
               F.make([[(n, 0.0, k + 1, 255) for k in range(254)] + [F.leaf(1), F.leaf(1)]]),
               F.make([[F.leaf(1)]] * 65)]
        d = N.FB_IF_MAX_DEPTH + 1
        bad.append(F.make([[(n, 0.0, d + k, k + 1 if k + 1 < d else 2 * d) for k in range(d)] + [F.leaf(1)] * (d + 1)]))
        for f in bad:
            with pytest.raises(N.FbError):
                install(cap, f)
        prm = np.zeros(1, dtype=N.AN_PARAMS_DTYPE)
        assert lib.fb_set_anomaly_model(cap.ctx, N.ptr(good.nodes), len(good.nodes), N.ptr(good.first), 0, N.ptr(prm), None) == N.FB_ERR_INVAL
        assert lib.fb_set_anomaly_model(cap.ctx, N.ptr(good.nodes), len(good.nodes), N.ptr(good.first), good.n_trees, None, None) == N.FB_ERR_INVAL
        prm[0]["std"][3] = float("inf")
        assert lib.fb_set_anomaly_model(cap.ctx, N.ptr(good.nodes), len(good.nodes), N.ptr(good.first), good.n_trees, N.ptr(prm), None) == N.FB_ERR_INVAL
        with pytest.raises(N.FbError):
            cap.set_anomaly_model(good, NO_STATS, (0.45, 0.55), service_codes=np.full(65536, 1000000, dtype=np.uint32))
        # the installed model is still the good one: the same pass, nothing changed
        assert cap.anomaly_pass() == dict(st) and cap.anomaly_records().tobytes() == ref
        assert lib.fb_flow_export_anomalous_dev(cap.ctx, 0, None, None, 0, x.ptr, None) == N.FB_ERR_INVAL   # min_level 1..3
        assert lib.fb_flow_export_anomalous_dev(cap.ctx, 4, None, None, 0, x.ptr, None) == N.FB_ERR_INVAL
    finally:
        cap.close()
        none.close()
