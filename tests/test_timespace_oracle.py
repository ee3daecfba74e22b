"""The reference for the capture-time corpora (tests/timespace.py) pinned before the GPU is compared
with it: the C restatement (coracle.Flows.update with ts, what tests/test_gpu_timespace.py compares
with) equals the independent Python restatement (pyoracle.SessionTable.process(c, now)) on every
enumerated flow; no placement of the update-call boundaries changes a flow's state; eleven flows are
spelled out by hand; and the corpora discriminate -- each named deviation of a third restatement
(timespace.sim: `>` for `>=` at the timeout, ms rounded, ms floored, a zero interarrival term
refused) differs from the oracle on hundreds of flows, so an edit to GAPS_NS that drops an edge
fails here."""
import ipaddress

import numpy as np
import pytest

import flagseq as fs
import timespace as tsp
from flodbadd_amd import _native as N
from oracle import coracle, pyoracle

CORPORA = {"quads": tsp.quads, "udp_triples": tsp.udp_triples, "ends": tsp.ends}
NONE = N.FB_SEEN_NONE


def _oracle(batches):
    """Batches (one per update call) through the C restatement -> coracle.Flows."""
    flows, cfg = coracle.Flows(), coracle.make_cfg(2)
    for b in batches:
        fr, of = tsp.frames(b)
        out, dns, _, _ = coracle.parse_classify(cfg, fr, of)
        assert len(out) == len(of) - 1 and len(dns) == 0  # every frame is a session packet
        flows.update(out, ts=b.t)
    return flows


def _fields(x):
    none = lambda v: None if int(v) == NONE else int(v)  # noqa: E731
    return (int(x["start_time_ns"]), int(x["last_activity_ns"]), none(x["end_time_ns"]),
            int(x["current_segment_start_ns"]), none(x["last_segment_end_ns"]),
            int(x["total_segment_interarrival_ms"]), int(x["segment_interarrival_div"]),
            int(x["segment_count"]), bool(x["in_segment"]))


def _by_flow(flows):
    """{flow id: _fields of its time record}, the flow read off start_time_ns and off the key."""
    recs, t = flows.export_sorted(), flows.export_times()
    ids = tsp.flow_of_recs(recs)
    assert ((t["start_time_ns"].astype(np.int64) - tsp.BASE_NS) // 1_000_000 == ids).all()
    assert (recs["segment_count"] == t["segment_count"]).all() and (recs["in_segment"] == t["in_segment"]).all()
    return {int(f): _fields(x) for f, x in zip(ids, t)}


@pytest.mark.parametrize("name", list(CORPORA))
def test_c_oracle_equals_python_oracle(name):
    """orc_flows_update_timed against pyoracle.SessionTable.process(c, now), field by field (the join
    of test_oracle_kat.test_timed_kat_c_oracle_equals_python_oracle), the corpus in two calls."""
    batches = tsp.layout(CORPORA[name](), 0b010)
    flows, table = _oracle(batches), pyoracle.SessionTable()
    pcfg = pyoracle.Config.from_bitmap(coracle.default_bitmap(), session_filter=2)
    for b in batches:
        fr, of = tsp.frames(b)
        classes, _, _, _ = pyoracle.run_batch(pcfg, fr, of, table=table, ts=b.t)
        assert set(classes) == {0}
    py = pyoracle.table_times(table)
    recs, t = flows.export_sorted(), flows.export_times()
    assert len(recs) == len(py) == CORPORA[name]().n_flows
    for r, x in zip(recs, t):
        key = (int(r["protocol"]), ipaddress.IPv4Address(int(r["src_ip"][0])), int(r["src_port"]),
               ipaddress.IPv4Address(int(r["dst_ip"][0])), int(r["dst_port"]))
        e = py[key]
        assert _fields(x) == e[:6] + e[7:], (key, _fields(x), e)
        assert abs(int(x["total_segment_interarrival_ms"]) / 1000.0 - e[6]) <= 1e-9
        assert int(r["segment_count"]) == e[8] and bool(r["in_segment"]) == e[9]


@pytest.mark.parametrize("name", list(CORPORA))
def test_cut_invariance(name):
    """All 8 placements of the update-call boundaries leave the same table: the time records byte for
    byte, and the flow records in every field but the three packet positions (first_seen, last_seen,
    end_seen name the update call and the frame's index in it), of which end_seen's presence is kept."""
    ref = None
    for mask in range(8):
        batches = tsp.layout(CORPORA[name](), mask)
        assert len(batches) == 1 + bin(mask).count("1")
        flows = _oracle(batches)
        recs, t = flows.export_sorted().copy(), flows.export_times()
        ended = recs["end_seen"] != NONE
        for f in ("first_seen", "last_seen", "end_seen"):
            recs[f] = 0
        got = (recs.tobytes(), ended.tobytes(), t.tobytes())
        ref = ref or got
        assert got == ref, (name, mask)


MS, S = 1_000_000, 1_000_000_000
A, P, F, FP, R = tsp.A_, tsp.P_, fs.PAY | fs.FIN | fs.ACK, fs.PAY | fs.FIN | fs.PSH | fs.ACK, fs.PAY | fs.RST
# (packets: (flags, gap in ns before the packet); udp) -> the record, times relative to the flow's
# first packet t0: (last_activity, end_time, current_segment_start, last_segment_end, total ms, div,
# segment_count, in_segment).  ms(x) is x / 1e6 truncated toward zero.
BY_HAND = [
    # P inserts: count 1, closed, end = t0.  P at t0 - 0.5 ms: ms(-0.5) = 0, no timeout; the closed flow
    # opens a segment at t1 and P ends it: count 2, term = ms(t1 - t0) = ms(-0.5) = 0, ACCEPTED: div 1
    (([(P, 0), (P, -500_000)], False), (-500_000, None, -500_000, -500_000, 0, 1, 2, False)),
    # the same a whole second back: term = -1000 < 0, skipped: div stays 0
    (([(P, 0), (P, -S)], False), (-S, None, -S, -S, 0, 0, 2, False)),
    # A inserts: count 0, open, no end.  4,999,999,999 ns later: ms = 4999 < 5000, nothing ends
    (([(A, 0), (A, 4_999_999_999)], False), (4_999_999_999, None, 0, None, 0, 0, 0, True)),
    # one ns more: ms = 5000, the open segment ends at t1 (count 1, no previous end: no term) and a
    # new one opens at t1
    (([(A, 0), (A, 5 * S)], False), (5 * S, None, 5 * S, 5 * S, 0, 0, 1, True)),
    # 5,000,999,999 ns still truncates to 5000: the same
    (([(A, 0), (A, 5_000_999_999)], False), (5_000_999_999, None, 5_000_999_999, 5_000_999_999, 0, 0, 1, True)),
    # 5 s BACK: ms = -5000, never a timeout
    (([(A, 0), (A, -5 * S)], False), (-5 * S, None, 0, None, 0, 0, 0, True)),
    # the first FIN (packet 1, t0 + 1 ms) is the end although the second (packet 2) is 1 s earlier
    (([(A, 0), (F, MS), (F, -S)], False), (MS - S, MS, 0, None, 0, 0, 0, True)),
    # P: count 1, closed, end t0.  A 12 s later: a timeout on a closed flow ends nothing, the segment
    # opens at t1.  P 1 ms later ends it: count 2, term = ms(t1 - t0) = 12000, div 1
    (([(P, 0), (A, 12 * S), (P, MS)], False), (12 * S + MS, None, 12 * S, 12 * S + MS, 12000, 1, 2, False)),
    # A, then P at the timeout: one end (count 1, no term), reopened at t1 by the timeout.  P 1 ms
    # later: count 2, term = ms(t1 - t1) = 0, accepted: div 1 with a total of 0
    (([(A, 0), (P, 5 * S), (P, MS)], False), (5 * S + MS, None, 5 * S, 5 * S + MS, 0, 1, 2, False)),
    # a RST that is also the third end: P (1), P 5 s later (2: term ms(t1 - t0) = 5000, div 1; reopened
    # at t1), FIN|PSH 1 s back (3: term ms(t1 - t1) = 0, div 2), RST: end_time stays the FIN's
    (([(P, 0), (P, 5 * S), (FP, -S), (R, MS)], False), (4 * S + MS, 4 * S, 4 * S + MS, 4 * S, 5000, 2, 3, True)),
    # UDP has no PSH: the timeout ends the segment at t1, 4,999,999,999 ns later nothing happens
    (([(0, 0), (0, 5 * S), (0, 4_999_999_999)], True), (9_999_999_999, None, 5 * S, 5 * S, 0, 0, 1, True)),
]


def test_records_by_hand():
    """Eleven flows whose records are worked out in the comments of BY_HAND, through the C oracle and
    through timespace.sim."""
    for k, ((pk, udp), exp) in enumerate(BY_HAND):
        n = len(pk)
        c = tsp.Corpus(np.full(n, k), np.arange(n), [p[0] for p in pk], [p[1] for p in pk], udp)
        t0 = tsp.BASE_NS + k * MS
        rel = lambda v: None if v is None else t0 + v  # noqa: E731
        want = (t0, rel(exp[0]), rel(exp[1]), rel(exp[2]), rel(exp[3])) + exp[4:]
        (got,) = _by_flow(_oracle(tsp.layout(c, 0))).values()
        assert got == want, (k, got, want)
        (row,) = c.rows()
        assert tsp.sim(*row) == want[:2] + want[3:], k
        for mask in range(1, 1 << (n - 1)):  # and under every cut
            (cut,) = _by_flow(_oracle(tsp.layout(c, mask))).values()
            assert cut == want, (k, mask)


def test_corpus_discriminates():
    """timespace.sim equals the oracle on all 8,192 quads flows, and each of its deviations differs on
    at least 100 (with this GAPS_NS: gt 3,852, round 3,619 -- both the gap and the term rounded, halves
    away from zero --, floor 587, pos 3,584)."""
    c = tsp.quads()
    got = _by_flow(_oracle(tsp.layout(c, 0)))
    assert sorted(got) == list(range(8192))
    rows = c.rows()
    differ = {}
    for dev in (None, "gt", "round", "floor", "pos"):
        differ[dev] = sum(tsp.sim(*rows[f], deviation=dev) != got[f][:2] + got[f][3:] for f in range(8192))
    print("flows differing per deviation:", differ)
    assert differ[None] == 0
    for dev in ("gt", "round", "floor", "pos"):
        assert differ[dev] >= 100, differ


def test_coverage_counts():
    t = _oracle(tsp.layout(tsp.quads(), 0)).export_times()
    assert set(np.unique(t["segment_count"]).tolist()) == {0, 1, 2, 3, 4}
    assert set(np.unique(t["segment_interarrival_div"]).tolist()) == {0, 1, 2, 3}
    assert set(np.unique(t["in_segment"]).tolist()) == {0, 1}
    zero_terms = int(((t["segment_interarrival_div"] > 0) & (t["total_segment_interarrival_ms"] == 0)).sum())
    print("flows with an accepted term and a total of 0 ms:", zero_terms)
    assert zero_terms >= 1000
    assert (t["last_activity_ns"] < t["start_time_ns"]).any()
    u = _oracle(tsp.layout(tsp.udp_triples(), 0)).export_times()
    assert set(np.unique(u["segment_count"]).tolist()) == {0, 1, 2, 3} and (u["segment_interarrival_div"] > 0).any()
    e = _oracle(tsp.layout(tsp.ends(), 0))
    et, er = e.export_times(), e.export_sorted()
    assert len(er) == 16875 and ((et["end_time_ns"] != NONE) == (er["end_seen"] != NONE)).all()
    assert (et["end_time_ns"] == NONE).any()
    ended = et["end_time_ns"] != NONE
    assert (et["end_time_ns"][ended] > et["last_activity_ns"][ended]).any()  # a later packet with an earlier time


def test_corpora_shapes():
    """The sizes the GPU tests are written for, and that replicas and cuts leave a packet's time alone."""
    q = tsp.quads()
    assert (q.n_flows, len(q.flow)) == (8192, 32768)
    assert tsp.udp_triples().n_flows == 512 and tsp.ends().n_flows == 16875
    assert len(set(tsp.GAPS_NS.tolist())) == 8
    when = lambda bs: {(int(f) % 8192, int(p)): int(t) - int(f) * MS for b in bs for f, p, t in zip(b.flow, b.pos, b.t)}  # noqa: E731
    base = when(tsp.layout(q, 0))
    assert when(tsp.layout(q, 0b101)) == base
    rep = tsp.layout(q, 0b111, replicas=2)
    assert [len(b.flow) for b in rep] == [16384] * 4 and when(rep) == base
    # every call of a layout is position-major
    for b in tsp.layout(q, 0b010):
        assert (np.diff(b.pos.astype(np.int64) * (1 << 32) + b.flow) > 0).all()
    s = tsp.shims()
    assert set(np.unique(s.lengths).tolist()) == {1, 2, 3} and int(s.flow.min()) > 8 * 8192


def test_hot_and_ladder_construction():
    for tiles in ((72,), (36, 72)):
        calls = tsp.hot(tiles)
        assert len(calls) == 2
        seen = {}
        for b in calls:
            cnt = np.bincount(b.flow)
            assert [int(cnt[i]) for i in range(len(tiles))] == [n * tsp.TILE for n in tiles]
            assert max(tiles) > tsp.WINDOW + 1  # more full tiles of one run than one look-back window
            for f, p in zip(b.flow[b.flow >= 1000].tolist(), b.pos[b.flow >= 1000].tolist()):
                assert p == seen.get(f, 0)  # a flow's packets in position order, over both calls
                seen[f] = p + 1
        assert len(seen) == 2000 and 4 <= min(seen.values()) and max(seen.values()) <= 40
    # the plan on slots of our own making (the GPU test takes them from the device table)
    F = 4096
    slots = np.random.default_rng(1).permutation(4 * F)[:F]
    counts, probes = tsp.ladder_plan(slots, L=5)
    start, end = tsp.run_spans(slots, counts)
    assert len(probes) == int(counts.sum()) // 256 or len(probes) == int(counts.sum()) // 256 - 1
    for k, (f, B, d) in enumerate(probes):
        assert B == 256 * (k + 1) and d == tsp.plan_offset(B) and counts[f] == 5 and start[f] == B - d
    # at the GPU test's size every offset falls on >= 80 wave boundaries, >= 8 of them tile boundaries
    big = tsp.ladder_plan(np.random.default_rng(2).permutation(1 << 19)[: 1 << 17], L=5)[1]
    per_d = np.zeros((6, 2), dtype=np.int64)
    for _, B, d in big:
        per_d[d] += (1, B % tsp.TILE == 0)
    assert per_d[:, 0].min() >= 80 and per_d[:, 1].min() >= 8, per_d
    assert int((counts == 5).sum()) == len(probes) and set(counts.tolist()) == {1, 5}
    lad = tsp.Ladder(F)
    b1, b2 = lad.call1(), lad.call2(counts)
    assert (b1.pos == 0).all() and len(b1.flow) == F and len(b2.flow) == int(counts.sum())
    assert (np.bincount(b2.flow, minlength=F) == counts).all() and b2.pos.min() == 1 and b2.pos.max() == 5
