"""The reference for the flag-sequence corpora (tests/flagseq.py) pinned twice: the C restatement
(coracle.Flows, what the GPU tests compare with) and the independent Python restatement
(pyoracle.SessionTable) build the same session table, history strings and capture-time records for
every two-symbol sequence under the three port pairs and for the long hot flows -- and the corpora
have the properties the GPU tests rely on (flow counts, every history character, the conn_state
codes, ends in mid-sequence)."""
import ipaddress

import numpy as np
import pytest

import flagseq as fs
from flodbadd_amd import _native as N
from oracle import coracle, pyoracle


def _py_cfg():
    return pyoracle.Config.from_bitmap(coracle.default_bitmap(), session_filter=2)


def _key_of(r):
    assert int(r["family"]) == 2
    return (int(r["protocol"]), ipaddress.IPv4Address(int(r["src_ip"][0])), int(r["src_port"]),
            ipaddress.IPv4Address(int(r["dst_ip"][0])), int(r["dst_port"]))


def _both(batches, pair, timed, hi_seed=5):
    """The batches through both restatements -> (coracle.Flows, pyoracle.SessionTable)."""
    flows, table = coracle.Flows(), pyoracle.SessionTable()
    cfg, pcfg = coracle.make_cfg(2), _py_cfg()
    ts = fs.times(batches, seed=9) if timed else [None] * len(batches)
    for b, t in zip(batches, ts):
        fr, of = fs.frames(b, pair, hi_seed=hi_seed)
        out, dns, cls, _ = coracle.parse_classify(cfg, fr, of)
        assert len(out) == len(of) - 1 and len(dns) == 0  # every frame is a session packet
        flows.update(out, ts=t)
        classes, _, _, _ = pyoracle.run_batch(pcfg, fr, of, table=table, ts=t)
        assert classes == cls.tolist()
    return flows, table


def _assert_same(flows, table, timed):
    recs = flows.export_sorted()
    if not timed:  # (a timed table's segment state follows the clock: compared below, from the time records)
        assert pyoracle.table_rows(table) == pyoracle.rows_of_flow_recs(recs)
    else:
        strip = lambda rows: {k: v[:8] for k, v in rows.items()}  # noqa: E731
        assert strip(pyoracle.table_rows(table)) == strip(pyoracle.rows_of_flow_recs(recs))
    assert len(recs) == len(table.sessions)
    for r in recs:
        h, cs = flows.history(r)
        s = table.sessions[_key_of(r)]
        assert (h, cs) == (s["history"], s["conn_state"]), (_key_of(r), h, s["history"])
    if timed:
        t = flows.export_times()
        py = pyoracle.table_times(table)
        none = lambda v: None if int(v) == N.FB_SEEN_NONE else int(v)  # noqa: E731
        for r, x in zip(recs, t):
            e = py[_key_of(r)]
            got = (int(x["start_time_ns"]), int(x["last_activity_ns"]), none(x["end_time_ns"]),
                   int(x["current_segment_start_ns"]), none(x["last_segment_end_ns"]),
                   int(x["total_segment_interarrival_ms"]), e[6], int(x["segment_interarrival_div"]),
                   int(x["segment_count"]), bool(x["in_segment"]))
            assert got == e, (_key_of(r), got, e)
            assert int(r["segment_count"]) == e[8] and bool(r["in_segment"]) == e[9]
    return recs


def test_port_pair_properties():
    """What flagseq's port pairs stand for under the default service bitmap."""
    bm = coracle.default_bitmap()
    svc = lambda p: bool(bm[p >> 3] & (1 << (p & 7)))  # noqa: E731
    assert [svc(p) for p in (443, 80, 40000, 50000, 1024)] == [True] * 5
    assert [svc(p) for p in (49152, 65535)] == [False] * 2
    assert len(set(fs.ALPHABET16.tolist())) == 16


PAIR_FLOWS = {fs.ONE_SVC: 16384, fs.TWO_SVC: 22528, fs.NO_SVC: 24576}


@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
@pytest.mark.parametrize("pair", fs.PORT_PAIRS, ids=["one_svc", "two_svc", "no_svc"])
def test_pairs_c_vs_python_oracle(pair, timed):
    flows, table = _both(fs.layout(fs.pairs_seq(), "pos"), pair, timed)
    recs = _assert_same(flows, table, timed)
    assert len(recs) == PAIR_FLOWS[pair]
    if pair == fs.ONE_SVC:
        chars = set("".join(s["history"] for s in table.sessions.values()))
        assert chars == set(N.FB_HIST_CHARS)
        assert set(np.unique(recs["conn_state"]).tolist()) == {0, 2, 3, 5}
        assert (recs["hist_len"] == 2).all()
    if timed:
        t = flows.export_times()
        assert (t["segment_interarrival_div"] > 0).any() and (t["end_time_ns"] != N.FB_SEEN_NONE).any()
        assert (t["last_activity_ns"] < t["start_time_ns"]).any()  # the step backwards


@pytest.mark.parametrize("how", ["flow", "split"])
def test_pairs_layouts_same_table(how):
    """The layouts reorder frames of different flows only: the oracle's table does not change."""
    ref = None
    for h in ("pos", how):
        flows = coracle.Flows()
        for b in fs.layout(fs.pairs_seq(), h):
            flows.update(coracle.parse_classify(coracle.make_cfg(2), *fs.frames(b, fs.TWO_SVC, hi_seed=5))[0])
        rows = pyoracle.rows_of_flow_recs(flows.export_sorted())
        ref = rows if ref is None else ref
        assert rows == ref


@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
def test_hot_c_vs_python_oracle(timed):
    batches = fs.hot_batches()
    assert len(batches) == 3
    flows, table = _both(batches, fs.ONE_SVC, timed)
    recs = _assert_same(flows, table, timed)
    assert len(recs) == 48
    assert (recs["end_seen"] != N.FB_SEEN_NONE).all()
    assert sorted(recs["hist_len"].tolist()) == sorted(fs.HOT_LENGTHS)
    # the first end falls inside the sequence: before the last packet for every flow, and after the
    # first packet for nearly all (a flow's first packet is a FIN / RST with probability 0.02)
    assert (recs["end_seen"] < recs["last_seen"]).all()
    assert (recs["end_seen"] > recs["first_seen"]).sum() >= 40
    if timed:
        t = flows.export_times()
        assert (t["segment_count"] > 100).any() and (t["total_segment_interarrival_ms"] > 0).all()


def test_quads_preconditions():
    """quads under one service port (C restatement alone: 262,144 frames): one flow per sequence,
    S1 is reached (S and H with neither F nor f at a SYN|RST end), SF is not (at the first FIN / RST
    only one of F / f exists)."""
    flows = coracle.Flows()
    (b,) = fs.layout(fs.quads_seq(), "pos")
    flows.update(coracle.parse_classify(coracle.make_cfg(2), *fs.frames(b, fs.ONE_SVC, hi_seed=5))[0])
    recs = flows.export_sorted()
    assert len(recs) == 65536 and (recs["hist_len"] == 4).all()
    codes = np.bincount(recs["conn_state"], minlength=6)
    assert codes[4] == 86 and codes[1] == 0
    assert (codes[[0, 2, 3, 5]] > 0).all()
