"""The TCP flag state machine on every update path, against the oracle, byte for byte.

The flag-sequence corpora of tests/flagseq.py (every two-symbol sequence over all 128 symbols, every
four-symbol sequence over a 16-symbol alphabet, and long hot flows over all 128 symbols) feed the
ordered per-flow state -- map_tcp_flags, the first FIN / RST position and conn_state, hist_mask /
end_mask / the first S, s, H, h, the PSH segment logic and its timed form, and the key
canonicalisation by SYN / ACK under two service ports -- through each way the GPU composes it:

  path      entry point                                     parse kernel
  dense     fb_process_dev                                  k_parse_dense
  seg       fb_process_seg_dev                              k_parse_seg<false, kPartOut>
  table     fb_process_seg_async_dev, session records off   k_parse_seg<false, kPartOut> writing update
                                                            entries only (the table-only update-entry path)
  parsed    fb_process_parsed                               the PARSED=true instance (fb_parsed_pkt in)

and through the layouts that put a flow's packets into different waves and chunks (pos), adjacent
lanes of one wave (flow) and two update calls (split).  Untimed contexts run K1 / K1c k_flow_combine
(hot corpus: checked on the host that a group passes its threshold) / K2 k_flow_apply and fb_hist.hip;
timed contexts run the plain K2 and fb_time.hip's segmented scans.  tests/test_flagspace_oracle.py
pins the reference these compare with on the same corpora.

Compared: every fb_flow_rec field but slot, every history string and conn_state, every fb_flow_time
field (timed), each batch's records (where the path returns them), new_sessions / updated_sessions,
and error == 0."""
import functools

import numpy as np
import pytest

import flagseq as fs
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.sessions import SessionFilter
from oracle import coracle
from test_gpu_timed import _check as _check_times

pytestmark = pytest.mark.gpu

PAIR_IDS = {fs.ONE_SVC: "one_svc", fs.TWO_SVC: "two_svc", fs.NO_SVC: "no_svc"}


@functools.lru_cache(maxsize=2)
def _reference(corpus, how, pair, timed, hi_seed=5):
    """The corpus through the oracle, once per (corpus, layout, pair, clock): per batch (frames,
    offsets, ts, records, stats), and the oracle's table.  Read-only for the tests."""
    if corpus == "hot":
        batches = fs.hot_batches()
    else:
        batches = fs.layout(fs.pairs_seq() if corpus == "pairs" else fs.quads_seq(), how)
    ts = fs.times(batches, seed=9) if timed else [None] * len(batches)
    flows, cfg, out = coracle.Flows(), coracle.make_cfg(2), []
    for b, t in zip(batches, ts):
        fr, of = fs.frames(b, pair, hi_seed=hi_seed)
        recs, dns, _, _ = coracle.parse_classify(cfg, fr, of)
        assert len(recs) == len(of) - 1 and len(dns) == 0
        st = np.zeros(1, dtype=N.STATS_DTYPE)
        flows.update(recs, st, ts=t)
        for a in (fr, of, recs, st):
            a.setflags(write=False)
        out.append((fr, of, t, recs, st))
    return out, flows


def _capacity(n_flows):
    """The smallest power of two that keeps the table at most half full (a partition's 512 slots then
    hold its share with room for the spread between partitions)."""
    return max(1 << 12, 1 << int(2 * n_flows - 1).bit_length())


def _table_only(cap, fr, of, ts):
    """fb_process_seg_async_dev with the session records off: the update reads the parse's update
    entries.  Returns the batch's stats after the join."""
    lib = N.gpu_lib()
    n = len(of) - 1
    nseg = max((n + 63) // 64, 1)
    d_fr, d_of = N.DeviceBuffer(fr.nbytes).upload(fr), N.DeviceBuffer(of.nbytes).upload(of)
    d_out, d_seg, d_st = N.DeviceBuffer(nseg * N.SEG_BYTES), N.DeviceBuffer(nseg * 4), N.DeviceBuffer(N.STATS_DTYPE.itemsize)
    d_ts = cap._frame_times(ts, n)  # noqa: F841 (alive until the join)
    N.check(lib.fb_process_seg_async_dev(cap.ctx, d_fr.ptr, fr.nbytes, d_of.ptr, n, d_out.ptr, d_seg.ptr, None,
                                         d_st.ptr, None))
    N.check(lib.fb_flow_join(cap.ctx, None))
    N.check(lib.fb_stream_sync(None))
    st = d_st.download(np.zeros(1, dtype=N.STATS_DTYPE))
    cap._pull_history(((n + 63) // 64) * 64)
    return {k: int(st[0][k]) for k in N.STATS_FIELDS if not k.startswith("reserved")}


def _check_tables(cap, flows, tag):
    """The GPU table against the oracle's: rows (slot zeroed), then every history string and
    conn_state.  Diagnostics name the first differing flow (its key and both histories)."""
    gf = cap.export_flows()
    rf = flows.export_sorted()
    assert len(gf) == len(rf), (tag, len(gf), len(rf))
    from flodbadd_amd.distributed import sort_by_ord
    gs = sort_by_ord(gf)
    slots = gs["slot"].copy()
    gz = gs.copy()
    gz["slot"] = 0
    w = N.FLOW_REC_DTYPE.itemsize
    bad = np.flatnonzero((gz.view(np.uint8).reshape(-1, w) != np.ascontiguousarray(rf).view(np.uint8).reshape(-1, w)).any(axis=1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s: %d of %d flow rows differ; first: gpu %s history %r, oracle %s history %r" %
                             (tag, bad.size, len(rf), gz[i], cap.histories.get(int(slots[i]), ""), rf[i],
                              flows.history(rf[i])[0]))
    for r, slot in zip(rf, slots.tolist()):
        h, cs = flows.history(r)
        g = cap.histories.get(slot, "")
        assert g == h, (tag, r, g, h)
        assert N.CONN_STATES[int(r["conn_state"])] == cs and int(r["hist_len"]) == len(h), (tag, r, h, cs)
    return gf


def _run(corpus, how, pair, path, timed=False, capacity=None, hi_seed=5, precondition=None):
    ref, flows = _reference(corpus, how, pair, timed, hi_seed)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, track_history=True, timed=timed,
                             flow_capacity=capacity or _capacity(flows.count()))
    tag = "%s/%s/%s/%s%s" % (corpus, how, PAIR_IDS[pair], path, "/timed" if timed else "")
    try:
        if precondition:
            precondition(cap, ref)
        if path == "table":
            N.check(N.gpu_lib().fb_set_session_records(cap.ctx, 0))
        for k, (fr, of, ts, recs, r_st) in enumerate(ref):
            if path == "table":
                st = _table_only(cap, fr, of, ts)
            else:
                if path == "dense":
                    g = cap.process_frames(fr, of, ts=ts)
                elif path == "seg":
                    g = cap.process_frames_seg(fr, of, ts=ts)
                else:
                    g = cap.process_parsed(fs.parsed_of(recs), ts=ts)
                assert g.records.tobytes() == recs.tobytes(), (tag, k)
                st = g.stats
            assert st["error"] == 0, (tag, k, st)
            assert (st["new_sessions"], st["updated_sessions"]) == \
                (int(r_st[0]["new_sessions"]), int(r_st[0]["updated_sessions"])), (tag, k, st)
            assert st["n_session"] == len(recs)
        gf = _check_tables(cap, flows, tag)
        if timed:
            _check_times(cap, flows, tag)
        hist = {r.tobytes()[:40]: cap.histories.get(int(r["slot"]), "") for r in gf}
        gf = gf.copy()
        gf["slot"] = 0
        return gf, hist
    finally:
        cap.close()


PAIRS_CASES = [(pair, how, path) for pair in fs.PORT_PAIRS for how in ("pos", "flow", "split") for path in ("dense", "seg")] + \
              [(pair, "pos", path) for pair in fs.PORT_PAIRS for path in ("table", "parsed")]


@pytest.mark.parametrize("pair,how,path", PAIRS_CASES, ids=["%s-%s-%s" % (PAIR_IDS[p], h, x) for p, h, x in PAIRS_CASES])
def test_flagspace_pairs(pair, how, path):
    """All 128^2 two-symbol sequences, one flow each (32,768 frames)."""
    gf, _ = _run("pairs", how, pair, path)
    assert len(gf) == {fs.ONE_SVC: 16384, fs.TWO_SVC: 22528, fs.NO_SVC: 24576}[pair]


QUADS_CASES = [(pair, how, path) for pair in (fs.ONE_SVC, fs.TWO_SVC) for how in ("pos", "split") for path in ("seg", "table")]


@pytest.mark.parametrize("pair,how,path", QUADS_CASES, ids=["%s-%s-%s" % (PAIR_IDS[p], h, x) for p, h, x in QUADS_CASES])
def test_flagspace_quads(pair, how, path):
    """All 16^4 four-symbol sequences over flagseq.ALPHABET16 (262,144 frames, 13 bucketing chunks)."""
    gf, _ = _run("quads", how, pair, path)
    assert len(gf) >= 65536
    if pair == fs.ONE_SVC:
        assert len(gf) == 65536 and (gf["conn_state"] == 4).sum() == 86  # S1 is reached


def _combine_runs(cap, ref):
    """Host-side precondition (the flow hash and K1's rule, fb_flow.hip: a (20,480-record chunk,
    partition) group of at least max(FB_COMB_MIN = 64, 4 x the chunk's mean per partition) records
    goes to k_flow_combine): the first batch has such a group."""
    lib = N.gpu_lib()
    parts = int(cap.table_info()["partitions"])
    assert parts >= 2 and parts & (parts - 1) == 0
    recs = ref[0][3]
    keys = np.ascontiguousarray(np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1)[:, :40])
    _, first, inv = np.unique(keys.view("V40").ravel(), return_index=True, return_inverse=True)
    part_of_key = np.array([lib.fb_flow_hash(N.ptr(recs[i: i + 1])) >> (64 - parts.bit_length() + 1) for i in first])
    part = part_of_key[inv]
    hot = 0
    for a in range(0, len(recs), 20480):
        c = np.bincount(part[a: a + 20480], minlength=parts)
        cnt = int(c.sum())
        hot += int((c >= max(64, 4 * ((cnt + parts - 1) // parts))).sum())
    assert hot >= 1, "no (chunk, partition) group reaches k_flow_combine's threshold"


@pytest.mark.parametrize("path", ["dense", "seg", "table"])
def test_flagspace_hot(path):
    """4 flows of 12,000 packets and 44 of 500 over all 128 symbols, interleaved, three update calls,
    a small table: the hot flows' groups are combined per key before the apply (k_flow_combine), so
    the first S / s / H / h, the first FIN / RST and conn_state come out of partial reductions."""
    gf, _ = _run("hot", "hot", fs.ONE_SVC, path, capacity=1 << 14, precondition=_combine_runs)
    assert len(gf) == 48 and sorted(gf["hist_len"].tolist()) == sorted(fs.HOT_LENGTHS)


TIMED_CASES = [("pairs", how, path) for how in ("pos", "split") for path in ("dense", "seg", "table")] + \
              [("hot", "hot", path) for path in ("dense", "seg", "table")]


@pytest.mark.parametrize("corpus,how,path", TIMED_CASES, ids=["%s-%s-%s" % c for c in TIMED_CASES])
def test_flagspace_timed(corpus, how, path):
    """Timed contexts (no combining: the plain K2 and fb_time.hip): gaps on both sides of the 5-s
    timeout, at it, and backwards, between a flow's packets; every fb_flow_time field equals the oracle's."""
    gf, _ = _run(corpus, how, fs.ONE_SVC, path, timed=True, capacity=(1 << 14) if corpus == "hot" else None)
    assert (gf["segment_count"] > 0).any()


def test_flagspace_high_flag_bits_change_nothing():
    """URG, ECE and CWR (bits 5-7 of the flag byte) zero or random: the exported table and the history
    strings are byte-identical (tcp_flags is not part of a flow record)."""
    a, ha = _run("pairs", "pos", fs.ONE_SVC, "seg", hi_seed=None)
    b, hb = _run("pairs", "pos", fs.ONE_SVC, "seg", hi_seed=5)
    fr0 = _reference("pairs", "pos", fs.ONE_SVC, False, None)[0][0][0]
    fr1 = _reference("pairs", "pos", fs.ONE_SVC, False, 5)[0][0][0]
    assert (fr0 != fr1).sum() > 20000 and ((fr0 ^ fr1) & 0x1F).max() == 0  # the corpora do differ, in those bits only
    order = lambda x: x[np.argsort(x.view(np.uint8).reshape(len(x), -1)[:, :40].copy().view("V40").ravel())]  # noqa: E731
    assert order(a).tobytes() == order(b).tobytes()
    assert ha == hb
