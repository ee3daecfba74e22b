"""Malformed frames through the parse instances test_gpu_fuzz.py does not reach (it runs
k_parse_dense and the plain k_parse_seg<false>), each bit-exact against the C oracle on records, DNS
side records, classes, segment counts and every stats field, and on the session table where one is
built:

  several batches in one launch    fb_parse_classify_seg_batches_dev   k_parse_seg<false, kFlagsProduct, true>
  the resident queue               fb_seg_queue_* (plain and shared)   k_parse_seg_queue
  fused parse + upsert             fb_process_seg_dev / _async_dev     k_parse_seg<false, kPartOut>, records on and
                                                                       off (the table-only update-entry path)
  timed contexts                   the same, with capture timestamps   + fb_time.hip
  the ingest ring                  fb_ring_push / fb_ring_push_block   the ring's batches
  parsed packets                   fb_process_parsed_dev / _seg_dev    the PARSED=true instances

The corpus is tests/fuzzframes.py at 4,317 frames (67 full segments and a 29-frame tail) for two
seeds, one batch whose last frame is cut inside its TCP header at the very end of the frame buffer
(the decode must not depend on bytes past frames_bytes), and one with two bad offsets; IPv6 LAN
prefixes and own IPs are configured as in test_gpu_fuzz.py.  The parsed-packet corpus fuzzes
fb_parsed_pkt itself: protocols and families outside 6 / 17 and 2 / 10 (dropped, as the header
documents), has_flags 0 / 1 / 2 on both protocols, random flags, ports 0 / 53 / 65535, LAN, loopback
and own addresses, a scrambled pkt_index."""
import numpy as np
import pytest

import framegen as fg
import fuzzframes
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture, IngestRing, lan_v6_table, own_ip_table
from flodbadd_amd.queue import DeviceSegBatch, SegQueue
from flodbadd_amd.sessions import SessionFilter, ip_to_words
from oracle import coracle
from test_gpu_flagspace import _check_tables
from test_gpu_parity import rows_sorted
from test_gpu_queue import _Batch, _Queue, _verify
from test_gpu_ring import _oracle_batches
from test_gpu_segmented import _check, _expected_seg, _run_batches
from test_gpu_timed import _check as _check_times
from test_gpu_timed import frame_times

pytestmark = pytest.mark.gpu

LAN = [("fd12::", 16), ("2001:db8:abcd:12::1", 64)]
OWN = ["10.0.0.1", "192.168.1.7", "fe80::1"]
N_FUZZ = 4317
STAT_KEYS = [k for k in N.STATS_FIELDS if not k.startswith("reserved")]


def _cfg(flt):
    return coracle.make_cfg(int(flt), lan_v6=lan_v6_table(LAN), own_ips=own_ip_table(OWN))


def _capture(flt=SessionFilter.All, **kw):
    return FlodbaddGpuCapture(0, session_filter=flt, lan_v6=LAN, own_ips=OWN, **kw)


@pytest.fixture(scope="module")
def corpus():
    """name -> (frames, offsets), read-only."""
    c = {"fuzz7": fuzzframes.generate(N_FUZZ, seed=7), "fuzz8": fuzzframes.generate(N_FUZZ, seed=8)}
    # the last frame ends 7 bytes into its TCP header's second half: the flag byte (frame byte 47) and
    # everything after it lie past the end of the frame buffer
    fr, of = fuzzframes.generate(129, seed=21)
    cut = np.frombuffer(fg.tcp_frame("10.0.0.1", 40000, "93.184.216.34", 443, fg.SYN, 0)[:47], dtype=np.uint8)
    c["cut_tail"] = (np.concatenate([fr, cut]), np.concatenate([of, [of[-1] + len(cut)]]).astype(np.uint32))
    # two bad offsets as in test_gpu_parity.test_bad_offsets: one decreasing, one past the buffer
    fr, of = fuzzframes.generate(200, seed=22)
    of = of.copy()
    of[50] = of[49] - 1
    of[-1] = of[-1] + 1000
    c["bad_offsets"] = (fr, of)
    for fr, of in c.values():
        fr.setflags(write=False)
        of.setflags(write=False)
    assert N_FUZZ % 64 == 29
    st = coracle.parse_classify(_cfg(2), *c["fuzz7"])[3][0]
    assert min(int(st[k]) for k in ("n_session", "n_dns", "n_drop")) > 100  # every class, many of each
    assert int(coracle.parse_classify(_cfg(2), *c["bad_offsets"])[3][0]["bad_offsets"]) == 2
    assert coracle.parse_classify(_cfg(2), *c["cut_tail"])[2][-1] == 2  # the cut frame is dropped
    return c


# ---- several batches in one launch ---------------------------------------------------------------
@pytest.mark.parametrize("flt", [SessionFilter.All, SessionFilter.GlobalOnly, SessionFilter.LocalOnly])
def test_fuzz_seg_batches_one_launch(corpus, flt):
    one = fg.pack([fg.tcp_frame("1.2.3.4", 1000, "5.6.7.8", 80, fg.SYN, 0)])
    batches = [corpus["fuzz7"], fg.pack([]), corpus["cut_tail"], one, corpus["fuzz8"], corpus["bad_offsets"]]
    cap = _capture(flt, flow_capacity=0)
    try:
        for rep in range(2):  # (the per-batch stats words are reused)
            for (frames, offs), res in zip(batches, _run_batches(cap, batches)):
                _check(cap, frames, offs, int(flt), res=res, lan_v6=lan_v6_table(LAN), own_ips=own_ip_table(OWN))
    finally:
        cap.close()


# ---- the resident queue --------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 4])
def test_fuzz_queue(corpus, depth):
    """The fuzz batches through k_parse_seg_queue, each submitted twice round the ring."""
    flt = SessionFilter.GlobalOnly
    cap = _capture(flt, flow_capacity=0)
    batches = [_Batch(*corpus[k], with_cls=k != "fuzz8") for k in ("fuzz7", "cut_tail", "fuzz8", "bad_offsets")]
    cap.parse_classify(*corpus["cut_tail"])  # (the configuration is on the device before the queue captures it)
    q = _Queue(cap, depth=depth)
    try:
        for rnd in range(2):
            for b in batches:
                b.reset()
            tickets = [q.submit(b) for b in batches]
            for t in tickets:
                q.wait(t)
            for b in batches:
                _verify(b, flt, cfg=_cfg(flt))
                assert int(b.result()[3][0]["error"]) == 0
    finally:
        q.close()
        cap.close()


def test_fuzz_shared_queue_builds_the_table(corpus):
    """A shared queue parses the fuzz batches while each completed batch is applied to the session
    table (fb_flow_update_seg_dev beside the resident kernel); the table equals the oracle's."""
    flt = SessionFilter.All
    cap = _capture(flt, flow_capacity=1 << 15, max_batch_packets=8192)
    names = ["fuzz7", "cut_tail", "fuzz8", "bad_offsets", "fuzz7"]
    sets = [DeviceSegBatch(*corpus[k]) for k in names]
    stream, ev = N.Stream(), N.Event()
    ref = coracle.Flows()
    cap.parse_classify(*corpus["cut_tail"])  # (the configuration is on the device before the queue captures it)
    q = SegQueue(cap, depth=4, idle_ms=4000, shared=True)
    try:
        for k, b in zip(names, sets):
            b.fill_outputs()
            q.wait(q.submit(b))
            b.update_table(cap, stream.ptr)
            ev.record(stream)
            ev.wait_spin()
            out, dns, cls, st = b.result()
            r_out, r_dns, r_cls, r_st = coracle.parse_classify(_cfg(flt), *corpus[k])
            r_st = r_st.copy()
            ref.update(r_out, r_st)
            assert out.tobytes() == r_out.tobytes() and dns.tobytes() == r_dns.tobytes() and np.array_equal(cls, r_cls)
            for f in STAT_KEYS:
                assert int(st[0][f]) == (0 if f == "error" else int(r_st[0][f])), (k, f)
        stream.sync()
    finally:
        q.close()
        for b in sets:
            b.free()
    try:
        assert rows_sorted(cap.export_flows()) == rows_sorted(ref.export_sorted())
    finally:
        cap.close()


# ---- fused parse + upsert, records on and off ---------------------------------------------------
def _fused(cap, frames, offs, asyn, ts=None):
    """fb_process_seg_dev / fb_process_seg_async_dev (+ join) -> (raw, seg, cls, stats); the history
    of the update is pulled when the capture tracks it."""
    lib = N.gpu_lib()
    frames, offs = np.ascontiguousarray(frames, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.uint32)
    n = offs.size - 1
    nseg = max((n + 63) // 64, 1)
    d_fr, d_of = N.DeviceBuffer(max(frames.nbytes, 1)).upload(frames), N.DeviceBuffer(offs.nbytes).upload(offs)
    d_out, d_seg, d_cls, d_st = N.DeviceBuffer(nseg * N.SEG_BYTES), N.DeviceBuffer(nseg * 4), N.DeviceBuffer(max(n, 1)), \
        N.DeviceBuffer(N.STATS_DTYPE.itemsize)
    d_out.memset(0xA5)  # unwritten bytes must stay untouched
    d_ts = cap._frame_times(ts, n)  # noqa: F841 (alive until the update is done)
    fn = lib.fb_process_seg_async_dev if asyn else lib.fb_process_seg_dev
    N.check(fn(cap.ctx, d_fr.ptr, frames.nbytes, d_of.ptr, n, d_out.ptr, d_seg.ptr, d_cls.ptr, d_st.ptr, None))
    if asyn:
        N.check(lib.fb_flow_join(cap.ctx, None))
    N.check(lib.fb_stream_sync(None))
    cap._pull_history(((n + 63) // 64) * 64)
    return (d_out.download(np.zeros(nseg * N.SEG_BYTES, dtype=np.uint8)),
            d_seg.download(np.zeros(nseg, dtype=np.uint32))[: (n + 63) // 64],
            d_cls.download(np.zeros(max(n, 1), dtype=np.uint8))[:n], d_st.download(np.zeros(1, dtype=N.STATS_DTYPE)))


def _check_fused(res, ref, r_st, records, tag):
    """One fused call against the oracle's parse (ref) and update (r_st: with new / updated)."""
    raw, seg, cls, st = res
    r_out, r_dns, r_cls, _ = ref
    assert np.array_equal(cls, r_cls), tag
    assert np.array_equal(seg, _expected_seg(r_out, r_dns, len(r_cls))), tag
    g_out, g_dns = N.seg_unpack(raw, seg)
    assert g_dns.tobytes() == r_dns.tobytes(), tag
    if records:
        assert g_out.tobytes() == r_out.tobytes(), tag
    for s, w in enumerate(seg.tolist()):  # nothing but the records (records on) and the DNS tail is written
        gap = raw[s * N.SEG_BYTES + (w & 0xFFFF) * 56 * int(records): (s + 1) * N.SEG_BYTES - 16 * (w >> 16)]
        assert (gap == 0xA5).all(), (tag, s)
    for f in STAT_KEYS:
        assert int(st[0][f]) == (0 if f == "error" else int(r_st[0][f])), (tag, f)


FUSED_ORDER = ["fuzz7", "cut_tail", "bad_offsets", "fuzz8", "fuzz7"]


@pytest.mark.parametrize("records", [True, False], ids=["records", "table_only"])
@pytest.mark.parametrize("asyn", [False, True], ids=["sync", "async"])
def test_fuzz_fused_parse_and_upsert(corpus, asyn, records):
    cap = _capture(flow_capacity=1 << 15, track_history=True)
    flows = coracle.Flows()
    try:
        if not records:
            N.check(N.gpu_lib().fb_set_session_records(cap.ctx, 0))
        for k in FUSED_ORDER:
            ref = coracle.parse_classify(_cfg(2), *corpus[k])
            r_st = ref[3].copy()
            flows.update(ref[0], r_st)
            _check_fused(_fused(cap, *corpus[k], asyn=asyn), ref, r_st, records, k)
        gf = _check_tables(cap, flows, "fused")
        assert len(gf) > 4000 and (gf["hist_len"] > 1).any()
    finally:
        cap.close()


@pytest.mark.parametrize("path", ["dense", "seg", "table_only"])
def test_fuzz_timed(corpus, path):
    """A timed context over the fuzz batches, timestamps stepping back as in frame_times(back=True):
    the time records of the flows the fuzz leaves equal the oracle's."""
    cap = _capture(flow_capacity=1 << 15, timed=True)
    flows = coracle.Flows()
    try:
        if path == "table_only":
            N.check(N.gpu_lib().fb_set_session_records(cap.ctx, 0))
        for call, k in enumerate(FUSED_ORDER):
            fr, of = corpus[k]
            ts = frame_times(len(of) - 1, seed=40 + call, call=call, back=True, jump_p=0.01)
            ref = coracle.parse_classify(_cfg(2), fr, of)
            r_st = ref[3].copy()
            flows.update(ref[0], r_st, ts=ts)
            if path == "dense":
                g = cap.process_frames(fr, of, ts=ts)
                assert g.records.tobytes() == ref[0].tobytes() and g.dns.tobytes() == ref[1].tobytes()
                assert np.array_equal(g.cls, ref[2])
                for f in STAT_KEYS:
                    assert g.stats[f] == (0 if f == "error" else int(r_st[0][f])), (k, f)
            else:
                _check_fused(_fused(cap, fr, of, asyn=path == "table_only", ts=ts), ref, r_st, path == "seg", k)
            _check_times(cap, flows, "%s call %d" % (path, call))
        t = flows.export_times()
        assert len(t) > 4000 and (t["segment_count"] > 0).any() and (t["end_time_ns"] != N.FB_SEEN_NONE).any()
    finally:
        cap.close()


# ---- the ingest ring -----------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["block", "push"])
def test_fuzz_ring(gpu_capture, corpus, how):
    """Both fuzz batches through the ring, cut into batches of 1,000 frames: totals, DNS payloads and
    the table as in test_gpu_ring.test_ring_vs_oracle."""
    (f7, o7), (f8, o8) = corpus["fuzz7"], corpus["fuzz8"]
    frames = np.concatenate([f7, f8])
    offs = np.concatenate([o7, o7[-1] + o8[1:]]).astype(np.uint32)
    n, per = len(offs) - 1, 1000
    gpu_capture.clear_all_sessions()
    ring = IngestRing(gpu_capture, slots=3, max_packets=per, max_bytes=4 << 20)
    try:
        if how == "block":
            ring.push_block(frames, offs)
        else:
            for i in range(n):
                ring.push(frames[offs[i]: offs[i + 1]].tobytes())
        ring.sync()
        tot, nb, nf = ring.stats()
        dns = ring.poll_dns()
    finally:
        ring.close()
    flows = coracle.Flows()
    r_tot, r_dns = _oracle_batches(frames, offs, per, flows)
    assert nf == n and nb == (n + per - 1) // per
    for k in STAT_KEYS:
        assert tot[k] == int(r_tot[0][k]), k
    assert [(s, p, pl) for s, p, _, pl in dns] == r_dns and len(r_dns) > 300
    assert rows_sorted(gpu_capture.export_flows()) == rows_sorted(flows.export_sorted())
    gpu_capture.clear_all_sessions()


# ---- parsed packets ------------------------------------------------------------------------------
def fuzz_parsed(n, seed):
    """Fuzzed fb_parsed_pkt records over a small pool of addresses and ports, so flows repeat."""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=N.PARSED_DTYPE)
    p["protocol"] = rng.choice([6, 17, 0, 1, 255], size=n, p=[0.45, 0.37, 0.06, 0.06, 0.06])
    p["family"] = rng.choice([2, 10, 0, 7], size=n, p=[0.6, 0.3, 0.05, 0.05])
    p["has_flags"] = rng.integers(0, 3, size=n)
    p["tcp_flags"] = rng.integers(0, 256, size=n)
    v4 = np.array([ip_to_words(a)[0] for a in ("10.0.0.1", "192.168.1.7", "127.0.0.1", "10.9.8.7", "172.16.3.4",
                                               "8.8.8.8", "93.184.216.34", "1.1.1.1", "224.0.0.251", "255.255.255.255")],
                  dtype=np.uint32)
    v6 = np.array([ip_to_words(a)[0] for a in ("fe80::1", "::1", "fd12::5", "2001:db8:abcd:12::9", "2001:db8:abcd:13::9",
                                               "2001:4860::8888", "2606:4700::1111", "ff02::fb")], dtype=np.uint32)
    # 200 conversations (address and port pairs), each packet one of them in either direction: a
    # flow sees several packets, from both sides, with and without flags
    n_conv = 200
    ports = np.array([0, 53, 65535, 80, 443, 49152, 40000, 22], dtype=np.int64)
    conv = rng.integers(0, n_conv, size=n)
    rev = rng.random(n) < 0.5
    is6 = p["family"] == 10
    ends = []
    for _ in range(2):
        a4, a6 = v4[rng.integers(0, len(v4), size=n_conv)], v6[rng.integers(0, len(v6), size=n_conv)]
        port = np.where(rng.random(n_conv) < 0.85, ports[rng.integers(0, len(ports), size=n_conv)],
                        rng.integers(0, 65536, size=n_conv))
        ends.append((np.where(is6[:, None], a6[conv], a4[conv]), port[conv]))
    (ip_a, port_a), (ip_b, port_b) = ends
    p["src_ip"], p["dst_ip"] = np.where(rev[:, None], ip_b, ip_a), np.where(rev[:, None], ip_a, ip_b)
    p["src_port"], p["dst_port"] = np.where(rev, port_b, port_a), np.where(rev, port_a, port_b)
    p["packet_length"] = np.where(rng.random(n) < 0.3, 0, rng.integers(0, 1501, size=n))
    p["ip_packet_length"] = rng.integers(0, 65536, size=n)
    p["pkt_index"] = (np.arange(n, dtype=np.uint64) * 7919 % 100003).astype(np.uint32)  # scrambled, unique
    return p


@pytest.fixture(scope="module")
def parsed_corpus():
    halves = [fuzz_parsed(N_FUZZ, 31), fuzz_parsed(1000, 32)]
    p = halves[0]
    ok = np.isin(p["protocol"], [6, 17]) & np.isin(p["family"], [2, 10])
    assert (~ok).sum() > 300 and {0, 1, 2} == set(p["has_flags"][ok & (p["protocol"] == 17)].tolist())
    return halves


def test_parsed_flags_option_literals():
    """What the fuzz found, by hand: flags is an Option -- any non-zero has_flags byte is Some (the
    kernel read bit 0 only, so has_flags = 2 lost the flags), and None carries no flag bits (the kernel
    copied tcp_flags into the record, where the frame decode and the oracle leave 0).  Both service
    ports, so the key also depends on the flags being seen."""
    from flodbadd_amd.sessions import Protocol, Session, SessionPacketData, packets_to_parsed
    a, b = Session(Protocol.TCP, "10.0.0.2", 80, "93.184.216.34", 443), Session(Protocol.TCP, "93.184.216.34", 443, "10.0.0.2", 80)
    parsed = packets_to_parsed([SessionPacketData(a, 0, 40, fg.SYN), SessionPacketData(b, 0, 40, fg.SYN | fg.ACK),
                                SessionPacketData(a, 0, 40, fg.SYN), SessionPacketData(a, 5, 45, None),
                                SessionPacketData(b, 0, 40, fg.FIN | fg.ACK)])
    parsed["has_flags"] = [1, 2, 0xFF, 0, 0x80]
    parsed["tcp_flags"][3] = fg.SYN | fg.PSH  # has_flags 0: not flags
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 10, track_history=True)
    try:
        g = cap.process_parsed(parsed)
        r_out, r_cls, _ = coracle.process_parsed(coracle.make_cfg(2), parsed)
        assert (g.records["meta"] & N.META_HAS_FLAGS).tolist() == [1, 1, 1, 0, 1]
        assert g.records["tcp_flags"].tolist() == [fg.SYN, fg.SYN | fg.ACK, fg.SYN, 0, fg.FIN | fg.ACK]
        assert bytes(g.records["hist_char"]) == b"ShS\0F"
        assert ((g.records["meta"] & N.META_SWAP) != 0).tolist() == [False, True, False, True, False]
        assert g.records.tobytes() == r_out.tobytes() and np.array_equal(g.cls, r_cls)
        flows = coracle.Flows()
        flows.update(r_out)
        gf = _check_tables(cap, flows, "literals")
        # the SYNs and the SYN|ACK share a's key; the flagless packet (no character, and its PSH bit ends
        # no segment) and the FIN fall to the port tiebreak: b's key
        assert sorted(cap.histories.values()) == ["F", "ShS"] and gf["segment_count"].tolist() == [0, 0]
    finally:
        cap.close()


@pytest.mark.parametrize("flt", [SessionFilter.All, SessionFilter.GlobalOnly, SessionFilter.LocalOnly])
def test_fuzz_parsed_dense(parsed_corpus, flt):
    """fb_process_parsed_dev (records, classes, stats) and fb_process_parsed (the same + the upsert)."""
    lib = N.gpu_lib()
    cap = _capture(flt, flow_capacity=1 << 13, track_history=True)
    flows = coracle.Flows()
    try:
        for parsed in parsed_corpus:
            n = len(parsed)
            r_out, r_cls, r_st = coracle.process_parsed(_cfg(flt), parsed)
            assert (r_cls == 2).sum() > 50 and len(r_out) > 50
            d_in, d_out = N.DeviceBuffer(parsed.nbytes).upload(parsed), N.DeviceBuffer(n * 56)
            d_cls, d_st = N.DeviceBuffer(n), N.DeviceBuffer(N.STATS_DTYPE.itemsize)
            d_out.memset(0xA5)
            N.check(lib.fb_process_parsed_dev(cap.ctx, d_in.ptr, n, d_out.ptr, d_cls.ptr, d_st.ptr, None))
            N.check(lib.fb_stream_sync(None))
            st = d_st.download(np.zeros(1, dtype=N.STATS_DTYPE))
            out = d_out.download(np.zeros(n, dtype=N.PKT_OUT_DTYPE))
            cls = d_cls.download(np.zeros(n, dtype=np.uint8))
            assert np.array_equal(cls, r_cls)
            bad = np.flatnonzero((out[: len(r_out)].view(np.uint8).reshape(-1, 56) != r_out.view(np.uint8).reshape(-1, 56)).any(axis=1))
            assert bad.size == 0, (bad.size, out[bad[:2]], r_out[bad[:2]])
            for f in STAT_KEYS:
                if f not in ("new_sessions", "updated_sessions"):
                    assert int(st[0][f]) == int(r_st[0][f]), f
            r_st = r_st.copy()
            flows.update(r_out, r_st)
            g = cap.process_parsed(parsed)
            assert g.records.tobytes() == r_out.tobytes() and np.array_equal(g.cls, r_cls)
            for f in STAT_KEYS:
                assert g.stats[f] == int(r_st[0][f]), f
        _check_tables(cap, flows, "parsed dense")
    finally:
        cap.close()


def test_fuzz_parsed_seg(parsed_corpus):
    """fb_process_parsed_seg_dev + fb_flow_update_seg_dev: segment counts, records, stats, table."""
    lib = N.gpu_lib()
    cap = _capture(flow_capacity=1 << 13, track_history=True)
    flows = coracle.Flows()
    try:
        for parsed in parsed_corpus:
            n = len(parsed)
            nseg = (n + 63) // 64
            r_out, r_cls, r_st = coracle.process_parsed(_cfg(2), parsed)
            r_st = r_st.copy()
            flows.update(r_out, r_st)
            d_in, d_out = N.DeviceBuffer(parsed.nbytes).upload(parsed), N.DeviceBuffer(nseg * N.SEG_BYTES)
            d_seg, d_cls, d_st = N.DeviceBuffer(nseg * 4), N.DeviceBuffer(n), N.DeviceBuffer(N.STATS_DTYPE.itemsize)
            d_out.memset(0xA5)
            N.check(lib.fb_process_parsed_seg_dev(cap.ctx, d_in.ptr, n, d_out.ptr, d_seg.ptr, d_cls.ptr, d_st.ptr, None))
            N.check(lib.fb_flow_update_seg_dev(cap.ctx, d_out.ptr, d_seg.ptr, n, d_st.ptr, None))
            N.check(lib.fb_stream_sync(None))
            cap._pull_history(nseg * 64)
            seg = d_seg.download(np.zeros(nseg, dtype=np.uint32))
            raw = d_out.download(np.zeros(nseg * N.SEG_BYTES, dtype=np.uint8))
            assert np.array_equal(d_cls.download(np.zeros(n, dtype=np.uint8)), r_cls)
            want = np.add.reduceat((r_cls == 0).astype(np.uint32), np.arange(0, n, 64))
            assert np.array_equal(seg, want)
            assert N.seg_unpack(raw, seg)[0].tobytes() == r_out.tobytes()
            for s, w in enumerate(seg.tolist()):
                assert (raw[s * N.SEG_BYTES + w * 56: (s + 1) * N.SEG_BYTES] == 0xA5).all(), s
            st = d_st.download(np.zeros(1, dtype=N.STATS_DTYPE))
            for f in STAT_KEYS:
                assert int(st[0][f]) == int(r_st[0][f]), f
        _check_tables(cap, flows, "parsed seg")
    finally:
        cap.close()
