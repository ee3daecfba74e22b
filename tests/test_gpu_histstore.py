"""The device-resident session history (fb_hist_store_*, flodbadd_amd/csrc/fb_histstore.hip; the capture's
history_on_device=True).

Every flow's string gathered from the store must equal the oracle's `history` (coracle.Flows().history, as in
test_gpu_history.py) character for character, and the store's counters must equal what the strings imply:
blocks_in_use = the sum of ceil(len / FB_HIST_BLOCK_CHARS), chars = the sum of the lengths.  The inputs sit on
the store's own edges: block boundaries reached in one run and character by character, runs and chains around
the cooperative thresholds (FB_HIST_COOP_RUN, FB_HIST_COOP_GATHER), table and pool growths, a purge with reuse
of the freed blocks, a clear, and the Zeek export from the store against the host-blob path and zeekref.  No
tolerance applies anywhere: the outputs are text and integers."""
import ctypes as C

import numpy as np
import pytest

import framegen as fg
import zeekref
from flodbadd_amd import _native as N
from flodbadd_amd import synth
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.sessions import SessionFilter
from oracle import coracle

pytestmark = pytest.mark.gpu

BLK, COOP_RUN, COOP_GATHER = N.FB_HIST_BLOCK_CHARS, N.FB_HIST_COOP_RUN, N.FB_HIST_COOP_GATHER
S = 10 ** 9
T0 = 1_752_800_000 * S
DAY = 86400 * S
FLAGS = (fg.SYN, fg.SYN | fg.ACK, fg.ACK, fg.PSH | fg.ACK, fg.FIN | fg.ACK, fg.RST)
CFG = None


def blocks_of(n):
    return (n + BLK - 1) // BLK


def frames_of(k, first, count):
    """`count` TCP frames of flow k, its flag cycle continued from packet `first` (one history character each);
    handshake packets travel the way their flags say, the others alternate."""
    a = "10.%d.%d.%d" % (k >> 16 & 255, k >> 8 & 255, k & 255)
    out = []
    for j in range(first, first + count):
        flags = FLAGS[(k + j) % len(FLAGS)]
        fwd = flags == fg.SYN if flags & fg.SYN else j % 2 == 0
        src, sp, dst, dp = (a, 40000 + k % 7, "93.184.216.34", 443) if fwd else ("93.184.216.34", 443, a, 40000 + k % 7)
        out.append(fg.tcp_frame(src, sp, dst, dp, flags, 10 * (j % 3)))
    return out


def interleave(per_flow):
    """Round-robin over the flows' frame lists: every flow's frames keep their order, the flows mix."""
    out = []
    for k in range(max((len(f) for f in per_flow), default=0)):
        out += [f[k] for f in per_flow if k < len(f)]
    return out


def records(frames, offs):
    global CFG
    if CFG is None:
        CFG = coracle.make_cfg(2)
    return coracle.parse_classify(CFG, frames, offs)[0]


def make_cap(**kw):
    kw.setdefault("flow_capacity", 1 << 12)
    return FlodbaddGpuCapture(0, session_filter=SessionFilter.All, track_history=True, history_on_device=True, **kw)


def feed(cap, ref, frames, seg=False, ts=None):
    buf, offs = fg.pack(frames)
    (cap.process_frames_seg if seg else cap.process_frames)(buf, offs, ts=ts)
    if ref is not None:
        ref.update(records(buf, offs))


def check(cap, ref, keys=None):
    """Every flow's gathered string against the oracle's, and the counters the strings imply -> {key: str}."""
    gf = cap.export_flows()
    got = cap.flow_histories()
    out, lens = {}, []
    for r in gf:
        h, _ = ref.history(r)
        assert got.get(int(r["slot"]), "") == h, (int(r["slot"]), len(h))
        assert int(r["hist_len"]) == len(h)
        out[r.tobytes()[:40]] = h
        lens.append(len(h))
    assert set(got) == {int(r["slot"]) for r in gf if int(r["hist_len"])}
    info = cap.history_store_info()
    assert info["blocks_in_use"] == sum(blocks_of(n) for n in lens)
    assert info["chars"] == sum(lens) and info["flows"] == sum(1 for n in lens if n)
    assert info["blocks_in_use"] == info["blocks_high_water"] - info["blocks_free"] <= info["blocks_capacity"]
    assert cap.histories == {}
    return out


# ---- 1. block edges ----------------------------------------------------------------------------------------
EDGES = (1, 2, 119, 120, 121, 239, 240, 241, 361)


@pytest.mark.parametrize("seg", [False, True], ids=["dense", "seg"])
def test_block_edges_in_one_batch(seg):
    cap, ref = make_cap(), coracle.Flows()
    try:
        feed(cap, ref, interleave([frames_of(k, 0, n) for k, n in enumerate(EDGES)]), seg)
        by_key = check(cap, ref)
        assert sorted(len(h) for h in by_key.values()) == sorted(EDGES)
        assert cap.history_store_info()["blocks_in_use"] == sum(blocks_of(n) for n in EDGES)
    finally:
        cap.close()


def test_block_edges_character_by_character():
    """119 characters first, then batches that add 1 to 3 to every flow still short of its target: every odd and
    even start nibble, and every way of exactly filling the tail block, occurs."""
    cap, ref = make_cap(), coracle.Flows()
    try:
        have = [min(n, 119) for n in EDGES]
        feed(cap, ref, interleave([frames_of(k, 0, n) for k, n in enumerate(have)]))
        b, starts = 0, set()
        while have != list(EDGES):
            per_flow = []
            for k, n in enumerate(EDGES):
                add = min(1 + (k + b) % 3, n - have[k])
                if add:
                    starts.add((have[k] % BLK, add))
                per_flow.append(frames_of(k, have[k], add))
                have[k] += add
            feed(cap, ref, interleave(per_flow), seg=b % 2 == 1)
            b += 1
            if b % 40 == 0:
                check(cap, ref)
        by_key = check(cap, ref)
        assert sorted(len(h) for h in by_key.values()) == sorted(EDGES)
        # a run that ends exactly at the block's end, one that starts a new block, odd and even starts
        assert any((s + a) % BLK == 0 for s, a in starts) and any(s == 0 for s, a in starts)
        assert {s % 2 for s, _ in starts} == {0, 1}
        assert cap.history_store_info()["appends"] == b + 1
    finally:
        cap.close()


# ---- 2. the run-size and chain-size paths ------------------------------------------------------------------
@pytest.mark.parametrize("seg", [False, True], ids=["dense", "seg"])
def test_runs_and_chains_around_the_cooperative_thresholds(seg):
    """One batch with runs of FB_HIST_COOP_RUN - 1, FB_HIST_COOP_RUN and + 1 characters on flows whose stored
    length is 0, 1 and 119, runs that the wave's 64-wide search ends at, inside and past its first step, and
    chains of FB_HIST_COOP_GATHER - 1, FB_HIST_COOP_GATHER and + 1 characters."""
    cap, ref = make_cap(), coracle.Flows()
    try:
        stored = [s for s in (0, 1, 119) for _ in range(3)]
        runs = [COOP_RUN - 1, COOP_RUN, COOP_RUN + 1] * 3
        wide = [COOP_RUN + 63, COOP_RUN + 64, COOP_RUN + 65, 500]
        chains = [COOP_GATHER - 1, COOP_GATHER, COOP_GATHER + 1]
        feed(cap, ref, interleave([frames_of(k, 0, s) for k, s in enumerate(stored)]), seg)
        check(cap, ref)
        per_flow = [frames_of(k, s, r) for k, (s, r) in enumerate(zip(stored, runs))]
        per_flow += [frames_of(100 + k, 0, r) for k, r in enumerate(wide)]
        per_flow += [frames_of(200 + k, 0, r) for k, r in enumerate(chains)]
        # (the runs are contiguous in the history output whatever the frame order: it is grouped per flow)
        feed(cap, ref, interleave(per_flow), seg)
        by_key = check(cap, ref)
        want = sorted([s + r for s, r in zip(stored, runs)] + wide + chains)
        assert sorted(len(h) for h in by_key.values()) == want
    finally:
        cap.close()


# ---- 3. oracle parity at width -----------------------------------------------------------------------------
def test_zipf_batches_equal_the_oracle_and_the_host_dict():
    """The three 150k-frame Zipf(1.1) batches of test_history_synthetic_zipf: hot flows of thousands of characters
    spanning batches; the host-dict capture runs beside the device store."""
    batches = [synth.generate(4, 150000, first=b * 150000, zipf=1, zipf_s=1.1) for b in range(3)]
    dev = make_cap(flow_capacity=1 << 20)
    host = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 20, track_history=True)
    ref = coracle.Flows()
    try:
        for frames, offs in batches:
            dev.process_frames_seg(frames, offs)
            host.process_frames(frames, offs)
            ref.update(records(frames, offs))
        by_key = check(dev, ref)
        assert max(len(h) for h in by_key.values()) > 2000
        hosts = {r.tobytes()[:40]: host.histories.get(int(r["slot"]), "") for r in host.export_flows()}
        assert hosts == by_key
        # the getter hands the same strings on
        got = {str(i.session): i.stats.history for i in dev.get_sessions()}
        assert got == {str(i.session): i.stats.history for i in host.get_sessions()}
        assert dev.history_store_info()["missed_updates"] == 0
    finally:
        dev.close()
        host.close()


# ---- 4. growth ---------------------------------------------------------------------------------------------
def _mk(k):
    return fg.tcp_frame("10.%d.%d.%d" % ((k >> 16) & 255, (k >> 8) & 255, k & 255), 40000 + (k % 7), "8.8.8.8", 443,
                        (fg.SYN, fg.ACK, fg.PSH | fg.ACK, fg.FIN | fg.ACK)[k % 4], 10 + k % 5)


def test_table_and_pool_growth():
    """The batches of test_grow_instead_of_table_full on a 512-slot table with a 64-block pool: the table grows at
    least twice, the pool several times, always by doubling, and the strings stay the oracle's after each."""
    cap, ref = make_cap(flow_capacity=512, history_block_capacity=64), coracle.Flows()
    try:
        assert cap.history_store_info()["blocks_capacity"] == 64
        caps = [64]
        for frames in [[_mk(k) for k in range(300)] * 3] + [[_mk(k) for k in range(m)] for m in (600, 1000, 1500, 2000)]:
            feed(cap, ref, frames)
            check(cap, ref)
            caps.append(cap.history_store_info()["blocks_capacity"])
        info = cap.table_info()
        assert info["generation"] >= 2 and info["capacity"] >= 4096, info
        assert all(c % 64 == 0 and (c // 64) & (c // 64 - 1) == 0 for c in caps) and caps == sorted(caps)
        assert len(set(caps)) >= 4, caps
    finally:
        cap.close()


def test_fixed_table_with_a_pool_too_small():
    cap, ref = make_cap(grow=False, history_block_capacity=64), coracle.Flows()
    lib = N.gpu_lib()
    try:
        feed(cap, ref, [_mk(k) for k in range(50)])
        before, info0 = check(cap, ref), cap.history_store_info()
        with pytest.raises(N.FbError) as e:                 # 50 blocks in use + 100 record slots > 64
            feed(cap, None, [_mk(k) for k in range(100)])
        assert e.value.code == N.FB_ERR_TABLE_FULL
        info1 = cap.history_store_info()
        assert dict(info1, missed_updates=0) == info0 and info1["missed_updates"] == 1
        assert lib.fb_hist_store_append_dev(cap.ctx, None) == N.FB_ERR_TABLE_FULL
        assert cap.history_store_info() == info1
        got = cap.flow_histories()
        assert {r.tobytes()[:40]: got.get(int(r["slot"]), "") for r in cap.export_flows()} == \
            {**{r.tobytes()[:40]: "" for r in cap.export_flows()}, **before}
    finally:
        cap.close()


# ---- 5. purge and reuse ------------------------------------------------------------------------------------
def _strings(cap):
    got = cap.flow_histories()
    return {r.tobytes()[:40]: got.get(int(r["slot"]), "") for r in cap.export_flows()}


def test_purge_frees_the_chains_and_new_flows_reuse_them():
    cap = make_cap(timed=True, flow_capacity=512)
    try:
        lens = [(3, 130, 250, 17)[k % 4] + k % 5 for k in range(200)]
        frames = interleave([frames_of(k, 0, n) for k, n in enumerate(lens)])
        feed(cap, None, frames, ts=T0 + np.arange(len(frames), dtype=np.uint64) * 1000)
        frames = interleave([frames_of(k, lens[k], 2) for k in range(100, 200)])
        feed(cap, None, frames, ts=T0 + 2 * DAY + np.arange(len(frames), dtype=np.uint64) * 1000)
        before, info0 = _strings(cap), cap.history_store_info()
        assert sorted(len(h) for h in before.values()) == sorted(lens[:100] + [n + 2 for n in lens[100:]])
        slots0 = {r.tobytes()[:40]: int(r["slot"]) for r in cap.export_flows()}
        ag = cap.update_sessions_status(T0 + 2 * DAY + 100 * S)      # flows 0 .. 99 are a day past retention
        assert ag["purged"] == 100 and cap.flow_count() == 100
        after, info1 = _strings(cap), cap.history_store_info()
        assert after == {k: h for k, h in before.items() if k in after} and len(after) == 100
        assert any(slots0[r.tobytes()[:40]] != int(r["slot"]) for r in cap.export_flows())  # survivors moved
        freed = sum(blocks_of(n) for n in lens[:100])
        assert info1["blocks_free"] == freed and info1["blocks_high_water"] == info0["blocks_high_water"]
        assert info1["blocks_in_use"] == info0["blocks_in_use"] - freed == sum(blocks_of(len(h)) for h in after.values())
        assert info1["chars"] == sum(len(h) for h in after.values()) and info1["flows"] == 100
        # new flows whose blocks fit the free stack, and a purged key that sends again
        new = [frames_of(k, 0, 1 + k % 4) for k in range(300, 320)] + [frames_of(5, 0, 3)]
        frames = interleave(new)
        assert len(new) < freed
        buf, offs = fg.pack(frames)
        fresh = coracle.Flows()
        fresh.update(records(buf, offs))
        cap.process_frames(buf, offs, ts=T0 + 2 * DAY + 200 * S + np.arange(len(frames), dtype=np.uint64) * 1000)
        info2 = cap.history_store_info()
        assert info2["blocks_high_water"] == info1["blocks_high_water"] and info2["blocks_free"] == freed - len(new)
        got = cap.flow_histories()
        for r in cap.export_flows():
            k = r.tobytes()[:40]
            h = got.get(int(r["slot"]), "")
            if k in after:
                assert h == after[k]
            else:
                assert h == fresh.history(r)[0] and 1 <= len(h) <= 4   # (flow 5 starts an empty history)
        assert cap.flow_count() == 121 and cap.histories == {}
    finally:
        cap.close()


# ---- 6. clear and misuse -----------------------------------------------------------------------------------
def test_clear_enable_rules_repeated_and_missing_appends():
    lib = N.gpu_lib()
    cap, ref = make_cap(timed=True), coracle.Flows()
    try:
        assert lib.fb_hist_store_enable(cap.ctx, None) == N.FB_ERR_INVAL          # already enabled
        frames = interleave([frames_of(k, 0, 5 + k) for k in range(30)])
        ts = T0 + np.arange(len(frames), dtype=np.uint64) * 1000
        feed(cap, None, frames, ts=ts)
        assert cap.history_store_info()["chars"] == len(frames)
        cap.clear_all_sessions()
        info = cap.history_store_info()
        assert (info["chars"], info["blocks_in_use"], info["blocks_free"], info["blocks_high_water"], info["flows"]) == \
            (0, 0, 0, 0, 0)
        assert cap.flow_histories() == {}
        feed(cap, ref, frames, ts=ts)
        check(cap, ref)
        # a second append for the same update adds nothing
        info = cap.history_store_info()
        N.check(lib.fb_hist_store_append_dev(cap.ctx, None))
        assert cap.history_store_info() == info and info["missed_updates"] == 0
        check(cap, ref)
        # an update no append follows: counted, and the export sees lengths that disagree
        cap.export_zeek()
        cap.track_history = False                      # (this batch's append is left out)
        try:
            more = interleave([frames_of(k, 5 + k, 2) for k in range(7)])
            feed(cap, None, more, ts=T0 + S + np.arange(len(more), dtype=np.uint64) * 1000)
        finally:
            cap.track_history = True
        assert cap.history_store_info()["missed_updates"] == 1
        with pytest.raises(N.FbError) as e:
            cap.export_zeek()
        assert e.value.code == N.FB_ERR_INTERNAL and "7 flows" in str(e.value)
    finally:
        cap.close()
    plain = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 12)
    try:
        assert lib.fb_hist_store_append_dev(plain.ctx, None) == N.FB_ERR_INVAL    # no store
        plain.process_frames(*fg.pack(frames_of(1, 0, 3)))
        assert lib.fb_hist_store_enable(plain.ctx, None) == N.FB_ERR_INVAL         # the table has taken an update
        bad = np.zeros(1, dtype=N.HIST_STORE_CONFIG_DTYPE)
        bad[0]["flags"] = 1
        plain.clear_all_sessions()
        assert lib.fb_hist_store_enable(plain.ctx, N.ptr(bad)) == N.FB_ERR_INVAL
        N.check(lib.fb_hist_store_enable(plain.ctx, None))
    finally:
        plain.close()
    none = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=0)
    try:
        assert lib.fb_hist_store_enable(none.ctx, None) == N.FB_ERR_INVAL          # no flow table
    finally:
        none.close()


# ---- 7. Zeek from the store --------------------------------------------------------------------------------
@pytest.mark.parametrize("step", ["empty", "clear", "purge"])
def test_no_history_of_an_update_whose_record_is_gone(step):
    """The record of the last update dies with an empty update call, a clear and a purge that removes flows.
    A 200-frame update (4 segments, the last one partial) whose append was left out, then the step:
    fb_flow_history_dev reports 0 characters, and the late fb_hist_store_append_dev succeeds without applying
    anything -- the update stays a missed one."""
    lib = N.gpu_lib()
    cap = make_cap(timed=True, flow_capacity=1 << 10)
    try:
        cap.track_history = False  # (no append after the batches below)
        frames = interleave([frames_of(k, 0, 4) for k in range(50)])
        feed(cap, None, frames, seg=True, ts=T0 + np.arange(len(frames), dtype=np.uint64) * 1000)
        assert sum(len(h) for h in cap.flow_history(256).values()) == len(frames) == 200  # the record is live
        if step == "empty":
            feed(cap, None, [], seg=True, ts=np.zeros(0, dtype=np.uint64))
        elif step == "clear":
            cap.clear_all_sessions()
        else:
            assert cap.update_sessions_status(T0 + 2 * DAY)["purged"] == 50
        d_n = N.DeviceBuffer(4)
        d_n.memset(0xFF)
        N.check(lib.fb_flow_history_dev(cap.ctx, None, None, d_n.ptr, None))
        assert int(d_n.download(np.zeros(1, dtype=np.uint32))[0]) == 0
        info = cap.history_store_info()
        N.check(lib.fb_hist_store_append_dev(cap.ctx, None))
        assert cap.history_store_info() == info
        assert (info["appends"], info["missed_updates"], info["chars"]) == (0, 1, 0)
    finally:
        cap.close()


def _zeek_batches():
    lens = [2 + k % 3 for k in range(3000)]
    for k, n in ((7, 63), (8, 64), (9, 65), (10, 119), (11, 120), (12, 121), (13, 700)):
        lens[k] = n
    b1 = interleave([frames_of(k, 0, n) for k, n in enumerate(lens)])
    b2 = interleave([frames_of(k, lens[k], 1 + k % 2) for k in range(2000, 3000)] + [frames_of(13, 700, 40)])
    return ((b1, T0 + np.arange(len(b1), dtype=np.uint64) * 1237),
            (b2, T0 + 50 * S + np.arange(len(b2), dtype=np.uint64) * 1237))


def _lines(log):
    """The log's lines cut at its offsets (each ends in its newline, the offsets cover the text), sorted."""
    raw, off = log.text.tobytes(), log.line_off.astype(np.int64)
    assert off[0] == 0 and off[-1] == len(raw) == log.stats["bytes"] and len(off) - 1 == log.stats["lines_written"]
    lines = [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    assert all(l.endswith(b"\n") and l.count(b"\n") == 1 for l in lines)
    return sorted(l[:-1].decode("ascii") for l in lines)


def test_zeek_from_the_store_equals_the_host_blob_path_and_zeekref():
    lib = N.gpu_lib()
    dev = make_cap(timed=True, flow_capacity=1 << 13)
    host = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 13, timed=True, track_history=True)
    try:
        (b1, ts1), (b2, ts2) = _zeek_batches()
        for frames, ts in ((b1, ts1), (b2, ts2)):
            buf, offs = fg.pack(frames)
            dev.process_frames(buf, offs, ts=ts)
            host.process_frames(buf, offs, ts=ts)
        for since in (None, T0 + 40 * S):
            views = dev.export_view(N.FB_VIEW_ALL, since, SessionFilter.All)
            assert len(views) == (3000 if since is None else 1001)
            # (a view export compacts with one atomic per workgroup, so its record order is not fixed, and a line
            # does not depend on its flow's slot: the logs are compared line by line, every line byte for byte,
            # with zeekref's lines over the twin's own records and host strings)
            theirs = host.export_view(N.FB_VIEW_ALL, since, SessionFilter.All)
            assert len(theirs) == len(views)
            want = sorted(zeekref.expected_lines(theirs, host.histories))
            blob = host.export_zeek(N.FB_VIEW_ALL, since, SessionFilter.All)
            assert _lines(blob) == want
            for direct in (0, 1):
                N.check(lib.fb_debug_set(dev.ctx, N.FB_DEBUG_ZEEK_DIRECT, direct))
                try:
                    log = dev.export_zeek(N.FB_VIEW_ALL, since, SessionFilter.All)
                finally:
                    lib.fb_debug_set(dev.ctx, N.FB_DEBUG_ZEEK_DIRECT, 0)
                assert _lines(log) == want
                assert log.stats == blob.stats and log.stats["hist_mismatch"] == 0
        assert dev.histories == {}
        got = {str(i.session): i.stats.history for i in dev.get_sessions()}
        assert got == {str(i.session): i.stats.history for i in host.get_sessions()} and max(map(len, got.values())) == 740
    finally:
        dev.close()
        host.close()


def test_gather_writes_nothing_at_or_past_cap():
    """A cap that cuts inside a flow's range: that flow and every later one are left out, the ones before are
    whole, and the canary after the buffer is untouched.  Slots given as a packed array and as NULL agree."""
    lib = N.gpu_lib()
    cap, ref = make_cap(), coracle.Flows()
    try:
        feed(cap, ref, interleave([frames_of(k, 0, (5, 70, 130)[k % 3] + k) for k in range(40)]))
        n = cap.table_info()["capacity"]
        d_off = N.DeviceBuffer(8 * (n + 1))
        N.check(lib.fb_hist_store_lengths_dev(cap.ctx, None, 0, n, d_off.ptr, None))
        off = d_off.download(np.zeros(n + 1, dtype=np.uint64)).astype(np.int64)
        total = int(off[n])
        assert total == cap.history_store_info()["chars"]
        full = N.DeviceBuffer(total)
        N.check(lib.fb_hist_store_gather_dev(cap.ctx, None, 0, n, d_off.ptr, full.ptr, total, None))
        full = full.download(np.zeros(total, dtype=np.uint8))
        whole = cap.flow_histories()
        assert {s: full[off[s]:off[s + 1]].tobytes().decode() for s in whole} == whole
        assert cap.flow_histories(np.array(sorted(whole), dtype=np.uint32)) == whole
        assert cap.flow_histories(np.array([n, n + 5, 0xFFFFFFFF], dtype=np.uint32)) == {}   # past the capacity
        lens = np.diff(off)
        for cut_slot in (int(np.flatnonzero(lens >= COOP_GATHER)[3]), int(np.flatnonzero((lens > 1) & (lens < COOP_GATHER))[2])):
            for cut in (int(off[cut_slot]) + 1, int(off[cut_slot + 1]) - 1):
                buf = N.DeviceBuffer(cut + 64)
                buf.memset(0xA5)
                N.check(lib.fb_hist_store_gather_dev(cap.ctx, None, 0, n, d_off.ptr, buf.ptr, cut, None))
                got = buf.download(np.zeros(cut + 64, dtype=np.uint8))
                assert got[:off[cut_slot]].tobytes() == full[:off[cut_slot]].tobytes()
                assert (got[off[cut_slot]:] == 0xA5).all()
    finally:
        cap.close()
