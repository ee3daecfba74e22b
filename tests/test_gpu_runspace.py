"""The history ordering (flodbadd_amd/csrc/fb_hist.hip) on enumerated run lengths, against the oracle.

The corpora of tests/runspace.py choose how many records every (bucketing chunk, partition) group holds,
so each data-dependent path of the launcher -- k_hist_uniform's three register networks, k_hist_general's
register / wavefront / bitmap sorts, long_run in record and in entry windows, combined groups read back
through e_sort, batch cuts at kHistCap, the second chunk round, the split over chunk blocks, the code
drop for an entry the table refused -- is reached by construction; tests/test_runspace_oracle.py asserts
that coverage on the CPU (runspace.census) and pins the reference strings (the CYCLE13 closed form).

  path      entry point                                                        corpora
  placed    fb_flow_update_seg_dev on a buffer built on the host (K1 hashes)    all
  records   fb_flow_update_records_dev on the dense records                     ladder, combined
  parsed    fb_process_parsed (the capture's process_parsed)                    ladder, combined
  seg       fb_process_seg_dev, the fused parse handing over rec_part and       ladder, combined
            update entries

On the dense and fused layouts the census is recomputed for the slots the path really uses (the record
index) and a stated subset of classes is asserted.  Compared in every case (test_gpu_flagspace._check_tables):
every fb_flow_rec field but slot, every history string and conn_state, hist_len, new / updated sessions
per call, error == 0; and on the raw fb_flow_history_dev output of every call: *n_hist == the call's TCP
records, one contiguous run per flow, partitions ascending.  `rounds` and `blocks` run once more with the
device history store (fb_hist_store_append_dev calls the launcher with its own arguments), and `ladder`
once on a timed context (the plain K2, no combining)."""
import functools

import numpy as np
import pytest

import flagseq as fs
import runspace as rs
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.sessions import SessionFilter
from oracle import coracle
from test_gpu_flagspace import _check_tables
from test_gpu_timed import _check as _check_times

pytestmark = pytest.mark.gpu

CORPORA = {"ladder": (rs.ladder, 16), "waves": (rs.waves, 16), "combined": (lambda: rs.combined()[0], 256),
           "blocks": (rs.blocks, 16), "rounds": (rs.rounds, 16), "scramble": (rs.scramble, 16)}
BASE_NS = 1_700_000_000 * 10 ** 9


def _times(call):
    """Capture timestamps indexed by pkt_index (= the record slot): 1 us a slot (_reference puts the calls 7 s apart)."""
    return (BASE_NS + np.arange(call.n_slots, dtype=np.uint64) * 1000).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _reference(name, by_frame=False, timed=False):
    """The corpus through the oracle's table, once: per call (Call, records, stats, ts) and the table.
    by_frame: pkt_index = the frame's index (what a parse of the call's frames gives), not the placed slot."""
    calls = CORPORA[name][0]() if name in CORPORA else rs.overfull()
    flows, out = coracle.Flows(), []
    for k, c in enumerate(calls):
        recs = c.recs.copy()
        if by_frame:
            recs["pkt_index"] = np.arange(len(recs))
        ts = _times(c) + np.uint64(k * 7 * 10 ** 9) if timed else None
        st = np.zeros(1, dtype=N.STATS_DTYPE)
        flows.update(recs, st, ts=ts)
        for a in (recs, st):
            a.setflags(write=False)
        out.append((c, recs, st, ts))
    return out, flows


def _capture(parts, **kw):
    return FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=parts * rs.SLOTS, grow=False, **kw)


def _stats(d_st):
    st = d_st.download(np.zeros(1, dtype=N.STATS_DTYPE))
    return {k: int(st[0][k]) for k in N.STATS_FIELDS if not k.startswith("reserved")}


def _raw_history(cap, n_slots, tag, n_tcp=None):
    """fb_flow_history_dev of the last update, checked as it comes from the device, then appended to
    cap.histories: *n_hist == the call's TCP records, one contiguous run per flow, partitions ascending."""
    m = max(int(n_slots), 1)
    d_h, d_s, d_n = N.DeviceBuffer(m), N.DeviceBuffer(4 * m), N.DeviceBuffer(4)
    N.check(N.gpu_lib().fb_flow_history_dev(cap.ctx, d_h.ptr, d_s.ptr, d_n.ptr, None))
    k = int(d_n.download(np.zeros(1, dtype=np.uint32))[0])
    assert n_tcp is None or k == n_tcp, "%s: *n_hist %d, the call holds %d TCP records" % (tag, k, n_tcp)
    if k == 0:
        return np.zeros(0, dtype=np.uint32)
    chars = d_h.download(np.zeros(k, dtype=np.uint8), k)
    slots = d_s.download(np.zeros(k, dtype=np.uint32), 4 * k)
    cut = np.flatnonzero(np.diff(slots)) + 1
    starts, ends = np.r_[0, cut], np.r_[cut, k]
    first = slots[starts]
    assert len(np.unique(first)) == len(first), "%s: a flow's characters come in more than one run" % tag
    assert (np.diff(first.astype(np.int64) // rs.SLOTS) >= 0).all(), "%s: partitions out of order" % tag
    for a, b in zip(starts.tolist(), ends.tolist()):
        cap.histories[int(slots[a])] = cap.histories.get(int(slots[a]), "") + chars[a:b].tobytes().decode("ascii")
    return slots


def _placed(cap, call, ts=None):
    """fb_flow_update_seg_dev on the placed buffer -> (stats, the device buffers the history still reads)."""
    out, seg = rs.place(call.recs, call.slots, call.n_slots)
    st0 = np.zeros(1, dtype=N.STATS_DTYPE)
    st0[0]["n_session"] = len(call.recs)
    d_out, d_seg = N.DeviceBuffer(out.nbytes).upload(out), N.DeviceBuffer(seg.nbytes).upload(seg)
    d_st = N.DeviceBuffer(st0.nbytes).upload(st0)
    d_ts = cap._frame_times(ts, call.n_slots)
    N.check(N.gpu_lib().fb_flow_update_seg_dev(cap.ctx, d_out.ptr, d_seg.ptr, call.n_slots, d_st.ptr, None))
    N.check(N.gpu_lib().fb_stream_sync(None))
    return _stats(d_st), (d_out, d_seg, d_st, d_ts)


def _records(cap, recs):
    """fb_flow_update_records_dev on the dense records."""
    r = rs.dense(recs)
    st0 = np.zeros(1, dtype=N.STATS_DTYPE)
    st0[0]["n_session"] = len(r)
    d_recs, d_st = N.DeviceBuffer(r.nbytes).upload(r), N.DeviceBuffer(st0.nbytes).upload(st0)
    N.check(N.gpu_lib().fb_flow_update_records_dev(cap.ctx, d_recs.ptr, len(r), d_st.ptr, None))
    N.check(N.gpu_lib().fb_stream_sync(None))
    return _stats(d_st), (d_recs, d_st)


def _fused(cap, call, want):
    """fb_process_seg_dev on the call's frames: the parse hands the update rec_part and update entries."""
    fr, of = rs.frames(call.flow, call.sym)
    n = len(of) - 1
    nseg = (n + 63) // 64
    d_fr, d_of = N.DeviceBuffer(fr.nbytes).upload(fr), N.DeviceBuffer(of.nbytes).upload(of)
    d_out, d_seg, d_st = N.DeviceBuffer(nseg * N.SEG_BYTES), N.DeviceBuffer(nseg * 4), N.DeviceBuffer(N.STATS_DTYPE.itemsize)
    N.check(N.gpu_lib().fb_process_seg_dev(cap.ctx, d_fr.ptr, fr.nbytes, d_of.ptr, n, d_out.ptr, d_seg.ptr, None,
                                           d_st.ptr, None))
    N.check(N.gpu_lib().fb_stream_sync(None))
    seg = d_seg.download(np.zeros(nseg, dtype=np.uint32))
    got, dns = N.seg_unpack(d_out.download(np.zeros(nseg * N.SEG_BYTES, dtype=np.uint8)), seg)
    assert len(dns) == 0 and got.tobytes() == want.tobytes()
    # every frame yields a session record, so the record slot is the frame's index
    assert (seg[:-1] == 64).all() and int(seg.sum()) == n
    return _stats(d_st), (d_fr, d_of, d_out, d_seg, d_st)


# classes the dense and fused layouts must still reach (their census, over the corpus' calls)
DENSE_CLASSES = {"ladder": {"reg4", "reg8", "reg16", "wave1", "wave2", "wave4", "wave8", "bitmap", "long_plain"},
                 "combined": {"combined", "long_combined"}}


def _run(name, path, timed=False, on_device=False):
    parts = CORPORA[name][1]
    ref, flows = _reference(name, by_frame=path == "seg", timed=timed)
    tag = "%s/%s%s%s" % (name, path, "/timed" if timed else "", "/store" if on_device else "")
    # (a fixed table's store cannot grow: it must hold one block per record slot of an update before the append)
    cap = _capture(parts, timed=timed, track_history=on_device, history_on_device=on_device,
                   history_block_capacity=max(c.n_slots for c, _, _, _ in ref) + 4096 if on_device else 0)
    seen = set()
    try:
        assert int(cap.table_info()["partitions"]) == parts
        for k, (call, recs, r_st, ts) in enumerate(ref):
            n = len(recs)
            if path == "placed":
                st, keep = _placed(cap, call, ts)
                n_slots, cen = call.n_slots, rs.census_of(call, parts, hot=not timed, overflow_ok=True)
            else:
                n_slots = n if path != "seg" else (n + 63) // 64 * 64
                cen = rs.census(np.arange(n), call.keys, call.codes, parts, n_slots, overflow_ok=True)
                if path == "records":
                    st, keep = _records(cap, recs)
                elif path == "parsed":
                    g = cap.process_parsed(fs.parsed_of(recs))
                    assert g.records.tobytes() == recs.tobytes(), (tag, k)
                    st, keep = g.stats, None
                else:
                    st, keep = _fused(cap, call, recs)
            seen |= rs.classes(cen)
            assert st["error"] == 0, (tag, k, st)
            got, want = (st["new_sessions"], st["updated_sessions"]), (int(r_st[0]["new_sessions"]), int(r_st[0]["updated_sessions"]))
            assert got == want, "%s, call %d: new / updated sessions %s, the oracle's %s" % (tag, k, got, want)
            assert st["n_session"] == n
            if on_device:
                cap._pull_history(n_slots)
            else:
                _raw_history(cap, n_slots, "%s, call %d" % (tag, k), n_tcp=int((call.codes != 0).sum()))
            del keep
        if path != "placed":
            assert DENSE_CLASSES[name] <= seen, (tag, sorted(seen))
        if on_device:
            cap.histories = cap.flow_histories()
        gf = _check_tables(cap, flows, tag)
        if timed:
            _check_times(cap, flows, tag)
        return gf, seen
    finally:
        cap.close()


@pytest.mark.parametrize("name", sorted(CORPORA))
def test_runspace_placed(name):
    """Every corpus through fb_flow_update_seg_dev on the placed buffer."""
    gf, _ = _run(name, "placed")
    assert len(gf) == len(rs.closed_form(CORPORA[name][0]()))


DENSE_CASES = [(name, path) for name in ("ladder", "combined") for path in ("records", "parsed", "seg")]


@pytest.mark.parametrize("name,path", DENSE_CASES, ids=["%s-%s" % c for c in DENSE_CASES])
def test_runspace_dense_and_fused(name, path):
    """The ladder and the combined corpus without gaps: the dense records, the parsed entry point and the
    fused parse + update (rec_part and update entries)."""
    _run(name, path)


@pytest.mark.parametrize("name", ["blocks", "rounds"])
def test_runspace_device_store(name):
    """The split over chunk blocks and the second chunk round once more through fb_hist_store_append_dev: the
    strings gathered from the device store equal the oracle's."""
    _run(name, "placed", on_device=True)


def test_runspace_timed_ladder():
    """A timed context: the plain K2, no group is combined (the census with hot=False)."""
    _, seen = _run("ladder", "placed", timed=True)
    assert seen >= DENSE_CLASSES["ladder"] and "combined" not in seen


def test_runspace_overfull():
    """600 flows for one partition of 512 slots, one call: error bit 4, 512 flows in the table, and the history
    holds exactly the characters of the flows that got a slot -- a key is taken with all of its batch's entries
    or with none, so every exported flow's string is the oracle's and no character is filed under a slot
    another flow holds (combined_slot / emit's dst < out_end)."""
    (call, recs, _, _), = _reference("overfull")[0]
    flows = _reference("overfull")[1]
    cap = _capture(1)
    try:
        st, keep = _placed(cap, call)
        assert st["error"] & 4, st
        slots = _raw_history(cap, call.n_slots, "overfull")
        gf = cap.export_flows()
        assert len(gf) == rs.SLOTS and sorted(gf["slot"].tolist()) == list(range(rs.SLOTS))
        assert len(slots) == int(gf["hist_len"].sum()), (len(slots), int(gf["hist_len"].sum()))
        assert set(np.unique(slots).tolist()) <= set(gf["slot"].tolist())
        want = {bytes(r.tobytes()[:40]): r for r in flows.export_sorted()}
        for r in gf:
            o = want[bytes(r.tobytes()[:40])]
            h, _ = flows.history(o)
            g = cap.histories.get(int(r["slot"]), "")
            assert g == h, ("overfull", r, g, h)
            z = r.copy()
            z["slot"] = 0
            assert z.tobytes() == o.tobytes(), ("overfull", z, o)
        del keep
    finally:
        cap.close()
