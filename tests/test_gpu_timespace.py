"""The capture-time pass (flodbadd_amd/csrc/fb_time.hip: the pair sort and k_time_runs) on every path
of its code, against the oracle, byte for byte: the enumerated gap / PSH corpora of tests/timespace.py
(pinned by tests/test_timespace_oracle.py) under every placement of the update-call boundaries, so a
run's position 0, 1 and 2+ each read the plane of an earlier call and the sorted neighbours of this
one in every combination; through a table that grows between a flow's packets; with runs placed on
thread, wave and tile boundaries (asserted on the host from the exported slots, never assumed); and
with one flow's run over more tiles than a look-back window holds.

  path      entry point
  dense     fb_process_dev
  seg       fb_process_seg_dev
  table     fb_process_seg_async_dev, session records off (the update reads update entries)
  parsed    fb_process_parsed

After EVERY update call: every fb_flow_time record and the timed segment state (test_gpu_timed._check),
every fb_flow_rec field but slot, new_sessions / updated_sessions and error == 0.  No tolerances."""
import functools
import time

import numpy as np
import pytest

import flagseq
import timespace as tsp
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.distributed import sort_by_ord
from flodbadd_amd.sessions import SessionFilter
from oracle import coracle
from test_gpu_flagspace import _table_only
from test_gpu_timed import _check

pytestmark = pytest.mark.gpu

CORPORA = {"quads": tsp.quads, "udp_triples": tsp.udp_triples, "ends": tsp.ends, "shims": tsp.shims}


def _capacity(n_flows):
    """The smallest power of two that keeps the table at most half full."""
    return max(1 << 12, 1 << int(2 * n_flows - 1).bit_length())


def _prepare(batches):
    """Batches -> per call (frames, offsets, ts, the oracle's records), read-only."""
    cfg, out = coracle.make_cfg(2), []
    for b in batches:
        fr, of = tsp.frames(b)
        recs, dns, _, _ = coracle.parse_classify(cfg, fr, of)
        assert len(recs) == len(of) - 1 and len(dns) == 0
        ts = np.ascontiguousarray(b.t)
        for a in (fr, of, ts, recs):
            a.setflags(write=False)
        out.append((fr, of, ts, recs))
    return out


@functools.lru_cache(maxsize=2)
def _calls(names, cutmask, replicas=1):
    """The corpora `names` (a tuple; several: together in every call) under a cut mask, prepared once."""
    layouts = [tsp.layout(CORPORA[n](), cutmask, replicas if n == "quads" else 1) for n in names]
    return _prepare([tsp.concat(*[lay[k] for lay in layouts if k < len(lay)]) for k in range(max(map(len, layouts)))])


def _apply(cap, path, fr, of, ts, recs, tag):
    if path == "table":
        return _table_only(cap, fr, of, ts)
    if path == "dense":
        g = cap.process_frames(fr, of, ts=ts)
    elif path == "seg":
        g = cap.process_frames_seg(fr, of, ts=ts)
    else:
        g = cap.process_parsed(flagseq.parsed_of(recs), ts=ts)
    assert g.records.tobytes() == recs.tobytes(), tag
    return g.stats


def _check_rows(cap, ref, tag):
    """Every fb_flow_rec field but slot; returns the GPU's records in the oracle's order."""
    gs, rf = sort_by_ord(cap.export_flows()), ref.export_sorted()
    assert len(gs) == len(rf), (tag, len(gs), len(rf))
    gz = gs.copy()
    gz["slot"] = 0
    w = N.FLOW_REC_DTYPE.itemsize
    bad = np.flatnonzero((gz.view(np.uint8).reshape(-1, w) != np.ascontiguousarray(rf).view(np.uint8).reshape(-1, w)).any(axis=1))
    assert bad.size == 0, (tag, bad.size, gz[bad[:2]], rf[bad[:2]])
    return gs, rf


def _run(calls, path, capacity, tag, after=None):
    """The prepared calls through one path; after every call the whole comparison, then after(k, cap,
    ref, gpu records, oracle records): the test's own conditions.  Returns the wall time of each
    update call."""
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, timed=True, flow_capacity=capacity)
    ref, wall = coracle.Flows(), []
    try:
        if path == "table":
            N.check(N.gpu_lib().fb_set_session_records(cap.ctx, 0))
        for k, (fr, of, ts, recs) in enumerate(calls):
            r_st = np.zeros(1, dtype=N.STATS_DTYPE)
            ref.update(recs, r_st, ts=ts)
            t0 = time.perf_counter()
            st = _apply(cap, path, fr, of, ts, recs, (tag, k))
            wall.append(time.perf_counter() - t0)
            assert st["error"] == 0, (tag, k, st)
            assert (st["new_sessions"], st["updated_sessions"]) == \
                (int(r_st[0]["new_sessions"]), int(r_st[0]["updated_sessions"])), (tag, k, st)
            assert st["n_session"] == len(recs)
            _check(cap, ref, "%s call %d" % (tag, k))
            gs, rf = _check_rows(cap, ref, "%s call %d" % (tag, k))
            if after:
                after(k, cap, ref, gs, rf)
        return wall
    finally:
        cap.close()


PATHS = ["dense", "seg", "table", "parsed"]
QUADS_CASES = [(("quads",), path, m) for m in range(8) for path in PATHS] + [(("udp_triples", "quads"), "seg", 0b101)]


@pytest.mark.parametrize("names,path,cutmask", QUADS_CASES,
                         ids=["%s-%s-%d" % ("+".join(n), p, m) for n, p, m in QUADS_CASES])
def test_timespace_quads(names, path, cutmask):
    """Every four-packet flow over PSH x the eight gaps (8,192 flows, 32,768 frames) under each of
    the 8 placements of the call boundaries; the last case adds the 512 UDP gap triples to the same
    context (no PSH: the timeout is the only end)."""
    calls = _calls(names, cutmask)
    flows = 8192 + (512 if len(names) > 1 else 0)
    assert sum(len(c[1]) - 1 for c in calls) == 4 * flows and len(calls) == 1 + bin(cutmask).count("1")
    _run(calls, path, _capacity(flows), "%s/%s/%d" % ("+".join(names), path, cutmask))


ENDS_CASES = [(path, m) for m in (0, 0b001, 0b010, 0b100, 0b111) for path in ("seg", "table")]


@pytest.mark.parametrize("path,cutmask", ENDS_CASES, ids=["%s-%d" % c for c in ENDS_CASES])
def test_timespace_ends(path, cutmask):
    """16,875 flows over ACK, PSH|ACK, FIN|ACK, RST, FIN|PSH|ACK x {1 ms, 5 s, -1 s}: end_time_ns is the
    time of the first FIN / RST in packet order (a later one may carry an earlier time) and is
    written once, whichever call holds it."""
    _run(_calls(("ends",), cutmask), path, _capacity(16875), "ends/%s/%d" % (path, cutmask))


GROWTH_GROUPS = [1024, 1024, 2048, 4096, 8192, 16384]


@pytest.mark.parametrize("path", ["dense", "seg"])
def test_timespace_growth(path):
    """quads x 4 replicas (32,768 flows), every packet of a flow in an update call of its own, into a
    table that starts at 4,096 slots.  The table grows before an update call from the occupancy the
    call before reported, so the flows arrive in groups that double (timespace.stagger: group g's
    position p is in call g + p; cut mask 0b111 as it stands would insert all 32,768 flows in the first
    call, which no 4,096-slot table takes).  Asserted: the generation advances between EVERY pair of
    consecutive packets of the flows of groups 1-3 (7,168 flows: the plane follows them to new slots
    three times), and at least five times in all."""
    staged = tsp.stagger(tsp.replicate(tsp.quads(), 4), GROWTH_GROUPS)
    calls = _prepare([b for b, _ in staged])
    assert len(calls) == len(GROWTH_GROUPS) + 3
    at = []  # the generation each call ran at (a call grows the table before its update)
    _run(calls, path, 1 << 12, "growth/" + path, after=lambda k, cap, *_: at.append(cap.table_info()["generation"]))
    print("growth %s: generation per call %s" % (path, at))
    assert at[-1] >= 5, at
    for g in (1, 2, 3):
        assert at[g] < at[g + 1] < at[g + 2] < at[g + 3], (g, at)


def _placement(gs, rf):
    """Each flow's sorted span in the call that made the table `gs` (GPU records, with slots) out of
    nothing: the oracle's packet counts `rf` of the flows with smaller slots."""
    return tsp.run_spans(gs["slot"], (rf["orig_pkts"] + rf["resp_pkts"]).astype(np.int64))


@pytest.mark.parametrize("path", ["dense", "table"])
def test_timespace_insert_runs_on_tile_edges(path):
    """quads x 8 replicas in one call: 65,536 inserted flows of 4 packets, 262,144 frames, 128 tiles --
    and, in the same call, timespace.shims: 4,096 flows of 1-3 packets.  Without them every run would
    be 4 packets long and start at a multiple of 4, a thread's first item, and none could straddle a
    tile boundary; with them a run's offset in its thread is as good as uniform.  Asserted from the
    exported slots: for each d in 1..3 at least 8 runs straddle a tile boundary d items in, at least 8
    start on a tile's first item and at least 8 end on a tile's last.
    Observed on an MI355X, both paths (their slots differ, these counts did not): 46, 36 and 27 runs
    straddling at d = 1, 2, 3; 24 starting on a tile's first item, 23 ending on its last; run starts per
    offset in the thread 18,806 / 17,209 / 17,415 / 16,202."""
    calls = _calls(("quads", "shims"), 0, 8)
    seen = {}

    def placed(k, cap, ref, gs, rf):
        assert cap.table_info()["generation"] == 0  # no growth: the exported slots are the call's
        start, end = _placement(gs, rf)
        assert int(end.max()) == len(calls[0][1]) - 1 > 128 * tsp.TILE
        off = start % tsp.TILE
        for d in (1, 2, 3):
            seen[d] = int(((off == tsp.TILE - d) & (end - start > d)).sum())
        seen["first"], seen["last"] = int((off == 0).sum()), int((end % tsp.TILE == 0).sum())
        seen["thread"] = np.bincount(start % tsp.THREAD_ITEMS, minlength=4).tolist()

    _run(calls, path, 1 << 18, "edges/" + path, after=placed)
    print("placement %s: %s" % (path, seen))
    assert min(seen[k] for k in (1, 2, 3, "first", "last")) >= 8, seen


@pytest.mark.parametrize("path", ["dense", "seg"])
def test_timespace_ladder(path):
    """131,072 flows insert one packet each; from the slots the table gave them, timespace.ladder_plan
    makes the second call (~133,000 frames) put a run of 5 packets on every multiple of 256 of the
    sorted order, its head 0..5 items before the boundary in turn (observed on an MI355X: 85-87 runs
    per offset on wave boundaries, 10-11 of each on tile boundaries; asserted: >= 80 and >= 8).  Asserted before the second call: the table has
    not grown and every planned run starts where the plan says."""
    F = 1 << 17
    lad = tsp.Ladder(F)
    (call1,) = _prepare([lad.call1()])
    plan = {}

    def calls():
        yield call1
        yield plan["call2"]

    def after(k, cap, ref, gs, rf):
        assert cap.table_info()["generation"] == 0
        if k:
            return
        slots = np.zeros(F, dtype=np.int64)
        slots[tsp.flow_of_recs(gs)] = gs["slot"]
        counts, probes = tsp.ladder_plan(slots, L=5)
        start, end = tsp.run_spans(slots, counts)
        per_d = np.zeros((6, 2), dtype=np.int64)
        for f, B, d in probes:
            assert B % tsp.WAVE_ITEMS == 0 and start[f] == B - d and end[f] == B - d + 5, (f, B, d)
            per_d[d] += (1, B % tsp.TILE == 0)
        print("ladder %s: probes per offset (on wave boundaries, of them tile boundaries) %s" % (path, per_d.tolist()))
        assert len(probes) >= 500 and per_d[:, 0].min() >= 80 and per_d[:, 1].min() >= 8, per_d
        (plan["call2"],) = _prepare([lad.call2(counts)])
        assert 132_000 < len(plan["call2"][1]) - 1 < 134_000

    _run(calls(), path, 1 << 19, "ladder/" + path, after=after)


@pytest.mark.parametrize("path", ["dense", "table"])
@pytest.mark.parametrize("tiles", [(72,), (36, 72)], ids=["one", "two"])
def test_timespace_long_runs(tiles, path):
    """One TCP flow of 72 x 2,048 packets in each of two calls (and, `two`: a second of 36 x 2,048, so
    that one of the long runs begins behind the other), among 2,000 short flows.  Asserted on the host,
    from the exported slots: in each call one run covers more than 65 tiles, which is what lets a tile's
    look-back leave its first window of 64 tiles without a run head or an inclusive value and fold a
    second one (`acc = have ? op(v, acc) : v`).  Whether a tile does take the second window depends on
    when its predecessors publish: this makes it reachable -- nothing else in the suite does -- and
    cannot assert it was taken.  A timed context does not combine a flow's records before the apply, so
    the update applies the hot flow's 147,456 entries one after the other.
    Wall time of an update call on an MI355X (upload, parse, update, the time pass, download): 6-7 ms the
    first call, 3-5 ms the second, on both paths and both variants -- far from the ~2 s at which the
    run would be cut to 66 tiles.  With the fold's operands swapped in a scratch build, all four cases
    failed on the hot flow's record alone: on that run the second window was taken."""
    batches = tsp.hot(tiles)
    calls = _prepare(batches)

    def covered(k, cap, ref, gs, rf):
        cnt = np.bincount(batches[k].flow, minlength=3000)[tsp.flow_of_recs(gs)]
        start, end = tsp.run_spans(gs["slot"], cnt)
        span = (end - 1) // tsp.TILE - start // tsp.TILE + 1
        assert int(span.max()) > tsp.WINDOW + 1, span.max()
        assert int((cnt >= 36 * tsp.TILE).sum()) == len(tiles)

    wall = _run(calls, path, 1 << 13, "long/%s/%s" % (len(tiles), path), after=covered)
    print("long runs %s %s: %s s per call" % (tiles, path, ["%.3f" % w for w in wall]))
