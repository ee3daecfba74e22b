"""Cross-rank ordered state on the device, against the oracle, byte for byte: the placement corpora of
tests/rankspace.py (every flag sequence placed on W ranks x K global batches in every way) through
the two ways the multi-GPU table is built, with W contexts in one process standing for the ranks.

  merged   every rank updates its own table from its shards (dense and segmented fused calls
           alternating, or the table-only pipelined call), exports it per owner
           (fb_flow_export_merge_map_dev, or fb_flow_export_merge_dev for equal shards) and each owner
           merges what it receives (fb_flow_merge_dev).  Checked: every exported group equals the
           oracle's (char_call included), every owner's merge equals the oracle's merge of the same
           records in first-record order, the union equals ONE oracle table fed the global stream.
           Also after the table grew and after a purge re-packed it (char_call has to follow its slot),
           with k_flow_combine's partial reductions (hot flows), at 1 / 2 / 63 / 64 owners and at the
           merge's block and scan boundaries.
  routed   every rank parses its shard (fb_parse_classify_dev), routes the records to their owners
           (fb_route_records_dev) and each owner applies what it received in one update call per
           global batch (fb_flow_update_records_dev): the owners' tables, positions and capture-time
           records included, equal the single table's.

tests/test_rankspace_oracle.py pins the reference on the same corpora.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import flagseq as fs
import rankspace as rs
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.sessions import SessionFilter
from oracle import coracle
from test_gpu_c5 import _export, _merge_dev
from test_gpu_flagspace import _capacity, _combine_runs, _table_only
from test_gpu_timed import _check as _check_times

pytestmark = pytest.mark.gpu

PAIR_IDS = {fs.ONE_SVC: "one_svc", fs.TWO_SVC: "two_svc", fs.NO_SVC: "no_svc"}
MREC = N.FLOW_MREC_DTYPE.itemsize
S = 10 ** 9


def _contexts(capacities, **kw):
    return [FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=c, **kw) for c in capacities]


def _close(caps):
    for c in caps:
        c.close()


def _update(cap, call, path, tag):
    """One rank's update call for its shard; path: dense / seg / table."""
    fr, of, _, ts, recs, r_st = call
    if path == "table":
        st = _table_only(cap, fr, of, ts)
    else:
        g = cap.process_frames_seg(fr, of, ts=ts) if path == "seg" else cap.process_frames(fr, of, ts=ts)
        assert g.records.tobytes() == recs.tobytes(), tag
        st = g.stats
    assert st["error"] == 0 and st["n_session"] == len(recs), (tag, st)
    assert (st["new_sessions"], st["updated_sessions"]) == \
        (int(r_st[0]["new_sessions"]), int(r_st[0]["updated_sessions"])), (tag, st)


def _run_ranks(caps, ref, paths=("dense", "seg"), batches=None, after_batch=None, made=None):
    """Every rank's update calls for the global batches `batches` (default: all), call j of a rank
    through paths[j % len(paths)]; a rank makes no call for an empty shard.  Returns the calls made
    per rank (`made`: those of an earlier run)."""
    made = list(made) if made else [0] * ref.world
    for k in (range(len(ref.calls)) if batches is None else batches):
        for r, cap in enumerate(caps):
            call = ref.calls[k][r]
            if call is None:
                continue
            _update(cap, call, paths[made[r] % len(paths)], (k, r))
            made[r] += 1
        if after_batch:
            after_batch(k)
    return made


def _export_map(cap, world, rank, cmap):
    lib = N.gpu_lib()
    n = cap.flow_count()
    cm = np.ascontiguousarray(np.asarray(cmap, dtype=np.uint64).reshape(-1))
    d_out, d_cnt = N.DeviceBuffer(max(n, 1) * MREC), N.DeviceBuffer(8 * world)
    N.check(lib.fb_flow_export_merge_map_dev(cap.ctx, world, rank, N.ptr(cm) if cm.size else None, int(cm.size),
                                             d_out.ptr, n, d_cnt.ptr, None))
    counts = d_cnt.download(np.zeros(world, dtype=np.uint64))
    m = d_out.download(np.zeros(max(n, 1), dtype=N.FLOW_MREC_DTYPE))[: int(counts.sum())]
    d_out.free()
    d_cnt.free()
    assert int(counts.sum()) == n
    return m, counts


def _export_rank(cap, ref, rank, world=None):
    world = world or ref.world
    if ref.call_maps is not None:
        return _export_map(cap, world, rank, ref.call_maps[rank])
    return _export(cap, world, rank, ref.shard_firsts[rank])


def _same_records(got, exp, tag):
    """Two record arrays byte for byte; the diagnostics name the first differing record."""
    assert len(got) == len(exp), (tag, len(got), len(exp))
    if got.tobytes() == exp.tobytes():
        return
    w = got.dtype.itemsize
    bad = np.flatnonzero((np.ascontiguousarray(got).view(np.uint8).reshape(-1, w) !=
                          np.ascontiguousarray(exp).view(np.uint8).reshape(-1, w)).any(axis=1))
    i = int(bad[0])
    raise AssertionError("%s: %d of %d records differ; first: device %s, oracle %s" %
                         (tag, bad.size, len(exp), got[i], exp[i]))


def _check_export(got, exp, rank, tag):
    """A device export against the oracle's: the group sizes, and every group's records sorted by
    key (the device's groups are in slot order, the oracle's in Ord); char_call is part of a record."""
    (m, counts), (em, ecounts) = got, exp
    assert np.array_equal(counts, ecounts), (tag, rank, counts, ecounts)
    assert (m["rec"]["slot"] == rank).all(), (tag, rank)
    for o, (a, b) in enumerate(zip(rs.groups_of(m, counts), rs.groups_of(em, ecounts))):
        _same_records(rs.by_key(a), rs.by_key(b), "%s: rank %d's group for owner %d" % (tag, rank, o))


def _check_merge(cap, recv, tag):
    """The device merge of one owner's received records against the oracle's merge of the same
    records, order included, and that order is the order of each key's first record."""
    got = _merge_dev(cap, recv)
    _same_records(got, coracle.flow_merge(recv), tag)
    if len(got):
        keys, first = np.unique(rs.key_ids(recv), return_index=True)
        at = first[np.searchsorted(keys, rs.key_ids(got))]
        assert (np.diff(at) > 0).all(), tag
    return got


def _check_all(caps, ref, tag, exports_expected=None, single_expected=None):
    """The three comparisons of a merged table: exports, merges, union."""
    exports = []
    for r, cap in enumerate(caps):
        e = _export_rank(cap, ref, r)
        _check_export(e, exports_expected[r] if exports_expected else ref.export(r), r, tag)
        exports.append(e)
    merged = [_check_merge(caps[o], rs.received(exports, o), "%s: owner %d's merge" % (tag, o))
              for o in range(ref.world)]
    single = ref.single.export_sorted() if single_expected is None else single_expected
    _same_records(rs.rows(np.concatenate(merged)), rs.rows(single), tag + ": union")
    return exports, merged


def _capacities(ref):
    return [_capacity(f.count()) for f in ref.ranks]


FIXED_CASES = [("triples", fs.ONE_SVC), ("triples", fs.TWO_SVC), ("pairs", fs.ONE_SVC), ("pairs", fs.TWO_SVC),
               ("pairs", fs.NO_SVC)]


@pytest.mark.parametrize("corpus,pair", FIXED_CASES, ids=["%s-%s" % (c, PAIR_IDS[p]) for c, p in FIXED_CASES])
def test_merge_fixed_table(corpus, pair):
    """Every placement of every sequence, tables that never move a slot."""
    ref = rs.reference(corpus, pair)
    caps = _contexts(_capacities(ref), grow=False)
    try:
        _run_ranks(caps, ref)
        assert all(c.table_info()["generation"] == 0 for c in caps)
        _check_all(caps, ref, "%s/%s" % (corpus, PAIR_IDS[pair]))
    finally:
        _close(caps)


def test_merge_single_owner_scan_two_blocks_per_thread():
    """One owner merges every record of all three ranks of triples / TWO_SVC (each rank's whole
    export, rank order): more than 1,024 x 256 records, so k_mg_scan's threads take two block counts
    each.  (The export itself refuses rank >= world, so the ranks export for three owners and the
    groups are concatenated.)"""
    ref = rs.reference("triples", fs.TWO_SVC)
    caps = _contexts(_capacities(ref))
    try:
        _run_ranks(caps, ref)
        recv = np.concatenate([_export_rank(cap, ref, r)[0] for r, cap in enumerate(caps)])
        assert len(recv) > 1024 * 256
        got = _check_merge(caps[0], recv, "single owner")
        _same_records(rs.rows(got), rs.rows(ref.single.export_sorted()), "single owner: union")
    finally:
        _close(caps)


def test_merge_rank_skips_a_call():
    """The triples that put no packet on rank 1 in global batch 0: it makes no call for that batch,
    so its call 0 is global batch 1 and k_mx_write has to take positions and char_call through the
    call map."""
    ref = rs.reference("triples", fs.ONE_SVC, "skip")
    assert ref.calls[0][1] is None
    caps = _contexts(_capacities(ref), grow=False)
    try:
        assert _run_ranks(caps, ref) == [2, 1, 2]
        _check_all(caps, ref, "triples/one_svc/skip")
    finally:
        _close(caps)


def test_merge_table_only_path():
    """The session records off: the update reads the parse's update entries (fb_process_seg_async_dev)."""
    ref = rs.reference("triples", fs.ONE_SVC)
    caps = _contexts(_capacities(ref), grow=False)
    try:
        for c in caps:
            N.check(N.gpu_lib().fb_set_session_records(c.ctx, 0))
        _run_ranks(caps, ref, paths=("table",))
        _check_all(caps, ref, "triples/one_svc/table")
    finally:
        _close(caps)


@pytest.mark.parametrize("path", ["dense", "seg"])
def test_merge_hot(path):
    """The hot flows cut into two contiguous shards (the export's shard_first form): a rank's hot
    groups pass k_flow_combine's threshold, so char_call comes out of its partial reductions."""
    ref = rs.reference("hot", fs.ONE_SVC)
    caps = _contexts([1 << 14] * ref.world)
    try:
        for r, cap in enumerate(caps):
            _combine_runs(cap, [(None, None, None, ref.calls[0][r][4])])
        _run_ranks(caps, ref, paths=(path,))
        exports, merged = _check_all(caps, ref, "hot/" + path)
        merged = np.concatenate(merged)
        assert len(merged) == 48 and sorted(merged["hist_len"].tolist()) == sorted(fs.HOT_LENGTHS)
        both = np.concatenate([m for m, _ in exports])
        assert len(both) == 96 and (both["char_call"] != N.FB_CALL_NONE).any()
    finally:
        _close(caps)


def test_char_call_follows_growth():
    """Tables that start at 2^12 slots (rankspace.growth_rows): they grow on the way to the corpus,
    and again during the filler batches after it -- after K2 wrote every corpus flow's char_call and
    before the export reads it."""
    ref = rs.reference("triples", fs.ONE_SVC, "growth")
    caps = _contexts([1 << 12] * ref.world)
    first_corpus, last_corpus = len(rs.RAMP), len(rs.RAMP) + 1
    gens = {}
    try:
        _run_ranks(caps, ref, after_batch=lambda k: gens.__setitem__(k, [c.table_info()["generation"] for c in caps]))
        last = len(ref.calls) - 1
        print("generations: first corpus call %s, before the filler %s, after it %s; capacities %s" %
              (gens[first_corpus], gens[last_corpus], gens[last], [c.table_info()["capacity"] for c in caps]))
        for r in range(ref.world):
            assert gens[first_corpus][r] > 0                              # (it grew on the way up)
            assert gens[last][r] > gens[last_corpus][r] >= gens[first_corpus][r]  # the filler raised it
        corpus_recs = np.concatenate([m for m, _ in ref.exports()])
        assert (corpus_recs["char_call"] != N.FB_CALL_NONE).any()
        _check_all(caps, ref, "triples/one_svc/growth")
    finally:
        _close(caps)


def test_char_call_follows_purge():
    """Timed contexts: after global batch 0 every rank purges the flows it last saw two days ago
    (k_flow_age re-packs their partitions and carries char_call by hand), then global batch 1, the
    export and the merge.  Expected: the oracle's records without the purged keys."""
    ref = rs.reference("triples", fs.ONE_SVC, "purge")
    now = rs.T0 + 2 * rs.DAY_NS + 100 * S
    caps = _contexts(_capacities(ref), timed=True)
    try:
        made = _run_ranks(caps, ref, batches=[0])
        stale, moved = [], []
        for r, cap in enumerate(caps):
            recs, times, em = ref.after_first[r]
            gone = rs.key_ids(recs[now > times["last_activity_ns"].astype(np.int64) + rs.DAY_NS])
            before = cap.export_flows()
            st = cap.update_sessions_status(now, purge=True)
            after = cap.export_flows()
            assert st["purged"] == len(gone) > 0 and st["remaining"] == len(recs) - len(gone) == len(after), (r, st)
            # survivors that hold a char_call by now (the oracle's export after batch 0) and changed slot
            holds = rs.key_ids(em[(em["char_call"] != N.FB_CALL_NONE).any(axis=1)])
            b = before[np.argsort(rs.key_ids(before))]
            a = after[np.argsort(rs.key_ids(after))]
            kb = rs.key_ids(b)
            keep = ~np.isin(kb, gone)
            assert (kb[keep] == rs.key_ids(a)).all()
            moved.append(int(((b["slot"][keep] != a["slot"]) & np.isin(kb[keep], holds)).sum()))
            stale.append(gone)
        print("purged %s, survivors with a char_call that changed slot %s" % ([len(g) for g in stale], moved))
        assert all(m > 0 for m in moved)
        _run_ranks(caps, ref, batches=[1], made=made)
        expected = []
        for r in range(ref.world):
            m, counts = ref.export(r)
            kept = [g[~np.isin(rs.key_ids(g), stale[r])] for g in rs.groups_of(m, counts)]
            expected.append((np.concatenate(kept), np.array([len(g) for g in kept], dtype=np.uint64)))
        single = ref.single.export_sorted()
        t = ref.single.export_times()
        single = single[~(now > t["last_activity_ns"].astype(np.int64) + rs.DAY_NS)]
        assert len(single) == len(np.unique(np.concatenate([rs.key_ids(m) for m, _ in expected])))
        _check_all(caps, ref, "triples/one_svc/purge", exports_expected=expected, single_expected=single)
    finally:
        _close(caps)


# ---- export and merge shape edges --------------------------------------------------------------

def _small():
    """586 flows of the pairs corpus on two ranks."""
    shards, cmaps = rs.placed("pairs", flows=np.arange(0, 4096, 7))
    return rs.Reference(shards, fs.ONE_SVC, call_maps=cmaps)


def test_export_owner_counts_and_refusals():
    """1, 2, 63 and 64 owners (one wavefront lane each) on tables of 2^10 slots, less than one
    4,096-slot export chunk; 0 and 65 owners, and a rank outside the world, are refused before
    anything is written."""
    ref = _small()
    lib = N.gpu_lib()
    caps = _contexts([1 << 10] * ref.world, grow=False)
    try:
        _run_ranks(caps, ref)
        assert all(c.table_info()["capacity"] == 1 << 10 for c in caps)
        for world in (1, 2, 63, 64):
            owners = set()
            for r, cap in enumerate(caps[:world]):
                got = _export_rank(cap, ref, r, world)
                _check_export(got, ref.export(r, world), r, "world %d" % world)
                owners |= set(np.flatnonzero(got[1]).tolist())
            assert world < 63 or len(owners) > 32  # (the high lanes do serve owners)
        n = caps[0].flow_count()
        cm = np.asarray(ref.call_maps[0], dtype=np.uint64)
        for world, rank in ((0, 0), (65, 0), (65, 64), (1, 1), (64, 64)):
            d_out, d_cnt = N.DeviceBuffer(n * MREC), N.DeviceBuffer(8 * 65)
            d_out.memset(0xA5)
            d_cnt.memset(0xA5)
            N.check(lib.fb_stream_sync(None))
            assert lib.fb_flow_export_merge_dev(caps[0].ctx, world, rank, 0, d_out.ptr, n, d_cnt.ptr,
                                                None) == N.FB_ERR_INVAL
            assert lib.fb_flow_export_merge_map_dev(caps[0].ctx, world, rank, N.ptr(cm), len(cm), d_out.ptr, n,
                                                    d_cnt.ptr, None) == N.FB_ERR_INVAL
            N.check(lib.fb_stream_sync(None))
            assert (d_out.download(np.zeros(n * MREC, dtype=np.uint8)) == 0xA5).all()
            assert (d_cnt.download(np.zeros(8 * 65, dtype=np.uint8)) == 0xA5).all()
            d_out.free()
            d_cnt.free()
    finally:
        _close(caps)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_merge_record_counts(n):
    """The merge's block boundary (256 records a block)."""
    ref = _small()
    e0, e1 = ref.export(0, 1)[0], ref.export(1, 1)[0]  # (both in Ord: the two halves share most keys)
    recv = np.concatenate([e0[: (n + 1) // 2], e1[: n // 2]])
    assert len(recv) == n and (n < 255 or len(np.unique(rs.key_ids(recv))) < n)
    cap = _contexts([1 << 10])[0]
    try:
        got = _check_merge(cap, recv, "n = %d" % n)
        assert len(got) == len(np.unique(rs.key_ids(recv)))
    finally:
        cap.close()


def test_merge_sixty_four_copies_of_one_key():
    """One flow of 128 packets, one per (global batch, rank) cell of 64 ranks x 2 batches, its first
    FIN in the second batch on rank 6 and a RST after it: 64 records of one key."""
    world = 64
    sym = np.random.default_rng(11).choice(np.flatnonzero((np.arange(128) & (fs.FIN | fs.RST)) == 0), size=2 * world)
    sym = sym.astype(np.uint8)
    sym[world + 6] = fs.FIN | fs.ACK
    sym[world + 40] = fs.REV | fs.RST | fs.ACK
    one = lambda i: (sym[i: i + 1], np.zeros(1, dtype=np.uint32), np.array([i], dtype=np.uint32))  # noqa: E731
    shards = [[one(k * world + r) for r in range(world)] for k in range(2)]
    ref = rs.Reference(shards, fs.ONE_SVC, call_maps=rs.call_maps_of(shards))
    recv = np.concatenate([ref.export(r, 1)[0] for r in range(world)])
    assert len(recv) == world and len(np.unique(rs.key_ids(recv))) == 1
    cap = _contexts([1 << 10])[0]
    try:
        got = _check_merge(cap, recv, "64 copies")
        single = ref.single.export_sorted()
        _same_records(rs.rows(got), rs.rows(single), "64 copies: the single table")
        assert int(single[0]["hist_len"]) == 2 * world and int(single[0]["end_seen"]) == (1 << 32) | 6
    finally:
        cap.close()


def test_merge_4096_distinct_keys():
    shards, cmaps = rs.placed("pairs", flows=np.arange(4096))
    ref = rs.Reference(shards, fs.ONE_SVC, call_maps=cmaps)
    recv = np.concatenate([ref.export(r, 1)[0] for r in range(ref.world)])
    assert len(np.unique(rs.key_ids(recv))) == 4096 < len(recv)
    cap = _contexts([1 << 10])[0]
    try:
        got = _check_merge(cap, recv, "4,096 keys")
        _same_records(rs.rows(got), rs.rows(ref.single.export_sorted()), "4,096 keys: the single table")
    finally:
        cap.close()


# ---- routed, in process ------------------------------------------------------------------------

def _owners(recs, world):
    """fb_flow_owner of every record's key (the library's host function, once per distinct key)."""
    lib = N.gpu_lib()
    keys, inv = np.unique(rs.key_ids(recs), return_inverse=True)
    kb = np.ascontiguousarray(keys.view(np.uint8).reshape(len(keys), 40))
    base = kb.ctypes.data
    own = np.array([lib.fb_flow_owner(C.c_void_p(base + 40 * i), world) for i in range(len(keys))], dtype=np.uint32)
    return own[inv.ravel()]


class _OwnerRows:
    """The single oracle table restricted to one owner's keys, as test_gpu_timed._check reads it."""

    def __init__(self, recs, times):
        self.recs, self.times = recs, times

    def export_sorted(self):
        return self.recs

    def export_times(self):
        return self.times


def _route(cap, call, world, timed):
    """fb_parse_classify_dev + fb_route_records_dev for one shard -> (groups, their capture times)."""
    lib = N.gpu_lib()
    fr, of, start, ts, recs, _ = call
    n = len(of) - 1
    bufs = dict(fr=N.DeviceBuffer(fr.nbytes).upload(fr), of=N.DeviceBuffer(of.nbytes).upload(of),
                recs=N.DeviceBuffer(n * 56), grouped=N.DeviceBuffer(n * 56), st=N.DeviceBuffer(N.STATS_DTYPE.itemsize),
                cnt=N.DeviceBuffer(8 * world))
    if timed:
        bufs["ts"], bufs["ts_out"] = N.DeviceBuffer(8 * n).upload(ts), N.DeviceBuffer(8 * n)
    try:
        N.check(lib.fb_parse_classify_dev(cap.ctx, bufs["fr"].ptr, fr.nbytes, bufs["of"].ptr, n, bufs["recs"].ptr, None,
                                          None, bufs["st"].ptr, None))
        N.check(lib.fb_route_records_dev(cap.ctx, bufs["recs"].ptr, bufs["st"].ptr, n, world, start,
                                         bufs["ts"].ptr if timed else None, bufs["grouped"].ptr,
                                         bufs["ts_out"].ptr if timed else None, bufs["cnt"].ptr, None))
        N.check(lib.fb_stream_sync(None))
        st = bufs["st"].download(np.zeros(1, dtype=N.STATS_DTYPE))
        assert int(st[0]["error"]) == 0 and int(st[0]["n_session"]) == n
        counts = bufs["cnt"].download(np.zeros(world, dtype=np.uint64))
        assert int(counts.sum()) == n
        grouped = bufs["grouped"].download(np.zeros(n, dtype=N.PKT_OUT_DTYPE))
        t_out = bufs["ts_out"].download(np.zeros(n, dtype=np.uint64)) if timed else None
    finally:
        for b in bufs.values():
            b.free()
    # the restatement: a stable partition of the shard's records by owner, pkt_index + shard start
    own = _owners(recs, world)
    order = np.argsort(own, kind="stable")
    exp = recs[order].copy()
    exp["pkt_index"] += np.uint32(start)
    assert np.array_equal(counts, np.bincount(own, minlength=world).astype(np.uint64)), (counts, start)
    _same_records(grouped, exp, "routed groups of the shard at %d" % start)
    if timed:
        assert np.array_equal(t_out, ts[recs["pkt_index"][order]])
    return rs.groups_of(grouped, counts), (rs.groups_of(t_out, counts) if timed else None)


def _apply(cap, recs, ts, global_n):
    """One owner's update call over the records it received (fb_flow_update_records_dev); ts: their
    capture times, scattered into a global-batch array by pkt_index."""
    lib = N.gpu_lib()
    k = len(recs)
    st = np.zeros(1, dtype=N.STATS_DTYPE)
    st[0]["n_session"] = k
    d_st = N.DeviceBuffer(st.nbytes).upload(st)
    d_recs = N.DeviceBuffer(max(k, 1) * 56)
    if k:
        d_recs.upload(recs)
    d_ts = None
    if ts is not None:
        g = np.zeros(max(global_n, 1), dtype=np.uint64)
        g[recs["pkt_index"]] = ts
        d_ts = N.DeviceBuffer(g.nbytes).upload(g)
        N.check(lib.fb_set_frame_times(cap.ctx, d_ts.ptr))
    N.check(lib.fb_flow_update_records_dev(cap.ctx, d_recs.ptr if k else None, k, d_st.ptr, None))
    N.check(lib.fb_stream_sync(None))
    out = d_st.download(np.zeros(1, dtype=N.STATS_DTYPE))
    for b in (d_st, d_recs, d_ts):
        if b is not None:
            b.free()
    assert int(out[0]["error"]) == 0, out
    return int(out[0]["new_sessions"])


ROUTED_CASES = [("triples", fs.ONE_SVC, ""), ("pairs", fs.ONE_SVC, "timed")]


@pytest.mark.parametrize("corpus,pair,variant", ROUTED_CASES, ids=["triples-one_svc", "pairs-one_svc-timed"])
def test_routed_in_process(corpus, pair, variant):
    """What RoutedSessionTable.process does, without the process group: per global batch every rank
    parses and routes its shard, every owner concatenates the ranks' groups in rank order and applies
    them in one update call.  The owners' tables are the single table, positions included."""
    ref = rs.reference(corpus, pair, variant)
    timed = variant == "timed"
    world = ref.world
    single = ref.single.export_sorted()
    own = _owners(single, world)
    caps = _contexts([_capacity(int(c)) for c in np.bincount(own, minlength=world)], timed=timed)
    try:
        new = 0
        for k, row in enumerate(ref.calls):
            routed = [_route(caps[r], row[r], world, timed) for r in range(world)]
            global_n = len(ref.global_calls[k][0])
            for o in range(world):
                recs = np.concatenate([g[o] for g, _ in routed])
                ts = np.concatenate([t[o] for _, t in routed]) if timed else None
                assert (np.diff(recs["pkt_index"].astype(np.int64)) > 0).all()  # global packet order
                new += _apply(caps[o], recs, ts, global_n)
        assert new == ref.new_sessions == len(single)
        tables = [c.export_flows() for c in caps]
        for o, t in enumerate(tables):
            assert (_owners(t, world) == o).all()
        _same_records(rs.rows(np.concatenate(tables)), rs.rows(single), "routed union")
        if timed:
            times = ref.single.export_times()
            for o, cap in enumerate(caps):
                _check_times(cap, _OwnerRows(single[own == o], times[own == o]), "owner %d" % o)
            assert (times["segment_count"] > 0).any() and (times["end_time_ns"] != N.FB_SEEN_NONE).any()
    finally:
        _close(caps)
