"""The session table's probe under forced tag collisions, on every update path, against the oracle.

The corpora of tests/keyspace.py put distinct flows where the probe cannot tell them apart without
comparing key words -- pairs equal in all but one 64-bit key word with equal tags in one partition
(F1), twelve IPv6 keys with one 64-bit hash (F2), an IPv6 key with the hash of an IPv4 key (F3) -- and
shape a partition's probe sequences by home slot (G: ladder, wrap, a forty-key cluster, a full
partition).  The oracle's table (FNV-1a over the 40 key bytes, memcmp) shares neither the hash nor the
probe; tests/test_keyspace_oracle.py pins it on the same corpora.

  path      entry point                                     as tests/test_gpu_flagspace.py
  layout    together: a group's first packets in one 64-record segment (adjacent lanes race on the claim)
            apart:    one update call per group member (a miss against published tags, then the insert)
            each followed by two find calls over every key, both directions, interleaved across groups

Compared in every case: every fb_flow_rec field but slot, every history string and conn_state, each
batch's records (where the path returns them), new_sessions / updated_sessions per call, error == 0
(timed contexts: every fb_flow_time field too); and then the open-addressing invariant on the exported
slots (keyspace.check_placement, with the library's own fb_flow_hash): every flow in its hash's
partition, no empty slot between its home slot and its slot."""
import numpy as np
import pytest

import flagseq as fs
import framegen as fg
import keyspace as ks
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.distributed import shard_range
from flodbadd_amd.sessions import SessionFilter
from oracle import coracle
from test_gpu_c5 import _merge_dev, _rows
from test_gpu_flagspace import _check_tables, _table_only
from test_gpu_timed import _check as _check_times

pytestmark = pytest.mark.gpu

S = 10 ** 9


def _lib_hash(words):
    """fb_flow_hash over [n, 10] key words."""
    lib = N.gpu_lib()
    w = np.ascontiguousarray(words, dtype="<u4").reshape(-1, 10)
    return np.array([lib.fb_flow_hash(N.ptr(w[i: i + 1])) for i in range(len(w))], dtype=np.uint64)


def _placement(cap, tag):
    gf = cap.export_flows()
    info = cap.table_info()
    assert int(info["capacity"]) == int(info["partitions"]) * ks.SLOTS, info
    try:
        ks.check_placement(gf, int(info["partitions"]), hash_fn=_lib_hash)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (tag, e)) from None
    return gf


def _step(cap, path, tag, k, fr, of, ts, recs, r_st):
    """One update call through `path`; its records and counters against the oracle's."""
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
    got, want = (st["new_sessions"], st["updated_sessions"]), (int(r_st[0]["new_sessions"]), int(r_st[0]["updated_sessions"]))
    assert got == want, "%s, call %d: new / updated sessions %s, the oracle's %s" % (tag, k, got, want)
    assert st["n_session"] == len(recs)


def _run(name, how, path, capacity, timed=False, grow=False, precondition=None, partitions=None):
    ref, flows = ks.reference(name, how, timed)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, track_history=True, timed=timed,
                             flow_capacity=capacity, grow=grow)
    tag = "%s/%s/%s%s" % (name, how, path, "/timed" if timed else "")
    try:
        if precondition:
            precondition(cap, ref)
        if path == "table":
            N.check(N.gpu_lib().fb_set_session_records(cap.ctx, 0))
        for k, call in enumerate(ref):
            _step(cap, path, tag, k, *call)
        _check_tables(cap, flows, tag)
        if timed:
            _check_times(cap, flows, tag)
        if partitions is not None:
            assert int(cap.table_info()["partitions"]) == partitions
        return _placement(cap, tag), cap.table_info()
    finally:
        cap.close()


def test_families_hold_under_the_library_hash():
    """fb_flow_hash agrees with the helper's restatement on every corpus key, and gives each family
    the property it was built for."""
    keys = []
    for name, how in ks.CASES:
        keys += list(ks.calls_of(name, how)[0].keys)
    keys = np.stack(keys + [ks.corpus_g4()[1]])
    assert (_lib_hash(keys) == ks.flow_hash(keys)).all()
    for fam, a, ka, kb, same in ks.f1_all():
        ha, hb = (int(x) for x in _lib_hash(np.stack([ka, kb])))
        assert ha >> 62 == hb >> 62 and (ha & 0xFFFFFFFF) | 2 == (hb & 0xFFFFFFFF) | 2, (fam, a)
        assert ((ha ^ hb) & 0xFFFFFFFF) == (0 if same else 2)
    for fam, H in zip(ks.f2_all(), ks.F2_HASHES):
        assert set(_lib_hash(np.stack(fam)).tolist()) == {H}
    for k4, k6 in ks.f3_pairs():
        assert len(set(_lib_hash(np.stack([k4, k6])).tolist())) == 1
    g4 = _lib_hash(np.stack(ks.g4_full()))
    assert set((g4 & np.uint64(511)).tolist()) == {ks.G4_HOME} and not (g4 >> np.uint64(48)).any()


F_CASES = [(how, path) for how in ("together", "apart") for path in ("dense", "seg", "table", "parsed")]


@pytest.mark.parametrize("how,path", F_CASES, ids=["%s-%s" % c for c in F_CASES])
def test_keyspace_families(how, path):
    """F1 + F2 + F3 and 300 filler flows in a fixed 2^11-slot table (4 partitions), then the find calls."""
    gf, _ = _run("f", how, path, 1 << 11, partitions=4)
    c = ks.corpus_f()
    assert len(gf) == 2 * len(c.keys)
    # an F2 family's twelve keys share one home, so they stand at twelve distances from it (home 507: the
    # farthest is past the partition's end)
    slot_of = dict(zip((bytes(r.tobytes()[:40]) for r in gf), gf["slot"].tolist()))
    for g, H in zip(c.groups[32:35], ks.F2_HASHES):
        dist = sorted((slot_of[ks.key_bytes(c.keys[i])] - (H & 511)) % ks.SLOTS for i in g)
        assert len(g) == 12 and len(set(dist)) == 12 and dist[-1] >= 11, (H, dist)


T_CASES = [(how, path) for how in ("together", "apart") for path in ("seg", "table")]


@pytest.mark.parametrize("how,path", T_CASES, ids=["%s-%s" % c for c in T_CASES])
def test_keyspace_families_timed(how, path):
    """The same corpus on a timed context: the plain K2 and fb_time.hip."""
    gf, _ = _run("f", how, path, 1 << 11, timed=True, partitions=4)
    assert (gf["segment_count"] > 0).any()


@pytest.mark.parametrize("path", ["seg", "table", "parsed"])
def test_keyspace_geometry(path):
    """G1-G3 in one fixed 512-slot partition: the occupiers in one call, then the ladder's climbers, the
    wrap and the cluster, then the find calls.  The climbers land in the group after their home's, the
    wrap's keys in 509..511 and 0..4, the cluster in 300..339."""
    gf, _ = _run("g123", "staged", path, 512, partitions=1)
    c, _ = ks.corpus_g123()
    slot_of = dict(zip((bytes(r.tobytes()[:40]) for r in gf), gf["slot"].tolist()))
    at = lambda g: sorted(slot_of[ks.key_bytes(c.keys[i])] for i in c.groups[g])  # noqa: E731
    occ = [slot_of[ks.key_bytes(c.keys[i])] for i in c.groups[0]]
    assert occ == [8 * g + q for r, g in enumerate(ks.G1_GROUPS) for q in range(r, 8)]  # each in its home
    assert at(1) == [8 * (g + 1) for g in ks.G1_GROUPS]
    assert at(2) == [0, 1, 2, 3, 4, 509, 510, 511]
    assert at(3) == list(range(ks.G3_HOME, ks.G3_HOME + ks.G3_SIZE))


def test_keyspace_full_partition():
    """G4: 512 keys with home slot 259 fill the fixed 512-slot table in one call -- the last one in sits
    in slot 258, which k2_lookup's 64 group reads do not reach -- and are all found again; one more key
    is refused with FB_ERR_TABLE_FULL and leaves the 512 rows as they were."""
    ref, flows = ks.reference("g4", "together")
    c, extra = ks.corpus_g4()
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, track_history=True, flow_capacity=512, grow=False)
    try:
        for k, call in enumerate(ref):
            _step(cap, "seg", "g4", k, *call)
        assert int(ref[0][4][0]["new_sessions"]) == 512 and int(ref[1][4][0]["new_sessions"]) == 0
        _check_tables(cap, flows, "g4")
        gf = _placement(cap, "g4")
        assert sorted(gf["slot"].tolist()) == list(range(512))
        with pytest.raises(N.FbError) as ei:
            cap.process_frames(*fg.pack([ks.frame_of(extra, fg.SYN, 0)]))
        assert ei.value.code == N.FB_ERR_TABLE_FULL
        _check_tables(cap, flows, "g4 after the refused key")
        _placement(cap, "g4 after the refused key")
    finally:
        cap.close()


def _both_groups_combine(cap, ref):
    """Host-side precondition (K1's rule, fb_flow.hip, with the library's hash): the F2 family's partition
    and every F1 pair's each reach max(FB_COMB_MIN = 64, 4 x the chunk's mean per partition) records."""
    c, _ = ks.corpus_hot()
    parts = int(cap.table_info()["partitions"])
    assert parts == 32
    recs = ref[0][3]
    assert len(recs) <= 20480
    part = (_lib_hash(ks.words_of(recs)) >> np.uint64(64 - 5)).astype(np.int64)
    cnt = np.bincount(part, minlength=parts)
    need = max(64, 4 * ((len(recs) + parts - 1) // parts))
    hot = {int(_lib_hash(c.keys[g[0]])[0] >> np.uint64(59)) for g in c.groups}
    assert len(c.groups) == 6 and len(hot) >= 2 and all(cnt[p] >= need for p in hot), (cnt.tolist(), need, hot)


@pytest.mark.parametrize("path", ["dense", "seg", "table"])
def test_keyspace_hot_groups(path):
    """A 2^14-slot table (32 partitions): the twelve keys of one F2 family are the hot flows of one
    (chunk, partition) group -- eleven with 60 to 70 records and one with a single record, so combined
    and plain entries of one tag stand side by side in k_flow_combine's table -- and for each of the
    five key words an equal-h32 F1 pair (one home in that 256-slot table) those of a group of its own."""
    gf, _ = _run("hot", "hot", path, 1 << 14, precondition=_both_groups_combine, partitions=32)
    assert len(gf) == len(ks.corpus_hot()[0].keys)


@pytest.mark.parametrize("path", ["dense", "seg"])
def test_keyspace_growth(path):
    """The family corpus, one call per group member, into a growing table that starts with 512 slots: rows
    and histories equal the oracle's across the slot remaps and the placement holds at the new geometry."""
    gf, info = _run("f", "apart", path, 512, grow=True)
    assert info["generation"] >= 1 and info["partitions"] >= 2 and info["capacity"] == 512 * info["partitions"], info
    assert len(gf) == 2 * len(ks.corpus_f().keys)


def test_keyspace_purge():
    """A timed 2^11-slot table holding G3's cluster, every F1 pair and filler: every other member of the
    cluster and one key of each pair expire (the way tests/test_gpu_age.py::test_purge_dense_partitions
    drives it), the table equals the oracle's subset replay, the re-packed partitions keep the placement
    invariant, and the next update finds every survivor and re-inserts every purged key as new."""
    c = ks.Corpus(reverse=False)
    cluster = c.add_group(ks.g3_cluster())
    pairs = [c.add_group([ka, kb]) for _, _, ka, kb, _ in ks.f1_all()]
    c.add_filler(ks.filler(200))
    gone = set(cluster[1::2]) | {g[1] for g in pairs}
    stay = [i for i in range(len(c.keys)) if i not in gone]
    call_a = ks.together(c)[0]
    call_b = [(i, fg.ACK if c.proto(i) == ks.TCP else 0, c.pay(i), False) for i in stay]
    call_c = [(i, fg.PSH | fg.ACK if c.proto(i) == ks.TCP else 0, c.pay(i), False) for i in range(len(c.keys))]
    T0 = ks.BASE_NS
    cfg = coracle.make_cfg(2)
    batches = []
    for call, at in ((call_a, 0), (call_b, 150), (call_c, 86600)):
        fr, of = ks.frames(c, call)
        recs = coracle.parse_classify(cfg, fr, of)[0]
        assert (ks.words_of(recs) == np.stack([c.keys[i] for i, _, _, _ in call])).all()
        batches.append((fr, of, (T0 + at * S + np.arange(len(call), dtype=np.uint64) * 1000).astype(np.uint64), recs))
    (frA, ofA, tsA, recA), (frB, ofB, tsB, recB), (frC, ofC, tsC, recC) = batches
    stay_keys = {ks.key_bytes(c.keys[i]) for i in stay}
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11, timed=True, grow=False,
                             track_history=True)
    try:
        cap.process_frames_seg(frA, ofA, ts=tsA)
        cap.process_frames(frB, ofB, ts=tsB)
        _placement(cap, "purge: before")
        st = cap.update_sessions_status(T0 + 86500 * S, purge=True)
        assert st["purged"] == len(gone) and st["remaining"] == len(stay), st
        sub = coracle.Flows()
        keep = np.array([bytes(r.tobytes()[:40]) in stay_keys for r in recA])
        sub.update(recA[keep], ts=tsA)
        sub.update(recB, ts=tsB)
        _check_tables(cap, sub, "purge: after")
        _check_times(cap, sub, "purge: after")
        _placement(cap, "purge: after")
        g = cap.process_frames_seg(frC, ofC, ts=tsC)
        ost = np.zeros(1, dtype=N.STATS_DTYPE)
        sub.update(recC, ost, ts=tsC)
        assert g.stats["error"] == 0 and int(ost[0]["new_sessions"]) == len(gone)
        assert (g.stats["new_sessions"], g.stats["updated_sessions"]) == (len(gone), len(stay))
        _check_tables(cap, sub, "purge: re-insert")
        _check_times(cap, sub, "purge: re-insert")
        gf = _placement(cap, "purge: re-insert")
        assert len(gf) == len(c.keys)
    finally:
        cap.close()


def _export_map(cap, world, rank, call_map):
    lib = N.gpu_lib()
    n = cap.flow_count()
    cm = np.ascontiguousarray(call_map, dtype=np.uint64)
    d_out, d_cnt = N.DeviceBuffer(max(n, 1) * N.FLOW_MREC_DTYPE.itemsize), N.DeviceBuffer(8 * world)
    N.check(lib.fb_flow_export_merge_map_dev(cap.ctx, world, rank, N.ptr(cm), len(cm), d_out.ptr, n, d_cnt.ptr, None))
    counts = d_cnt.download(np.zeros(world, dtype=np.uint64))
    m = d_out.download(np.zeros(max(n, 1), dtype=N.FLOW_MREC_DTYPE))[: int(counts.sum())]
    d_out.free()
    d_cnt.free()
    assert int(counts.sum()) == n
    return m, counts


@pytest.mark.parametrize("world", [2, 3])
def test_keyspace_merge(world):
    """The family corpus split by packet index over `world` contexts and merged on the device (the
    single-process shape of tests/test_gpu_c5.py): every exported group and every owner's merge equal the
    oracle's, the merged table equals one table fed everything, and an F2 family's twelve keys all fall to
    one owner (one hash: one rank, one slot of k_mg_claim's table)."""
    c, calls = ks.calls_of("f", "together")
    _, single = ks.reference("f", "together")
    caps = [FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11, grow=False)
            for _ in range(world)]
    try:
        groups = []
        for r, cap in enumerate(caps):
            ref, cmap = coracle.Flows(), []
            for k, call in enumerate(calls):
                first, count = shard_range(len(call), r, world)
                fr, of = ks.frames(c, call[first: first + count])
                g = cap.process_frames_seg(fr, of) if k % 2 else cap.process_frames(fr, of)
                assert g.stats["error"] == 0
                ref.update(coracle.parse_classify(coracle.make_cfg(2), fr, of)[0])
                cmap.append(k << 32 | first)
            _placement(cap, "merge: rank %d of %d" % (r, world))
            m, counts = _export_map(cap, world, r, cmap)
            em, ecounts = ref.export_merge(world, r, call_map=cmap)
            assert np.array_equal(counts, ecounts)
            w = N.FLOW_MREC_DTYPE.itemsize
            for o in range(world):
                a = m[int(counts[:o].sum()): int(counts[: o + 1].sum())]
                b = em[int(ecounts[:o].sum()): int(ecounts[: o + 1].sum())]
                ka = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), w)
                kb = np.ascontiguousarray(b).view(np.uint8).reshape(len(b), w)
                ka, kb = ka[np.lexsort(ka[:, :40].T[::-1])], kb[np.lexsort(kb[:, :40].T[::-1])]
                assert ka.tobytes() == kb.tobytes(), (r, o)
            groups.append((m, counts))
        merged = []
        for o in range(world):
            recv = np.concatenate([m[int(n[:o].sum()): int(n[: o + 1].sum())] for m, n in groups])
            got = _merge_dev(caps[o], recv)
            assert _rows(got).tobytes() == _rows(coracle.flow_merge(recv)).tobytes(), o
            merged.append(got)
        for g, H in zip(c.groups[32:35], ks.F2_HASHES):
            owner = ((H >> 32) * world) >> 32
            fam = {ks.key_bytes(c.keys[i]) for i in g}
            assert fam <= {bytes(x.tobytes()[:40]) for x in merged[owner]}
            assert all(N.gpu_lib().fb_flow_owner(N.ptr(np.frombuffer(k, dtype=np.uint8).copy()), world) == owner for k in fam)
        table = np.concatenate(merged)
        want = single.export_sorted()
        assert len(table) == len(want) == 2 * len(c.keys)
        assert _rows(table).tobytes() == _rows(want).tobytes()
    finally:
        for x in caps:
            x.close()
