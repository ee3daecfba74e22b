"""The run-space corpora (tests/runspace.py) pinned on the CPU, before anything runs on a GPU: the census'
constants equal the sources', the census gives the hand-worked dispatch on six toy inputs (one on each
threshold), every corpus contains the run classes and boundary lengths it was built for (literal sets), the
placement round-trips through the segmented layout, and the oracle's history of every flow equals the
CYCLE13 closed form (coracle on every corpus, pyoracle on the ladder)."""
import os
import shutil

import numpy as np
import pytest

import flagseq as fs
import keyspace as ks
import runspace as rs
from flodbadd_amd import _native as N
from oracle import coracle, pyoracle
from test_flagspace_oracle import _key_of, _py_cfg

CH = rs.CH


# ---- constants ------------------------------------------------------------------------------------
def test_constants_equal_the_sources():
    assert rs.source_constants() == rs.CONSTANTS
    assert N.FB_SEG_FRAMES == rs.SEG and ks.SLOTS == rs.SLOTS


@pytest.mark.parametrize("old,new,name", [
    ("constexpr uint32_t kRunSort = 16;", "constexpr uint32_t kRunSort = 15;", "kRunSort"),
    ("constexpr uint32_t kWaveSortMax = 512;", "constexpr uint32_t kWaveSortMax = 256;", "kWaveSortMax"),
    ("#define FB_HIST_CAP 4096", "#define FB_HIST_CAP 2048", "kHistCap")])
def test_constants_guard_sees_a_changed_threshold(tmp_path, old, new, name):
    """A copy of the sources with one dispatch threshold changed no longer equals the census' table."""
    for fn in ("fb_internal.h", "fb_flow.hip", "fb_hist.hip"):
        shutil.copy(os.path.join(rs.CSRC, fn), tmp_path / fn)
    text = (tmp_path / "fb_hist.hip").read_text()
    assert text.count(old) == 1
    (tmp_path / "fb_hist.hip").write_text(text.replace(old, new))
    got = rs.source_constants(str(tmp_path))
    assert got != rs.CONSTANTS and {k for k in got if got[k] != rs.CONSTANTS[k]} == {name}


# ---- the census on hand-worked inputs ---------------------------------------------------------------
def _toy(parts, groups, n_slots, **kw):
    """groups: [(chunk, partition, [(index into the partition's pool, records)], UDP records)], each chunk's
    records consecutive from its first slot -> the census."""
    T, U = rs.pool(parts)
    at, slots, flows = {}, [], []
    for c, p, items, udp in groups:
        fl = [T[p][i] for i, k in items for _ in range(k)] + [U[p][0]] * udp
        a = at.get(c, 0)
        slots += list(range(c * CH + a, c * CH + a + len(fl)))
        flows += fl
        at[c] = a + len(fl)
    order = np.argsort(slots, kind="stable")
    flows = np.array(flows, dtype=np.int64)[order]
    codes = np.where(flows & rs.UDP, 0, 1)
    return rs.census(np.array(slots)[order], rs.keys_of(flows), codes, parts, n_slots, **kw)


def _part(kernel, read, applied, runs, batches=(), blocks=1, block_chunks=None, rounds=1, chunks=1):
    return dict(kernel=kernel, read=read, applied=applied, runs=runs, batches=list(batches), blocks=blocks,
                block_chunks=block_chunks or [(0, chunks)], rounds=rounds)


def test_census_hot_threshold():
    """16 partitions, one chunk of 1,024 slots: hot_min = max(64, 4 * ceil(1024 / 16)) = 256.
    Partition 0 holds 256 records of two flows (128 each): on the threshold, hot; both keys repeat, so the
    group becomes 2 combined entries (applied 2, read 256) and the partition is the general kernel's, one
    batch of 256 entries, class combined.  Partition 1 holds 255 records: below, plain; 255 > 16 sends it to
    the general kernel, 129..256 entries is wave_sort_run<4>.  Partition 2 holds 300 records of 300 flows:
    hot by count, but no key repeats, so k_flow_combine leaves it plain: 257..512 is wave_sort_run<8>.
    With hot=False (a timed context) partition 0 stays plain: 256 entries, wave_sort_run<4>."""
    g = [(0, 0, [(0, 128), (1, 128)], 0), (0, 1, [(0, 128), (1, 127)], 0), (0, 2, [(i, 1) for i in range(300)], 0)]
    want = {"chunks": 1, "nblk": 1, "partitions": {
        0: _part("general", 256, 2, {0: ("combined", 256)}, [(0, 1, 256)]),
        1: _part("general", 255, 255, {0: ("wave4", 255)}, [(0, 1, 255)]),
        2: _part("general", 300, 300, {0: ("wave8", 300)}, [(0, 1, 300)])}}
    assert _toy(16, g, 1024) == want
    want["partitions"][0] = _part("general", 256, 256, {0: ("wave4", 256)}, [(0, 1, 256)])
    assert _toy(16, g, 1024, hot=False) == want


def test_census_register_sort_limit():
    """16 partitions, two full chunks.  Partition 0: runs of 16 and 16: every run <= kRunSort, 32 entries,
    one wave's share 32 <= 512: uniform; the wave's longest run is 16 > 8: sort_net<16> for both.
    Partition 1: runs of 17 and 1: 17 > kRunSort: general; both runs fit one batch of 18 entries; the 17-run is
    a wavefront's (17..64: wave_sort_run<1>), the 1-run is thread 1's, and the longest register run of its
    wave is 1: no network.  Partition 2: 5 records, all UDP: no characters, both kernels return at once."""
    g = [(0, 0, [(0, 8), (1, 8)], 0), (1, 0, [(0, 16)], 0), (0, 1, [(0, 17)], 0), (1, 1, [(1, 1)], 0), (0, 2, [], 5)]
    want = {"chunks": 2, "nblk": 1, "partitions": {
        0: _part("uniform", 32, 32, {0: ("reg16", 16), 1: ("reg16", 16)}, chunks=2),
        1: _part("general", 18, 18, {0: ("wave1", 17), 1: ("single", 1)}, [(0, 2, 18)], chunks=2),
        2: _part("idle", 5, 5, {}, rounds=0, chunks=2)}}
    assert _toy(16, g, 2 * CH) == want


def test_census_wave_share_and_wave_sort_limit():
    """16 partitions, 64 full chunks (one wave of the uniform kernel; nblk = 16, nobody reads 8,192).
    Partition 0: 8 records in each chunk: 64 x 8 = 512 = kHistPer * 64: uniform, sort_net<8>.
    Partition 1: 9 in chunk 0 and 8 in the others: 513: general; one round, one batch of 513 entries; the
    wave's longest run is 9: sort_net<16> for all 64 runs.
    Partition 2: one run of 512: the longest wave_sort_run<8>.  Partition 3: one run of 513: the bitmap rank."""
    g = [(c, 0, [(0, 4), (1, 4)], 0) for c in range(64)] + [(c, 1, [(0, 9 if c == 0 else 8)], 0) for c in range(64)] + \
        [(0, 2, [(0, 512)], 0), (0, 3, [(0, 513)], 0)]
    want = {"chunks": 64, "nblk": 16, "partitions": {
        0: _part("uniform", 512, 512, {c: ("reg8", 8) for c in range(64)}, chunks=64),
        1: _part("general", 513, 513, {c: ("reg16", 9 if c == 0 else 8) for c in range(64)}, [(0, 64, 513)], chunks=64),
        2: _part("general", 512, 512, {0: ("wave8", 512)}, [(0, 64, 512)], chunks=64),
        3: _part("general", 513, 513, {0: ("bitmap", 513)}, [(0, 64, 513)], chunks=64)}}
    assert _toy(16, g, 64 * CH) == want


def test_census_batch_capacity():
    """16 partitions, two full chunks (hot_min 5,120).  Partition 0: runs of 4,096 and 1: the first batch takes
    whole runs while rp <= rp[0] + 4096: run 0 alone (4,096 entries, bitmap rank), then run 1 (one entry, no
    network).  Partition 1: runs of 4,097 and 1: 4,097 > kHistCap goes through long_run alone (no batch),
    then a batch with run 1."""
    g = [(0, 0, [(0, 2048), (1, 2048)], 0), (1, 0, [(0, 1)], 0), (0, 1, [(0, 2048), (1, 2049)], 0), (1, 1, [(0, 1)], 0)]
    want = {"chunks": 2, "nblk": 1, "partitions": {
        0: _part("general", 4097, 4097, {0: ("bitmap", 4096), 1: ("single", 1)}, [(0, 1, 4096), (1, 2, 1)], chunks=2),
        1: _part("general", 4098, 4098, {0: ("long_plain", 4097), 1: ("single", 1)}, [(1, 2, 1)], chunks=2)}}
    assert _toy(16, g, 2 * CH) == want


def test_census_split_threshold():
    """16 partitions, eight full chunks: nblk = min(128, ceil(8 / 4)) = 2.
    Partition 0: 1,024 in every chunk = 8,192 entries to read: not above kHistSplitEntries, one workgroup,
    batches of four runs (4,096 entries) each.
    Partition 1: 1,024 in seven chunks and 1,025 in the last = 8,193: split; it asks for ceil(8193 / 4096) = 3
    blocks and gets nblk = 2, of ceil(8 / 2) = 4 chunks; block 0 is one batch of 4,096, block 1 cuts after three
    runs (3,072; the fourth would make 4,097) and takes the last run alone."""
    g = [(c, 0, [(0, 512), (1, 512)], 0) for c in range(8)] + [(c, 1, [(0, 512), (1, 512 + (c == 7))], 0) for c in range(8)]
    want = {"chunks": 8, "nblk": 2, "partitions": {
        0: _part("general", 8192, 8192, {c: ("bitmap", 1024) for c in range(8)}, [(0, 4, 4096), (4, 8, 4096)], chunks=8),
        1: _part("general", 8193, 8193, {c: ("bitmap", 1025 if c == 7 else 1024) for c in range(8)},
                 [(0, 4, 4096), (4, 7, 3072), (7, 8, 1025)], blocks=2, block_chunks=[(0, 4), (4, 8)], rounds=2)}}
    assert _toy(16, g, 8 * CH) == want


def test_census_chunk_rounds():
    """16 partitions, 513 chunks (one more than kHistRuns; nblk = 128): partition 0 holds 4 records in chunk 0 and
    4 in chunk 512 -- uniform by its runs, but chunks > kHistRuns hands every partition to the general kernel,
    which takes two rounds (chunks 0..511, then 512), one batch each, sort_net<4>.  The same records with 512
    chunks are the uniform kernel's; chunk 511 is then run 63 of wave 7."""
    g = [(0, 0, [(0, 4)], 0), (512, 0, [(0, 4)], 0)]
    want = {"chunks": 513, "nblk": 128, "partitions": {
        0: _part("general", 8, 8, {0: ("reg4", 4), 512: ("reg4", 4)}, [(0, 512, 4), (512, 513, 4)], rounds=2, chunks=513)}}
    assert _toy(16, g, 513 * CH) == want
    g = [(0, 0, [(0, 4)], 0), (511, 0, [(0, 4)], 0)]
    want = {"chunks": 512, "nblk": 128, "partitions": {
        0: _part("uniform", 8, 8, {0: ("reg4", 4), 511: ("reg4", 4)}, chunks=512)}}
    assert _toy(16, g, 512 * CH) == want


def test_census_raises_on_more_keys_than_the_combine_table():
    g = [(0, 0, [(i, 2) for i in range(257)], 0)]
    with pytest.raises(ValueError):
        _toy(16, g, 1024)
    cen = _toy(16, g, 1024, overflow_ok=True)
    assert cen["partitions"][0]["runs"] == {0: ("overflow", 514)} and cen["partitions"][0]["applied"] is None


# ---- coverage of the corpora ------------------------------------------------------------------------
def _run_flows(call, parts, chunk, p):
    """The flows of run (chunk, partition p) in record order."""
    part = ks.part_of(ks.flow_hash(call.keys), parts)
    sel = (part == p) & (call.slots // CH == chunk)
    return call.flow[sel], call.slots[sel] % CH


def test_ladder_coverage():
    a, b = rs.ladder()
    ca, cb = rs.census_of(a, 16), rs.census_of(b, 16)
    assert rs.classes(ca) == {"single", "reg4", "reg8", "reg16", "wave1", "wave2", "wave4", "wave8", "bitmap", "long_plain"}
    plain = {1, 2, 3, 4, 5, 8, 9, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 5000}
    assert plain <= rs.lengths(ca) and rs.lengths(ca) - plain == {3300, 505, 506, 1052, 1053, 2029}  # (the fill)
    P = ca["partitions"]
    assert {p for p in P if P[p]["kernel"] == "uniform"} == {0} and P[0]["runs"] == {0: ("reg16", 3), 1: ("reg16", 9), 2: ("reg16", 16)}
    assert P[1]["runs"] == {0: ("long_plain", 5000), 1: ("reg8", 4), 2: ("reg8", 8)}  # register sorts in k_hist_general
    assert P[2]["batches"] == [(0, 2, 4096), (2, 3, 17)] and P[3]["batches"][0] == (0, 1, 4096)  # cuts on a run boundary
    assert P[4]["runs"][1] == ("long_plain", 4097)
    assert all(i["blocks"] == 1 and i["rounds"] == 1 for i in P.values())
    assert rs.lengths(ca, "wave1") == {17, 63, 64} and rs.lengths(ca, "wave2") == {65, 127, 128}
    assert rs.lengths(ca, "wave4") == {129, 255, 256} and rs.lengths(ca, "wave8") >= {257, 511, 512}
    assert rs.lengths(ca, "bitmap") >= {513, 4095, 4096}
    # every slot is taken: the dense and the fused layout cut the same chunks
    assert len(a.recs) == a.n_slots == rs.LADDER_SLOTS and (a.slots == np.arange(a.n_slots)).all()
    # the long runs: records on long_run's window edges, 3 to 40 flows, a flow with more than 64 consecutive
    # entries and a flow whose entries are at least 64 apart
    T, _ = rs.pool(16)
    for chunk, p, nf in ((0, 1, 40), (1, 4, 3)):
        fl, pos = _run_flows(a, 16, chunk, p)
        assert set(rs.LADDER_EDGES) <= set(pos.tolist()), (chunk, p)
        assert len({f for f in fl.tolist() if not f & rs.UDP}) == nf and (fl & rs.UDP).any()
    fl, _ = _run_flows(a, 16, 0, 1)
    w = np.flatnonzero(fl == T[1][rs.LADDER_WAVE_FLOW])
    longest = max(len(r) for r in np.split(w, np.flatnonzero(np.diff(w) != 1) + 1))
    assert longest > 64
    s = np.flatnonzero(fl == T[1][rs.LADDER_STRIDE_FLOW])
    assert len(s) >= 64 and np.diff(s).min() >= 64
    # the second call continues every flow of the first
    tcp = lambda c: {f for f in c.flow.tolist() if not f & rs.UDP}  # noqa: E731
    assert tcp(a) == tcp(b) and rs.classes(cb) == {"reg16", "wave1", "wave2"}
    assert {i["kernel"] for i in cb["partitions"].values()} == {"uniform", "general"}


def test_waves_coverage():
    (a,) = rs.waves()
    cen = rs.census_of(a, 16)
    P = cen["partitions"]
    assert cen["chunks"] == 257 and set(P) == {0, 1, 2}
    # partition 0: uniform, a network width per wave, wave 0's share exactly 512 entries
    assert P[0]["kernel"] == "uniform"
    by_wave = [{P[0]["runs"][c][0] for c in range(w, w + 64)} for w in range(0, 256, 64)]
    assert by_wave == [{"reg8"}, {"reg4"}, {"reg16"}, {"single"}]
    assert sum(P[0]["runs"][c][1] for c in range(64)) == 512
    # partition 1: a wave's share of 513 in small runs only
    assert P[1]["kernel"] == "general" and P[1]["read"] == 513 and max(L for _, L in P[1]["runs"].values()) == 9
    assert P[1]["batches"] == [(0, 257, 513)]
    # partition 2: 4,097 applied entries in runs <= 16 (tp > kHistCap), cut at 4,096 on a run boundary
    assert P[2]["kernel"] == "general" and P[2]["applied"] == 4097 and max(L for _, L in P[2]["runs"].values()) == 16
    assert P[2]["batches"] == [(0, 256, 4096), (256, 257, 1)]


def test_combined_coverage():
    (a,), where = rs.combined()
    cen = rs.census_of(a, 256, overflow_ok=True)
    with pytest.raises(ValueError):
        rs.census_of(a, 256)
    assert rs.classes(cen) == {"combined", "long_combined", "overflow", "wave1", "wave8"}
    got = {g: (cen["partitions"][p]["runs"][c], cen["partitions"][p]["applied"]) for g, (c, p) in where.items()}
    assert got == {"on_threshold": (("combined", 320), 11),     # ten flows and a UDP key, each repeated
                   "below_threshold": (("wave8", 319), 319),
                   "one_key": (("combined", 400), 1),
                   "keys_256": (("combined", 512), 256),
                   "half_once": (("combined", 320), 210),       # 100 keys once stay plain + 110 combined
                   "long": (("long_combined", 4100), 7),
                   "overflow": (("overflow", 600), None),
                   "tail_on": (("combined", 64), 4),            # the 4,096-slot tail chunk: hot_min 64
                   "tail_below": (("wave1", 63), 63)}
    assert a.n_slots == 2 * CH + 4096
    part = ks.part_of(ks.flow_hash(a.keys), 256)
    c, p = where["overflow"]
    k = np.unique(a.flow[(part == p) & (a.slots // CH == c)], return_counts=True)[1]
    assert len(k) == 300 and (k == 2).all()
    c, p = where["half_once"]
    k = np.unique(a.flow[(part == p) & (a.slots // CH == c)], return_counts=True)[1]
    assert sorted(np.unique(k, return_counts=True)[1].tolist()) == [100, 110]


def test_blocks_coverage():
    (a,) = rs.blocks()
    cen = rs.census_of(a, 16)
    P = cen["partitions"]
    assert (cen["chunks"], cen["nblk"]) == (12, 3)
    assert {p: (i["read"], i["blocks"]) for p, i in P.items()} == {0: (12300, 3), 1: (8192, 1), 2: (8193, 3), 3: (8500, 3)}
    assert all(i["block_chunks"] == [(0, 4), (4, 8), (8, 12)] for p, i in P.items() if i["blocks"] == 3)
    assert P[3]["runs"][5] == ("long_combined", 5200) and {P[3]["runs"][c] for c in range(12) if c != 5} == {("wave8", 300)}
    assert rs.lengths(cen, "bitmap") == {682, 683, 1025}
    T, _ = rs.pool(16)
    blk = {}
    for c in range(12):
        for f in _run_flows(a, 16, c, 0)[0].tolist():
            blk.setdefault(f, set()).add(c // 4)
    assert blk.pop(T[0][rs.BLOCKS_FIRST_ONLY]) == {0} and blk.pop(T[0][rs.BLOCKS_LAST_ONLY]) == {2}
    assert len(blk) == 22 and all(v == {0, 1, 2} for v in blk.values())


def test_rounds_coverage():
    (a,) = rs.rounds()
    cen = rs.census_of(a, 16)
    P = cen["partitions"]
    assert cen["chunks"] == 514 and a.n_slots == 10_526_720 and len(a.recs) < 1000
    assert all(i["kernel"] == "general" and i["rounds"] == 2 and i["blocks"] == 1 for i in P.values())
    assert set(np.unique(a.slots // CH).tolist()) == set(rs.ROUNDS_AT)
    assert max(L for _, L in P[0]["runs"].values()) <= 16 and set(P[0]["runs"]) == set(rs.ROUNDS_AT)
    assert P[1]["runs"][512] == ("bitmap", 600) and P[1]["batches"] == [(0, 512, 15), (512, 514, 609)]
    T, _ = rs.pool(16)
    assert all(T[0][0] in _run_flows(a, 16, c, 0)[0] for c in rs.ROUNDS_AT)


def test_scramble_coverage():
    (a,) = rs.scramble()
    cen = rs.census_of(a, 16)
    P = cen["partitions"]
    assert {p: (i["kernel"], i["runs"]) for p, i in P.items() if p not in rs.SCRAMBLE_BALLAST} == {
        0: ("uniform", {0: ("reg4", 4)}), 1: ("uniform", {0: ("reg8", 8)}), 2: ("uniform", {0: ("reg16", 16)}),
        3: ("general", {0: ("reg4", 4), 1: ("wave1", 17)}), 4: ("general", {0: ("reg8", 8), 1: ("wave1", 17)}),
        5: ("general", {0: ("reg16", 16), 1: ("wave1", 17)}),
        6: ("general", {0: ("wave1", 40)}), 7: ("general", {0: ("wave2", 100)}), 8: ("general", {0: ("wave4", 200)}),
        9: ("general", {0: ("wave8", 400)}), 10: ("general", {1: ("bitmap", 600)})}
    # the first half of every run in the last iteration of wavefronts 0..7, the second in that of wavefronts 8..15;
    # every earlier iteration of wavefronts 0..7 holds ballast, of wavefronts 8..15 nothing
    part = ks.part_of(ks.flow_hash(a.keys), 16)
    pos = a.slots % CH
    it, wave = pos // 1024, pos % 1024 // 64
    run = ~np.isin(part, rs.SCRAMBLE_BALLAST)
    assert (it[run] == rs.SCRAMBLE_ITER).all() and (it[~run] < rs.SCRAMBLE_ITER).all() and (wave[~run] < 8).all()
    assert len(np.unique(pos[~run])) == rs.SCRAMBLE_ITER * 512
    for p in rs.SCRAMBLE:
        for c in range(2):
            w = wave[(part == p) & (a.slots // CH == c)]
            assert (w[:len(w) // 2] < 8).all() and (w[len(w) // 2:] >= 8).all(), (p, c)


def test_overfull_coverage():
    (a,) = rs.overfull()
    cen = rs.census_of(a, 1)
    k = np.unique(a.flow, return_counts=True)[1]
    assert len(k) == 600 and (k.min(), k.max()) == (2, 40)
    assert cen["partitions"][0]["runs"] == {0: ("long_plain", len(a.recs))} and len(a.recs) > rs.CAP


# ---- placement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder", "waves", "blocks", "scramble"])
def test_place_round_trips(name):
    calls = getattr(rs, name)()
    for c in calls:
        out, seg = rs.place(c.recs, c.slots, c.n_slots)
        assert out.nbytes == c.n_slots * 56 and len(seg) == c.n_slots // 64 and int(seg.sum()) == len(c.recs)
        back, dns = N.seg_unpack(out, seg)
        assert len(dns) == 0 and back.tobytes() == c.recs.tobytes()
        assert (back["pkt_index"] == c.slots).all()
        assert rs.dense(c.recs).tobytes() == c.recs.tobytes()


def test_place_refuses_a_segment_with_a_gap():
    (c,) = rs.overfull()
    with pytest.raises(AssertionError):
        rs.place(c.recs[:3], np.array([0, 1, 3]), 64)
    with pytest.raises(AssertionError):
        rs.place(c.recs[:2], np.array([65, 66]), 128)
    rs.place(c.recs[:3], np.array([0, 64, 65]), 128)


# ---- the strings ------------------------------------------------------------------------------------
def test_cycle13_symbols_give_the_thirteen_characters():
    recs = rs.parse(np.arange(13), rs.CYCLE13)
    assert "".join(chr(c) for c in recs["hist_char"]) == rs.HIST_CHARS == N.FB_HIST_CHARS
    # one key for both directions of a flow; the UDP flow of the same addresses is another key without a character
    both = rs.parse([7, 7, 7 | rs.UDP], [fs.SYN, fs.REV | fs.SYN | fs.ACK, 0])
    kw = ks.words_of(both)
    assert (kw[0] == kw[1]).all() and (kw[0] != kw[2]).any() and not (both["meta"][2] & N.META_HAS_FLAGS)


def _oracle(calls):
    flows = coracle.Flows()
    for c in calls:
        flows.update(c.recs)
    return flows


CORPORA = {"ladder": rs.ladder, "waves": rs.waves, "scramble": rs.scramble, "combined": lambda: rs.combined()[0], "blocks": rs.blocks,
           "rounds": rs.rounds, "overfull": rs.overfull}


@pytest.mark.parametrize("name", sorted(CORPORA))
def test_oracle_history_is_the_closed_form(name):
    calls = CORPORA[name]()
    flows, want = _oracle(calls), rs.closed_form(calls)
    rec_of = {}
    for c in calls:
        f, first = np.unique(c.flow, return_index=True)
        for x, i in zip(f.tolist(), first.tolist()):
            rec_of.setdefault(x, c.recs[i])
    assert flows.count() == len(want) == len(rec_of)
    for f, h in want.items():
        got, _ = flows.history(rec_of[f])
        assert got == h, (name, f, got, h)
        assert all(x != y for x, y in zip(h, h[1:])) and all(h[i] != h[i + k] for k in range(1, 13) for i in range(len(h) - k))
    assert sum(len(h) for h in want.values()) == sum(int((c.codes != 0).sum()) for c in calls)


def test_pyoracle_agrees_on_the_ladder():
    calls = rs.ladder()
    flows, table, pcfg = _oracle(calls), pyoracle.SessionTable(), _py_cfg()
    for c in calls:
        fr, of = rs.frames(c.flow, c.sym)
        pyoracle.run_batch(pcfg, fr, of, table=table)
    recs = flows.export_sorted()
    assert len(recs) == len(table.sessions)
    for r in recs:
        h, cs = flows.history(r)
        s = table.sessions[_key_of(r)]
        assert (h, cs) == (s["history"], s["conn_state"]) and int(r["hist_len"]) == len(h), (_key_of(r), h, s["history"])
