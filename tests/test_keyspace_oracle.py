"""The key-space helper (tests/keyspace.py) against what it restates, on the CPU: its hash against the
oracle's orc_flow_hash, the hash inverse, the property every key family claims, every corpus and
layout through the C oracle's table (one flow per distinct key, the six counters equal to plain dict
sums of the packet pattern, histories of the designed lengths), and check_placement on hand-made
placements.  tests/test_gpu_keyspace.py runs the same corpora through the GPU table."""
import ctypes as C

import numpy as np
import pytest

import keyspace as ks
from flodbadd_amd import _native as N
from oracle import coracle


def _orc_hash(words):
    w = np.ascontiguousarray(words, dtype="<u4").reshape(-1, 10)
    lib = coracle.lib()
    return np.array([lib.orc_flow_hash(C.c_void_p(w[i: i + 1].ctypes.data)) for i in range(len(w))], dtype=np.uint64)


def _all_corpus_keys():
    out = []
    for name, how in ks.CASES:
        c, calls = ks.calls_of(name, how)
        out += list(c.keys) + [ks.mirror(k) for k in c.keys]
    out.append(ks.corpus_g4()[1])
    return np.stack(out)


def test_flow_hash_equals_the_oracles():
    rng = np.random.default_rng(11)
    w = rng.integers(0, 1 << 32, size=(10000, 10), dtype=np.uint64).astype(np.uint32)
    w[:, 9] &= 0xFFFF
    assert (ks.flow_hash(w) == _orc_hash(w)).all()
    k = _all_corpus_keys()
    assert len(k) > 2000 and (ks.flow_hash(k) == _orc_hash(k)).all()


def test_solve_round_trips():
    rng = np.random.default_rng(12)
    targets = [0, (1 << 64) - 1] + [int(x) for x in rng.integers(0, 1 << 63, size=200, dtype=np.uint64) * 2 + 1] + \
              [int(x) for x in rng.integers(0, 1 << 63, size=200, dtype=np.uint64)]
    keys = rng.integers(0, 1 << 32, size=(len(targets), 10), dtype=np.uint64).astype(np.uint32)
    keys[:, 9] &= 0xFFFF
    for n, (k, H) in enumerate(zip(keys, targets)):
        pair = n % 4  # (not word 4: its upper 32 bits are not key material)
        s = ks.solve(k, pair, H)
        assert int(ks.flow_hash(s)[0]) == H and int(_orc_hash(s)[0]) == H
        other = [j for j in range(10) if j // 2 != pair]
        assert (s[other] == k[other]).all()


def test_f1_pairs_differ_in_one_word_and_share_partition_and_tag():
    got = ks.f1_all()
    assert len(got) == 4 * len(ks.F1_WORDS)
    for fam, a in ks.F1_WORDS:
        mine = [g for g in got if g[:2] == (fam, a)]
        assert len(mine) >= 4 and sum(g[4] for g in mine) == len(mine) // 2
    for fam, a, ka, kb, same in got:
        diff = np.flatnonzero(ka != kb)
        assert diff.size and set(diff // 2) == {a}
        assert (int(ka[9]) >> 8, int(kb[9]) >> 8) == (fam, fam)
        ha, hb = ks.flow_hash(ka)[0], ks.flow_hash(kb)[0]
        assert ks.part_of(ha, 4) == ks.part_of(hb, 4) and ks.tag_of(ha) == ks.tag_of(hb)
        if same:
            assert ks.h32_of(ha) == ks.h32_of(hb) and ks.home_of(ha) == ks.home_of(hb)
        else:
            assert ks.h32_of(ha) ^ ks.h32_of(hb) == 2 and abs(int(ks.home_of(ha)) - int(ks.home_of(hb))) == 2
            assert ks.home_of(ha) >> 3 == ks.home_of(hb) >> 3
    hot = ks.f1_hot()
    assert [a for a, _, _ in hot] == [0, 1, 2, 3, 4]
    for a, ka, kb in hot:
        ha, hb = ks.flow_hash(ka)[0], ks.flow_hash(kb)[0]
        assert set(np.flatnonzero(ka != kb) // 2) == {a} and ks.h32_of(ha) == ks.h32_of(hb) and ha != hb
        assert ks.part_of(ha, 32) == ks.part_of(hb, 32)


def test_f2_families_share_one_hash():
    fams = ks.f2_all()
    assert len(fams) == 3
    for fam, H in zip(fams, ks.F2_HASHES):
        assert len(fam) == 12 and len({ks.key_bytes(k) for k in fam}) == 12
        assert all(int(h) == H for h in ks.flow_hash(np.stack(fam)))
        assert all(set(np.flatnonzero(k != fam[0]) // 2) <= {1, 3} for k in fam)
    h = np.array(ks.F2_HASHES, dtype=np.uint64)
    for parts in (1, 4, 32):
        assert ks.part_of(h, parts).tolist() == [0, parts - 1, parts // 2]
    assert ks.home_of(h).tolist() == [0, 507, 250]
    for world in (2, 3):  # the merge's owner rank: one per family
        assert all(((int(H) >> 32) * world) >> 32 in range(world) for H in ks.F2_HASHES)


def test_f3_pairs_cross_the_families():
    pairs = ks.f3_pairs()
    assert len(pairs) >= 4
    for k4, k6 in pairs:
        assert (int(k4[9]) >> 8, int(k6[9]) >> 8) == (ks.V4, ks.V6) and not k4[1:4].any() and not k4[5:8].any()
        assert ks.flow_hash(k4)[0] == ks.flow_hash(k6)[0]


def test_geometry_families_have_the_homes_they_claim():
    occ, climb = ks.g1_ladder()
    homes = ks.home_of(ks.flow_hash(np.stack(occ))).tolist()
    assert len(occ) == 36 and len(climb) == 8
    want = [8 * g + q for r, g in enumerate(ks.G1_GROUPS) for q in range(r, 8)]
    assert homes == want
    assert ks.home_of(ks.flow_hash(np.stack(climb))).tolist() == [8 * g + r for r, g in enumerate(ks.G1_GROUPS)]
    assert sorted(ks.home_of(ks.flow_hash(np.stack(ks.g2_wrap()))).tolist()) == [509] * 3 + [510] * 3 + [511] * 2
    g3 = ks.flow_hash(np.stack(ks.g3_cluster()))
    assert len(g3) == 40 and set(ks.home_of(g3).tolist()) == {ks.G3_HOME}
    tags = ks.tag_of(g3).tolist()
    assert len(set(tags)) == 39 and tags[-1] == tags[-2] and g3[-1] != g3[-2]
    g4 = ks.flow_hash(np.stack(ks.g4_full()))
    assert len(g4) == 513 and set(ks.home_of(g4).tolist()) == {ks.G4_HOME} and len(set(ks.tag_of(g4).tolist())) == 513
    every = np.concatenate([ks.flow_hash(np.stack(x)) for x in (occ, climb, ks.g2_wrap(), ks.g3_cluster(), ks.g4_full())])
    for parts in (1, 4, 32):
        assert not ks.part_of(every, parts).any()


def test_hot_corpus_reaches_the_combine_threshold():
    """K1's rule on the host with the helper's own hash: every hot group's partition of the 32 holds at
    least max(64, 4 x the mean per partition) records of the one chunk."""
    c, calls = ks.calls_of("hot", "hot")
    call = calls[0]
    assert len(call) <= 20480
    part = ks.part_of(ks.flow_hash(np.stack([c.keys[i] for i, _, _, _ in call])), 32)
    cnt = np.bincount(part, minlength=32)
    need = max(64, 4 * ((len(call) + 31) // 32))
    hot_parts = {int(ks.part_of(ks.flow_hash(c.keys[g[0]]), 32)[0]) for g in c.groups}
    assert len(c.groups) == 6 and len(hot_parts) >= 2 and all(cnt[p] >= need for p in hot_parts), (cnt, need)
    _, counts = ks.corpus_hot()
    fam = c.groups[0]
    assert sorted(counts[i] for i in fam)[:2] == [1, ks.HOT_RECORDS] and len(fam) == 12


@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
@pytest.mark.parametrize("name,how", ks.CASES, ids=["%s-%s" % c for c in ks.CASES])
def test_oracle_holds_one_flow_per_key(name, how, timed):
    c, calls = ks.calls_of(name, how)
    ref, flows = ks.reference(name, how, timed)  # (asserts: every frame parses to its intended key)
    want = ks.expected(c, calls)
    rf = flows.export_sorted()
    assert len(rf) == len(want) == flows.count()
    assert len(want) == len(c.keys) * (2 if c.reverse else 1)
    rows = {bytes(r.tobytes()[:40]): r for r in rf}
    assert set(rows) == set(want)
    fields = ("outbound_bytes", "inbound_bytes", "orig_pkts", "resp_pkts", "orig_ip_bytes", "resp_ip_bytes")
    for k, e in want.items():
        r = rows[k]
        assert [int(r[f]) for f in fields] == e[:6], (k, e)
        h, _ = flows.history(r)
        assert len(h) == int(r["hist_len"]) == e[6], (k, h, e)
    # every key's pattern is its own: no two flows have the same (bytes, packets)
    sig = [(e[0], e[2]) for e in want.values()]
    assert len(set(sig)) == len(sig)
    assert sum(int(st[0]["new_sessions"]) for *_, st in ref) == len(want)


def _placed(keys, slots):
    fl = np.zeros(len(keys), dtype=N.FLOW_REC_DTYPE)
    raw = fl.view(np.uint8).reshape(len(fl), -1)
    for i, k in enumerate(keys):
        raw[i, :40] = np.frombuffer(ks.key_bytes(k), dtype=np.uint8)
    fl["slot"] = slots
    return fl


def test_check_placement_accepts_and_rejects():
    g2, g3 = ks.g2_wrap(), ks.g3_cluster()[:4]  # eight keys with homes 509..511 / four with home 300
    homes = ks.home_of(ks.flow_hash(np.stack(g2))).tolist()
    assert homes == [509, 510, 511, 509, 510, 511, 509, 510]
    good = _placed(g2 + g3, [509, 510, 511, 0, 1, 2, 3, 4, 300, 301, 302, 303])
    ks.check_placement(good, 1)
    ks.check_placement(good[::-1], 1)
    ks.check_placement(good[:0], 1)
    # the same keys in a 4-partition table: the F2 families sit in partitions 0, 3 and 2
    fams = ks.f2_all()
    f2 = _placed([fams[0][0], fams[0][1], fams[1][0], fams[1][1], fams[2][0]], [0, 1, 3 * 512 + 507, 3 * 512 + 508, 2 * 512 + 250])
    ks.check_placement(f2, 4)
    wrap = _placed(fams[1][:6], [3 * 512 + s for s in (507, 508, 509, 510, 511, 0)])
    ks.check_placement(wrap, 4)

    def rejects(fl, parts, what):
        with pytest.raises(AssertionError, match=what):
            ks.check_placement(fl, parts)

    hole = good.copy()
    hole["slot"][7] = 5  # slot 4 is empty now, before slot 5
    rejects(hole, 1, "empty slot before")
    hole = good.copy()
    hole["slot"][11] = 299  # before its home: the whole partition would have to be full
    rejects(hole, 1, "empty slot before")
    wrong = f2.copy()
    wrong["slot"][4] = 1 * 512 + 250
    rejects(wrong, 4, "partition")
    shared = good.copy()
    shared["slot"][9] = 300
    rejects(shared, 1, "share a slot")
    twice = _placed(g2 + g3 + [g3[0]], [509, 510, 511, 0, 1, 2, 3, 4, 300, 301, 302, 303, 304])
    rejects(twice, 1, "twice")
