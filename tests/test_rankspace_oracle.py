"""The reference for the placement corpora (tests/rankspace.py), pinned on the CPU: per-rank oracle
tables, exported per owner (orc_flows_export_merge[_map]) and merged (orc_flow_merge), give the
table ONE oracle table builds from the same packets in global order, byte for byte -- so a device
test that fails against either is a finding about the kernels.  The corpora must keep exercising the
merge's end rule: the counts below (flows that end, that live on more than one rank, whose merged
end_mask holds a bit the ending rank did not have) are asserted exactly, and mutations of the
records (char_call dropped, plain call numbers for a rank that skipped a call) and of the rule's
same-call term each break the comparison."""
import numpy as np
import pytest

import flagseq as fs
import rankspace as rs
from flodbadd_amd import _native as N
from oracle import coracle

PAIR_IDS = {fs.ONE_SVC: "one_svc", fs.TWO_SVC: "two_svc", fs.NO_SVC: "no_svc"}
NONE = np.uint64(N.FB_SEEN_NONE)


def _borrowed(ref, exports):
    """Flows whose merged end_mask holds a bit that their ending rank's own record did not."""
    n = 0
    for o in range(ref.world):
        recv = rs.received(exports, o)
        merged = coracle.flow_merge(recv)
        keys, inv = np.unique(rs.key_ids(recv), return_inverse=True)
        inv = inv.ravel()
        end = recv["rec"]["end_seen"]
        e_key = np.full(len(keys), NONE, dtype=np.uint64)
        np.minimum.at(e_key, inv, end)
        is_end = (end != NONE) & (end == e_key[inv])
        own = np.zeros(len(keys), dtype=np.uint8)
        own[inv[is_end]] = recv["rec"]["end_mask"][is_end]
        assert np.bincount(inv[is_end], minlength=len(keys)).max() <= 1  # global positions are distinct
        m = merged[np.argsort(rs.key_ids(merged))]
        assert (rs.key_ids(m) == keys).all()
        n += int(((m["end_mask"] & ~own) != 0).sum())
    return n


# corpus, pair -> flows, borrowed (and for triples / ONE_SVC: ended, on more than one rank, conn_state 4)
COUNTS = {("triples", fs.ONE_SVC): (229376, 24942), ("triples", fs.TWO_SVC): (334208, 13185),
          ("pairs", fs.ONE_SVC): (163840, 5376), ("pairs", fs.TWO_SVC): (225280, 2304),
          ("pairs", fs.NO_SVC): (245760, 2304)}


@pytest.mark.parametrize("corpus,pair", list(COUNTS), ids=["%s-%s" % (c, PAIR_IDS[p]) for c, p in COUNTS])
def test_oracle_chain_equals_single_table(corpus, pair):
    ref = rs.reference(corpus, pair)
    world, batches = rs.GEOMETRY[corpus]
    assert ref.world == world and len(ref.calls) == batches
    exports = ref.exports()
    single = ref.single.export_sorted()
    assert rs.rows(ref.union(exports)).tobytes() == rs.rows(single).tobytes()
    flows, borrowed = COUNTS[corpus, pair]
    assert len(single) == flows
    assert _borrowed(ref, exports) == borrowed
    if (corpus, pair) == ("triples", fs.ONE_SVC):
        assert int((single["end_seen"] != NONE).sum()) == 188552
        allrecs = np.concatenate([m for m, _ in exports])
        _, per_key = np.unique(rs.key_ids(allrecs), return_counts=True)
        assert int((per_key > 1).sum()) == 180224
        assert int((single["conn_state"] == 4).sum()) == 112
        assert (single["hist_len"] == 3).all()
    # every (batch, rank) cell holds packets: no rank skips a call, call k is global batch k
    assert all(c is not None for row in ref.calls for c in row)


def test_corpus_sizes():
    for corpus, maps, flows, frames in (("triples", 56, 229376, 688128), ("pairs", 10, 163840, 327680)):
        world, batches = rs.GEOMETRY[corpus]
        seq = rs.sequences(corpus)
        m = rs.placement_maps(world, batches, seq.shape[1])
        assert len(m) == maps and (np.diff(m.astype(np.int64), axis=1) >= 0).all()
        assert len(np.unique(m, axis=0)) == maps
        shards, cmaps = rs.placed(corpus)
        assert sum(len(b[0]) for row in shards for b in row) == frames == flows * seq.shape[1]
        allf = np.concatenate([b[1] for row in shards for b in row])
        assert int(allf.max()) == flows - 1
        for k, row in enumerate(shards):  # the call map: global batch << 32 | the lower ranks' shard sizes
            start = 0
            for r, b in enumerate(row):
                assert cmaps[r][k] == (k << 32) | start
                start += len(b[0])
                assert (np.diff(b[2].astype(np.int64)) >= 0).all()  # position-major inside a shard


def test_placement_keeps_a_flows_packet_order():
    """Global order (batch, rank, place in the shard) visits every flow's positions in order."""
    shards, _ = rs.placed("triples", flows=np.arange(0, 229376, 37))
    flow = np.concatenate([rs.global_batch(row)[1] for row in shards]).astype(np.int64)
    pos = np.concatenate([rs.global_batch(row)[2] for row in shards]).astype(np.int64)
    order = np.argsort(flow, kind="stable")
    assert (pos[order].reshape(-1, 3) == np.arange(3)).all()


def test_hot_placement_chain_equals_single_table():
    """The shard_first form of the export (no call map) on the hot flows cut into two shards."""
    ref = rs.reference("hot", fs.ONE_SVC)
    assert ref.shard_firsts == [0, 11666] and len(ref.calls) == 3
    for row in ref.calls:  # rank 1's shard starts where shard_first says, in every batch
        assert row[1][2] == 11666 == len(row[0][1]) - 1
    single = ref.single.export_sorted()
    assert rs.rows(ref.union()).tobytes() == rs.rows(single).tobytes()
    assert len(single) == 48 and sorted(single["hist_len"].tolist()) == sorted(fs.HOT_LENGTHS)
    assert (single["end_seen"] != NONE).all()


def test_skipped_call_chain_equals_single_table():
    """The triples that put no packet on rank 1 in global batch 0: rank 1's only call is global batch
    1, so its positions and char_call come out right only through the call map."""
    ref = rs.reference("triples", fs.ONE_SVC, "skip")
    assert ref.calls[0][1] is None and all(c is not None for c in ref.calls[1])
    assert ref.call_maps[1] == [(1 << 32) | len(ref.calls[1][0][1]) - 1]
    exports = ref.exports()
    single = ref.single.export_sorted()
    assert len(single) == 229376 * 35 // 56
    assert rs.rows(ref.union(exports)).tobytes() == rs.rows(single).tobytes()
    m = exports[1][0]
    assert ((m["char_call"] == 1).any(axis=1)).any() and not (m["char_call"] == 0).any()
    assert _borrowed(ref, exports) > 0
    # the plain numbering (call 0 = global batch 0) gives another table
    renumber = lambda cm: [k << 32 | (e & 0xFFFFFFFF) for k, e in enumerate(cm)]  # noqa: E731
    plain = [ref.ranks[r].export_merge(ref.world, r, call_map=renumber(ref.call_maps[r])) for r in range(ref.world)]
    assert rs.rows(ref.union(plain)).tobytes() != rs.rows(single).tobytes()


def test_growth_layout_chain_equals_single_table():
    ref = rs.reference("triples", fs.ONE_SVC, "growth")
    assert len(ref.calls) == len(rs.RAMP) + 2 + len(rs.RAMP_FILL)
    single = ref.single.export_sorted()
    assert rs.rows(ref.union()).tobytes() == rs.rows(single).tobytes()
    assert len(single) == 229376 + 3 * (sum(rs.RAMP) + sum(rs.RAMP_FILL))


def test_purge_layout_chain_equals_single_table():
    """Timed tables under rankspace.purge_times (no gap reaches the segment timeout): the merged
    fb_flow_rec rows equal the single timed table's, and the clock splits the flows as the purge test
    needs -- a rank's stale flows after global batch 0 never come back to it."""
    ref = rs.reference("triples", fs.ONE_SVC, "purge")
    single = ref.single.export_sorted()
    assert rs.rows(ref.union()).tobytes() == rs.rows(single).tobytes()
    now = rs.T0 + 2 * rs.DAY_NS + 100 * 10 ** 9
    stale_all = set()
    for r in range(ref.world):
        recs, times, _ = ref.after_first[r]
        stale = recs[now > times["last_activity_ns"].astype(np.int64) + rs.DAY_NS]
        assert 0 < len(stale) < len(recs)
        later = ref.calls[1][r][4]
        assert not np.isin(rs.key_ids(stale), rs.key_ids(later)).any()
        stale_all |= {k.tobytes() for k in rs.key_ids(stale)}
    t = ref.single.export_times()
    gone = single[now > t["last_activity_ns"].astype(np.int64) + rs.DAY_NS]
    assert {k.tobytes() for k in rs.key_ids(gone)} == stale_all


def _mutated_union(ref, mutate):
    exports = ref.exports()
    return np.concatenate([mutate(rs.received(exports, o)) for o in range(ref.world)])


def test_mutation_char_call_dropped():
    """Every non-ending record's char_call set to FB_CALL_NONE: the union differs from the single table."""
    ref = rs.reference("triples", fs.ONE_SVC)

    def mutate(recv):
        recv = recv.copy()
        _, inv = np.unique(rs.key_ids(recv), return_inverse=True)
        inv = inv.ravel()
        e_key = np.full(int(inv.max()) + 1, NONE, dtype=np.uint64)
        np.minimum.at(e_key, inv, recv["rec"]["end_seen"])
        ending = (recv["rec"]["end_seen"] != NONE) & (recv["rec"]["end_seen"] == e_key[inv])
        recv["char_call"][~ending] = N.FB_CALL_NONE
        return coracle.flow_merge(recv)

    single = rs.rows(ref.single.export_sorted())
    got = rs.rows(_mutated_union(ref, mutate))
    assert len(got) == len(single) and got.tobytes() != single.tobytes()
    # only end_mask and conn_state change: a stale char_call is silent everywhere else
    for f in single.dtype.names:
        same = np.array_equal(got[f], single[f])
        assert same == (f not in ("end_mask", "conn_state")), f


# flows of triples / ONE_SVC whose end_mask changes under each restated rule
RULE_DIFFERS = {"rule": 0, "lower_or_equal_rank": 0, "higher_rank": 35184, "earlier_call_only": 13152,
                "any_rank_in_the_call": 22320}


@pytest.mark.parametrize("rule", rs.RULES)
def test_mutation_same_call_term(rule):
    """The numpy restatement of the end rule (the ending record skipped, as k_mg_before and
    orc_flow_merge skip it) reproduces the oracle's end_mask.  `rank <= r0` for `rank < r0` is the
    same rule there -- only the ending record has rank == r0 -- so it reproduces it too; the corpus
    pins the tie-break through the mutations that do change the rule: the higher ranks instead of the
    lower ones, no same-call term, any rank of the end's call.  Each of those gives another table."""
    ref = rs.reference("triples", fs.ONE_SVC)
    single = ref.single.export_sorted()
    differ = []

    def mutate(recv):
        merged = coracle.flow_merge(recv)
        keys, mask = rs.end_mask_by_rule(recv, rule)
        order = np.argsort(rs.key_ids(merged))
        idx = order[np.searchsorted(rs.key_ids(merged)[order], keys)]
        assert (rs.key_ids(merged)[idx] == keys).all()
        differ.append(int((merged["end_mask"][idx] != mask).sum()))
        merged["end_mask"][idx] = mask
        return merged

    got = rs.rows(_mutated_union(ref, mutate))
    print("%s: %d flows differ" % (rule, sum(differ)))
    assert (got.tobytes() == rs.rows(single).tobytes()) == (rule in ("rule", "lower_or_equal_rank"))
    assert sum(differ) == RULE_DIFFERS[rule]
