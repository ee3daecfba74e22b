"""Placement corpora for the cross-rank ordered state (test helper, no tests): the flag sequences of
tests/flagseq.py, each placed on W ranks x K global batches in every way, so a rank / call order that
the merge (fb_merge.hip) or the routing decides wrongly has a flow that shows it.

A cell is (global batch k, rank r), numbered k * W + r: increasing cell number is global packet
order (global batch k is the ranks' shards of it, concatenated in rank order).  A placement of an
L-symbol sequence is a non-decreasing map of its positions to cells -- the C(W * K + L - 1, L)
tuples of itertools.combinations_with_replacement(range(W * K), L), in that order.  A corpus is
sequence x placement, one flow each: flow id = sequence index * n_maps + map index.

  triples  all 16^3 sequences over flagseq.ALPHABET16, W = 3, K = 2: 56 maps, 229,376 flows,
           688,128 frames (three symbols: a first S / s / H / h, the end, a second end elsewhere)
  pairs    all 128^2 two-symbol sequences, W = 2, K = 2: 10 maps, 163,840 flows, 327,680 frames
  hot      flagseq.hot_batches(), each batch cut into W = 2 contiguous shards at the same index
           (the shard_first form of the export: no call map)

`Reference` runs a placed corpus through the oracle both ways -- ONE table fed the global batches,
and one table per rank fed its shards (a rank makes no call for an empty shard), exported per owner
and merged -- and keeps every shard's frames for the device tests.  It is computed once per case
(`reference`) and read-only for the tests."""
import functools
import itertools

import numpy as np

import flagseq as fs
from flodbadd_amd import _native as N
from flodbadd_amd.distributed import call_map_entry, shard_range, sort_by_ord
from oracle import coracle

GEOMETRY = {"triples": (3, 2), "pairs": (2, 2), "hot": (2, 3)}  # corpus -> (W ranks, K global batches)
DAY_NS = 86400 * 10 ** 9
T0 = fs.BASE_NS


def sequences(corpus):
    if corpus == "pairs":
        return fs.pairs_seq()
    if corpus == "triples":
        a = np.arange(16 ** 3)
        return fs.ALPHABET16[np.stack([(a >> 8) & 15, (a >> 4) & 15, a & 15], axis=1)]
    raise ValueError(corpus)


def placement_maps(world, batches, length):
    """[n_maps, length]: every non-decreasing map of `length` positions to world * batches cells."""
    return np.array(list(itertools.combinations_with_replacement(range(world * batches), length)), dtype=np.uint32)


def call_maps_of(shards):
    """Per rank, call_map_entry(global batch, shard start) of every non-empty shard: the shard start
    is the sum of the lower ranks' shard sizes in that batch."""
    cmaps = [[] for _ in shards[0]]
    for k, row in enumerate(shards):
        start = 0
        for r, (sym, _, _) in enumerate(row):
            if len(sym):
                cmaps[r].append(call_map_entry(k, start))
            start += len(sym)
    return cmaps


def placed(corpus, flows=None):
    """-> (shards, call_maps): shards[k][r] = rank r's shard of global batch k as a flagseq batch
    (sym, flow, pos), position-major inside the shard; call_maps[r] = that rank's export call map.
    flows: the flow ids to keep (default: the whole corpus)."""
    world, batches = GEOMETRY[corpus]
    seq = sequences(corpus)
    length = seq.shape[1]
    maps = placement_maps(world, batches, length)
    ids = np.arange(len(seq) * len(maps), dtype=np.uint32) if flows is None else np.asarray(flows, dtype=np.uint32)
    assert len(ids) and int(ids.max()) < len(seq) * len(maps) < 1 << 24
    sym = np.ascontiguousarray(seq[ids // len(maps)].T).reshape(-1)   # position-major
    cell = np.ascontiguousarray(maps[ids % len(maps)].T).reshape(-1)
    flow = np.tile(ids, length)
    pos = np.repeat(np.arange(length, dtype=np.uint32), len(ids))
    shards = []
    for k in range(batches):
        row = []
        for r in range(world):
            m = cell == k * world + r
            row.append((sym[m], flow[m], pos[m]))
        shards.append(row)
    return shards, call_maps_of(shards)


def flows_avoiding(corpus, cell):
    """The ids of the corpus's flows whose placement puts no packet into `cell`: placed(corpus,
    flows=...) then has an empty shard there, the rank makes no call for it, and its later calls
    are numbered one below their global batches (what the export's call map is for)."""
    world, batches = GEOMETRY[corpus]
    seq = sequences(corpus)
    maps = placement_maps(world, batches, seq.shape[1])
    ids = np.arange(len(seq) * len(maps), dtype=np.uint32)
    return ids[~(maps == cell).any(axis=1)[ids % len(maps)]]


def filler_row(first_flow, n, world):
    """One more global batch of n new flows (ids from first_flow), one ACK-only packet each, cut
    into `world` contiguous shards."""
    assert first_flow + n <= 1 << 24
    flow = np.arange(first_flow, first_flow + n, dtype=np.uint32)
    sym = np.full(n, fs.ACK, dtype=np.uint8)
    pos = np.zeros(n, dtype=np.uint32)
    row = []
    for r in range(world):
        a, c = shard_range(n, r, world)
        row.append((sym[a: a + c], flow[a: a + c], pos[a: a + c]))
    return row


# The growth layout.  A table grows BEFORE an update call, from the last completed call's report: it
# is sized for the flows it holds plus twice that call's new flows (maybe_grow, fb_capi.hip), and a
# call that brings more than a partition has room for reports FB_ERR_TABLE_FULL.  So a table that
# starts at 2^12 slots is led up to the corpus by ramp batches that double (768 new flows per rank,
# then 1,536, ... 49,152: each call brings exactly what the last one announced, and the last one
# announces more than a corpus call brings), and the filler after the corpus is three batches:
# 30,000 and 60,000 new flows per rank (again what was announced), then 64, whose growth decision
# sees the rank's ~335,000 flows + 2 x 60,000 against 3/4 of the 2^19 slots the corpus left.
RAMP = [768 << j for j in range(7)]
RAMP_FILL = [30_000, 60_000, 64]


def growth_rows(shards):
    """Global batches of ACK-only flows (ids above the corpus) around a placed corpus: len(RAMP)
    ramp batches before it, len(RAMP_FILL) filler batches after it; the sizes are per rank.
    -> (shards, call_maps)."""
    world = len(shards[0])
    nxt = 1 + max(int(b[1].max()) for row in shards for b in row if len(b[1]))
    head, tail = [], []
    for dst, sizes in ((head, RAMP), (tail, RAMP_FILL)):
        for per_rank in sizes:
            dst.append(filler_row(nxt, per_rank * world, world))
            nxt += per_rank * world
    out = head + shards + tail
    return out, call_maps_of(out)


def hot_placed():
    """-> (shards, shard_firsts): flagseq.hot_batches() cut into contiguous shards.  The export's
    shard_first form assumes that rank r's shard starts at the same index in every global batch, and
    the three batches are not equally long (23,333 / 23,333 / 23,334 frames), so the starts are
    shard_range's of the shortest batch and the last rank takes the rest of each."""
    world, _ = GEOMETRY["hot"]
    batches = fs.hot_batches()
    firsts = [shard_range(min(len(b[0]) for b in batches), r, world)[0] for r in range(world)]
    shards = []
    for b in batches:
        ends = firsts[1:] + [len(b[0])]
        shards.append([tuple(x[a:e] for x in b) for a, e in zip(firsts, ends)])
    return shards, firsts


def global_batch(row):
    """The ranks' shards of one global batch, concatenated in rank order."""
    return tuple(np.concatenate(x) for x in zip(*row))


def purge_times(shards):
    """Capture times per global batch for the purge tests: the flows with an odd id whose every
    packet is in global batch 0 are captured at T0, everything else two days later; inside a batch
    the packets are 1 us apart in global order (no gap reaches the 5-s segment timeout)."""
    late = np.zeros(1 << 24, dtype=bool)
    for row in shards[1:]:
        late[global_batch(row)[1]] = True
    out = []
    for k, row in enumerate(shards):
        flow = global_batch(row)[1]
        old = ((flow & 1) == 1) & ~late[flow]
        t = T0 + np.where(old, 0, 2 * DAY_NS) + k * 10 ** 9 + np.arange(len(flow), dtype=np.int64) * 1000
        out.append(t.astype(np.uint64))
    return out


def key_bytes(a):
    """[n, 40] uint8: the session keys of any record array whose first 40 bytes are the key."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), a.dtype.itemsize)[:, :40]


def key_ids(a):
    """The keys as one V40 scalar per record (np.unique / np.isin / dict keys via .tobytes())."""
    return np.ascontiguousarray(key_bytes(a)).view("V40").ravel()


def rows(a):
    """fb_flow_rec records in Session's Ord with the table placement zeroed: what two tables that
    hold the same flows compare equal on."""
    a = sort_by_ord(np.ascontiguousarray(a).copy())
    a["slot"] = 0
    return a


def by_key(a):
    """Records sorted by their key bytes (a group's order is the exporter's own: slot order on the
    device, Ord in the oracle)."""
    a = np.ascontiguousarray(a)
    return a[np.lexsort(key_bytes(a).T[::-1])] if len(a) else a


def groups_of(mrecs, counts):
    """An export's records split into its owner groups."""
    ends = np.cumsum(np.asarray(counts, dtype=np.int64))
    return [mrecs[int(e - c): int(e)] for e, c in zip(ends, np.asarray(counts, dtype=np.int64))]


def received(exports, owner):
    """What `owner` receives: every rank's group `owner`, in rank order."""
    return np.concatenate([groups_of(m, c)[owner] for m, c in exports])


class Reference:
    """A placed corpus through the oracle.  shards[k][r]: flagseq batches; ts: capture times per
    global batch (timed tables) or None.  Per shard it keeps (frames, offsets, shard start, times,
    records, the rank table's batch stats) in .calls[k][r] (None for an empty shard) with the high
    flag bits zero; the single table is fed the global batches with the high flag bits drawn
    (hi_seed=5), which must change nothing.  snapshot_first (timed tables): keep every rank's table
    as it stands once global batch 0 is in (.after_first)."""

    def __init__(self, shards, pair, call_maps=None, shard_firsts=None, ts=None, snapshot_first=False):
        assert (call_maps is None) != (shard_firsts is None)
        self.world, self.pair, self.timed = len(shards[0]), pair, ts is not None
        self.call_maps, self.shard_firsts = call_maps, shard_firsts
        cfg = coracle.make_cfg(2)
        self.single, self.ranks = coracle.Flows(), [coracle.Flows() for _ in range(self.world)]
        self.calls, self.global_calls, self.new_sessions = [], [], 0
        self.after_first = None  # per rank (flow rows, time rows, export for one owner) after global batch 0
        for k, row in enumerate(shards):
            g = global_batch(row)
            fr, of = fs.frames(g, pair, hi_seed=5)
            recs = coracle.parse_classify(cfg, fr, of)[0]
            assert len(recs) == len(of) - 1  # every frame is a session packet
            st = np.zeros(1, dtype=N.STATS_DTYPE)
            self.single.update(recs, st, ts=None if ts is None else ts[k])
            self.new_sessions += int(st[0]["new_sessions"])
            self.global_calls.append((recs, None if ts is None else ts[k]))
            start, out = 0, []
            for r, b in enumerate(row):
                n = len(b[0])
                if n == 0:
                    out.append(None)
                    continue
                sfr, sof = fs.frames(b, pair, hi_seed=None)
                srecs = coracle.parse_classify(cfg, sfr, sof)[0]
                t = None if ts is None else np.ascontiguousarray(ts[k][start: start + n])
                sst = np.zeros(1, dtype=N.STATS_DTYPE)
                self.ranks[r].update(srecs, sst, ts=t)
                for a in (sfr, sof, srecs, sst) + (() if t is None else (t,)):
                    a.setflags(write=False)
                out.append((sfr, sof, start, t, srecs, sst))
                start += n
            self.calls.append(out)
            if k == 0 and snapshot_first:
                self.after_first = [(f.export_sorted(), f.export_times(), self.export(r, 1)[0])
                                    for r, f in enumerate(self.ranks)]

    def export(self, rank, world=None):
        """The oracle's export of rank `rank` for `world` owners -> (mrecs, counts)."""
        world = world or self.world
        if self.call_maps is not None:
            return self.ranks[rank].export_merge(world, rank, call_map=self.call_maps[rank])
        return self.ranks[rank].export_merge(world, rank, self.shard_firsts[rank])

    def exports(self, world=None):
        return [self.export(r, world) for r in range(self.world)]

    def union(self, exports=None):
        """Every owner's oracle merge of what it receives, concatenated."""
        exports = exports or self.exports()
        return np.concatenate([coracle.flow_merge(received(exports, o)) for o in range(len(exports[0][1]))])


@functools.lru_cache(maxsize=2)
def reference(corpus, pair, variant=""):
    """One Reference per case, shared by the tests of a module.  variant: "" (untimed), "timed"
    (flagseq.times over the global batches), "purge" (purge_times), "growth" (growth_rows), "skip"
    (the flows that avoid cell 1: rank 1 makes no call for global batch 0)."""
    if corpus == "hot":
        shards, firsts = hot_placed()
        return Reference(shards, pair, shard_firsts=firsts)
    shards, cmaps = placed(corpus, flows=flows_avoiding(corpus, 1) if variant == "skip" else None)
    ts = None
    if variant == "growth":
        shards, cmaps = growth_rows(shards)
    elif variant == "timed":
        ts = fs.times([global_batch(row) for row in shards], seed=9)
    elif variant == "purge":
        ts = purge_times(shards)
    else:
        assert variant in ("", "skip")
    return Reference(shards, pair, call_maps=cmaps, ts=ts, snapshot_first=variant == "purge")


RULES = ("rule", "lower_or_equal_rank", "higher_rank", "earlier_call_only", "any_rank_in_the_call")


def end_mask_by_rule(recv, rule="rule"):
    """A numpy restatement of the merge's end rule (k_mg_end / k_mg_before, orc_flow_merge) over one
    owner's received records -> (keys V40, end_mask) per ended key: the record with the key's
    smallest end_seen is the ending one and gives its own end_mask and nothing else; every other
    record gives those of S s H h whose first call c precedes the end packet: c < call_e, or
    c == call_e on a rank below the ending one, r0.  The other `rule`s change the same-call term:
      lower_or_equal_rank    rank <= r0 -- the SAME rule: a key has one record per rank, so only the
                             ending record has rank == r0, and the rule never sees it
      higher_rank            rank > r0
      earlier_call_only      no same-call term
      any_rank_in_the_call   c <= call_e"""
    recv = np.ascontiguousarray(recv)
    keys, inv = np.unique(key_ids(recv), return_inverse=True)
    inv = inv.ravel()
    end = recv["rec"]["end_seen"]
    e_key = np.full(len(keys), N.FB_SEEN_NONE, dtype=np.uint64)
    np.minimum.at(e_key, inv, end)
    ended = e_key[inv] != np.uint64(N.FB_SEEN_NONE)
    is_end = ended & (end == e_key[inv])
    r0 = np.zeros(len(keys), dtype=np.int64)
    r0[inv[is_end]] = recv["rec"]["slot"][is_end]
    call_e = (e_key >> np.uint64(32)).astype(np.int64)[inv]
    rank = recv["rec"]["slot"].astype(np.int64)
    same = {"rule": rank < r0[inv], "lower_or_equal_rank": rank <= r0[inv], "higher_rank": rank > r0[inv],
            "earlier_call_only": np.zeros(len(recv), dtype=bool),
            "any_rank_in_the_call": np.ones(len(recv), dtype=bool)}[rule]
    bits = np.zeros(len(recv), dtype=np.uint8)
    for b in range(4):
        c = recv["char_call"][:, b].astype(np.int64)
        ok = (recv["char_call"][:, b] != N.FB_CALL_NONE) & ((c < call_e) | ((c == call_e) & same))
        bits |= (ok.astype(np.uint8) << b)
    contrib = np.where(is_end, recv["rec"]["end_mask"], bits)  # (the ending record is not put to the rule)
    contrib[~ended] = 0
    mask = np.zeros(len(keys), dtype=np.uint8)
    np.bitwise_or.at(mask, inv, contrib)
    sel = e_key != np.uint64(N.FB_SEEN_NONE)
    return keys[sel], mask[sel]
