"""Capture-time corpora for the timed session state (test helper, no tests): where tests/flagseq.py
enumerates the flag sequences of a flow and draws the gaps between its packets, these enumerate the
GAPS -- both sides of the 5-s segment timeout to the nanosecond, the last instant that still
truncates to 5000 ms, a long pause, and three steps backwards -- together with the one flag that the
segment state machine reads (PSH), over every four-packet flow, and they place long and short runs
where the fused pass of flodbadd_amd/csrc/fb_time.hip changes code path: a run's position 0, 1 and
2+, thread (4 items), wave (256) and tile (2,048) boundaries, and more tiles than one look-back
window (64).

A symbol is P << 3 | gap class: P selects PSH|ACK against ACK (both with 6 B of payload), the gap
class the time since the flow's previous packet (GAPS_NS).  Flow f's first packet is at BASE_NS +
f ms, so start_time_ns names the flow; the time of a packet is a function of (flow, position)
alone, whatever the layout, the cuts and the replica.

A batch (one update call) is a Batch of equally long arrays in frame order: flags (a flagseq symbol:
the TCP flag bits and flagseq.PAY), flow, pos, t (capture time, ns, indexed by the frame's place in
the batch) and udp.  TCP frames come from flagseq.frames (flow f is 10.(f >> 16).(f >> 8).(f) port
49152 -> 93.184.216.34 port 443, never swapped), UDP frames from one framegen.udp_frame template."""
import collections

import numpy as np

import flagseq as fs
import framegen as fg

BASE_NS = fs.BASE_NS
GAPS_NS = np.array([1_000_000, 4_999_999_999, 5_000_000_000, 5_000_999_999, 12_000_000_000,
                    -1_000_000_000, -500_000, -5_000_000_000], dtype=np.int64)
N_SYMBOLS = 16
A_, P_ = fs.PAY | fs.ACK, fs.PAY | fs.PSH | fs.ACK
PAIR = fs.ONE_SVC
TILE, WAVE_ITEMS, THREAD_ITEMS, WINDOW = 2048, 256, 4, 64  # fb_time.hip: kRunTile, 64 x kRunItems, kRunItems, lookback

Batch = collections.namedtuple("Batch", "flags flow pos t udp")


class Corpus:
    """Flows as flat per-packet arrays in (flow, pos) order: flags (flagseq symbols), gap (ns before
    the packet, 0 at pos 0), and the capture times that follow from them."""

    def __init__(self, flow, pos, flags, gap, udp=False):
        self.flow = np.ascontiguousarray(flow, dtype=np.uint32)
        self.pos = np.ascontiguousarray(pos, dtype=np.uint32)
        self.flags = np.ascontiguousarray(flags, dtype=np.uint8)
        self.udp = bool(udp)
        gap = np.where(self.pos == 0, 0, np.asarray(gap, dtype=np.int64))
        f, p = self.flow.astype(np.int64), self.pos.astype(np.int64)
        assert ((p == 0) | ((np.r_[-1, f[:-1]] == f) & (np.r_[-1, p[:-1]] + 1 == p))).all(), "positions 0..L-1 per flow"
        assert (np.diff(f) >= 0).all()
        c = np.cumsum(gap)
        head = np.maximum.accumulate(np.where(p == 0, np.arange(len(f)), 0))
        self.t = (BASE_NS + f * 1_000_000 + (c - c[head])).astype(np.uint64)
        self.n_flows = int((p == 0).sum())
        self.lengths = np.diff(np.r_[np.flatnonzero(p == 0), len(f)])

    def batch(self, ix):
        ix = np.asarray(ix, dtype=np.intp)
        return Batch(self.flags[ix], self.flow[ix], self.pos[ix], self.t[ix], np.full(len(ix), self.udp))

    def rows(self):
        """Per flow (P of each packet, time of each packet) as Python lists, for `sim`."""
        P = ((self.flags & fs.PSH) != 0) & (not self.udp)
        cuts = np.r_[np.flatnonzero(self.pos == 0), len(self.pos)]
        return [(P[a:b].tolist(), self.t[a:b].astype(np.int64).tolist()) for a, b in zip(cuts[:-1], cuts[1:])]


def _enumerated(flags, gap, flow0=0, udp=False):
    """[F, L] flag symbols and gaps -> Corpus, flows flow0..flow0 + F - 1."""
    F, L = flags.shape
    f, p = np.meshgrid(np.arange(flow0, flow0 + F), np.arange(L), indexing="ij")
    return Corpus(f.reshape(-1), p.reshape(-1), flags.reshape(-1), gap.reshape(-1), udp)


def symbols(sym):
    """Symbols (P << 3 | gap class) -> (flagseq symbols, gaps in ns)."""
    sym = np.asarray(sym)
    return np.where(sym & 8, P_, A_).astype(np.uint8), GAPS_NS[sym & 7]


def quads_seq():
    """Every four-symbol sequence, the first symbol's P alone (its gap class is 0): [8192, 4]."""
    a = np.arange(2 * 16 ** 3)
    return np.stack([((a >> 12) & 1) << 3, (a >> 8) & 15, (a >> 4) & 15, a & 15], axis=1).astype(np.uint8)


def quads():
    """2 x 16^3 = 8,192 TCP flows of 4 packets, flows 0..8191."""
    return _enumerated(*symbols(quads_seq()))


UDP_FLOW0 = 1 << 20


def udp_triples():
    """The 8^3 gap triples on UDP flows of 4 packets (no PSH: the timeout is the only segment end),
    flows UDP_FLOW0.. (disjoint from every replica of quads)."""
    a = np.arange(8 ** 3)
    cls = np.stack([a * 0, (a >> 6) & 7, (a >> 3) & 7, a & 7], axis=1)
    return _enumerated(np.zeros(cls.shape, dtype=np.uint8), GAPS_NS[cls], flow0=UDP_FLOW0, udp=True)


END_FLAGS = np.array([fs.ACK, fs.PSH | fs.ACK, fs.FIN | fs.ACK, fs.RST, fs.FIN | fs.PSH | fs.ACK], dtype=np.uint8) | fs.PAY
END_GAPS_NS = np.array([1_000_000, 5_000_000_000, -1_000_000_000], dtype=np.int64)


def ends_seq():
    """[16875, 4, 2]: (flag class 0..4, gap class 0..2) of every length-4 sequence, the first
    packet's flag class alone."""
    a = np.arange(5 * 15 ** 3)
    s = np.stack([(a // 15 ** 3) * 3, (a // 225) % 15, (a // 15) % 15, a % 15], axis=1)
    return np.stack([s // 3, s % 3], axis=2)


def ends():
    """5 x 15^3 = 16,875 TCP flows over ACK, PSH|ACK, FIN|ACK, RST, FIN|PSH|ACK x {1 ms, 5 s, -1 s}:
    end_time_ns is the time of the first FIN / RST in packet order, whatever the later ones carry."""
    s = ends_seq()
    return _enumerated(END_FLAGS[s[..., 0]], END_GAPS_NS[s[..., 1]])


SHIM_FLOW0 = 1 << 19


def shims(n=4096, seed=11):
    """n TCP flows of 1-3 packets (symbols drawn over all 16), flows SHIM_FLOW0..: every other corpus
    here has flows of exactly 4 packets, which alone would start every run on a thread's first item."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 4, size=n)
    flow = np.repeat(np.arange(SHIM_FLOW0, SHIM_FLOW0 + n), lens)
    pos = np.arange(len(flow)) - np.repeat(np.r_[0, np.cumsum(lens)[:-1]], lens)
    fl, gap = symbols(rng.integers(0, N_SYMBOLS, size=len(flow)))
    return Corpus(flow, pos, fl, gap)


def replicate(c, replicas):
    """The corpus `replicas` times under disjoint flow ids (replica r: + r x the corpus's flow span);
    the gaps repeat, the times follow the flow ids."""
    if replicas == 1:
        return c
    span = int(c.flow.max()) - int(c.flow.min()) + 1
    gap = np.r_[0, np.diff(c.t.astype(np.int64))]  # (pos 0 is zeroed by Corpus)
    r = np.repeat(np.arange(replicas, dtype=np.uint32), len(c.flow))
    tile = lambda a: np.tile(a, replicas)  # noqa: E731
    return Corpus(tile(c.flow) + r * span, tile(c.pos), tile(c.flags), tile(gap), c.udp)


def layout(c, cutmask, replicas=1):
    """Corpus -> list of Batches: bit k of cutmask puts an update-call boundary before position k + 1;
    each call is position-major (a flow's packets are a whole corpus of flows apart)."""
    c = replicate(c, replicas)
    call = np.r_[0, np.cumsum([(int(cutmask) >> k) & 1 for k in range(int(c.pos.max()))])][c.pos]
    out = []
    for k in range(int(call.max()) + 1):
        ix = np.flatnonzero(call == k)
        out.append(c.batch(ix[np.lexsort((c.flow[ix], c.pos[ix]))]))
    return out


def stagger(c, sizes, seed=41):
    """Corpus -> (list of Batches, group of every packet's flow per Batch): the flows are dealt at
    random into groups of `sizes` flows, and group g's position p goes into call g + p -- every
    packet of a flow in a call of its own, as under cut mask 0b111, while each call also inserts a
    new group (a table that doubles as the groups do then grows between a flow's packets)."""
    ids = np.unique(c.flow)
    assert sum(sizes) == len(ids)
    grp_of = np.zeros(len(ids), dtype=np.int64)
    grp_of[np.random.default_rng(seed).permutation(len(ids))] = np.repeat(np.arange(len(sizes)), sizes)
    grp = grp_of[np.searchsorted(ids, c.flow)]
    call = grp + c.pos
    out = []
    for k in range(int(call.max()) + 1):
        ix = np.flatnonzero(call == k)
        ix = ix[np.lexsort((c.flow[ix], c.pos[ix]))]
        out.append((c.batch(ix), grp[ix]))
    return out


def concat(*batches):
    """The frames of several batches of one update call, one after the other."""
    return Batch(*[np.concatenate([b[k] for b in batches]) for k in range(5)])


_UDP_TEMPLATE = []


def frames(b):
    """One Batch -> (frames u8, offsets u32[n + 1]): 60-B TCP frames, 48-B UDP frames."""
    n = len(b.flow)
    fr = np.zeros((n, 60), dtype=np.uint8)
    tcp = ~b.udp
    if tcp.any():
        assert ((b.flags[tcp] & fs.PAY) != 0).all() and ((b.flags[tcp] & fs.REV) == 0).all()
        t, _ = fs.frames((b.flags[tcp], b.flow[tcp], b.pos[tcp]), PAIR)
        fr[tcp] = t.reshape(-1, 60)
    if b.udp.any():
        if not _UDP_TEMPLATE:
            _UDP_TEMPLATE.append(np.frombuffer(fg.udp_frame("10.0.0.0", PAIR[0], fs.SERVER, PAIR[1], 6), dtype=np.uint8))
            assert len(_UDP_TEMPLATE[0]) == 48
        u = np.tile(_UDP_TEMPLATE[0], (int(b.udp.sum()), 1))
        f = b.flow[b.udp]
        u[:, 27], u[:, 28], u[:, 29] = (f >> 16) & 0xFF, (f >> 8) & 0xFF, f & 0xFF
        fr[b.udp, :48] = u
    ln = np.where(b.udp, 48, 60)
    offs = np.zeros(n + 1, dtype=np.uint32)
    offs[1:] = np.cumsum(ln)
    return np.ascontiguousarray(fr[np.arange(60)[None, :] < ln[:, None]]), offs


def flow_of_recs(recs):
    """The flow id of fb_flow_rec / fb_pkt_out records (the client address's low 24 bits)."""
    return (recs["src_ip"][:, 0] & 0xFFFFFF).astype(np.uint32)


# ---------------------------------------------------------------------------------------------
# Long runs: more tiles of one flow than a look-back window holds.
def hot(tiles=(72,), n_small=2000, seed=21):
    """Two update calls; in each, hot flow i (flows 0..) sends tiles[i] x 2,048 packets, symbols drawn
    over all 16, interleaved at random with n_small flows (1000..) of 2-20 packets per call (run heads
    elsewhere, and whatever slot the hot flows take, their runs begin and end inside a tile).  The
    second call starts from the plane records the first one left."""
    rng = np.random.default_rng(seed)
    per_call = np.r_[np.array(tiles) * TILE, np.zeros(n_small, dtype=np.int64)]
    ids = np.r_[np.arange(len(tiles)), 1000 + np.arange(n_small)].astype(np.uint32)
    counts = [per_call + np.r_[np.zeros(len(tiles), dtype=np.int64), rng.integers(2, 21, size=n_small)] for _ in range(2)]
    lens = counts[0] + counts[1]
    flow = np.repeat(ids, lens)
    first = np.r_[0, np.cumsum(lens)[:-1]]
    pos = np.arange(len(flow)) - np.repeat(first, lens)
    fl, gap = symbols(rng.integers(0, N_SYMBOLS, size=len(flow)))
    c = Corpus(flow, pos, fl, gap)
    out, done = [], np.zeros(len(ids), dtype=np.int64)
    for cnt in counts:
        who = np.repeat(np.arange(len(ids)), cnt)
        rng.shuffle(who)
        order = np.argsort(who, kind="stable")
        k = np.zeros(len(who), dtype=np.int64)  # the packet's place in its flow's packets of this call
        k[order] = np.arange(len(who)) - np.repeat(np.r_[0, np.cumsum(cnt)[:-1]], cnt)
        out.append(c.batch(first[who] + done[who] + k))
        done += cnt
    return out


# ---------------------------------------------------------------------------------------------
# The ladder: runs of L packets placed on every wave boundary of the sorted order.
class Ladder:
    """F flows (0..F-1) of up to L + 1 packets, symbols seeded over all 16.  Call 1 inserts one packet
    per flow; the table slots it leaves decide the second call (ladder_plan)."""

    def __init__(self, F, L=5, seed=31):
        self.F, self.L = F, L
        self.sym = np.random.default_rng(seed).integers(0, N_SYMBOLS, size=(F, L + 1))
        self.c = _enumerated(*symbols(self.sym))

    def call1(self):
        return self.c.batch(np.arange(self.F) * (self.L + 1))

    def call2(self, counts):
        """counts[f] packets of flow f (positions 1..counts[f]), position-major."""
        counts = np.asarray(counts)
        f = np.repeat(np.arange(self.F), counts)
        p = 1 + np.arange(len(f)) - np.repeat(np.r_[0, np.cumsum(counts)[:-1]], counts)
        o = np.lexsort((f, p))
        return self.c.batch(f[o] * (self.L + 1) + p[o])


def plan_offset(B, L=5):
    """The probe offset d at boundary B of ladder_plan."""
    w = B // WAVE_ITEMS
    t = w // (TILE // WAVE_ITEMS)  # tile boundaries up to B
    return (t if B % TILE == 0 else w - t) % (L + 1)


def ladder_plan(slots, L=5):
    """slots[f]: flow f's table slot.  -> (counts[f], probes): every flow sends one packet in the next
    call but the probes, which send L; a flow's sorted position is the number of packets of flows with
    smaller slots, and walking the flows in slot order, at every multiple B of 256 the flow at position
    B - d becomes a probe, d cycling through 0..L (d = 0: its head is the first item after the
    boundary; d = L: its tail the last item before it; between: the run straddles it d items in).
    The tile boundaries (every eighth B) cycle on their own -- one cycle of L + 1 = 6 over all B would
    only ever put odd d on them.  probes: [(flow, B, d)]."""
    slots = np.asarray(slots)
    order = np.argsort(slots, kind="stable")
    F = len(order)
    counts = np.ones(F, dtype=np.int64)
    probes, k = [], 0
    B = WAVE_ITEMS
    while True:
        d = plan_offset(B, L)
        idx = B - d - (L - 1) * k  # k probes before it, each L - 1 items longer than a filler
        if idx >= F:
            break
        counts[order[idx]] = L
        probes.append((int(order[idx]), B, d))
        k += 1
        B += WAVE_ITEMS
    return counts, probes


def run_spans(slots, counts):
    """Sorted span [start, end) of every flow's run: the packets of the flows with smaller slots."""
    slots, counts = np.asarray(slots), np.asarray(counts, dtype=np.int64)
    order = np.argsort(slots, kind="stable")
    start = np.zeros(len(slots), dtype=np.int64)
    start[order] = np.r_[0, np.cumsum(counts[order])[:-1]]
    return start, start + counts


# ---------------------------------------------------------------------------------------------
def sim(P_row, t_row, deviation=None):
    """The segment state machine of one flow, restated a third time, with named deviations: "gt" (a
    gap of exactly 5000 ms is no timeout), "round" (ms rounded to nearest, halves away from zero),
    "floor" (ms floored), "pos" (a term accepted only when > 0).  -> (start, last, segment start,
    last segment end or None, total ms, divisor, segment count, in_segment)."""
    def ms(a, b):
        d = a - b
        if deviation == "floor":
            return d // 1_000_000
        q = (abs(d) + (500_000 if deviation == "round" else 0)) // 1_000_000
        return q if d >= 0 else -q

    t0 = t_row[0]
    start = last = seg_start = t0
    seg_end, total, div = (t0 if P_row[0] else None), 0, 0
    count, is_open = (1 if P_row[0] else 0), not P_row[0]
    for P, t in zip(P_row[1:], t_row[1:]):
        gap = ms(t, last)
        late = gap > 5000 if deviation == "gt" else gap >= 5000
        ends = P or (is_open and late)
        if not is_open:
            is_open, seg_start = True, t
        if ends:
            prev, seg_end, is_open = seg_end, t, False
            count += 1
            if prev is not None:
                term = ms(seg_start, prev)
                if term > 0 or (term == 0 and deviation != "pos"):
                    total += term
                    div = count - 1 if count > 1 else 0
            if late:
                is_open, seg_start = True, t
        last = t
    return (start, last, seg_start, seg_end, total, div, count, is_open)
