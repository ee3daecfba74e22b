"""Flag-sequence corpora for the ordered per-flow state (test helper, no tests): every flow is a
sequence of symbols, each symbol one TCP packet, and the corpora enumerate the sequences instead of
sampling them, so a state composition that is wrong for one rare symbol pair has a flow that shows it.

A symbol is 7 bits: bits 0-4 are the TCP flag bits FIN, SYN, RST, PSH, ACK as they stand in the flag
byte, bit 5 (REV) is the direction (set: server -> client) and bit 6 (PAY) the payload (set: 6 B,
clear: 0 B).  Bits 5-7 of the flag BYTE (URG, ECE, CWR) are not part of a symbol: `frames` draws them
from a seeded generator (or leaves them zero), and they must change nothing.

Frames are two framegen.tcp_frame templates (54 B, 60 B) patched with numpy: bytes 26-38 (addresses
and ports, swapped for the reverse direction) and byte 47 (the flags); flow f is 10.(f>>16).(f>>8).(f)
talking to 93.184.216.34.  A batch is three equally long arrays (sym, flow, pos) in frame order; a
layout is a list of batches (one per update call).
"""
import numpy as np

import framegen as fg

FIN, SYN, RST, PSH, ACK = fg.FIN, fg.SYN, fg.RST, fg.PSH, fg.ACK
REV, PAY = 0x20, 0x40
N_SYMBOLS = 128
SERVER = "93.184.216.34"

# (client port, server port).  Under the default service bitmap 443 and 80 are service ports, 49152
# and 65535 are not (test_flagspace_oracle.test_port_pair_properties):
#   ONE_SVC  both directions share a key, all 13 history characters are reachable
#   TWO_SVC  the key depends on each packet's SYN and ACK bits, one conversation splits over two keys
#   NO_SVC   packets are never swapped, each direction has its own key
ONE_SVC, TWO_SVC, NO_SVC = (49152, 443), (80, 443), (49152, 65535)
PORT_PAIRS = [ONE_SVC, TWO_SVC, NO_SVC]

# the quads alphabet: S SA s sa FA fa R ra A a PA+payload pa+payload SYN|FIN syn|rst FIN|PSH|ACK+payload
# and a reverse packet without flags (lower case: server -> client)
ALPHABET16 = np.array([SYN, SYN | ACK, REV | SYN, REV | SYN | ACK, FIN | ACK, REV | FIN | ACK, RST, REV | RST | ACK,
                       ACK, REV | ACK, PAY | PSH | ACK, REV | PAY | PSH | ACK, SYN | FIN, REV | SYN | RST,
                       PAY | FIN | PSH | ACK, REV], dtype=np.uint8)

BASE_NS = 1_700_000_000 * 10 ** 9
# gaps between a flow's consecutive packets: both sides of the 5-s segment timeout, the exact
# boundary, a long pause and a step backwards
GAPS_NS = np.array([1_000_000, 4_999_000_000, 5_000_000_000, 5_001_000_000, 12_000_000_000, -1_000_000_000],
                   dtype=np.int64)


def pairs_seq():
    """All 128^2 two-symbol sequences: [16384, 2]."""
    a = np.arange(N_SYMBOLS * N_SYMBOLS)
    return np.stack([a // N_SYMBOLS, a % N_SYMBOLS], axis=1).astype(np.uint8)


def quads_seq():
    """All 16^4 sequences over ALPHABET16: [65536, 4]."""
    a = np.arange(16 ** 4)
    return ALPHABET16[np.stack([(a >> 12) & 15, (a >> 8) & 15, (a >> 4) & 15, a & 15], axis=1)]


def layout(seq, how):
    """[F, L] sequences -> list of batches (sym, flow, pos).  pos: position-major (a flow's packets
    are F frames apart, in different waves and chunks); flow: flow-major (adjacent lanes of one
    wave); split: the first ceil(L / 2) positions in call 1 and the rest in call 2, each
    position-major (the state is carried between updates)."""
    F, L = seq.shape
    f, p = np.meshgrid(np.arange(F, dtype=np.uint32), np.arange(L, dtype=np.uint32), indexing="ij")
    if how == "flow":
        return [(seq.reshape(-1), f.reshape(-1), p.reshape(-1))]
    pm = lambda a, b: (np.ascontiguousarray(seq[:, a:b].T).reshape(-1), np.ascontiguousarray(f[:, a:b].T).reshape(-1),  # noqa: E731
                       np.ascontiguousarray(p[:, a:b].T).reshape(-1))
    if how == "pos":
        return [pm(0, L)]
    if how == "split":
        h = (L + 1) // 2
        return [pm(0, h), pm(h, L)]
    raise ValueError(how)


HOT_LENGTHS = [12000] * 4 + [500] * 44


def hot_batches(seed=3, n_batches=3, end_share=0.02):
    """4 flows of 12,000 packets and 44 of 500, symbols drawn over all 128 with the FIN / RST classes
    down-weighted (together `end_share` of the packets, so a flow's first end falls mid-sequence),
    the flows' packets interleaved at random, cut into n_batches update calls."""
    rng = np.random.default_rng(seed)
    lens = np.array(HOT_LENGTHS)
    n = int(lens.sum())
    flow = np.repeat(np.arange(len(lens), dtype=np.uint32), lens)
    rng.shuffle(flow)
    order = np.argsort(flow, kind="stable")
    pos = np.zeros(n, dtype=np.uint32)
    first = np.r_[0, np.cumsum(lens)[:-1]]
    pos[order] = (np.arange(n) - np.repeat(first, lens)).astype(np.uint32)
    ends = (np.arange(N_SYMBOLS) & (FIN | RST)) != 0
    w = np.where(ends, end_share / ends.sum(), (1.0 - end_share) / (~ends).sum())
    sym = rng.choice(N_SYMBOLS, size=n, p=w).astype(np.uint8)
    cuts = [n * k // n_batches for k in range(n_batches + 1)]
    return [(sym[a:b], flow[a:b], pos[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


_TEMPLATES = {}


def _templates(pair):
    if pair not in _TEMPLATES:
        t = np.zeros((2, 60), dtype=np.uint8)
        for k, pay in enumerate((0, 6)):
            f = fg.tcp_frame("10.0.0.0", pair[0], SERVER, pair[1], 0, pay)
            assert len(f) == 54 + pay
            t[k, :len(f)] = np.frombuffer(f, dtype=np.uint8)
        _TEMPLATES[pair] = t
    return _TEMPLATES[pair]


def frames(batch, pair, hi_seed=None):
    """One batch -> (frames u8, offsets u32[n + 1]).  hi_seed: the seed of the flag byte's bits 5-7
    (None: zero)."""
    sym, flow, _ = batch
    n = len(sym)
    pay = (sym & PAY) != 0
    rev = (sym & REV) != 0
    fr = _templates(pair)[pay.astype(np.intp)]  # [n, 60] copies
    fr[:, 27] = (flow >> 16) & 0xFF
    fr[:, 28] = (flow >> 8) & 0xFF
    fr[:, 29] = flow & 0xFF
    swapped = fr[rev]
    swapped[:, 26:30], swapped[:, 30:34] = fr[rev, 30:34], fr[rev, 26:30]
    swapped[:, 34:36], swapped[:, 36:38] = fr[rev, 36:38], fr[rev, 34:36]
    fr[rev] = swapped
    hi = np.zeros(n, dtype=np.uint8) if hi_seed is None else \
        (np.random.default_rng(hi_seed).integers(0, 8, size=n).astype(np.uint8) << 5)
    fr[:, 47] = (sym & 0x1F) | hi
    ln = np.where(pay, 60, 54)
    offs = np.zeros(n + 1, dtype=np.uint32)
    offs[1:] = np.cumsum(ln)
    return np.ascontiguousarray(fr[np.arange(60)[None, :] < ln[:, None]]), offs


def times(batches, seed):
    """Capture timestamps (uint64 ns) for every batch of a layout, indexed by pkt_index (the frame's
    place in its batch): a flow's consecutive packets (by pos) are GAPS_NS apart, whatever the
    layout and the cuts -- the gap before a packet is a function of (seed, flow, pos) alone."""
    flow = np.concatenate([b[1] for b in batches]).astype(np.int64)
    pos = np.concatenate([b[2] for b in batches]).astype(np.int64)
    order = np.lexsort((pos, flow))
    fs, ps = flow[order], pos[order]
    assert ((ps == 0) | ((np.r_[-1, fs[:-1]] == fs) & (np.r_[-1, ps[:-1]] + 1 == ps))).all(), "positions 0..L-1 per flow"
    # one generator per corpus; the draw is made in (flow, pos) order, which no layout changes
    gaps = GAPS_NS[np.random.default_rng(seed).integers(0, len(GAPS_NS), size=len(fs))]
    gaps[ps == 0] = 0
    c = np.cumsum(gaps)
    start = np.maximum.accumulate(np.where(ps == 0, np.arange(len(fs)), 0))
    t_sorted = BASE_NS + fs * 1_000_000 + (c - c[start])
    t = np.zeros(len(fs), dtype=np.int64)
    t[order] = t_sorted
    assert (t > 0).all()
    out, a = [], 0
    for b in batches:
        out.append(t[a: a + len(b[0])].astype(np.uint64))
        a += len(b[0])
    return out


def parsed_of(recs):
    """The oracle's fb_pkt_out records of a batch -> the fb_parsed_pkt records a host with its own
    decode would hand in: the session as parsed (the raw direction restored from the SWAP bit)."""
    from flodbadd_amd import _native as N
    p = np.zeros(len(recs), dtype=N.PARSED_DTYPE)
    sw = (recs["meta"] & N.META_SWAP) != 0
    p["src_ip"] = np.where(sw[:, None], recs["dst_ip"], recs["src_ip"])
    p["dst_ip"] = np.where(sw[:, None], recs["src_ip"], recs["dst_ip"])
    p["src_port"] = np.where(sw, recs["dst_port"], recs["src_port"])
    p["dst_port"] = np.where(sw, recs["src_port"], recs["dst_port"])
    for f in ("protocol", "family", "packet_length", "ip_packet_length", "tcp_flags", "pkt_index"):
        p[f] = recs[f]
    p["has_flags"] = ((recs["meta"] & N.META_HAS_FLAGS) != 0).astype(np.uint8)
    return p
