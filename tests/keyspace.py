"""Key-space corpora for the session table's probe (test helper, no tests): small, deterministic key
sets in which distinct flows share what the probe filters on, built by inverting the flow hash.

A key's 64-bit hash (flow_hash_words, flodbadd_amd/csrc/fb_internal.h) gives its partition (top
bits), its home slot (h32 & 511) and its 32-bit tag (h32 | 2); a lookup compares tags first and the
five 64-bit key words only on a tag match.  Every step of the hash is a bijection on 64 bits (xor a
word, multiply by an odd constant, xor-shift), so one free 64-bit key word can be solved to give a key
any chosen hash (`solve`), and a birthday search over 2^20 keys that differ in one word finds pairs with
equal tags (`f1_pairs`).

Families (each returns keys and the property it claims; tests/test_keyspace_oracle.py asserts the
property again, and tests/test_gpu_keyspace.py through the library's own fb_flow_hash):

  F1  pairs equal in every key word but one, in one partition of a 4-partition table, equal tags; half
      with equal h32 (one home slot), half with h32 differing in bit 1 only (homes two apart)
  F2  twelve IPv6 keys with one 64-bit hash: partition, home, tag, merge owner shared at every size
  F3  an IPv6 key with the full hash of an IPv4 key
  G   probe geometry by home slot in partition 0: ladder (G1), wrap (G2), a forty-key cluster with an
      equal-tag pair inside (G3), and a full partition of 512 keys with one home (G4)

A key is ten uint32 words as the table holds them: 0-3 source address, 4-7 destination address (IPv4:
word 0 / 4, the rest zero; IPv6: four big-endian words), 8 = src_port | dst_port << 16, 9 = protocol |
family << 8.  Frames come from framegen; ports carry no service name, so no packet is swapped and the
key a frame parses to is the one it was built from (asserted through the oracle's parse by the callers
of `reference`).  A packet in the reverse direction therefore belongs to the mirrored key, a flow of
its own.

Every key has its own packet pattern -- a payload length no other key (or direction) of its corpus has,
and a packet count distinct within its collision group -- so a record credited to the wrong slot
changes a sum no other key reproduces; TCP keys carry a few flag characters, so the histories differ
too.  `expected` restates the six counters and the history length as plain dict sums."""
import functools
import ipaddress

import numpy as np

import framegen as fg

M64 = (1 << 64) - 1
SEED, C1, C2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0xFF51AFD7ED558CCD
C1_INV, C2_INV = pow(C1, -1, 1 << 64), pow(C2, -1, 1 << 64)
SLOTS = 512  # slots of a partition
V4, V6, TCP, UDP = 2, 10, 6, 17
REV_PAY = 700  # a key's reverse direction carries its payload length + REV_PAY


# ---- the hash -------------------------------------------------------------------------------------
def flow_hash(words):
    """flow_hash_words over [n, 10] uint32 key words -> uint64[n]."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 10).astype(np.uint64)
    h = np.full(len(w), SEED, dtype=np.uint64)
    for j in range(0, 10, 2):
        h ^= w[:, j] | (w[:, j + 1] << np.uint64(32))
        h *= np.uint64(C1)
        h ^= h >> np.uint64(31)
    h ^= h >> np.uint64(33)
    h *= np.uint64(C2)
    h ^= h >> np.uint64(33)
    return h


def _finish(h):
    h ^= h >> np.uint64(33)
    h *= np.uint64(C2)
    h ^= h >> np.uint64(33)
    return h


def _round(s, w):
    s = ((s ^ w) * C1) & M64
    return s ^ (s >> 31)


def _unshift(y, s):
    """The x with x ^ (x >> s) == y."""
    x, t = y, y >> s
    while t:
        x ^= t
        t >>= s
    return x


def _w64(key):
    k = [int(x) for x in key]
    return [k[2 * j] | (k[2 * j + 1] << 32) for j in range(5)]


def solve(key_words, pair, H):
    """A copy of the key with 64-bit word `pair` (words 2 * pair, 2 * pair + 1) set so that the key's
    hash is exactly H: the finaliser and the rounds after `pair` inverted, the rounds before it run
    forward.  Use it on the low half of an IPv6 address only (pair 1 or 3)."""
    w = _w64(key_words)
    s = SEED
    for j in range(pair):
        s = _round(s, w[j])
    t = _unshift(int(H) & M64, 33)
    t = _unshift((t * C2_INV) & M64, 33)
    for j in range(4, pair, -1):  # the state after round j -> the state before it
        t = ((_unshift(t, 31) * C1_INV) & M64) ^ w[j]
    x = ((_unshift(t, 31) * C1_INV) & M64) ^ s
    out = np.array(key_words, dtype=np.uint32).copy()
    out[2 * pair], out[2 * pair + 1] = x & 0xFFFFFFFF, x >> 32
    return out


def _hash_varying(base, pair, values):
    """The hashes of `base` with 64-bit word `pair` replaced by each of values (uint64[n])."""
    w = _w64(base)
    s = SEED
    for j in range(pair):
        s = _round(s, w[j])
    h = np.full(len(values), s, dtype=np.uint64)
    for j in range(pair, 5):
        h ^= values if j == pair else np.uint64(w[j])
        h *= np.uint64(C1)
        h ^= h >> np.uint64(31)
    return _finish(h)


def part_of(h, partitions):
    """The partition of hashes in a table of `partitions` (a power of two) partitions."""
    h = np.asarray(h, dtype=np.uint64)
    if partitions == 1:
        return np.zeros(h.shape, dtype=np.int64)
    return (h >> np.uint64(64 - (partitions.bit_length() - 1))).astype(np.int64)


def h32_of(h):
    return (np.asarray(h, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


def home_of(h):
    return h32_of(h) & (SLOTS - 1)


def tag_of(h):
    return h32_of(h) | 2


# ---- keys -----------------------------------------------------------------------------------------
def key_v4(src, dst, sport, dport, proto=TCP):
    return np.array([src, 0, 0, 0, dst, 0, 0, 0, sport | dport << 16, proto | V4 << 8], dtype=np.uint32)


def key_v6(src, dst, sport, dport, proto=TCP):
    """src / dst: four big-endian 32-bit words each."""
    return np.array(list(src) + list(dst) + [sport | dport << 16, proto | V6 << 8], dtype=np.uint32)


def mirror(key):
    k = np.asarray(key, dtype=np.uint32)
    p = int(k[8])
    return np.array(list(k[4:8]) + list(k[0:4]) + [(p >> 16) | (p & 0xFFFF) << 16, int(k[9])], dtype=np.uint32)


def key_bytes(key):
    return np.asarray(key, dtype="<u4").tobytes()


def words_of(recs):
    """[n, 10] key words of records whose first 40 bytes are a session key (padding masked off)."""
    a = np.ascontiguousarray(recs)
    w = a.view(np.uint8).reshape(len(a), -1)[:, :40].copy().view("<u4").reshape(len(a), 10)
    w[:, 9] &= 0xFFFF
    return w


def _addr(words, family):
    if family == V4:
        return str(ipaddress.IPv4Address(int(words[0])))
    return str(ipaddress.IPv6Address(b"".join(int(x).to_bytes(4, "big") for x in words)))


_FRAMES = {}


def frame_of(key, flags, pay, rev=False):
    """The frame of one packet of `key` (rev: from its destination to its source)."""
    kb = (key_bytes(key), flags, pay, rev)
    if kb not in _FRAMES:
        k = [int(x) for x in key]
        fam, proto = (k[9] >> 8) & 0xFF, k[9] & 0xFF
        a, b = (_addr(k[0:4], fam), k[8] & 0xFFFF), (_addr(k[4:8], fam), k[8] >> 16)
        if rev:
            a, b = b, a
        _FRAMES[kb] = fg.tcp_frame(a[0], a[1], b[0], b[1], flags, pay) if proto == TCP else \
            fg.udp_frame(a[0], a[1], b[0], b[1], pay)
    return _FRAMES[kb]


@functools.lru_cache(maxsize=None)
def plain_ports():
    """Ports without a service name under the default bitmap (and not 53, which diverts to DNS),
    ascending from 1024."""
    from oracle import coracle
    bm = np.frombuffer(coracle.default_bitmap(), dtype=np.uint8)
    bits = np.unpackbits(bm, bitorder="little")
    p = np.flatnonzero(bits == 0)
    p = p[(p >= 1024) & (p != 53)]
    assert len(p) >= 4096
    return p


# fixed address material: documentation / public ranges, nothing local
V6_SRC, V6_DST = (0x20010DB8, 0x00A10000, 0x00000000, 0x00000011), (0x26001F18, 0x00B20000, 0x00000000, 0x00000022)
V4_SRC, V4_DST = 0x2D210000, 0x5DB8D822  # 45.33.0.0, 93.184.216.34


def _base(family):
    p = plain_ports()
    return (key_v6(V6_SRC, V6_DST, int(p[100]), int(p[200])) if family == V6 else
            key_v4(V4_SRC, V4_DST, int(p[100]), int(p[200])))


# ---- F1 -------------------------------------------------------------------------------------------
def _f1_values(base, a, n):
    """n values of 64-bit key word `a` of `base`, its free bits counted through.  Words 0-3: address
    bits; word 4: TCP / UDP and the two ports, drawn from disjoint ranges of plain_ports()."""
    idx = np.arange(n, dtype=np.uint64)
    w = _w64(base)[a]
    if a < 4:
        fam = (int(base[9]) >> 8) & 0xFF
        if fam == V4:  # the address is the low 32 bits; its low 24 bits counted
            assert n <= 1 << 24
            return np.uint64(w & ~0xFFFFFF & M64) | idx
        # IPv6: the half's second word (bits 32-63) counted, the first kept
        return np.uint64(w & 0xFFFFFFFF) | ((idx + np.uint64(1)) << np.uint64(32))
    p = plain_ports().astype(np.uint64)
    assert n <= 1 << 22
    proto = np.where(idx & np.uint64(1), np.uint64(UDP), np.uint64(TCP))
    sp = p[((idx >> np.uint64(1)) & np.uint64(1023)).astype(np.intp)]
    dp = p[(1024 + (idx >> np.uint64(11))).astype(np.intp)]
    return sp | (dp << np.uint64(16)) | ((proto | np.uint64(((int(base[9]) >> 8) & 0xFF) << 8)) << np.uint64(32))


def _with_word(base, a, v):
    k = np.array(base, dtype=np.uint32).copy()
    k[2 * a], k[2 * a + 1] = int(v) & 0xFFFFFFFF, int(v) >> 32
    return k


def f1_search(family, a, partitions, n):
    """Every pair among n keys that differ from the family's base key in 64-bit word `a` only, lie in
    one partition of `partitions` and have equal tags -> (base, values, [(i, j, same_h32)], hashes)."""
    base = _base(family)
    vals = _f1_values(base, a, n)
    h = _hash_varying(base, a, vals)
    comp = (part_of(h, partitions).astype(np.uint64) << np.uint64(32)) | tag_of(h).astype(np.uint64)
    order = np.argsort(comp, kind="stable")
    cs = comp[order]
    at = np.flatnonzero(cs[1:] == cs[:-1])
    pairs = [(int(order[k]), int(order[k + 1]), bool(h32_of(h[order[k]]) == h32_of(h[order[k + 1]]))) for k in at]
    return base, vals, pairs, h


def f1_pairs(family, a, partitions=4, per_kind=2, n=1 << 20):
    """per_kind pairs with equal h32 and per_kind with h32 differing in bit 1 only (equal tags), each
    pair equal in every key word but `a` and in one partition of `partitions`: a list of
    (key, key, same_h32).  Fails if the search does not find them."""
    base, vals, pairs, _ = f1_search(family, a, partitions, n)
    out, used = [], set()
    for same in (True, False):
        got = 0
        for i, j, s in pairs:
            if s == same and got < per_kind and i not in used and j not in used:
                out.append((_with_word(base, a, vals[i]), _with_word(base, a, vals[j]), same))
                used |= {i, j}
                got += 1
        if got < per_kind:
            raise AssertionError("F1: %d of %d pairs (family %d, word %d, same_h32 %s) among %d keys" %
                                 (got, per_kind, family, a, same, n))
    return out


F1_WORDS = [(V6, 0), (V6, 1), (V6, 2), (V6, 3), (V6, 4), (V4, 0), (V4, 2), (V4, 4)]


@functools.lru_cache(maxsize=None)
def f1_all():
    """[(family, word, key, key, same_h32)]: four pairs for each word of each family."""
    return [(fam, a) + p for fam, a in F1_WORDS for p in f1_pairs(fam, a)]


@functools.lru_cache(maxsize=None)
def f1_hot(partitions=32, n=1 << 21):
    """For each 64-bit key word, one IPv6 pair differing in that word only with EQUAL h32 in one
    partition of `partitions`: one home slot in K1c's 256-slot table too -> [(word, key, key)]."""
    out = []
    for a in range(5):
        base, vals, pairs, _ = f1_search(V6, a, partitions, n)
        same = [(i, j) for i, j, s in pairs if s]
        if not same:
            raise AssertionError("F1 hot: no equal-h32 pair for word %d in one of %d partitions among %d keys" %
                                 (a, partitions, n))
        i, j = same[0]
        out.append((a, _with_word(base, a, vals[i]), _with_word(base, a, vals[j])))
    return out


# ---- F2, F3 ---------------------------------------------------------------------------------------
# partition 0 / home 0; the last partition / home 507 (twelve keys wrap 511 -> 0); the middle
F2_HASHES = [0x00005A5A12349A00, 0xFFFFA5A50BADC1FB, 0x800013572468ACFA]
F2_SIZE = 12


def f2_family(H, size=F2_SIZE, salt=0):
    """`size` IPv6 keys with the 64-bit hash H: the low half of the destination address counts up,
    the low half of the source address is solved."""
    base = _base(V6)
    out = []
    for i in range(size):
        k = base.copy()
        k[6], k[7] = 0x00F20000 + salt, 0x1000 + i
        out.append(solve(k, 1, H))
    return out


def f2_all():
    return [f2_family(H, salt=s) for s, H in enumerate(F2_HASHES)]


def f3_pairs(count=4):
    """[(IPv4 key, IPv6 key)] with equal 64-bit hashes."""
    p = plain_ports()
    out = []
    for i in range(count):
        k4 = key_v4(0x08080000 + 257 * (i + 1), V4_DST, int(p[300 + i]), int(p[400 + i]), TCP if i % 2 == 0 else UDP)
        k6 = _base(V6).copy()
        k6[6], k6[7], k6[8] = 0x00F30000, 0x2000 + i, int(k4[8])
        k6[9] = (int(k4[9]) & 0xFF) | V6 << 8
        out.append((k4, solve(k6, 1, int(flow_hash(k4)[0]))))
    return out


def filler(count, first=0):
    """Plain IPv4 TCP flows, 46.33.x.y -> 93.184.216.34 (no F1 key: those count through 45.x.y.z)."""
    p = plain_ports()
    return [key_v4(0x2E210100 + first + i, V4_DST, int(p[500 + (first + i) % 7]), int(p[600])) for i in range(count)]


# ---- G: geometry in partition 0 -------------------------------------------------------------------
def g_key(h32, serial, hi=None):
    """An IPv6 key whose hash has the low word h32 (home h32 & 511, tag h32 | 2) and top bits zero
    (partition 0 at every table size up to 2^16 partitions)."""
    hi = ((serial * 0x9E37 + 0x1B) & 0xFFFF) if hi is None else hi
    k = _base(V6).copy()
    k[6], k[7] = 0x00A60000, 0x3000 + serial
    return solve(k, 1, (hi << 32) | (h32 & 0xFFFFFFFF))


def _h32(home, n):
    return (home & (SLOTS - 1)) | ((n + 1) << 9)


G1_GROUPS = [2 + 2 * r for r in range(8)]  # 8-slot groups 2, 4, .., 16: the group after each is empty
G3_HOME, G3_SIZE = 300, 40


def g1_ladder():
    """(occupiers, climbers): for r = 0..7, group G1_GROUPS[r] has slots r..7 taken by keys at home
    there (the slots below r stay empty), and one more key with home r: it finds its home's group full
    from r on and lands in the next group."""
    occ, climb, s = [], [], 0
    for r, g in enumerate(G1_GROUPS):
        for q in range(r, 8):
            occ.append(g_key(_h32(8 * g + q, s), s))
            s += 1
        climb.append(g_key(_h32(8 * g + r, s), s))
        s += 1
    return occ, climb


def g2_wrap():
    """Eight keys with homes 509, 510, 511 (3 + 3 + 2): five of them wrap to slots 0..4."""
    return [g_key(_h32(509 + i % 3, 100 + i), 100 + i) for i in range(8)]


def g3_cluster():
    """Forty keys with home 300 (five 8-slot groups); the last two have equal h32 (one tag)."""
    ks = [g_key(_h32(G3_HOME, 200 + i), 200 + i) for i in range(G3_SIZE - 1)]
    ks.append(g_key(_h32(G3_HOME, 200 + G3_SIZE - 2), 200 + G3_SIZE, hi=0x0777))
    return ks


G4_HOME = 259  # slot 3 of group 32: the last key inserted lands in slot 258, past the 64 groups k2_lookup reads


def g4_full(extra=1):
    """512 keys with home 259, and `extra` more with that home: whichever of the 512 is inserted
    last sits in slot 258, just before its home after wrapping the whole partition."""
    return [g_key(_h32(G4_HOME, 1000 + i), 1000 + i) for i in range(SLOTS + extra)]


# ---- corpora, layouts -----------------------------------------------------------------------------
class Corpus:
    """Keys in collision groups (pairs, families, clusters) and filler.  Key i carries payload length
    8 + i (no other key of the corpus has it) and 3 + its place in its group packets (filler: 1 + i % 3)."""

    def __init__(self, reverse=True):
        self.keys, self.group, self.member, self.groups, self.reverse = [], [], [], [], reverse

    def add_group(self, keys):
        g = len(self.groups)
        self.groups.append(list(range(len(self.keys), len(self.keys) + len(keys))))
        for m, k in enumerate(keys):
            self.keys.append(np.asarray(k, dtype=np.uint32))
            self.group.append(g)
            self.member.append(m)
        return self.groups[-1]

    def add_filler(self, keys):
        for k in keys:
            self.keys.append(np.asarray(k, dtype=np.uint32))
            self.group.append(-1)
            self.member.append(0)

    def filler(self):
        return [i for i, g in enumerate(self.group) if g < 0]

    def pay(self, i):
        return 8 + i

    def count(self, i):
        return 3 + self.member[i] if self.group[i] >= 0 else 1 + i % 3

    def proto(self, i):
        return int(self.keys[i][9]) & 0xFF

    def packets(self, i, count=None):
        """The insert phase's packets of key i: [(i, flags, payload, rev)].  TCP: SYN first, then
        PSH|ACK with the key's payload, then by the bits of i either that again or a bare ACK, and for
        every third key FIN|ACK last."""
        n, L = self.count(i) if count is None else count, self.pay(i)
        if self.proto(i) != TCP:
            return [(i, 0, L, False)] * n
        out = []
        for j in range(n):
            if j == 0:
                out.append((i, fg.SYN, 0, False))
            elif j == n - 1 and n >= 3 and i % 3 == 0:
                out.append((i, fg.FIN | fg.ACK, 0, False))
            elif j == 1 or (i >> ((j - 2) % 5)) & 1:
                out.append((i, fg.PSH | fg.ACK, L, False))
            else:
                out.append((i, fg.ACK, 0, False))
        return out


def _position_major(lists):
    out = []
    for j in range(max([len(x) for x in lists] + [0])):
        out += [x[j] for x in lists if j < len(x)]
    return out


def together(c, counts=None):
    """One call: every group's first packets stand inside one 64-record segment (filler pads a segment
    a group would straddle), then the filler's, then every key's later packets position-major."""
    pk = [c.packets(i, None if counts is None else counts.get(i)) for i in range(len(c.keys))]
    spare, call = c.filler(), []
    for g in c.groups:
        assert len(g) <= 64
        while len(call) % 64 + len(g) > 64:
            call.append(pk[spare.pop()][0])  # (runs out: IndexError, a corpus without enough filler)
        call += [pk[i][0] for i in g]
    call += [pk[i][0] for i in spare]
    call += _position_major([p[1:] for p in pk])
    return [call]


def apart(c):
    """One call per group member: call m holds member m of every group (call 0 the filler too), so
    each member misses against the tags the earlier calls published, then inserts."""
    calls = []
    for m in range(max(len(g) for g in c.groups)):
        ids = [g[m] for g in c.groups if m < len(g)] + (c.filler() if m == 0 else [])
        calls.append(_position_major([c.packets(i) for i in ids]))
    return calls


def staged(c, stages):
    """One call per stage (a list of key indices), position-major."""
    return [_position_major([c.packets(i) for i in ids]) for ids in stages]


def find(c):
    """Two calls over every key, interleaved across the groups (member 0 of every group, member 1 of
    every group, ...): a forward packet and (c.reverse) one in the reverse direction each."""
    order = sorted(range(len(c.keys)), key=lambda i: (c.member[i], c.group[i], i))
    calls = []
    for fwd in ((fg.PSH | fg.ACK, None), (fg.ACK, 0)):
        call = []
        for i in order:
            tcp = c.proto(i) == TCP
            call.append((i, fwd[0] if tcp else 0, c.pay(i) if fwd[1] is None or not tcp else fwd[1], False))
            if c.reverse:
                call.append((i, (fg.PSH | fg.ACK) if tcp else 0, c.pay(i) + REV_PAY, True))
        calls.append(call)
    return calls


def frames(c, call):
    return fg.pack([frame_of(c.keys[i], fl, pay, rev) for i, fl, pay, rev in call])


def packet_key(c, pkt):
    i, _, _, rev = pkt
    return key_bytes(mirror(c.keys[i]) if rev else c.keys[i])


def expected(c, calls):
    """The second restatement: {40-B key: [outbound_bytes, inbound_bytes, orig_pkts, resp_pkts,
    orig_ip_bytes, resp_ip_bytes, history length]} as plain sums over the packets (no packet is swapped,
    so every packet is its key's originator's)."""
    out = {}
    for call in calls:
        for pkt in call:
            i, _, pay, _ = pkt
            k = c.keys[i]
            fam, proto = (int(k[9]) >> 8) & 0xFF, int(k[9]) & 0xFF
            ip_len = (20 if fam == V4 else 40) + (20 if proto == TCP else 8) + pay
            e = out.setdefault(packet_key(c, pkt), [0] * 7)
            e[0] += pay
            e[2] += 1
            e[4] += ip_len
            e[6] += 1 if proto == TCP else 0
    return out


# ---- the corpora ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus_f(n_filler=300):
    """F1 + F2 + F3 and filler, for a 2^11-slot table (4 partitions)."""
    c = Corpus()
    for _, _, ka, kb, _ in f1_all():
        c.add_group([ka, kb])
    for fam in f2_all():
        c.add_group(fam)
    for k4, k6 in f3_pairs():
        c.add_group([k4, k6])
    c.add_filler(filler(n_filler))
    return c


@functools.lru_cache(maxsize=None)
def corpus_g123():
    """G1-G3 for the fixed 512-slot table -> (corpus, stages): the occupiers go in first."""
    c = Corpus(reverse=False)
    occ, climb = g1_ladder()
    first = c.add_group(occ)
    later = c.add_group(climb) + c.add_group(g2_wrap()) + c.add_group(g3_cluster())
    return c, [first, later]


@functools.lru_cache(maxsize=None)
def corpus_g4():
    """G4 -> (corpus of the 512 keys, the key that finds the table full)."""
    c = Corpus(reverse=False)
    ks = g4_full()
    c.add_filler(ks[:SLOTS])
    return c, ks[SLOTS]


HOT_RECORDS, HOT_PAIR_RECORDS = 60, 220


@functools.lru_cache(maxsize=None)
def corpus_hot(n_cold=200):
    """For a 2^14-slot table (32 partitions): one F2 family with eleven keys of >= 60 records and one of
    a single record; for each key word an equal-h32 F1 pair of >= 220 records per key, a hot group of
    its own; and cold filler -> (corpus, {key index: packet count})."""
    c = Corpus(reverse=False)
    fam = c.add_group(f2_family(F2_HASHES[2], salt=2))
    counts = {i: HOT_RECORDS + m for m, i in enumerate(fam[:-1])}
    counts[fam[-1]] = 1
    for _, ka, kb in f1_hot():
        for i in c.add_group([ka, kb]):
            counts[i] = HOT_PAIR_RECORDS + c.member[i] + 2 * c.group[i]
    c.add_filler(filler(n_cold, first=1000))
    return c, counts


def hot(c, counts):
    """One call: the hot keys' packets interleaved key by key (position-major), the cold filler spread
    between them."""
    hot_pk = _position_major([c.packets(i, counts[i]) for g in c.groups for i in g])
    cold = _position_major([c.packets(i) for i in c.filler()])
    call, step, q = [], max(len(hot_pk) // max(len(cold), 1), 1), 0
    for a in range(0, len(hot_pk), step):
        call += hot_pk[a: a + step]
        if q < len(cold):
            call.append(cold[q])
            q += 1
    return [call + cold[q:]]


CASES = [("f", "together"), ("f", "apart"), ("g123", "staged"), ("g4", "together"), ("hot", "hot")]
BASE_NS = 1_700_000_000 * 10 ** 9


@functools.lru_cache(maxsize=None)
def calls_of(name, how):
    """(corpus, the update calls of the insert layout `how` followed by the two find calls)."""
    if name == "f":
        c = corpus_f()
        ins = {"together": together, "apart": apart}[how](c)
    elif name == "g123":
        c, stages = corpus_g123()
        ins = staged(c, stages)
    elif name == "g4":
        c = corpus_g4()[0]
        ins = together(c)
    elif name == "hot":
        c, counts = corpus_hot()
        ins = hot(c, counts)
    else:
        raise ValueError(name)
    return c, ins + find(c)


def times_of(k, n):
    """Capture timestamps of call k: the calls 7 s apart (past the 5-s segment timeout), frames 1 us apart."""
    return (BASE_NS + k * 7 * 10 ** 9 + np.arange(n, dtype=np.uint64) * 1000).astype(np.uint64)


def through_oracle(c, calls, timed=False, flows=None, first_call=0):
    """The calls through the oracle's parse and table: per call (frames, offsets, ts, records, stats), and the
    table.  Asserts that every frame parses to the key it was built for, unswapped."""
    from flodbadd_amd import _native as N
    from oracle import coracle
    flows, cfg, out = flows or coracle.Flows(), coracle.make_cfg(2), []
    for k, call in enumerate(calls):
        fr, of = frames(c, call)
        recs, dns, _, _ = coracle.parse_classify(cfg, fr, of)
        assert len(recs) == len(call) and len(dns) == 0, (k, len(recs), len(call), len(dns))
        want = np.stack([mirror(c.keys[i]) if rev else c.keys[i] for i, _, _, rev in call])
        assert (words_of(recs) == want).all(), "call %d: a frame parses to another key than intended" % k
        assert not (recs["meta"] & N.META_SWAP).any()
        ts = times_of(first_call + k, len(call)) if timed else None
        st = np.zeros(1, dtype=N.STATS_DTYPE)
        flows.update(recs, st, ts=ts)
        for a in (fr, of, recs, st):
            a.setflags(write=False)
        out.append((fr, of, ts, recs, st))
    return out, flows


@functools.lru_cache(maxsize=None)
def reference(name, how, timed=False):
    """calls_of(name, how) through the oracle, once; read-only for the tests."""
    c, calls = calls_of(name, how)
    return through_oracle(c, calls, timed)


# ---- the placement invariant ----------------------------------------------------------------------
def check_placement(flows, partitions, hash_fn=flow_hash):
    """An export_flows() array taken under SessionFilter.All: no slot and no key twice, every flow in
    its hash's partition (slot // 512), and no empty slot from its home (h32 & 511) to its slot,
    cyclically -- what every later lookup relies on.  Raises AssertionError naming the first offender."""
    n = len(flows)
    if n == 0:
        return
    w = words_of(flows)
    slot = np.asarray(flows["slot"], dtype=np.int64)
    name = lambda i: "key %s (slot %d)" % (w[i].tolist(), slot[i])  # noqa: E731

    def first_dup(a):
        o = np.argsort(a, kind="stable")
        d = np.flatnonzero(a[o][1:] == a[o][:-1])
        return None if d.size == 0 else int(min(o[d[0]], o[d[0] + 1])), None if d.size == 0 else int(max(o[d[0]], o[d[0] + 1]))

    a, b = first_dup(slot)
    if a is not None:
        raise AssertionError("placement: %s and %s share a slot" % (name(a), name(b)))
    a, b = first_dup(np.ascontiguousarray(w).view("V40").ravel())
    if a is not None:
        raise AssertionError("placement: %s is in the table twice (also slot %d)" % (name(a), slot[b]))
    h = hash_fn(w)
    part, home = part_of(h, partitions), home_of(h)
    bad = np.flatnonzero((slot // SLOTS != part) | (slot < 0) | (slot >= partitions * SLOTS))
    if bad.size:
        i = int(bad[0])
        raise AssertionError("placement: %s is in partition %d, its hash's is %d" % (name(i), slot[i] // SLOTS, part[i]))
    occ = np.zeros(partitions * SLOTS, dtype=np.int64)
    occ[slot] = 1
    occ2 = np.concatenate([occ.reshape(partitions, SLOTS)] * 2, axis=1)  # a partition's slots twice: cyclic runs
    filled = np.concatenate([np.zeros((partitions, 1), dtype=np.int64), np.cumsum(occ2, axis=1)], axis=1)
    dist = (slot % SLOTS - home) % SLOTS
    run = filled[part, home + dist + 1] - filled[part, home]
    bad = np.flatnonzero(run != dist + 1)
    if bad.size:
        i = int(bad[0])
        raise AssertionError("placement: %s has home %d and an empty slot before it" % (name(i), home[i]))
