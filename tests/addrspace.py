"""Address-space corpora for flow enrichment (test helper, no tests): one table of hand-placed flows, a
ladder of table configurations to sweep it under, a plain-Python restatement of what every flow must
get, and a census of the outcome classes the two together reach.

k_flow_enrich (flodbadd_amd/csrc/fb_enrich.hip) does not call asn_lookup / bl_lookup: flow_lookups
restates them as four searches advanced in one loop (ASN and blacklist, source and destination), each
retiring on its own.  What can go wrong there shows only when the four differ -- one ends at its first
probe beside one at full depth, one table is empty beside a deep one, one address is local -- and when
an address sits exactly on a range end or an interval start.  The corpus enumerates those classes:

  addresses  every ASN range start and end of the master tables and every first address of an elementary
             blacklist interval of every document, each with its two neighbours (clipped at 0 and
             all-ones); 0.0.0.0, 255.255.255.255, ::, ::1, all-ones; every is_lan_ip edge of both
             families from both sides; the edges of the configured lan_v6 prefixes; the own addresses;
             IPv6 range ends that differ in one word only (each of words 0-3), that carry across words,
             and whose deciding word is 0x7fffffff on one side and 0x80000000 on the other
  pairs      each pair is two flows, one per packet direction (ports carry no service name, so the key
             stored is the one sent): neighbours and a stride over the core addresses (all four
             local / public combinations), equal addresses, interval starts among themselves and against
             core addresses, and per ladder step a first-probe ASN hit beside a full-depth miss
  ladder     eleven steps (steps()) over the same resident flows: ASN tables of 0, 1, 2, 3, 4, 5, 7, 8, 9, 16,
             17 kept ranges per family (handed over unsorted, with start > end rows, a duplicate range
             with another record, adjacent ranges, single addresses, a nested triple, ranges over LAN
             space), blacklist documents of 0, 1, 2, 3 and about 930 elementary intervals per family
             (a /0, the all-ones /32 and /128 that never close, adjacent CIDRs of one list, one range
             in two lists, host bits set, list 63, 64 lists), own tables of 0, 1 and FB_MAX_OWN_IPS
             entries, lan_v6 tables of 0, 1 and FB_MAX_LAN_V6 entries with /1, /64, /127 and /128

The restatement works on int addresses and shares nothing with oracle/oracle.c: Db::from_tsv's filter
and stable sort and Db::lookup's probe sequence (src/asn_db.rs:111-166; the path is returned, since with
overlapping ranges the probe sequence decides the answer), the literal blacklist scan through
ipaddress.ip_network containment (src/blacklists.rs:205-260), is_lan_ip and the own-address membership
(src/ip.rs:55-156), and the per-flow rule that a local address gets no lookup (src/packets.rs:429-485).
tests/test_addrspace_oracle.py pins it against the C oracle and asserts the census on the CPU;
tests/test_gpu_addrspace.py sweeps the device."""
import collections
import functools
import ipaddress

import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.sessions import Protocol, Session, SessionPacketData

V4, V6 = 2, 10
TOP = {V4: (1 << 32) - 1, V6: (1 << 128) - 1}
LOCAL_SRC, LOCAL_DST, SELF_SRC, SELF_DST = 1, 2, 4, 8
FIELDS = ("flags", "src_asn", "dst_asn", "src_blacklists", "dst_blacklists")
SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17)
FWD_PORTS, REV_PORTS = (40001, 40003), (40005, 40007)  # no service names: no key is swapped


def ip4(s):
    return int(ipaddress.IPv4Address(s))


def ip6(s):
    return int(ipaddress.IPv6Address(s))


def w6(a, b, c, d):
    """An IPv6 address from its four key words (word 0 most significant)."""
    return (a << 96) | (b << 64) | (c << 32) | d


def words(fam, v):
    """The four key words of an address."""
    return (v, 0, 0, 0) if fam == V4 else tuple((v >> (96 - 32 * k)) & 0xFFFFFFFF for k in range(4))


def text(fam, v):
    return str(ipaddress.IPv4Address(v) if fam == V4 else ipaddress.IPv6Address(v))


def near(fam, v):
    """An address and its two neighbours, clipped at 0 and all-ones."""
    return [x for x in (v - 1, v, v + 1) if 0 <= x <= TOP[fam]]


# ---- the restatement: ASN ---------------------------------------------------------------------------
def asn_prepare(rows):
    """Db::from_tsv (src/asn_db.rs:111-137): rows [(start, end, record)] in file order; start > end is
    skipped, then `records.sort()` -- stable, by (start, end) as far as a lookup can tell."""
    return sorted((r for r in rows if r[0] <= r[1]), key=lambda r: (r[0], r[1]))


Lookup = collections.namedtuple("Lookup", "record path hit low")  # low: where a miss ended


def asn_lookup(table, ip):
    """Db::lookup (src/asn_db.rs:144-166) over a prepared table: the record (-1: None) and the probes."""
    low, high, path = 0, len(table), []
    while low < high:
        mid = (low + high) >> 1
        start, end, rec = table[mid]
        path.append(mid)
        if start <= ip and ip <= end:
            return Lookup(rec, tuple(path), True, mid)
        elif ip < start:
            high = mid
        else:
            low = mid + 1
    return Lookup(-1, tuple(path), False, low)


def asn_endings(table, ip, lk):
    """The census classes of one search's ending."""
    n, out = len(table), set()
    if lk.hit:
        if len(lk.path) == 1:
            out.add("hit_first")
        if len(lk.path) == n.bit_length():  # a bisection of n entries probes at most floor(log2 n) + 1
            out.add("hit_last")
        s, e, _ = table[lk.low]
        if sum(1 for r in table if (r[0], r[1]) == (s, e)) > 1:
            out.add("hit_dup")
    elif n:
        if any(r[0] <= ip <= r[1] for r in table):
            out.add("miss_inside")
        elif lk.low == 0:
            out.add("miss_left")
        elif lk.low == n:
            out.add("miss_right")
        else:
            out.add("miss_between")
        if len(lk.path) == n.bit_length():
            out.add("miss_full_depth")
    return out


ENDINGS = ("hit_first", "hit_last", "hit_dup", "miss_inside", "miss_left", "miss_right", "miss_between")


def deciding_words(table, ip, lk):
    """For every comparison an IPv6 search makes (ip against start, then against end): the first key word
    in which the two differ and whether that word's top bit differs -> {(word, top_bit_differs)}."""
    out = set()
    for mid in lk.path:
        for other in table[mid][:2]:
            a, b = words(V6, ip), words(V6, other)
            for k in range(4):
                if a[k] != b[k]:
                    out.add((k, (a[k] ^ b[k]) >> 31 == 1))
                    break
    return out


# ---- the restatement: blacklists ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nets(doc):
    return tuple((ipaddress.ip_network(c, strict=False), l) for c, l in doc)


def bl_mask(doc, fam, ip):
    """is_ip_in_blacklist for every list (src/blacklists.rs:205-260): doc is ((cidr text, list), ...);
    bit l is set iff some range of list l contains the address (IpNet::contains: never across families)."""
    a = ipaddress.IPv4Address(ip) if fam == V4 else ipaddress.IPv6Address(ip)
    m = 0
    for net, l in _nets(doc):
        if a in net:
            m |= 1 << l
    return m


@functools.lru_cache(maxsize=None)
def bl_intervals(doc, fam):
    """The elementary intervals of one family of a document, from the literal scan alone: every network's
    first address and the address behind its last are candidates; a candidate whose mask equals its
    predecessor's starts nothing -> ((first address, mask), ...)."""
    pts = set()
    for net, _ in _nets(doc):
        if net.version == (4 if fam == V4 else 6):
            pts.add(int(net.network_address))
            if int(net.broadcast_address) != TOP[fam]:
                pts.add(int(net.broadcast_address) + 1)
    out = []
    for p in sorted(pts):
        m = bl_mask(doc, fam, p)
        if not out or out[-1][1] != m:
            out.append((p, m))
    return tuple(out)


def bl_search(intervals, ip):
    """The bisection for the first interval starting above ip -> (mask of the one before it, probes)."""
    lo, hi, n = 0, len(intervals), 0
    while lo < hi:
        mid = (lo + hi) >> 1
        n += 1
        if ip < intervals[mid][0]:
            hi = mid
        else:
            lo = mid + 1
    return (intervals[lo - 1][1] if lo else 0), n


# ---- the restatement: flags ---------------------------------------------------------------------------
def is_lan_v4(v):
    """is_lan_ipv4_fast, src/ip.rs:55-91."""
    if v == 0 or v == 0xFFFFFFFF:
        return True
    if (v >> 24) == 127 or (v >> 28) == 0xE or (v >> 16) == 0xA9FE or (v >> 24) == 10:
        return True
    if (v >> 24) == 172 and 16 <= ((v >> 16) & 0xFF) <= 31:
        return True
    return (v >> 16) == 0xC0A8


def is_lan_v6(v, lan):
    """is_local_ipv6 then is_lan_ipv6_fast (src/ip.rs:112-156); lan: [(address, prefix)], the network
    numbers being apply_mask_v6 of the addresses (src/ip.rs:44-51)."""
    seg0 = v >> 112
    if v == 0 or v == 1:
        return True
    if (seg0 & 0xFFC0) == 0xFE80 or (seg0 & 0xFF00) == 0xFF00 or (seg0 & 0xFE00) == 0xFC00:
        return True
    for net, prefix in lan:
        mask = 0 if prefix == 0 else (TOP[V6] << (128 - prefix)) & TOP[V6]
        if (v & mask) == (net & mask):
            return True
    return False


def is_lan(fam, v, lan):
    return is_lan_v4(v) if fam == V4 else is_lan_v6(v, lan)


def is_own(own, fam, v):
    """own_ips.contains(&ip): an IpAddr equals another of its own family only."""
    return any(f == fam and a == v for f, a in own)


# ---- the ladder ---------------------------------------------------------------------------------------
def _r4(a, b):
    return ip4(a), ip4(b)


def _r6(a, b):
    return ip6(a), ip6(b)


# Master range lists in priority order: a table of n kept ranges is the first n.  1-3 are a nested triple
# (the outer range sorts first, so a search that leaves the inner two to the right misses an address the
# outer one contains), 4 repeats 3 with another record, 5 is adjacent to 3 (end + 1 == start).
MASTER4 = [_r4("20.0.0.0", "20.255.255.255"), _r4("20.1.0.0", "20.1.0.255"), _r4("20.2.0.0", "20.2.0.255"),
           _r4("20.2.0.0", "20.2.0.255"), _r4("20.2.1.0", "20.2.1.255"), _r4("5.5.5.5", "5.5.5.5"),
           _r4("10.0.0.0", "10.255.255.255"),                                     # LAN space
           _r4("0.0.0.0", "0.0.0.255"), _r4("255.255.255.0", "255.255.255.255"),   # the two ends of the space
           _r4("100.0.0.0", "100.0.0.0"), _r4("100.0.0.1", "100.0.0.1"),           # adjacent single addresses
           _r4("192.168.0.0", "192.168.255.255"),                                 # LAN space
           _r4("1.0.0.0", "1.0.0.255"), _r4("1.0.1.0", "1.0.1.255"), _r4("128.0.0.0", "128.0.0.255"),
           _r4("200.0.0.0", "200.0.0.0"), _r4("223.255.255.0", "223.255.255.255")]
MASTER6 = [_r6("2001:db8::", "2001:db8:ffff:ffff:ffff:ffff:ffff:ffff"), _r6("2001:db8:1::", "2001:db8:1::ff"),
           _r6("2001:db8:2::", "2001:db8:2::ff"), _r6("2001:db8:2::", "2001:db8:2::ff"),
           _r6("2001:db8:2::100", "2001:db8:2::1ff"), _r6("2400::5", "2400::5"),
           _r6("fc00::", "fdff:ffff:ffff:ffff:ffff:ffff:ffff:ffff"),              # LAN space
           _r6("::", "::ff"), _r6("ffff:ffff:ffff:ffff:ffff:ffff:ffff:ff00", "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff"),
           (w6(0x26000000, 1, 2, 0x10), w6(0x26000000, 1, 2, 0x20)),              # ends differ in word 3 only
           (w6(0x26010000, 1, 0x10, 5), w6(0x26010000, 1, 0x20, 5)),              # ... word 2
           (w6(0x26020000, 0x10, 7, 5), w6(0x26020000, 0x20, 7, 5)),              # ... word 1
           (w6(0x26030000, 3, 7, 5), w6(0x26040000, 3, 7, 5)),                    # ... word 0
           (w6(0x27000000, 0, 0, 0), w6(0x27000000, 0, 0xFFFFFFFF, 0xFFFFFFFF)),  # end + 1 carries across two words
           (w6(0x27000000, 1, 0, 0), w6(0x27000000, 1, 0, 0xFF)),                 # ... into this start
           (w6(0x2A000000, 5, 0x7FFFFF00, 0), w6(0x2A000000, 5, 0x7FFFFFFF, 0xFFFFFFFF)),  # deciding word 0x7fffffff
           (w6(0x2A000000, 5, 0x80000000, 0), w6(0x2A000000, 5, 0x80000000, 0xFF))]        # ... against 0x80000000
assert len(MASTER4) == len(MASTER6) == max(SIZES)
RECORD0 = {V4: 1, V6: 101}  # a range's record is RECORD0 + its master index; 900 + k: a row that must be dropped


def asn_rows(fam, n):
    """The table of n kept ranges as handed over: last range first (so the duplicate pair arrives in the
    order 4, 3 and the stable sort must keep it), with two start > end rows among them (n = 0: only
    those for IPv6, nothing at all for IPv4)."""
    m = (MASTER4 if fam == V4 else MASTER6)[:n]
    rows = [(s, e, RECORD0[fam] + k) for k, (s, e) in enumerate(m)][::-1]
    if n or fam == V6:
        s, e = (MASTER4 if fam == V4 else MASTER6)[1]
        rows.insert(len(rows) // 2, (e, s, 900))
        rows.append((TOP[fam], 0, 901))
    return rows


OWN4 = ip4("93.184.216.34")
OWN6 = w6(OWN4, 0, 0, 0)  # the same 32 bits in word 0, the other words zero

# configured lan_v6 prefixes (public space, so they decide the flag) -> (address with host bits, prefix)
P1 = (ip6("2a00::77"), 1)                    # ::/1: last inside 7fff:..:ffff, first outside 8000::
P64 = (ip6("2001:db8:abcd:12::1"), 64)
P127 = (ip6("2620:0:0:1::7"), 127)
P128 = (ip6("2620:0:0:2::9"), 128)


def _lan_full(flip):
    """FB_MAX_LAN_V6 entries: the /64, /127 and /128 in the first, a middle and the last position."""
    fill = [(w6(0x3FFF0000 + k, 0, 0, 0), 64) for k in range(N.FB_MAX_LAN_V6 - 3)]
    t = [P64] + fill[:30] + [P127] + fill[30:] + [P128]
    return t[::-1] if flip else t


def _own_full(flip):
    """FB_MAX_OWN_IPS entries: OWN4 first and OWN6 last (flip: the other way round); between them the key
    words of OWN4's neighbour as an IPv6 entry (that IPv4 corpus address must not be flagged), one more
    corpus address that is own (OWN4's 32 bits in word 3), and addresses no flow has."""
    fill = [(V6, w6(OWN4 + 1, 0, 0, 0)), (V6, w6(0, 0, 0, OWN4))]
    fill += [(V4, ip4("198.51.100.0") + k) for k in range(N.FB_MAX_OWN_IPS - 2 - len(fill))]
    t = [(V4, OWN4)] + fill + [(V6, OWN6)]
    return t[::-1] if flip else t


# ---- blacklist documents: level -> ((cidr, list), ...) per family -------------------------------------
DENSE, BLOCKS = 880, 20
TOP1_END, TOP2_START, CARRY_END = MASTER6[15][1], MASTER6[16][0], MASTER6[13][1]


def _deep4():
    d = [("30.0.%d.%d/32" % (j >> 8, j & 255), j % 61) for j in range(DENSE)]        # adjacent, lists differ
    d += [("40.%d.0.4/30" % k, k % 64) for k in range(BLOCKS)]
    d += [("10.0.0.0/8", 62), ("192.168.0.0/16", 62), ("50.0.0.0/16", 61), ("255.255.255.255/32", 63),
          ("20.2.0.0/24", 3), ("20.2.0.0/25", 4)]
    return tuple(d)


def _deep6():
    d = [("a000::%x/128" % j, j % 61) for j in range(DENSE)]
    d += [("a100:%x::4/126" % k, k % 64) for k in range(BLOCKS)]
    d += [("fc00::/7", 62), ("2001:db8::/32", 61), ("ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff/128", 63),
          (text(V6, TOP2_START) + "/128", 7), (text(V6, TOP1_END) + "/128", 8), (text(V6, CARRY_END) + "/128", 9),
          ("2620:0:0:1::/64", 10)]
    return tuple(d)


BL4 = ((),
       (("0.0.0.0/0", 63),),                                                    # one interval, never closed
       (("8.8.8.0/25", 0), ("8.8.8.128/25", 0)),                                # adjacent, one list: they merge
       (("8.8.8.77/24", 5), ("8.8.8.0/24", 6), ("255.255.255.255/32", 63)),     # host bits; one range, two lists
       _deep4())
BL6 = ((),
       (("ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff/128", 63),),
       (("2620:0:0:5::/65", 2), ("2620:0:0:5:8000::/65", 2)),
       (("::/0", 0), ("2001:db8::1/33", 1), ("2001:db8:8000::/33", 1)),
       _deep6())
BL_COUNTS = (0, 1, 2, 3)  # levels 0-3 give exactly their number of intervals; level 4 about 930

Step = collections.namedtuple("Step", "idx n4 n6 rows4 rows6 asn4 asn6 l4 l6 doc own lan")
_L4 = (4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 0)   # with SIZES: (no IPv4 range, deep intervals) at step 0, the reverse at 10
_L6 = (0, 3, 2, 1, 0, 4, 3, 2, 1, 0, 4)   # IPv6 takes SIZES backwards: (17 ranges, no interval) at 0, the reverse at 10
_OWN = ([], [(V4, OWN4)], _own_full(False), [], [(V6, OWN6)], _own_full(True), [], [(V4, OWN4)], _own_full(False),
        [(V6, OWN6)], [])
_LAN = ([], [P64], _lan_full(False), [], [P1], _lan_full(True), [], [P127], _lan_full(False), [P128], [])


@functools.lru_cache(maxsize=None)
def step(k):
    n4, n6 = SIZES[k], SIZES[len(SIZES) - 1 - k]
    rows4, rows6 = asn_rows(V4, n4), asn_rows(V6, n6)
    return Step(k, n4, n6, rows4, rows6, asn_prepare(rows4), asn_prepare(rows6), _L4[k], _L6[k],
                BL4[_L4[k]] + BL6[_L6[k]], tuple(_OWN[k]), tuple(_LAN[k]))


def steps():
    return [step(k) for k in range(len(SIZES))]


LARGEST = 5  # about 930 intervals in both families, full own and lan_v6 tables


def with_blacklists(st, other):
    """`st` with the blacklists of `other`."""
    return st._replace(l4=other.l4, l6=other.l6, doc=other.doc)


def with_asn(st, other):
    return st._replace(n4=other.n4, n6=other.n6, rows4=other.rows4, rows6=other.rows6, asn4=other.asn4, asn6=other.asn6)


def empty_step(like):
    """`like` with no ASN range and no blacklist: every record -1, every mask 0, the flags as before."""
    return like._replace(n4=0, n6=0, rows4=[], rows6=[], asn4=[], asn6=[], l4=0, l6=0, doc=())


# ---- the restatement: per flow ------------------------------------------------------------------------
def fam_doc(st, fam):
    """The step's ranges of one family (IpNet::contains is false across families, so a scan for an address
    of the other family finds nothing in them)."""
    return BL4[st.l4] if fam == V4 else BL6[st.l6]


@functools.lru_cache(maxsize=None)
def _mask_cached(fam, level, ip):
    return bl_mask((BL4 if fam == V4 else BL6)[level], fam, ip)


def step_mask(st, fam, ip):
    return _mask_cached(fam, st.l4 if fam == V4 else st.l6, ip)


def lookup_ip(st, fam, ip):
    """get_asn + the blacklist scan for one address, without the local rule -> (Lookup, mask)."""
    return asn_lookup(st.asn4 if fam == V4 else st.asn6, ip), step_mask(st, fam, ip)


def enrich_key(st, key):
    """What a new session gets (src/packets.rs:429-485); key: (protocol, family, src, sport, dst, dport) as
    the table stores it -> {field: value} and the two Lookups (None for a local address)."""
    _, fam, src, _, dst, _ = key
    ls, ld = is_lan(fam, src, st.lan), is_lan(fam, dst, st.lan)
    flags = (LOCAL_SRC if ls else 0) | (LOCAL_DST if ld else 0) | (SELF_SRC if is_own(st.own, fam, src) else 0) | \
        (SELF_DST if is_own(st.own, fam, dst) else 0)
    a, ma = (None, 0) if ls else lookup_ip(st, fam, src)
    b, mb = (None, 0) if ld else lookup_ip(st, fam, dst)
    return dict(flags=flags, src_asn=a.record if a else -1, dst_asn=b.record if b else -1, src_blacklists=ma,
                dst_blacklists=mb), (a, b)


# ---- arrays for the device and the C oracle -----------------------------------------------------------
def asn_array(rows, fam):
    t = np.zeros(len(rows), dtype=N.ASN_RANGE_DTYPE)
    for i, (s, e, rec) in enumerate(rows):
        t[i]["start"], t[i]["end"], t[i]["record"], t[i]["as_number"] = words(fam, s), words(fam, e), rec, 64500 + rec
    return t


def cidr_array(doc):
    """The document as fb_cidr entries, host bits left as written."""
    t = np.zeros(len(doc), dtype=N.CIDR_DTYPE)
    for i, (c, l) in enumerate(doc):
        addr, prefix = c.split("/")
        a = ipaddress.ip_address(addr)
        fam = V4 if a.version == 4 else V6
        t[i]["addr"], t[i]["family"], t[i]["prefix"], t[i]["list"] = words(fam, int(a)), fam, int(prefix), l
    return t


def ip_array(ips):
    """[(family, address)] -> fb_ip entries (the own-address table, or a lookup's input)."""
    t = np.zeros(len(ips), dtype=N.FB_IP_DTYPE)
    for i, (fam, v) in enumerate(ips):
        t[i]["addr"], t[i]["family"] = words(fam, v), fam
    return t


def lan_pairs(st):
    """The step's lan_v6 table as FlodbaddGpuCapture.set_lan_v6 / capture.lan_v6_table take it."""
    return [(text(V6, a), p) for a, p in st.lan]


# ---- addresses ----------------------------------------------------------------------------------------
LAN_EDGES4 = ["9.255.255.255", "10.0.0.0", "10.255.255.255", "11.0.0.0", "172.15.255.255", "172.16.0.0",
              "172.31.255.255", "172.32.0.0", "169.253.255.255", "169.254.0.0", "169.254.255.255", "169.255.0.0",
              "126.255.255.255", "127.0.0.0", "127.255.255.255", "128.0.0.0", "192.167.255.255", "192.168.0.0",
              "192.168.255.255", "192.169.0.0", "223.255.255.255", "224.0.0.0", "239.255.255.255", "240.0.0.0"]
LAN_EDGES6 = ["fe7f:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "fe80::", "febf:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "fec0::",
              "feff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "ff00::", "fbff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "fc00::",
              "fdff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "fe00::"]


def _prefix_edges(net, prefix):
    """The first and last address inside a prefix and the ones just outside."""
    mask = (TOP[V6] << (128 - prefix)) & TOP[V6]
    lo = net & mask
    hi = lo | (TOP[V6] ^ mask)
    return [x for x in (lo - 1, lo, hi, hi + 1) if 0 <= x <= TOP[V6]]


@functools.lru_cache(maxsize=None)
def core_addresses(fam):
    """Everything but the deep documents' interval starts, ascending."""
    out = set()
    for s, e in (MASTER4 if fam == V4 else MASTER6):
        out.update(near(fam, s) + near(fam, e))
    for doc in (BL4 if fam == V4 else BL6)[:4]:
        for p, _ in bl_intervals(doc, fam):
            out.update(near(fam, p))
    out.update([0, 1, 2, TOP[fam], TOP[fam] - 1])
    if fam == V4:
        out.update(ip4(a) for a in LAN_EDGES4)
        out.update([OWN4, OWN4 + 1, ip4("8.8.8.8"), ip4("150.1.2.3")])
    else:
        out.update(ip6(a) for a in LAN_EDGES6)
        out.update([OWN6, OWN6 + 1, w6(0, 0, 0, OWN4), ip6("2a00::1"), ip6("a000:ffff::1")])
        for net, prefix in (P1, P64, P127, P128):
            out.update(_prefix_edges(net, prefix))
    return tuple(sorted(out))


@functools.lru_cache(maxsize=None)
def bulk_addresses(fam):
    """The deep document's interval starts and their neighbours that the core does not hold, ascending."""
    out = set()
    for p, _ in bl_intervals((BL4 if fam == V4 else BL6)[4], fam):
        out.update(near(fam, p))
    return tuple(sorted(out - set(core_addresses(fam))))


def addresses(fam):
    return core_addresses(fam) + bulk_addresses(fam)


# ---- pairs and flows ----------------------------------------------------------------------------------
def _depth_pairs(fam):
    """Per ladder step: a core address whose ASN search hits at its first probe beside one whose search
    misses at full depth (both public under that step's configuration)."""
    out = []
    for st in steps():
        table = st.asn4 if fam == V4 else st.asn6
        if len(table) < 2:
            continue
        first = full = None
        for a in core_addresses(fam):
            if is_lan(fam, a, st.lan):
                continue
            lk = asn_lookup(table, a)
            if first is None and lk.hit and len(lk.path) == 1:
                first = a
            if full is None and not lk.hit and len(lk.path) == len(table).bit_length():
                full = a
        if first is not None and full is not None:
            out.append((first, full))
    return out


@functools.lru_cache(maxsize=None)
def pairs(fam):
    """Ordered address pairs, each once."""
    c, b = core_addresses(fam), bulk_addresses(fam)
    out = []
    for i, a in enumerate(c):
        out += [(a, c[(i + 1) % len(c)]), (a, c[(7 * i + 3) % len(c)])]
    out += [(a, a) for a in c[::9]]                                        # equal addresses
    out += [(x, c[(5 * i) % len(c)]) for i, x in enumerate(b[::8])]        # a deep interval search beside a core one
    rest = [x for i, x in enumerate(b) if i % 8]
    half = len(rest) // 2
    out += [(rest[i], rest[i + half]) for i in range(half)] + [(x, c[0]) for x in rest[2 * half:]]
    out += _depth_pairs(fam)
    seen, uniq = set(), []
    for p in out:
        if p not in seen and (p[1], p[0]) not in seen:
            seen.add(p)
            uniq.append(p)
    return tuple(uniq)


@functools.lru_cache(maxsize=None)
def keys():
    """Every flow of the corpus as its stored key (protocol, family, src, sport, dst, dport), in packet order:
    each pair forward and reversed, on different ports."""
    out = []
    for fam in (V4, V6):
        for i, (a, b) in enumerate(pairs(fam)):
            proto = 6 if i % 3 else 17
            out.append((proto, fam, a, FWD_PORTS[0], b, FWD_PORTS[1]))
            out.append((proto, fam, b, REV_PORTS[0], a, REV_PORTS[1]))
    assert len(set(out)) == len(out)
    return tuple(out)


def packet(key):
    proto, fam, src, sport, dst, dport = key
    mk = ipaddress.IPv4Address if fam == V4 else ipaddress.IPv6Address
    s = Session(Protocol(proto), mk(src), sport, mk(dst), dport)
    return SessionPacketData(s, 100, 120, 2 if proto == 6 else None)  # (SYN: no key is reversed)


@functools.lru_cache(maxsize=None)
def parsed():
    """The corpus as fb_parsed_pkt records (one packet per flow), read-only."""
    from flodbadd_amd.sessions import packets_to_parsed
    a = packets_to_parsed([packet(k) for k in keys()])
    a.setflags(write=False)
    return a


def key_of(rec):
    """A record's key fields (fb_flow_rec, fb_pkt_out) as a corpus key."""
    fam = int(rec["family"])

    def addr(w):
        return int(w[0]) if fam == V4 else w6(*(int(x) for x in w))
    return (int(rec["protocol"]), fam, addr(rec["src_ip"]), int(rec["src_port"]), addr(rec["dst_ip"]),
            int(rec["dst_port"]))


def key_records(ks):
    """Corpus keys as fb_flow_rec records (only the key fields set) for coracle.enrich_keys."""
    t = np.zeros(len(ks), dtype=N.FLOW_REC_DTYPE)
    for i, (proto, fam, src, sport, dst, dport) in enumerate(ks):
        t[i]["src_ip"], t[i]["dst_ip"] = words(fam, src), words(fam, dst)
        t[i]["src_port"], t[i]["dst_port"], t[i]["protocol"], t[i]["family"] = sport, dport, proto, fam
    return t


def describe(key):
    proto, fam, src, sport, dst, dport = key
    fmt = "%s %s:%d -> %s:%d" if fam == V4 else "%s [%s]:%d -> [%s]:%d"
    return fmt % ("TCP" if proto == 6 else "UDP", text(fam, src), sport, text(fam, dst), dport)


def describe_path(lk):
    if lk is None:
        return "local: no search"
    return "probes %s, %s" % (list(lk.path), "hit" if lk.hit else "miss at %d" % lk.low)


@functools.lru_cache(maxsize=None)
def expected(k):
    """The restatement over every corpus key under step k -> {key: ({field: value}, (Lookup, Lookup))}."""
    st = step(k)
    return {key: enrich_key(st, key) for key in keys()}


# ---- census -------------------------------------------------------------------------------------------
def census():
    """Which outcome classes the corpus reaches over the ladder -> {class: count}.  Every entry must be
    positive (tests/test_addrspace_oracle.py); all of it follows from the restatement alone."""
    c = collections.Counter()
    for st in steps():
        exp = expected(st.idx)
        iv = {V4: bl_intervals(fam_doc(st, V4), V4), V6: bl_intervals(fam_doc(st, V6), V6)}
        for key, (f, (a, b)) in exp.items():
            fam, tag = key[1], "v4" if key[1] == V4 else "v6"
            table = st.asn4 if fam == V4 else st.asn6
            c["%s_local_%d%d" % (tag, bool(f["flags"] & LOCAL_SRC), bool(f["flags"] & LOCAL_DST))] += 1
            for bit, name in ((LOCAL_SRC, "local_src"), (LOCAL_DST, "local_dst"), (SELF_SRC, "self_src"), (SELF_DST, "self_dst")):
                c["%s_%s_%s" % (tag, name, "set" if f["flags"] & bit else "clear")] += 1
            c["equal_addresses"] += key[2] == key[4]
            for ip, lk in ((key[2], a), (key[4], b)):
                if lk is None:
                    c["%s_local_in_asn_range" % tag] += any(r[0] <= ip <= r[1] for r in table)
                    c["%s_local_in_blacklist" % tag] += step_mask(st, fam, ip) != 0
                    continue
                for e in asn_endings(table, ip, lk):
                    c["%s_%s" % (tag, e)] += 1
                nb = bl_search(iv[fam], ip)[1]
                c["asn_longer_than_bl"] += len(lk.path) > nb > 0
                c["bl_longer_than_asn"] += nb > len(lk.path) > 0
                c["asn_empty_bl_deep"] += len(table) == 0 and nb >= 9
                c["bl_empty_asn_deep"] += len(iv[fam]) == 0 and len(lk.path) >= 4
                if fam == V6:
                    for k, topbit in deciding_words(table, ip, lk):
                        c["v6_decided_at_word_%d" % k] += 1
                        c["v6_top_bit_differs"] += topbit
            if a is not None and b is not None:
                la, lb = len(a.path), len(b.path)
                c["%s_src_%s_dst" % (tag, "shorter_than" if la < lb else "equal_to" if la == lb else "longer_than")] += 1
                full = len(table).bit_length()
                c["%s_first_hit_beside_full_miss" % tag] += a.hit and la == 1 and not b.hit and lb == full and full > 1
                c["%s_full_miss_beside_first_hit" % tag] += b.hit and lb == 1 and not a.hit and la == full and full > 1
    return c


def census_classes():
    """The names census() must fill."""
    out = ["equal_addresses", "asn_longer_than_bl", "bl_longer_than_asn", "asn_empty_bl_deep", "bl_empty_asn_deep",
           "v6_top_bit_differs"] + ["v6_decided_at_word_%d" % k for k in range(4)]
    for tag in ("v4", "v6"):
        out += ["%s_local_%d%d" % (tag, s, d) for s in (0, 1) for d in (0, 1)]
        out += ["%s_%s_%s" % (tag, n, v) for n in ("local_src", "local_dst", "self_src", "self_dst") for v in ("set", "clear")]
        out += ["%s_%s" % (tag, e) for e in ENDINGS]
        out += ["%s_src_%s_dst" % (tag, r) for r in ("shorter_than", "equal_to", "longer_than")]
        out += ["%s_first_hit_beside_full_miss" % tag, "%s_full_miss_beside_first_hit" % tag,
                "%s_local_in_asn_range" % tag, "%s_local_in_blacklist" % tag]
    return out
