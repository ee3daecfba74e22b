"""Frame-decode corpora (test helper, no tests): where fuzzframes.py samples mutations, these
enumerate the decode's thresholds -- every cut of every header shape at every start alignment, every
value of every length field around the sizes that matter, and every cut at the very end of the frame
buffer -- so a decoder that uses a field one byte early, or is right for one alignment only, meets a
frame that shows it.

  shapes()          name -> frame bytes (at most 140 B): IPv4 IHL {0, 4, 5, 6, 15} x {TCP doff 0, 5, 8, 15,
                    UDP}, IPv6 x the same five, DNS over TCP / UDP for v4 / v6 with port 53 on either side
                    (4-B payload: the TCP `plen < 2` rule has both sides), IP length fields shorter and
                    longer than the frame
  cuts(shapes)      (a) per start alignment a, shape X and cut c in 0..len(X): a pad frame of 0-3 B of 0xFF,
                    the head X[:c] at offset % 4 == a, the tail X[c:].  The bytes behind a head's caplen
                    are the valid continuation of its headers (a decoder that looks one field too far sees
                    plausible values, not zeros); zero-length frames occur at both ends of every shape
  fields()          (b) whole 140-B frames, one decode field swept: IHL x doff x total_length, doff x
                    payload_length, the protocol / next-header byte, the EtherType
  buffer_ends(...)  (c) one-frame batches whose frame ends at frames_bytes while its continuation lies in
                    memory right behind it: the range check against frames_bytes, per cut and alignment

THRESHOLDS is the hand table of each shape's first decodable cut, written from the header sizes (not
from an oracle); tests/test_framespace_oracle.py holds the oracles to it."""
import struct

import numpy as np

import framegen as fg

ALIGNMENTS = (0, 1, 2, 3)
PAYLOAD = b"abcdef"
MAX_FRAME = 140
IHLS = (0, 4, 5, 6, 15)
DOFFS = (0, 5, 8, 15)

# v4 TCP: own LAN address -> global; v4 UDP: LAN -> LAN; v6 TCP: configured LAN prefix -> global; v6 UDP:
# ULA -> link-local own address (tests configure lan_v6 / own_ips as test_gpu_fuzz_paths.py does), so
# every filter keeps some shapes and filters others
V4_TCP, V4_UDP = ("10.0.0.1", "93.184.216.34"), ("192.168.1.7", "10.9.8.7")
V6_TCP, V6_UDP = ("2001:db8:abcd:12::5", "2001:4860::8888"), ("fd12::5", "fe80::1")
V4_LAN = ("192.168.1.7", "10.9.8.7")  # shapes(lan_v4=True): both v4 addresses of every shape

LAN = [("fd12::", 16), ("2001:db8:abcd:12::1", 64)]  # as test_gpu_fuzz_paths.py: the table lookups are live
OWN = ["10.0.0.1", "192.168.1.7", "fe80::1"]


def cfg(flt):
    """The C oracle's configuration under LAN / OWN."""
    from flodbadd_amd.capture import lan_v6_table, own_ip_table
    from oracle import coracle
    return coracle.make_cfg(int(flt), lan_v6=lan_v6_table(LAN), own_ips=own_ip_table(OWN))


def pycfg(flt):
    """The Python restatement's configuration under LAN / OWN."""
    from oracle import coracle, pyoracle
    return pyoracle.Config.from_bitmap(coracle.default_bitmap(), session_filter=int(flt), lan_v6=LAN, own_ips=OWN)


TAG_DTYPE = np.dtype([("shape", "<i2"), ("c", "<i2"), ("a", "i1"), ("piece", "i1")])
PAD, HEAD, TAIL = 0, 1, 2


def _tcp(doff, client, payload=PAYLOAD, ports=None):
    # doff 0 / 5 client -> service port, doff 8 / 15 service port -> client (the key is swapped)
    sport, dport = ports or ((client, 443) if doff <= 5 else (443, client))
    flags = {0: fg.SYN, 5: fg.PSH | fg.ACK, 8: fg.SYN | fg.ACK, 15: fg.FIN | fg.ACK}[doff]
    return fg.tcp(sport, dport, flags, payload, doff=doff, options=b"\x01" * 40)


def _v4(pair, proto, l4, ihl=5, **kw):
    return fg.eth(0x0800, fg.ipv4(pair[0], pair[1], proto, l4, ihl=ihl, options=b"\x01" * 40, **kw))


def _v6(pair, nh, l4, **kw):
    return fg.eth(0x86DD, fg.ipv6(pair[0], pair[1], nh, l4, **kw))


def shapes(lan_v4=False):
    """name -> frame bytes, in a fixed order.  lan_v4: both IPv4 addresses of every shape are LAN
    addresses (LocalOnly then keeps the v4 sessions and filters the v6 TCP ones)."""
    t4, u4 = (V4_LAN, V4_LAN) if lan_v4 else (V4_TCP, V4_UDP)
    s = {}

    def cp():  # a client port per shape: every shape is a flow of its own
        return 40000 + len(s)

    for ihl in IHLS:
        for doff in DOFFS:
            s["v4_ihl%d_tcp%d" % (ihl, doff)] = _v4(t4, 6, _tcp(doff, cp()), ihl=ihl)
        s["v4_ihl%d_udp" % ihl] = _v4(u4, 17, fg.udp(cp(), 123, PAYLOAD), ihl=ihl)
    for doff in DOFFS:
        s["v6_tcp%d" % doff] = _v6(V6_TCP, 6, _tcp(doff, cp()))
    s["v6_udp"] = _v6(V6_UDP, 17, fg.udp(cp(), 123, PAYLOAD))
    for side in ("src", "dst"):
        for name, mk, pair, proto in (("dns_v4_tcp_", _v4, t4, 6), ("dns_v4_udp_", _v4, u4, 17),
                                      ("dns_v6_tcp_", _v6, V6_TCP, 6), ("dns_v6_udp_", _v6, V6_UDP, 17)):
            ports = (53, cp()) if side == "src" else (cp(), 53)
            l4 = _tcp(5, 0, b"\x00\x02hi", ports) if proto == 6 else fg.udp(ports[0], ports[1], b"hi!!")
            s[name + side] = mk(pair, proto, l4)
    s["v4_tot_short_padded"] = _v4(t4, 6, _tcp(5, cp()), total_length=46) + b"\0" * 11
    s["v4_tot_1400"] = _v4(t4, 6, _tcp(5, cp()), total_length=1400)
    s["v6_plen_21_padded"] = _v6(V6_TCP, 6, _tcp(5, cp()), payload_length=21) + b"\0" * 5
    s["v6_plen_3000"] = _v6(V6_TCP, 6, _tcp(5, cp()), payload_length=3000)
    assert len(s) >= 39 and max(len(f) for f in s.values()) == MAX_FRAME
    return s


# Per shape (first, grow_from, cap), from the header sizes: `first` is the smallest cut whose head is not
# DROP -- 14 (Ethernet) + the IP header (max(4 * IHL, 20), or 40) + 20 (TcpPacket::new) or 8
# (UdpPacket::new), and for DNS over TCP + the TCP header (hs = 20 for doff 5) + the 2-B length prefix.
# The decoded length (packet_length, or the DNS payload_length) is min(max(c - grow_from, 0), cap):
# grow_from is where the L4 payload starts (behind the TCP options: 4 * doff when doff > 5), cap what
# the IP length field or the frame's end leaves (6 = len(PAYLOAD), 4 or 4 - 2 for the DNS shapes).
THRESHOLDS = {
    "v4_ihl0_tcp0": (14 + 20 + 20, 14 + 20 + 20, 6), "v4_ihl0_tcp5": (14 + 20 + 20, 14 + 20 + 20, 6),
    "v4_ihl0_tcp8": (14 + 20 + 20, 14 + 20 + 32, 6), "v4_ihl0_tcp15": (14 + 20 + 20, 14 + 20 + 60, 6),
    "v4_ihl0_udp": (14 + 20 + 8, 14 + 20 + 8, 6),
    "v4_ihl4_tcp0": (14 + 20 + 20, 14 + 20 + 20, 6), "v4_ihl4_tcp5": (14 + 20 + 20, 14 + 20 + 20, 6),
    "v4_ihl4_tcp8": (14 + 20 + 20, 14 + 20 + 32, 6), "v4_ihl4_tcp15": (14 + 20 + 20, 14 + 20 + 60, 6),
    "v4_ihl4_udp": (14 + 20 + 8, 14 + 20 + 8, 6),
    "v4_ihl5_tcp0": (14 + 20 + 20, 14 + 20 + 20, 6), "v4_ihl5_tcp5": (14 + 20 + 20, 14 + 20 + 20, 6),
    "v4_ihl5_tcp8": (14 + 20 + 20, 14 + 20 + 32, 6), "v4_ihl5_tcp15": (14 + 20 + 20, 14 + 20 + 60, 6),
    "v4_ihl5_udp": (14 + 20 + 8, 14 + 20 + 8, 6),
    "v4_ihl6_tcp0": (14 + 24 + 20, 14 + 24 + 20, 6), "v4_ihl6_tcp5": (14 + 24 + 20, 14 + 24 + 20, 6),
    "v4_ihl6_tcp8": (14 + 24 + 20, 14 + 24 + 32, 6), "v4_ihl6_tcp15": (14 + 24 + 20, 14 + 24 + 60, 6),
    "v4_ihl6_udp": (14 + 24 + 8, 14 + 24 + 8, 6),
    "v4_ihl15_tcp0": (14 + 60 + 20, 14 + 60 + 20, 6), "v4_ihl15_tcp5": (14 + 60 + 20, 14 + 60 + 20, 6),
    "v4_ihl15_tcp8": (14 + 60 + 20, 14 + 60 + 32, 6), "v4_ihl15_tcp15": (14 + 60 + 20, 14 + 60 + 60, 6),
    "v4_ihl15_udp": (14 + 60 + 8, 14 + 60 + 8, 6),
    "v6_tcp0": (14 + 40 + 20, 14 + 40 + 20, 6), "v6_tcp5": (14 + 40 + 20, 14 + 40 + 20, 6),
    "v6_tcp8": (14 + 40 + 20, 14 + 40 + 32, 6), "v6_tcp15": (14 + 40 + 20, 14 + 40 + 60, 6),
    "v6_udp": (14 + 40 + 8, 14 + 40 + 8, 6),
    "dns_v4_tcp_src": (14 + 20 + 20 + 2, 14 + 20 + 20 + 2, 4 - 2),
    "dns_v4_tcp_dst": (14 + 20 + 20 + 2, 14 + 20 + 20 + 2, 4 - 2),
    "dns_v4_udp_src": (14 + 20 + 8, 14 + 20 + 8, 4), "dns_v4_udp_dst": (14 + 20 + 8, 14 + 20 + 8, 4),
    "dns_v6_tcp_src": (14 + 40 + 20 + 2, 14 + 40 + 20 + 2, 4 - 2),
    "dns_v6_tcp_dst": (14 + 40 + 20 + 2, 14 + 40 + 20 + 2, 4 - 2),
    "dns_v6_udp_src": (14 + 40 + 8, 14 + 40 + 8, 4), "dns_v6_udp_dst": (14 + 40 + 8, 14 + 40 + 8, 4),
    "v4_tot_short_padded": (14 + 20 + 20, 14 + 20 + 20, 6),  # total_length 46 = 20 + 20 + 6, 11 B of padding
    "v4_tot_1400": (14 + 20 + 20, 14 + 20 + 20, 6),          # the frame ends first
    "v6_plen_21_padded": (14 + 40 + 20, 14 + 40 + 20, 1),    # payload_length 21 = the TCP header + 1
    "v6_plen_3000": (14 + 40 + 20, 14 + 40 + 20, 6),
}

# the shapes of buffer_ends (every family, L4 protocol, options on either layer, one DNS divert)
END_SHAPES = ("v4_ihl5_tcp5", "v4_ihl5_tcp15", "v4_ihl6_tcp5", "v4_ihl15_tcp5", "v4_ihl15_udp", "v4_ihl5_udp",
              "v6_tcp5", "v6_tcp15", "v6_udp", "dns_v4_tcp_dst")


def cuts(shapes_):
    """(a) -> (frames uint8, offsets uint32[n + 1], tags TAG_DTYPE[n]): for every a, shape and c the
    three frames pad, head, tail (module docstring); the head's offset % 4 == a."""
    parts, lens, tags = [], [], []
    pos = 0
    for a in ALIGNMENTS:
        for si, x in enumerate(shapes_.values()):
            for c in range(len(x) + 1):
                pad = (a - pos) % 4
                assert (pos + pad) % 4 == a
                parts += [b"\xff" * pad, x]  # head + tail = x
                lens += [pad, c, len(x) - c]
                tags += [(si, c, a, PAD), (si, c, a, HEAD), (si, c, a, TAIL)]
                pos += pad + len(x)
    frames = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    tags = np.array(tags, dtype=TAG_DTYPE)
    heads = tags["piece"] == HEAD
    assert int(offs[-1]) == len(frames) and (offs[:-1][heads] % 4 == tags["a"][heads]).all()
    return frames, offs, tags


def _frame(et, ip, l4_at, l4):
    f = bytearray(b"\x5a" * MAX_FRAME)
    f[:14] = fg.MACS + struct.pack("!H", et)
    f[14:14 + len(ip)] = ip
    f[l4_at:l4_at + len(l4)] = l4
    return bytes(f)


def _v4_field(ihl, proto, total_length, l4):
    """A 140-B IPv4 frame: 20-B header with IHL and total_length as given, options 0x01, the L4 header
    where the IHL puts it (14 + max(4 * IHL, 20)), 0x5A behind."""
    ip = fg.ipv4(V4_TCP[0], V4_TCP[1], proto, b"", ihl=ihl, total_length=total_length, options=b"\x01" * 40)
    return _frame(0x0800, ip, 14 + max(4 * ihl, 20), l4)


def _v6_field(nh, payload_length, l4):
    return _frame(0x86DD, fg.ipv6(V6_TCP[0], V6_TCP[1], nh, b"", payload_length=payload_length), 54, l4)


def fields():
    """(b) -> (frames, offsets, kinds): `kinds` one tuple per frame, ("v4tcp", ihl, doff, total_length,
    dport), ("v4udp", ihl, total_length, dport), ("v6tcp", doff, payload_length, dport), ("v6udp",
    payload_length, dport), ("proto", family, value) or ("ethertype", family, value)."""
    out, kinds = [], []
    n4, n6 = MAX_FRAME - 14, MAX_FRAME - 54  # 126, 86: the IP packet / the IPv6 payload the caplen holds

    def tcp_hdr(doff, dport):
        return fg.tcp(40000, dport, fg.PSH | fg.ACK, doff=doff)[:20]

    for dport in (443, 53):
        for ihl in range(16):
            h = 4 * ihl
            for doff in range(16):
                d = max(4 * doff, 20)
                tls = {0, 19, 20, h - 1, h, h + 1, h + 19, h + 20, h + d - 1, h + d, h + d + 1, h + d + 2, h + d + 3,
                       n4 - 1, n4, n4 + 1, 65535}
                for tl in sorted(t for t in tls if t >= 0):
                    out.append(_v4_field(ihl, 6, tl, tcp_hdr(doff, dport)))
                    kinds.append(("v4tcp", ihl, doff, tl, dport))
            for tl in sorted(t for t in {0, 20, h - 1, h, h + 7, h + 8, h + 9, n4 - 1, n4, n4 + 1, 65535} if t >= 0):
                out.append(_v4_field(ihl, 17, tl, fg.udp(40000, dport)))
                kinds.append(("v4udp", ihl, tl, dport))
        for doff in range(16):
            d = max(4 * doff, 20)
            for pl in sorted({0, 19, 20, d - 1, d, d + 1, d + 2, d + 3, n6 - 1, n6, n6 + 1, 65535}):
                out.append(_v6_field(6, pl, tcp_hdr(doff, dport)))
                kinds.append(("v6tcp", doff, pl, dport))
        for pl in (0, 7, 8, 9, n6 - 1, n6, n6 + 1, 65535):
            out.append(_v6_field(17, pl, fg.udp(40000, dport)))
            kinds.append(("v6udp", pl, dport))
    for p in range(256):
        out.append(_v4_field(5, p, n4, tcp_hdr(5, 443)))
        kinds.append(("proto", 4, p))
        out.append(_v6_field(p, n6, tcp_hdr(5, 443)))
        kinds.append(("proto", 6, p))
    for et in (0x0800, 0x86DD, 0x8100, 0x88A8, 0x0806, 0x0008, 0xDD86, 0x0000, 0xFFFF):
        for fam, f in ((4, _v4_field(5, 6, n4, tcp_hdr(5, 443))), (6, _v6_field(6, n6, tcp_hdr(5, 443)))):
            out.append(f[:12] + struct.pack("!H", et) + f[14:])
            kinds.append(("ethertype", fam, et))
    assert all(len(f) == MAX_FRAME for f in out)
    frames, offs = fg.pack(out)
    return frames, offs, kinds


END_SLACK = 80    # bytes of 0xFF behind every shape: the allocation reaches that far past every frames_bytes
END_REGION = 256  # a (shape, a) region's size and alignment in `mem`


def buffer_ends(shapes_, names=END_SHAPES):
    """(c) -> (mem uint8, cases): `mem` is the physical buffer, one END_REGION-B region per (shape, a)
    holding a pad bytes of 0xFF, the whole shape, then 0xFF to the region's end (at least END_SLACK
    B).  A case is (name, a, c, base): the one-frame batch frames = mem[base:], offsets = [a, a + c],
    frames_bytes = a + c.  The continuation X[c:] lies right behind frames_bytes and is no part of
    the batch; the oracle is given mem[base : base + a + c] only."""
    mem, cases = [], []
    for name in names:
        x = shapes_[name]
        for a in ALIGNMENTS:
            assert a + len(x) + END_SLACK <= END_REGION
            base = len(mem) * END_REGION
            mem.append((b"\xff" * a + x).ljust(END_REGION, b"\xff"))
            cases += [(name, a, c, base) for c in range(len(x) + 1)]
    return np.frombuffer(b"".join(mem), dtype=np.uint8).copy(), cases
