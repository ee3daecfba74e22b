"""Enumerated DNS message corpora for the divert parse (test helper, no tests): the bytes a DNS
parser walks are attacker-controlled and self-referential (label lengths, compression pointers),
so the corpora enumerate the positions, values, lengths and alignments at which a parser can go
wrong instead of sampling them.  Every builder is deterministic and returns a list of `bytes`; no
message is longer than 600 bytes and no corpus has more than 70,000 messages.

    single_byte           three canonical messages: every byte x all 256 values, every truncation
    name_heads            all 65,536 values of the first two bytes of the question name
    label_masks           one label of 0..9 bytes at every offset mod 4, a 0x80 byte before / inside /
                          after it, ended by a root byte or a pointer; labels read out of the header
    stage_edge            total lengths and 16-bit fields, pointers, labels, RDATA across byte 250..258
    names_long            Display lengths around the 255-byte cut, reverse-lookup suffixes
    counts_and_sections   section counts, the address limit, OPT placement, RDATA bounds

The kernel-side reasons for the shapes (the dword-wide label masks, the 256-byte LDS stage) are in
DESIGN §3.6; tests/test_gpu_dns_corpora.py packs each corpus at every payload alignment.
"""
import struct

import dnsgen as G

CORPORA = ("single_byte", "name_heads", "label_masks", "stage_edge", "names_long", "counts_and_sections")
Q11 = struct.pack("!HH", 1, 1)  # QTYPE A, QCLASS IN


def ptr(off):
    return struct.pack("!H", 0xC000 | off)


def txt_rdata(n, fill=b"t"):
    """n bytes of TXT RDATA (n >= 1): strings of at most 255 bytes."""
    out = b""
    while n > 0:
        k = min(255, n - 1)
        out += bytes([k]) + fill * k
        n -= k + 1
    return out


# ---- single_byte -------------------------------------------------------------------------------
def canonical():
    """A query with OPT, a compressed CNAME + A + AAAA response, an MX / TXT / SOA / SRV response
    (231 bytes together)."""
    q = G.query(0x1234, "a.bc")
    r = (G.header(0x2345, True, qd=1, an=3) + G.question("w.ex") +                 # "ex" at 14
         G.rr(ptr(12), 5, b"\x01c" + ptr(14)) +                                    # CNAME c.ex, RDATA at 34
         G.rr(ptr(34), 1, G.a("192.0.2.1")) + G.rr(ptr(34), 28, G.aaaa("2001:db8::1")))
    m = (G.header(0x3456, True, qd=1, an=2, ns=1, ar=1) + G.question("m.ex", 15) +
         G.rr(ptr(12), 15, b"\x00\x0a\x01x" + ptr(14)) + G.rr(ptr(12), 16, b"\x02ab\x00") +
         G.rr(ptr(14), 6, ptr(12) + b"\x01h" + ptr(14) + bytes(range(1, 21))) +
         G.rr(ptr(12), 33, b"\x00\x01\x00\x02\x00\x35\x01t" + ptr(14)))
    return [q, r, m]


def single_byte():
    out = []
    for m in canonical():
        for i in range(len(m)):
            for v in range(256):
                out.append(m[:i] + bytes([v]) + m[i + 1:])
        out += [m[:k] for k in range(len(m) + 1)]
    return out


# ---- name_heads --------------------------------------------------------------------------------
def name_heads():
    """The id and flag bytes (01 'A' 01 00) read as labels when a pointer lands in the header; the
    filler is a chain of one-byte labels, so a long first label ends on a length byte or inside a
    label depending on its parity."""
    head = b"\x01A" + struct.pack("!HHHHH", 0x0100, 1, 0, 0, 0)
    tail = b"\x01a" * 35 + b"\x00" + Q11
    return [head + bytes([a, b]) + tail for a in range(256) for b in range(256)]


# ---- label_masks -------------------------------------------------------------------------------
_PREFIX = {1: b"", 3: b"\x01p", 0: b"\x02pp", 2: b"\x01p\x02pp"}  # content offset mod 4 -> labels in front


def label_masks(meta=False):
    """With meta=True returns (messages, [(content offset mod 4, L) or None]) for the coverage
    assertions; None marks the header-label messages and the 0xFF-tailed ones in front of them."""
    out, info = [], []
    content = b"abcdefghi"
    for o in range(4):
        for L in range(10):
            for term in (b"\x00", ptr(4)):  # offset 4 is the 0 byte of QDCOUNT = 1: the root
                # the label in the question itself, behind _PREFIX[o]
                name = _PREFIX[o] + bytes([L]) + content[:L] + term
                at = 12 + len(_PREFIX[o]) + 1  # the label's first content byte
                assert at % 4 == o
                base = G.header(0x4000 + L, False, qd=1) + name + Q11
                # the label behind a forward pointer, 0xFF bytes in front of its length byte
                pad = (o - 1 - 18) % 4
                far = G.header(0x5000 + L, False, qd=1) + ptr(18 + pad) + Q11 + b"\xff" * pad + bytes([L]) + \
                    content[:L] + term
                assert (18 + pad + 1) % 4 == o
                for msg, c0 in ((base, at), (far, 18 + pad + 1)):
                    out.append(msg)
                    info.append((o, L))
                    for k in range(-2, L + 2):  # 0x80 two before .. two after the content
                        m = bytearray(msg)
                        if c0 + k < len(m):
                            m[c0 + k] |= 0x80
                            out.append(bytes(m))
                            info.append((o, L))
    # labels read out of the header: a pointer to offset t = 0, 1, 2 where a length byte L stands,
    # its content in the id / flag bytes; each follows a message that ends in FF FF FF
    for t in range(3):
        for L in range(0, 4 - t + 1):
            n_bad = min(L, 4 - t - 1)
            for bad in [None] + list(range(n_bad)):
                h = bytearray(b"ABCD" + struct.pack("!HHHH", 1, 0, 0, 0))
                h[t] = L
                if t + L + 1 <= 3:  # a second label up to offset 3, so the walk ends on QDCOUNT's 0 byte
                    h[t + L + 1] = 3 - (t + L + 1)
                if bad is not None:
                    h[t + 1 + bad] |= 0x80
                out.append(G.query(0x6000, "ff.example", edns=False) + b"\xff\xff\xff")
                out.append(bytes(h) + ptr(t) + Q11)
                info += [None, None]
    return (out, info) if meta else out


# ---- stage_edge --------------------------------------------------------------------------------
_EDGE_Q = G.question("edge.example")  # 18 bytes: the first record starts at 30


def _edge_message(marker_rel, records, target, total=310):
    """header + question + TXT filler + records + TXT pad: records[0]'s byte `marker_rel` at `target`."""
    fill = target - marker_rel - (30 + 12)
    body = G.rr(ptr(12), 16, txt_rdata(fill)) + b"".join(records)
    n = 1 + len(records)
    left = total - (30 + len(body))
    if left >= 13:
        body += G.rr(ptr(12), 16, txt_rdata(left - 12, b"p"))
        n += 1
    return G.header(0x7000 + target, True, qd=1, an=n) + _EDGE_Q + body


def stage_edge():
    out = []
    for total in range(248, 265):  # an A answer in the last four bytes
        out.append(G.header(total, True, qd=1, an=2) + _EDGE_Q + G.rr(ptr(12), 16, txt_rdata(total - 30 - 12 - 16)) +
                   G.rr(ptr(12), 1, bytes([198, 51, 100, total & 255])))
        assert len(out[-1]) == total
    a_rr = G.rr(ptr(12), 1, G.a("203.0.113.77"))
    for target in range(250, 259):
        markers = [
            (12, [G.rr(ptr(12), 5, b"\x05label\x03two" + ptr(17)), a_rr]),        # a label's length byte
            (13, [G.rr(ptr(12), 5, b"\x06labels\x03two" + ptr(17)), a_rr]),       # a label's content
            (13, [G.rr(ptr(12), 5, b"\x06label\xe9\x03two" + ptr(17)), a_rr]),    # ... with a non-ASCII end
            (13, [G.rr(ptr(12), 5, b"\x06\xe9abels\x03two" + ptr(17)), a_rr]),    # ... and start
            (14, [G.rr(ptr(12), 5, b"\x01x" + ptr(12)), a_rr]),                   # the two bytes of a pointer
            (12, [G.rr(ptr(12), 5, b"\x03tgt" + ptr(17)), G.rr(ptr(target), 1, G.a("203.0.113.78"))]),  # a target
            (2, [a_rr]), (4, [a_rr]), (10, [a_rr]),                               # TYPE, CLASS, RDLENGTH
            (12, [a_rr]),                                                         # A RDATA
            (12, [G.rr(ptr(12), 28, G.aaaa("2001:db8:1:2:3:4:5:6")), a_rr]),      # AAAA RDATA
            (0, [G.rr(ptr(12), 28, G.aaaa("2001:db8::99"))]),                     # a record's owner pointer
        ]
        for rel, recs in markers:
            out.append(_edge_message(rel, recs, target))
            assert 290 <= len(out[-1]) <= 330
        # the same markers in a message that ends right behind them (no pad record)
        out.append(_edge_message(12, [a_rr], target, total=0))
    return out


# ---- names_long --------------------------------------------------------------------------------
def _labels(n, suffix=()):
    """Labels whose Display ('.'-joined) is exactly n bytes long and ends with `suffix`."""
    tail = ".".join(suffix)
    left = n - len(tail) - (1 if tail else 0)
    labs, k = [], 0
    while left > 0:
        take = min(63, left)
        if left - take == 1:  # a dot needs a label behind it
            take -= 1
        labs.append(chr(ord("a") + k % 26) * take)
        k += 1
        left -= take
        if left > 0:
            left -= 1
    labs += list(suffix)
    assert len(".".join(labs)) == n, (n, suffix)
    return labs


def _wire(labs):
    return b"".join(bytes([len(x)]) + x.encode("latin-1") for x in labs)


def _q_plain(tx, labs):
    return G.header(tx, False, qd=1) + _wire(labs) + b"\x00" + Q11


def _q_chain(tx, labs, split):
    """The first `split` labels in the question, then a pointer to the rest behind the question."""
    first = _wire(labs[:split])
    return G.header(tx, False, qd=1) + first + ptr(12 + len(first) + 2 + 4) + Q11 + _wire(labs[split:]) + b"\x00"


def names_long():
    out = []
    v4, v6 = ("in-addr", "arpa"), ("ip6", "arpa")
    for n in list(range(250, 261)) + [268, 280]:
        for sfx in ((), v4, v6):
            labs = _labels(n, sfx)
            out.append(_q_plain(n, labs))
            out.append(_q_chain(n, labs, 2))
            if sfx:
                out.append(_q_chain(n, labs, len(labs) - 1))  # the jump inside the suffix
    # the bare suffixes and their near misses (Display lengths 8, 9, 10, 12, 13, 14)
    for k, nm in enumerate(["ip6.arpa", "xip6.arpa", "x.ip6.arpa", "in-addr.arpa", "xin-addr.arpa", "x.in-addr.arpa",
                            "x.ip6.arpb", "y.in-addr.arpa.x", "x.ip6xarpa", "in-addr.arpa.ip6.arpa"]):
        out.append(G.query(0x100 + k, nm, qtype=12))
    root = ptr(4)  # the 0 byte of QDCOUNT
    out.append(G.header(0x120, False, qd=1) + _wire(["ip6", "arpa"]) + root + Q11)             # "ip6.arpa." (9)
    out.append(G.header(0x121, False, qd=1) + _wire(["1", "in-addr", "arpa"]) + root + Q11)    # suffix, then a dot
    out.append(G.header(0x122, False, qd=1) + _wire(["1", "ip6", "arpa"]) + root + Q11)
    # a suffix assembled across a pointer, the pointer before / inside / after the dot
    for k, cut in enumerate((4, 5)):
        out.append(_q_chain(0x130 + k, ["4", "3", "2", "1", "in-addr", "arpa"], cut))
        out.append(_q_chain(0x134 + k, ["f", "e", "d", "c", "ip6", "arpa"], cut))
    out.append(G.header(0x138, False, qd=1) + ptr(18) + Q11 + _wire(["7", "in-addr", "arpa"]) + b"\x00")  # all behind it
    for k, nm in enumerate(["4.3.2.1.IN-ADDR.ARPA", "4.3.2.1.in-addr.ARPA", "f.e.IP6.ARPA", "f.e.ip6.arpA"]):
        out.append(G.query(0x140 + k, nm, qtype=12))
    return out


# ---- counts_and_sections -----------------------------------------------------------------------
def counts_and_sections():
    out = []
    own = ptr(12)
    q = G.question("cs.example")  # 16 bytes: a second question or the first record starts at 28
    a4 = [G.rr(own, 1, G.a("10.1.0.%d" % i)) for i in range(12)]
    a6 = [G.rr(own, 28, G.aaaa("2001:db8::%x" % i)) for i in range(12)]

    def msg(tx, an=(), ns=(), ar=(), qd=1, qs=None, counts=None):
        c = counts or (qd, len(an), len(ns), len(ar))
        return G.header(tx, True, *c) + (q * qd if qs is None else qs) + b"".join(an) + b"".join(ns) + b"".join(ar)

    # question counts
    out.append(msg(1, an=[G.rr(G.name("x.example"), 1, G.a("10.0.0.1"))], qd=0))
    out.append(msg(2, qd=2, qs=q + G.question("second.example", 28)))
    out.append(msg(3, an=[G.rr(ptr(28), 1, G.a("10.0.0.3"))], qd=2, qs=q + G.question("second.example", 28)))
    out.append(msg(4, counts=(65535, 0, 0, 0)))
    out.append(msg(5, counts=(65535, 65535, 65535, 65535)))
    # address limits
    for n in (7, 8, 9):
        out.append(msg(10 + n, an=a4[:n]))
        out.append(msg(20 + n, an=a6[:n]))
    out.append(msg(30, an=[x for p in zip(a4[:4], a6[:4]) for x in p]))
    out.append(msg(31, an=[x for p in zip(a4[:5], a6[:5]) for x in p][:9]))
    out.append(msg(32, an=a4[:8] + [G.rr(own, 5, G.name("c", 12))]))  # a ninth answer that is no address
    # addresses outside the answer section
    out.append(msg(40, an=a4[:1], ns=a4[1:3], ar=a6[:2]))
    out.append(msg(41, ns=a4[:2]))
    out.append(msg(42, ar=a6[:1] + a4[:1]))
    out.append(msg(43, an=a4[:8], ns=a4[8:9]))   # the ninth address is not an answer: nothing truncated
    out.append(msg(44, an=a6[:1], ns=[G.rr(own, 2, G.name("ns", 12))], ar=a4[:9]))
    # OPT placement
    opt = G.opt()
    out.append(msg(50, ar=[opt, a4[0], a6[0]]))
    out.append(msg(51, ar=[a4[0], opt, a6[0]]))
    out.append(msg(52, ar=[a4[0], a6[0], opt]))
    out.append(msg(53, ar=[opt, opt]))
    out.append(msg(54, ar=[opt, a4[0], opt]))
    out.append(msg(55, ar=[opt, b"\x00\x00\x29"]))                     # a second OPT start, three bytes left
    out.append(msg(56, ar=[opt, b"\x00\x00"]))                         # ... two bytes left: a record cut short
    out.append(msg(57, ar=[b"\x00\x00\x29"]))
    out.append(msg(58, ar=[b"\x00\x00"]))
    out.append(msg(59, ar=[G.opt(rdata=b"\x00\x0a\x00\x02zz")]))
    out.append(msg(60, ar=[G.opt(rdata=b"\x00\x0a\x00\x02zz")[:-1]]))  # rdlen one past the end
    out.append(msg(61, ar=[opt[:10]]))
    out.append(msg(62, an=[G.rr(own, 41, b"")]))                        # type 41 in the answer section
    out.append(msg(63, an=[G.rr(own, 41, b"", cls=1232)]))              # ... with a UDP size for a class
    out.append(msg(64, an=[opt]))                                       # 00 00 29 where no OPT may start
    out.append(msg(65, ns=[opt], ar=[opt]))
    # SOA: 19 and 20 bytes behind its two names
    for k, n in enumerate((19, 20, 21)):
        out.append(msg(70 + k, ns=[G.rr(own, 6, G.name("ns1", 12) + G.name("host", 12) + b"\x07" * n)]))
        out.append(msg(75 + k, ns=[G.rr(own, 6, G.name("ns1.example") + G.name("") + b"\x07" * n)]))
    out.append(msg(78, ns=[G.rr(own, 6, G.name("ns1", 12))]))           # no second name
    # MX / SRV: the name up to, and one byte past, the end of RDATA; pointing outside RDATA
    for k, (typ, pre) in enumerate(((15, b"\x00\x0a"), (33, b"\x00\x01\x00\x02\x00\x35"))):
        nm = G.name("mail.cs.example")
        full = G.rr(own, typ, pre + nm)
        cut = G.rr(own, typ, pre + nm[:-1]) + nm[-1:]  # rdlen ends before the root byte
        out.append(msg(80 + 10 * k, an=[full, a4[0]]))
        out.append(msg(81 + 10 * k, an=[cut, a4[0]]))
        out.append(msg(82 + 10 * k, an=[G.rr(own, typ, pre + b"\x04mail" + ptr(12)), a4[0]]))
        out.append(msg(83 + 10 * k, an=[G.rr(own, typ, pre + b"\x04mail" + ptr(12)[:1]) + ptr(12)[1:], a4[0]]))
        out.append(msg(84 + 10 * k, an=[G.rr(own, typ, pre + ptr(15)), a4[0]]))
        fwd = 28 + 12 + len(pre) + 2 + 12  # the next record's RDATA: a TXT that also reads as the name "abc"
        out.append(msg(85 + 10 * k, an=[G.rr(own, typ, pre + ptr(fwd)), G.rr(own, 16, b"\x03abc\x00")]))
        out.append(msg(86 + 10 * k, an=[G.rr(own, typ, pre)]))
        out.append(msg(87 + 10 * k, an=[G.rr(own, typ, pre + b"\x00")]))
        out.append(msg(88 + 10 * k, an=[G.rr(own, typ, pre[:-1])]))
    # TXT: strings that end at, and one byte past, rdlen; rdlen 0
    out.append(msg(100, an=[G.rr(own, 16, b"\x03abc\x02de"), a4[0]]))
    out.append(msg(101, an=[G.rr(own, 16, b"\x03abc\x03de") + b"f", a4[0]]))
    out.append(msg(102, an=[G.rr(own, 16, b""), a4[0]]))
    out.append(msg(103, an=[G.rr(own, 16, b"\x00"), a4[0]]))
    out.append(msg(104, an=[G.rr(own, 16, b"\x03abc\x00"), a4[0]]))
    out.append(msg(105, an=[G.rr(own, 16, b"\x03abc\x01") + b"x", a4[0]]))
    # rdlen equal to, and one more than, the bytes left
    for typ in (10, 1, 16):
        body = {10: b"nullnull", 1: G.a("10.9.8.7"), 16: b"\x03abc"}[typ]
        whole = G.rr(own, typ, body)
        out.append(msg(110 + typ, an=[whole]))
        out.append(msg(130 + typ, an=[whole[:-1]]))
        out.append(msg(150 + typ, an=[whole[:12]]))  # nothing behind RDLENGTH
        out.append(msg(170 + typ, an=[whole[:11]]))  # RDLENGTH itself cut
    return out


def build(name):
    assert name in CORPORA
    return globals()[name]()
