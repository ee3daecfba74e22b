"""GPU: k_dns_parse (fb_dns_parse_dev) against the oracle on the enumerated corpora of
tests/dnscorpus.py, byte for byte on fb_dns_msg, name[:name_len] and addrs[:n_addrs], with the
payloads packed so that every kernel path meets every message: back to back (the payload's offset
in its dword cycles with the lengths), dword-aligned, and with a 300-byte message in every wave
(the wave-wide choice then takes the mixed LDS / HBM instance instead of the LDS-only one).  Then the
edges no corpus reaches by itself: a last message that ends exactly at frames_bytes for every
frames_bytes mod 4 and payload alignment, records that lie outside the frame buffer, and raw calls
over poisoned outputs (the d_stats->n_dns bound, partial waves, the name's zero fill).

The oracle is pinned by a second restatement on the same corpora (tests/test_dns_corpora.py);
parity with dns-parser 0.8.0 itself stays unpinned.
"""
import functools

import numpy as np
import pytest

import dnscorpus as DC
import dnsgen as G
from flodbadd_amd import _native as N
from flodbadd_amd import dns as D
from flodbadd_amd.dns import parse_dns
from oracle import coracle

pytestmark = pytest.mark.gpu

MSG_B, IP_B = N.DNS_MSG_DTYPE.itemsize, N.FB_IP_DTYPE.itemsize
POISON = 0xA5


def _oracle(msgs):
    """(fb_dns_msg with pkt_index 0, names zero-padded to 256, addrs) of the oracle, as arrays."""
    n = len(msgs)
    om = np.zeros(n, dtype=N.DNS_MSG_DTYPE)
    on = np.zeros((n, N.FB_DNS_MAX_NAME), dtype=np.uint8)
    oa = np.zeros((n, N.FB_DNS_MAX_ADDRS), dtype=N.FB_IP_DTYPE)
    for i, m in enumerate(msgs):
        r, nm, ad = coracle.dns_parse(m, 0)
        om[i] = r
        on[i, : len(nm)] = np.frombuffer(nm, dtype=np.uint8)
        oa[i, : len(ad)] = ad
    for a in (om, on, oa):
        a.setflags(write=False)
    return om, on, oa


@functools.lru_cache(maxsize=None)
def _reference(name):
    """A corpus and the oracle's results, once (they do not depend on the packing).  Read-only."""
    msgs = DC.build(name)
    return msgs, _oracle(msgs)


# a valid response longer than the kernel's 256-byte stage: the wave that holds it runs MsgMixed
LONG = G.header(0x4C4C, True, qd=1, an=3) + G.question("long.example") + \
    G.rr(b"\xc0\x0c", 16, DC.txt_rdata(212)) + G.rr(b"\xc0\x0c", 5, b"\x04tail\xc0\x0c") + \
    G.rr(b"\xc0\x0c", 28, G.aaaa("2001:db8::4c"))
assert 290 <= len(LONG) <= 310


def _pack(msgs, align=1, front=0):
    """Payloads one after the other, each padded to `align`, behind `front` bytes -> (buffer, records)."""
    parts, off = [b"\xee" * front], np.zeros(len(msgs), dtype=np.int64)
    o = front
    for i, m in enumerate(msgs):
        off[i] = o
        gap = -len(m) % align
        parts += [m, b"\xee" * gap]
        o += len(m) + gap
    recs = np.zeros(len(msgs), dtype=N.DNS_OUT_DTYPE)
    recs["pkt_index"] = np.arange(len(msgs), dtype=np.uint32) * 3 + 7
    recs["payload_offset"] = off
    recs["payload_length"] = [len(m) for m in msgs]
    recs["protocol"], recs["family"] = 17, 2
    return np.frombuffer(b"".join(parts), dtype=np.uint8), recs


def _mismatch(got, exp, pkt_index):
    """Index of the first record whose fb_dns_msg, name[:name_len] or addrs[:n_addrs] differs, or None."""
    (gm, gn, ga), (em, en, ea) = got, exp
    em = em.copy()
    em["pkt_index"] = pkt_index
    n = len(em)
    bad = (gm.view(np.uint8).reshape(n, MSG_B) != em.view(np.uint8).reshape(n, MSG_B)).any(axis=1)
    keep = np.arange(N.FB_DNS_MAX_NAME)[None, :] < em["name_len"][:, None].astype(np.int64)
    bad |= ((gn != en) & keep).any(axis=1)
    keep = np.arange(N.FB_DNS_MAX_ADDRS)[None, :] < em["n_addrs"][:, None].astype(np.int64)
    ga8 = np.ascontiguousarray(ga).view(np.uint8).reshape(n, N.FB_DNS_MAX_ADDRS, IP_B)
    ea8 = np.ascontiguousarray(ea).view(np.uint8).reshape(n, N.FB_DNS_MAX_ADDRS, IP_B)
    bad |= ((ga8 != ea8).any(axis=2) & keep).any(axis=1)
    return int(np.flatnonzero(bad)[0]) if bad.any() else None


def _check_packing(name, how, front=0):
    msgs, exp = _reference(name)
    if how == "with_long":  # LONG is record 0, 64, 128, ...: 63 corpus messages behind each
        batch, where = [], []
        for k, m in enumerate(msgs):
            if k % 63 == 0:
                batch.append(LONG)
            where.append(len(batch))
            batch.append(m)
        where = np.array(where)
        assert batch[0] is LONG and all(batch[j] is LONG for j in range(0, len(batch), 64))
    else:
        batch, where = msgs, np.arange(len(msgs))
    buf, recs = _pack(batch, align=4 if how == "aligned4" else 1, front=front)
    if how == "packed" and len(msgs) > 64:
        assert set((recs["payload_offset"] & 3).tolist()) == {0, 1, 2, 3}
    if how == "aligned4":
        assert ((recs["payload_offset"] & 3) == front).all()
    gm, gn, ga = parse_dns(buf, recs)
    bad = _mismatch((gm[where], gn[where], ga[where]), exp, recs["pkt_index"][where])
    if bad is not None:
        o = coracle.dns_parse(msgs[bad], 0)
        pytest.fail("%s/%s front=%d message %d at offset %d: %s\n gpu %s %r\n ref %s %r" % (
            name, how, front, bad, int(recs["payload_offset"][where[bad]]), msgs[bad].hex(), gm[where[bad]],
            bytes(gn[where[bad]][: int(gm[where[bad]]["name_len"])]), o[0], o[1]))
    if how == "with_long":
        lm = np.arange(0, len(batch), 64)
        assert _mismatch((gm[lm], gn[lm], ga[lm]), tuple(np.repeat(a, len(lm), axis=0) for a in _oracle([LONG])),
                         recs["pkt_index"][lm]) is None


@pytest.mark.parametrize("how", ["packed", "aligned4", "with_long"])
@pytest.mark.parametrize("name", DC.CORPORA)
def test_corpus_vs_oracle(name, how):
    _check_packing(name, how)


@pytest.mark.parametrize("front", [1, 2, 3])
def test_stage_edge_at_every_alignment(front):
    """`front` bytes ahead of the buffer shift every payload: with the packed run above (front = 0),
    every length in 248..264 and every marker offset in 250..258 meets all four alignments, alone in
    LDS-or-mixed waves and beside a 300-byte message."""
    _check_packing("stage_edge", "packed", front)
    _check_packing("stage_edge", "with_long", front)
    _check_packing("stage_edge", "aligned4", front)  # every payload at the same alignment `front`


# ---- raw calls ---------------------------------------------------------------------------------
def _raw(buf, recs, n=None, n_dns=None, poison=None):
    """fb_dns_parse_dev over a device frame buffer of exactly len(buf) bytes -> (msgs, names, addrs)
    for all len(recs) records, the outputs filled with `poison` first."""
    lib = N.gpu_lib()
    cnt = len(recs)
    n = cnt if n is None else n
    bufs = []

    def dev(nbytes):
        bufs.append(N.DeviceBuffer(nbytes))
        return bufs[-1]

    try:
        d_fr = dev(len(buf)).upload(np.frombuffer(bytes(buf), dtype=np.uint8))
        d_dns = dev(recs.nbytes).upload(recs)
        d_msg, d_names = dev(cnt * MSG_B), dev(cnt * N.FB_DNS_MAX_NAME)
        d_addrs = dev(cnt * N.FB_DNS_MAX_ADDRS * IP_B)
        if poison is not None:
            for b in (d_msg, d_names, d_addrs):
                b.memset(poison)
        d_st = None
        if n_dns is not None:
            st = np.zeros(1, dtype=N.STATS_DTYPE)
            st["n_dns"] = n_dns
            d_st = dev(st.nbytes).upload(st)
        N.check(lib.fb_dns_parse_dev(D._ctx(), d_fr.ptr, len(buf), d_dns.ptr, n, d_st.ptr if d_st else None, d_msg.ptr,
                                     d_names.ptr, d_addrs.ptr, None))
        return (d_msg.download(np.zeros(cnt, dtype=N.DNS_MSG_DTYPE)),
                d_names.download(np.zeros((cnt, N.FB_DNS_MAX_NAME), dtype=np.uint8)),
                d_addrs.download(np.zeros((cnt, N.FB_DNS_MAX_ADDRS), dtype=N.FB_IP_DTYPE)))
    finally:
        for b in bufs:
            b.free()


def _end_message(length, tx):
    """A compressed response of exactly `length` bytes whose last four bytes are an A answer."""
    q = G.question("end.example")
    cname = G.rr(b"\xc0\x0c", 5, b"\x01c\xc0\x0c")
    fill = length - 12 - len(q) - len(cname) - 12 - 16
    owner = DC.ptr(12 + len(q) + 12)  # the CNAME's RDATA: c.end.example
    m = G.header(tx, True, qd=1, an=3) + q + cname + G.rr(b"\xc0\x0c", 16, DC.txt_rdata(fill)) + \
        G.rr(owner, 1, bytes([192, 0, 2, 0x80 | (tx & 0x7F)]))
    assert len(m) == length
    return m


@pytest.mark.parametrize("long", [False, True], ids=["lds", "mixed"])
def test_last_message_ends_at_frames_bytes(long):
    """The stage copy reads whole dwords through a range-checked descriptor of frames_bytes bytes: a
    last message that ends at frames_bytes when frames_bytes % 4 = tail != 0 has its final dword
    partly outside the range, and such a dword loads as 0: the kernel refills it from byte loads.
    (Found by single_byte/with_long, whose last message then lost its final byte.)  The device
    allocation is exactly frames_bytes long."""
    head = [G.query(1, "first.example"), G.response(2, "second.example", [("A", "198.51.100.2")])]
    for tail in range(4):
        for mis in range(4):
            front = b"".join(head)
            front += b"\xee" * ((mis - len(front)) % 4)
            length = (300 if long else 80) + (tail - mis - (300 if long else 80)) % 4
            last = _end_message(length, 16 * tail + mis)
            buf = front + last
            assert len(buf) % 4 == tail and len(front) % 4 == mis and (long or len(last) <= 256 - mis)
            recs = np.zeros(3, dtype=N.DNS_OUT_DTYPE)
            recs["pkt_index"] = [5, 6, 9]
            recs["payload_offset"] = [0, len(head[0]), len(front)]
            recs["payload_length"] = [len(head[0]), len(head[1]), len(last)]
            got = _raw(buf, recs)
            exp = _oracle(head + [last])
            assert exp[0][2]["status"] == 0 and exp[0][2]["n_addrs"] == 1
            assert exp[2][2][0]["addr"][0] == int.from_bytes(last[-4:], "big")
            bad = _mismatch(got, exp, recs["pkt_index"])
            assert bad is None, (tail, mis, bad, got[0][bad], exp[0][bad], got[2][bad][0], exp[2][bad][0])


def test_records_outside_the_frame_buffer():
    """A record that does not lie within frames_bytes is given length 0 (header_too_short, pkt_index
    kept, everything else zero) whatever its offset; its neighbours in the wave parse as usual."""
    msgs = DC.build("counts_and_sections")[:61]
    buf, packed = _pack(msgs)
    fb = len(buf)
    n = len(msgs)
    recs = np.zeros(n + 3, dtype=N.DNS_OUT_DTYPE)
    recs[:n] = packed
    last_len = int(recs["payload_length"][n - 1])
    recs[n] = (900, fb - last_len + 1, last_len, 17, 2, 0)       # one byte past frames_bytes
    recs[n + 1] = (901, 0xFFFFFFF0, 40, 17, 2, 0)
    recs[n + 2] = (902, int(recs["payload_offset"][5]), 0, 17, 2, 0)
    order = np.array([0, n, 1, 2, n + 1, 3, n + 2] + list(range(4, n)))  # the three in among the others
    recs = recs[order]
    assert len(recs) == 64
    gm, gn, ga = _raw(buf, recs, poison=POISON)
    inside = order < n
    assert _mismatch((gm[inside], gn[inside], ga[inside]), _oracle(msgs), recs["pkt_index"][inside]) is None
    for k in np.flatnonzero(~inside):
        exp = np.zeros(1, dtype=N.DNS_MSG_DTYPE)
        exp["pkt_index"], exp["status"] = recs["pkt_index"][k], 1
        assert gm[k].tobytes() == exp.tobytes(), (k, gm[k])
        assert (gn[k] == POISON).all() and (ga[k].view(np.uint8) == POISON).all()


@functools.lru_cache(maxsize=None)
def _raw_pool():
    """129 messages: long and short names of every length mod 4, cut names, 0..8 addresses, rejections."""
    a, b = DC.build("names_long"), DC.build("counts_and_sections")
    pool = [m for pair in zip(a, b) for m in pair][:129]
    return pool, _oracle(pool)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_raw_calls_over_poisoned_outputs(n):
    """Exactly min(n, d_stats->n_dns) records are written (n alone without d_stats); every other
    output byte keeps its poison: the records past the count, a name's bytes past the dword that
    holds its last byte (that dword's tail is zero), the address slots at and past n_addrs."""
    pool, (om, on, oa) = _raw_pool()
    buf, recs = _pack(pool)
    total = len(pool)
    for n_dns in (None, 0, n - 1, n, n + 5):
        gm, gn, ga = _raw(buf, recs, n=n, n_dns=n_dns, poison=POISON)
        w = n if n_dns is None else min(n, n_dns)
        assert _mismatch((gm[:w], gn[:w], ga[:w]), (om[:w], on[:w], oa[:w]), recs["pkt_index"][:w]) is None, (n, n_dns)
        assert (gm[w:].view(np.uint8) == POISON).all() and (gn[w:] == POISON).all(), (n, n_dns)
        assert (ga[w:].view(np.uint8) == POISON).all(), (n, n_dns)
        for i in range(w):
            nl, na = int(om[i]["name_len"]), int(om[i]["n_addrs"])
            up = (nl + 3) // 4 * 4
            assert not gn[i, nl:up].any() and (gn[i, up:] == POISON).all(), (n, n_dns, i, nl)
            if int(om[i]["status"]) == 0:
                assert (ga[i, na:].view(np.uint8) == POISON).all(), (n, n_dns, i, na)
    assert total == 129


def test_raw_pool_is_not_hollow():
    _, (om, _, _) = _raw_pool()
    ok = om[om["status"] == 0]
    assert {int(x) % 4 for x in ok["name_len"]} == {0, 1, 2, 3} and 255 in ok["name_len"]
    assert (ok["flags"] & N.DNS_NAME_TRUNCATED).any() and (om["status"] != 0).any()
    assert {0, 1, 7, 8} <= {int(x) for x in ok["n_addrs"]}
