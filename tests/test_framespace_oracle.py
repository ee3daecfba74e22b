"""The frame-decode corpora of tests/framespace.py are right and sharp, on the CPU: the two
restatements (coracle.parse_classify, what the GPU tests compare with, and pyoracle.run_batch) agree
on every frame under every filter; a head's class and record do not depend on its start alignment; the
first decodable cut of every shape equals a table written by hand from the header sizes, and the
decoded length grows by one per byte from there to its cap; a decoder that may see the bytes behind
caplen decides differently for at least one cut of EVERY shape (so a kernel that looks one field too
far cannot pass); and the field sweeps reach every class from every IHL x doff pair."""
import numpy as np
import pytest

import framespace as fsp
from oracle import coracle, pyoracle

N_SHAPES = 42
N_CUTS, CUTS_BYTES = 38328, 1041299
N_FIELDS = 9378
N_ENDS = 3184
SESSION, DNS, DROP, FILTERED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def space():
    """The corpora and the C oracle's results under filter All; read-only."""
    sh = fsp.shapes()
    fr, of, tags = fsp.cuts(sh)
    ff, fo, kinds = fsp.fields()
    mem, cases = fsp.buffer_ends(sh)
    s = dict(shapes=sh, cuts=(fr, of), tags=tags, fields=(ff, fo), kinds=kinds, mem=mem, cases=cases,
             cuts_ref=coracle.parse_classify(fsp.cfg(2), fr, of), fields_ref=coracle.parse_classify(fsp.cfg(2), ff, fo))
    for a in (fr, of, tags, ff, fo, mem):
        a.setflags(write=False)
    return s


def test_corpus_sizes_and_classes(space):
    assert len(space["shapes"]) == N_SHAPES and set(space["shapes"]) == set(fsp.THRESHOLDS)
    fr, of = space["cuts"]
    assert (len(of) - 1, len(fr)) == (N_CUTS, CUTS_BYTES)
    assert N_CUTS == 3 * 4 * sum(len(x) + 1 for x in space["shapes"].values())
    assert np.bincount(space["cuts_ref"][2], minlength=3).tolist() == CUTS_CLASSES
    assert len(space["fields"][1]) - 1 == N_FIELDS
    assert np.bincount(space["fields_ref"][2], minlength=3).tolist() == FIELDS_CLASSES
    assert len(space["cases"]) == N_ENDS == 4 * sum(len(space["shapes"][k]) + 1 for k in fsp.END_SHAPES)
    assert len(fsp.END_SHAPES) >= 10
    # zero-length frames at both ends of every shape, pads of every length
    tags, ln = space["tags"], np.diff(of.astype(np.int64))
    for piece in (fsp.HEAD, fsp.TAIL):
        z = tags[(tags["piece"] == piece) & (ln == 0)]
        assert len(z) == 4 * N_SHAPES
    assert set(ln[tags["piece"] == fsp.PAD].tolist()) == {0, 1, 2, 3}


CUTS_CLASSES = [2400, 160, 35768]  # SESSION, DNS, DROP under filter All
FIELDS_CLASSES = [2627, 1737, 5014]


def _assert_restatements_agree(flt, frames, offs):
    out, dns, cls, st = coracle.parse_classify(fsp.cfg(flt), frames, offs)
    classes, records, pdns, pst = pyoracle.run_batch(fsp.pycfg(flt), frames, offs)
    assert classes == cls.tolist()
    assert len(records) == len(out)
    for r, row in zip(records, out):
        want = pyoracle.record_to_row(r)
        for k, v in want.items():
            got = row[k].tolist() if isinstance(v, list) else int(row[k])
            assert got == v, (k, got, v, int(row["pkt_index"]))
    assert [(int(d["pkt_index"]), int(d["payload_offset"]), int(d["payload_length"]), int(d["protocol"]),
             int(d["family"])) for d in dns] == pdns
    for k, v in pst.items():
        assert int(st[0][k]) == v, k
    return set(classes)


@pytest.mark.parametrize("flt", [0, 1, 2])
@pytest.mark.parametrize("corpus", ["cuts", "fields"])
def test_restatements_agree(space, corpus, flt):
    seen = _assert_restatements_agree(flt, *space[corpus])
    if corpus == "cuts":  # (the field sweeps use one global address pair: nothing is local)
        assert seen == ({SESSION, DNS, DROP} if flt == 2 else {SESSION, DNS, DROP, FILTERED})


def test_restatements_agree_on_buffer_ends(space):
    """Case by case: the one-frame batch mem[base : base + a + c] with offsets [a, a + c]."""
    cfg, pcfg, mem = fsp.cfg(2), fsp.pycfg(2), space["mem"]
    seen = set()
    for name, a, c, base in space["cases"]:
        buf, offs = mem[base: base + a + c], np.array([a, a + c], dtype=np.uint32)
        out, dns, cls, st = coracle.parse_classify(cfg, buf, offs)
        classes, records, pdns, pst = pyoracle.run_batch(pcfg, buf, offs)
        assert classes == cls.tolist(), (name, a, c)
        assert len(records) == len(out) and len(pdns) == len(dns)
        for r, row in zip(records, out):
            for k, v in pyoracle.record_to_row(r).items():
                assert (row[k].tolist() if isinstance(v, list) else int(row[k])) == v, (name, a, c, k)
        for d, p in zip(dns, pdns):
            assert (int(d["pkt_index"]), int(d["payload_offset"]), int(d["payload_length"])) == p[:3], (name, a, c)
        for k, v in pst.items():
            assert int(st[0][k]) == v, (name, a, c, k)
        seen.add(classes[0])
    assert seen == {SESSION, DNS, DROP}


def _per_frame(ref, offs):
    """(class, record bytes with pkt_index zeroed, DNS (offset within the frame, length, protocol,
    family)) per frame, zeros where a frame has none."""
    out, dns, cls, _ = ref
    n = len(cls)
    rec = np.zeros((n, 56), dtype=np.uint8)
    o = out.copy()
    o["pkt_index"] = 0
    rec[out["pkt_index"]] = o.view(np.uint8).reshape(-1, 56)
    d = np.zeros((n, 4), dtype=np.int64)
    i = dns["pkt_index"]
    d[i] = np.stack([dns["payload_offset"].astype(np.int64) - offs[:-1][i].astype(np.int64), dns["payload_length"],
                     dns["protocol"], dns["family"]], axis=1)
    return cls, rec, d


def test_alignment_invariance(space):
    """The corpus repeats the same (shape, c, piece) sequence for a = 0..3: class, record (apart from
    pkt_index) and the DNS payload's place within its frame are the same in all four."""
    tags, (fr, of) = space["tags"], space["cuts"]
    q = N_CUTS // 4
    t = tags.reshape(4, q)
    for a in range(4):
        assert (t[a]["a"] == a).all()
        for f in ("shape", "c", "piece"):
            assert (t[a][f] == t[0][f]).all()
    for flt in (0, 1, 2):
        ref = space["cuts_ref"] if flt == 2 else coracle.parse_classify(fsp.cfg(flt), fr, of)
        cls, rec, d = _per_frame(ref, of)
        heads = t[0]["piece"] != fsp.PAD  # (a pad frame's length is what differs)
        for a in range(1, 4):
            assert (cls.reshape(4, q)[a][heads] == cls.reshape(4, q)[0][heads]).all()
            assert (rec.reshape(4, q, 56)[a] == rec.reshape(4, q, 56)[0]).all()
            assert (d.reshape(4, q, 4)[a] == d.reshape(4, q, 4)[0]).all()
        assert (cls == DNS).sum() > 0 and rec.any()


def test_thresholds_by_hand(space):
    """fsp.THRESHOLDS (written from the header sizes) against both oracles: the first cut whose head
    is not DROP, every later cut decodable too, and the decoded length min(max(c - grow_from, 0), cap)
    -- one more per byte until the IP length field or the frame's end caps it."""
    tags, (fr, of) = space["tags"], space["cuts"]
    cls, rec, d = _per_frame(space["cuts_ref"], of)
    plen = rec[:, 40:44].copy().view("<u4").ravel()  # fb_pkt_out.packet_length
    assert coracle.PKT_OUT_DTYPE.fields["packet_length"][1] == 40
    names = list(space["shapes"])
    for si, name in enumerate(names):
        first, grow, cap = fsp.THRESHOLDS[name]
        want_cls = DNS if name.startswith("dns_") else SESSION
        for a in range(4):
            h = np.flatnonzero((tags["shape"] == si) & (tags["a"] == a) & (tags["piece"] == fsp.HEAD))
            assert tags["c"][h].tolist() == list(range(len(space["shapes"][name]) + 1))
            c_cls = cls[h]
            assert int(np.flatnonzero(c_cls != DROP)[0]) == first, (name, a)
            assert (c_cls[:first] == DROP).all() and (c_cls[first:] == want_cls).all(), (name, a)
            got = (d[h, 1] if want_cls == DNS else plen[h])[first:].tolist()
            assert got == [min(max(c - grow, 0), cap) for c in range(first, len(c_cls))], (name, a)
            assert max(got) == cap
            # the Python restatement, on the bare frames (a = 0 only: it is alignment-free)
            if a == 0:
                x = space["shapes"][name]
                for c in (first - 1, first, grow + 1, len(x)):
                    p = pyoracle.parse_packet_pcap(x[:c])
                    assert (p is None) == (c < first), (name, c)
                    if p is not None:
                        assert p[0] == ("dns" if want_cls == DNS else "session")
                        assert (p[2] if p[0] == "dns" else p[6]) == min(max(c - grow, 0), cap), (name, c)


def _greedy_class(buf):
    p = pyoracle.parse_packet_pcap(buf)
    return DROP if p is None else DNS if p[0] == "dns" else SESSION


def test_sharp_against_a_greedy_decoder(space):
    """Every head of at least 14 B decoded with the 80 bytes behind its caplen visible (the same start,
    the continuation in view): the class differs from the honest one for at least one cut of every
    shape, in (a) and in (c) -- a decoder that reads a field before the length rules allow it cannot
    agree with the oracle on any shape."""
    tags, (fr, of) = space["tags"], space["cuts"]
    cls = space["cuts_ref"][2]
    buf = fr.tobytes()
    hit, differing = set(), 0
    for i in np.flatnonzero((tags["piece"] == fsp.HEAD) & (tags["c"] >= 14)).tolist():
        if _greedy_class(buf[of[i]: of[i + 1] + 80]) != cls[i]:
            hit.add(int(tags["shape"][i]))
            differing += 1
    assert hit == set(range(N_SHAPES)), sorted(set(range(N_SHAPES)) - hit)
    assert differing > 7000
    mem, cfg = space["mem"], fsp.cfg(2)
    membytes = mem.tobytes()
    hit = set()
    for name, a, c, base in space["cases"]:
        if c >= 14:
            honest = coracle.parse_classify(cfg, mem[base: base + a + c], np.array([a, a + c], dtype=np.uint32))[2][0]
            if _greedy_class(membytes[base + a: base + a + c + 80]) != honest:
                hit.add(name)
    assert hit == set(fsp.END_SHAPES)


def test_fields_coverage(space):
    """(b): at least 1,000 frames of each class, every IHL x doff pair in both SESSION and DROP, many
    distinct decoded lengths."""
    out, dns, cls, _ = space["fields_ref"]
    assert min(np.bincount(cls, minlength=3).tolist()) >= 1000
    by = {SESSION: set(), DROP: set()}
    for k, c in zip(space["kinds"], cls.tolist()):
        if k[0] == "v4tcp" and c in by:
            by[c].add((k[1], k[2]))
    every = {(i, d) for i in range(16) for d in range(16)}
    assert by[SESSION] == every and by[DROP] == every
    assert len(set(out["packet_length"].tolist())) >= 50 and len(set(dns["payload_length"].tolist())) >= 50
    kinds = {k[0] for k in space["kinds"]}
    assert kinds == {"v4tcp", "v4udp", "v6tcp", "v6udp", "proto", "ethertype"}
    # the protocol and EtherType sweeps: only 6 / 17 and 0800 / 86DD decode
    for k, c in zip(space["kinds"], cls.tolist()):
        if k[0] == "proto":
            assert (c != DROP) == (k[2] in (6, 17)), k
        elif k[0] == "ethertype":
            assert (c != DROP) == (k[2] == (0x0800 if k[1] == 4 else 0x86DD)), k


def test_lan_variant_reaches_both_filters():
    """cuts(shapes(lan_v4=True)): GlobalOnly and LocalOnly each keep some sessions and filter others
    (All filters nothing), so the GPU runs of the variant exercise the LAN lookups on both sides."""
    fr, of, _ = fsp.cuts(fsp.shapes(lan_v4=True))
    for flt in (0, 1, 2):
        cls = coracle.parse_classify(fsp.cfg(flt), fr, of)[2]
        n = np.bincount(cls, minlength=4)
        assert n[SESSION] > 100 and (n[FILTERED] > 100) == (flt != 2) and n[DNS] > 0, (flt, n)
