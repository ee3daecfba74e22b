"""CPU: the two restatements of the DNS divert parse (oracle/oracle.c orc_dns_parse and
tests/dnsref.py, written separately from DESIGN §3.6; parity with dns-parser 0.8.0 itself stays
unpinned) agree on every message of the enumerated corpora (tests/dnscorpus.py), the corpora reach
what they are built to reach (computed from the reference results, so a corpus cannot go hollow),
and each of eight plausible parser mistakes, applied to a copy of dnsref, is caught by a named corpus.

Disagreements found while the second restatement was written: none.  The two agreed on all
126,780 corpus messages at the first comparison.
"""
import functools

import pytest

import dnscorpus as DC
import dnsref as R
from flodbadd_amd import _native as N
from oracle import coracle


@functools.lru_cache(maxsize=None)
def _corpus(name):
    return tuple(DC.build(name))


@functools.lru_cache(maxsize=None)
def _ref(name):
    """dnsref over a corpus, once: [(fields, name, addrs)].  Read-only for the tests."""
    return tuple(R.parse_fields(m) for m in _corpus(name))


def _oracle_plain(m):
    r, nm, ad = coracle.dns_parse(m)
    return tuple(r.tolist()), nm, [(int(a["family"]), tuple(int(w) for w in a["addr"])) for a in ad]


STATUS, FLAGS, NAME_LEN, N_ADDRS = 2, 3, 6, 7  # positions in the DNS_MSG_DTYPE field tuple


def test_field_positions():
    names = N.DNS_MSG_DTYPE.names
    assert (names[STATUS], names[FLAGS], names[NAME_LEN], names[N_ADDRS]) == ("status", "flags", "name_len", "n_addrs")


@pytest.mark.parametrize("name", DC.CORPORA)
def test_restatements_agree(name):
    msgs = _corpus(name)
    assert 0 < len(msgs) <= 70000 and max(len(m) for m in msgs) <= 600
    for m, ref in zip(msgs, _ref(name)):
        assert _oracle_plain(m) == ref, (name, m.hex())


def test_numpy_triple_matches_coracle():
    """dnsref.dns_parse returns what coracle.dns_parse returns, type for type."""
    for m in _corpus("counts_and_sections") + _corpus("names_long")[:20]:
        a, b = R.dns_parse(m, 7), coracle.dns_parse(m, 7)
        assert a[0].dtype == b[0].dtype and a[0].tobytes() == b[0].tobytes()
        assert a[1] == b[1] and a[2].dtype == b[2].dtype and a[2].tobytes() == b[2].tobytes()


def test_corpus_sizes():
    assert len(_corpus("single_byte")) == sum(257 * len(m) + 1 for m in DC.canonical())
    assert all(len(m) <= 120 for m in DC.canonical())
    assert len(_corpus("name_heads")) == 65536 == max(len(_corpus(c)) for c in DC.CORPORA)
    assert len(set(_corpus("name_heads"))) == 65536


def test_every_status_and_flag_is_reached():
    seen = {c: {r[0][STATUS] for r in _ref(c)} for c in DC.CORPORA}
    assert set().union(*seen.values()) == set(range(len(N.DNS_STATUS)))
    # where each corpus is meant to end up
    assert seen["single_byte"] == set(range(11))          # everything but a second OPT
    assert {0, 2, 3, 4, 5} <= seen["name_heads"]
    assert {0, 4, 5} <= seen["label_masks"]
    assert seen["names_long"] == {0}
    assert {0, 2, 10, 11} <= seen["counts_and_sections"]
    flags = {c: {r[0][FLAGS] for r in _ref(c)} for c in DC.CORPORA}
    cut = N.DNS_NAME_TRUNCATED
    assert any(f & cut and f & N.DNS_REVERSE for f in flags["names_long"])
    assert any(f & cut and not f & N.DNS_REVERSE for f in flags["names_long"])
    assert any(not f & cut and f & N.DNS_REVERSE for f in flags["names_long"])
    assert any(f & N.DNS_ADDRS_TRUNCATED for f in flags["counts_and_sections"])
    assert {r[0][N_ADDRS] for r in _ref("counts_and_sections")} >= {0, 1, 7, 8}


def test_names_long_lengths():
    refs = _ref("names_long")
    lens = {r[0][NAME_LEN] for r in refs}
    assert set(range(250, 256)) <= lens and {8, 9, 10, 12, 13, 14} <= lens
    for fields, name, _ in refs:
        assert len(name) == fields[NAME_LEN] <= 255
    # 255 is reached by a name that fits exactly and by longer ones that are cut
    at255 = [r[0][FLAGS] & N.DNS_NAME_TRUNCATED for r in refs if r[0][NAME_LEN] == 255]
    assert 0 in at255 and N.DNS_NAME_TRUNCATED in at255
    # the known answers among the short names
    by_name = {r[1]: bool(r[0][FLAGS] & N.DNS_REVERSE) for r in refs}
    assert by_name[b"x.ip6.arpa"] and by_name[b"x.in-addr.arpa"] and by_name[b"4.3.2.1.in-addr.arpa"]
    assert by_name[b"f.e.d.c.ip6.arpa"] and by_name[b"7.in-addr.arpa"] and by_name[b"in-addr.arpa.ip6.arpa"]
    for miss in (b"ip6.arpa", b"xip6.arpa", b"in-addr.arpa", b"xin-addr.arpa", b"ip6.arpa.", b"1.in-addr.arpa.",
                 b"4.3.2.1.IN-ADDR.ARPA", b"f.e.ip6.arpA", b"x.ip6.arpb", b"y.in-addr.arpa.x"):
        assert by_name[miss] is False, miss


def test_label_masks_coverage():
    msgs, info = DC.label_masks(meta=True)
    assert list(msgs) == list(_corpus("label_masks"))
    seen = {}
    for (fields, _, _), key in zip(_ref("label_masks"), info):
        if key is not None:
            seen.setdefault(key, set()).add(fields[STATUS])
    for o in range(4):
        for L in range(1, 10):
            assert {R.OK, R.LABEL_NOT_ASCII} <= seen[(o, L)], (o, L)
        assert R.OK in seen[(o, 0)]
    # the labels read out of the header: accepted when clean, label_not_ascii otherwise, and every
    # one of them stands behind a message that ends in FF FF FF
    header = [(m, r) for m, r, key in zip(msgs, _ref("label_masks"), info) if key is None]
    assert len(header) % 2 == 0 and len(header) >= 2 * 9
    for (prev, _), (m, r) in zip(header[0::2], header[1::2]):
        assert prev.endswith(b"\xff\xff\xff")
        dirty = any(b & 0x80 for b in m[:4])
        assert r[0][STATUS] == (R.LABEL_NOT_ASCII if dirty else R.OK), m.hex()
    assert {r[0][STATUS] for _, r in header[1::2]} == {R.OK, R.LABEL_NOT_ASCII}


def test_stage_edge_shapes():
    msgs = _corpus("stage_edge")
    assert set(range(248, 265)) <= {len(m) for m in msgs}
    ok = [r for r in _ref("stage_edge") if r[0][STATUS] == R.OK]
    assert len(ok) >= len(msgs) - 18 and all(r[0][N_ADDRS] >= 1 for r in ok)  # each ends in an address past the edge


def test_counts_and_sections_known_answers():
    by_id = {r[0][1]: r for r in _ref("counts_and_sections")}

    def st(tx):
        return N.DNS_STATUS[by_id[tx][0][STATUS]]

    assert st(1) == "ok" and by_id[1][0][FLAGS] == 0 and by_id[1][0][N_ADDRS] == 1  # no question, one address
    assert st(2) == "ok" and by_id[2][1] == b"cs.example" and st(3) == "ok"
    assert st(4) == "unexpected_eof" and st(5) == "unexpected_eof"
    for tx, n, cut in ((17, 7, False), (18, 8, False), (19, 8, True), (27, 7, False), (28, 8, False), (29, 8, True),
                       (30, 8, False), (31, 8, True), (32, 8, False), (43, 8, False)):
        assert by_id[tx][0][N_ADDRS] == n and bool(by_id[tx][0][FLAGS] & N.DNS_ADDRS_TRUNCATED) == cut, tx
    assert [by_id[tx][0][N_ADDRS] for tx in (40, 41, 42, 44)] == [1, 0, 0, 1]
    assert [st(tx) for tx in (50, 51, 52)] == ["ok"] * 3
    assert [st(tx) for tx in (53, 54, 55)] == ["additional_opt"] * 3
    assert [st(tx) for tx in (56, 57, 58, 60, 61)] == ["unexpected_eof"] * 5
    assert [st(tx) for tx in (59, 62, 63, 65)] == ["ok"] * 4 and st(64) == "ok"
    assert [st(tx) for tx in (70, 71, 72, 75, 76, 77)] == ["wrong_rdata_length", "ok", "ok"] * 2
    assert st(78) == "unexpected_eof"
    for base in (80, 90):
        assert [st(base + k) for k in range(9)] == ["ok", "unexpected_eof", "ok", "unexpected_eof", "ok", "ok",
                                                    "wrong_rdata_length", "ok", "wrong_rdata_length"], base
    assert [st(tx) for tx in range(100, 106)] == ["ok", "wrong_rdata_length", "wrong_rdata_length", "ok", "ok",
                                                  "wrong_rdata_length"]
    for typ in (10, 1, 16):
        assert [st(k + typ) for k in (110, 130, 150, 170)] == ["ok"] + ["unexpected_eof"] * 3


# ---- discrimination: a plausible mistake in the parser must change some corpus message's result ----
MUTANTS = [
    (R.SkipsFirstLabelByte, "label_masks"),
    (R.SkipsLastLabelByte, "label_masks"),
    (R.PointerMayRepeatTarget, "name_heads"),
    (R.SuffixIgnoresCase, "names_long"),
    (R.SuffixOfStoredName, "names_long"),
    (R.TruncatesAt255, "names_long"),
    (R.CollectsAuthority, "counts_and_sections"),
    (R.OptNeedsFourBytes, "counts_and_sections"),
]


@pytest.mark.parametrize("mutant,corpus", MUTANTS, ids=[m.__name__ for m, _ in MUTANTS])
def test_corpus_catches_mutant(mutant, corpus):
    wrong = mutant()
    caught = [m for m, ref in zip(_corpus(corpus), _ref(corpus)) if wrong.parse_fields(m) != ref]
    assert caught, "%s is not caught by %s" % (mutant.__name__, corpus)
    # and the mistake is a narrow one: most of the corpus does not notice
    assert len(caught) < len(_corpus(corpus)) // 2


def test_single_byte_also_catches_the_label_and_pointer_mutants():
    """The byte-enumeration corpus alone catches the three name-walk mutants too (a 0x80 written
    over the first / last byte of a label, a pointer rewritten to its own earlier target)."""
    for mutant in (R.SkipsFirstLabelByte, R.SkipsLastLabelByte, R.PointerMayRepeatTarget):
        wrong = mutant()
        assert any(wrong.parse_fields(m) != ref for m, ref in zip(_corpus("single_byte"), _ref("single_byte"))), mutant
