"""CPU: the enrichment corpora of tests/addrspace.py -- its plain-Python restatement against the C oracle
(oracle/oracle.c orc_asn_* / orc_blacklist_mask / orc_enrich_keys) bit for bit on every corpus flow and
address under every ladder step, against the reference's known answers, against hand-worked records,
masks and probe paths, and the census: every outcome class the GPU sweep relies on is inhabited.  The
census conditions follow from the restatement alone; none is a measurement."""
import numpy as np
import pytest

import addrspace as A
from addrspace import V4, V6, ip4, ip6
from flodbadd_amd import _native as N
from flodbadd_amd.capture import lan_v6_table
from flodbadd_amd.enrich import asn_tables_from_tsv
from flodbadd_amd.sessions import words_to_ip
from oracle import coracle
from test_enrich_oracle import TSV

STEPS = list(range(len(A.SIZES)))


def _oracle_tables(st):
    return (coracle.asn_prepare(A.asn_array(st.rows4, V4), V4), coracle.asn_prepare(A.asn_array(st.rows6, V6), V6),
            A.cidr_array(st.doc))


def _rows_of(arr, fam):
    return [(int(words_to_ip(r["start"], fam)), int(words_to_ip(r["end"], fam)), int(r["record"])) for r in arr]


@pytest.mark.parametrize("k", STEPS)
def test_restatement_equals_the_c_oracle(k):
    """Prepared tables row for row, every field of every corpus flow, and every corpus address without the
    local rule."""
    st = A.step(k)
    a4, a6, cidrs = _oracle_tables(st)
    assert _rows_of(a4, V4) == st.asn4 and _rows_of(a6, V6) == st.asn6
    assert (len(st.asn4), len(st.asn6)) == (st.n4, st.n6)
    cfg = coracle.make_cfg(2, lan_v6=lan_v6_table(A.lan_pairs(st)), own_ips=A.ip_array(st.own))
    keys = A.keys()
    ref = coracle.enrich_keys(cfg, a4, a6, cidrs, A.key_records(keys))
    exp = A.expected(k)
    for i, key in enumerate(keys):
        want, paths = exp[key]
        for f in A.FIELDS:
            assert int(ref[i][f]) == want[f], (k, A.describe(key), f, int(ref[i][f]), want[f],
                                               [A.describe_path(p) for p in paths])
    for fam in (V4, V6):
        ips = A.addresses(fam)
        ra, rl = coracle.ip_lookup(a4, a6, cidrs, [A.text(fam, v) for v in ips])
        for v, x, m in zip(ips, ra, rl):
            lk, mask = A.lookup_ip(st, fam, v)
            assert (int(x), int(m)) == (lk.record, mask), (k, A.text(fam, v), int(x), hex(int(m)), A.describe_path(lk), hex(mask))


def test_intervals_answer_as_the_scan():
    """The elementary intervals derived from the scan answer every corpus address as the scan does: the
    flattening the device relies on loses nothing on these documents."""
    for fam, docs in ((V4, A.BL4), (V6, A.BL6)):
        for level, doc in enumerate(docs):
            iv = A.bl_intervals(doc, fam)
            assert [p for p, _ in iv] == sorted({p for p, _ in iv}) and all(a[1] != b[1] for a, b in zip(iv, iv[1:]))
            for v in A.addresses(fam):
                assert A.bl_search(iv, v)[0] == A._mask_cached(fam, level, v), (level, A.text(fam, v))


def test_reference_known_answers():
    """What tests/test_enrich_oracle.py quotes from the reference's own tests, through the restatement."""
    v4, v6, recs = asn_tables_from_tsv(TSV)
    t4, t6 = A.asn_prepare(_rows_of(v4, V4)), A.asn_prepare(_rows_of(v6, V6))
    assert recs[A.asn_lookup(t4, ip4("217.147.96.0")).record] == (174, "US", "COGENT-174")
    assert recs[A.asn_lookup(t6, ip6("2001:200::1")).record] == (2500, "JP", "WIDE-BB WIDE Project")
    assert A.asn_lookup(t4, 0).record == -1 and A.asn_lookup(t4, ip4("217.147.120.1")).record == -1
    rows = [("10.0.0.0", "10.255.255.255"), ("10.1.0.0", "10.1.0.255"), ("10.2.0.0", "10.2.0.255"),
            ("11.0.0.0", "11.0.0.255"), ("12.0.0.0", "12.0.0.255")]
    t = A.asn_prepare([(ip4(a), ip4(b), i + 1) for i, (a, b) in enumerate(rows)])
    assert A.asn_lookup(t, ip4("10.2.0.9")) == A.Lookup(3, (2,), True, 2)
    assert A.asn_lookup(t, ip4("10.3.0.1")) == A.Lookup(-1, (2, 4, 3), False, 3)  # 10/8 contains it
    assert A.asn_lookup(t, ip4("10.1.0.5")).record == 2
    doc = (("192.168.0.0/16", 0), ("10.0.0.0/8", 0), ("8.8.8.8/32", 0), ("172.16.0.0/12", 1), ("169.254.0.0/16", 1),
           ("9.9.9.9/32", 1), ("2001:db8::/32", 2), ("::1/128", 2), ("192.168.1.1/32", 3), ("2001:db8::1/128", 3),
           ("10.0.0.0/8", 3), ("2001:db8:1::/64", 3))
    want = {"192.168.1.1": 0b1001, "1.2.3.4": 0, "8.8.8.8": 1, "172.16.1.1": 2, "192.168.1.10": 1, "10.1.2.3": 0b1001,
            "192.168.1.2": 1}
    assert {a: A.bl_mask(doc, V4, ip4(a)) for a in want} == want
    want6 = {"2001:db8:1:2:3:4:5:6": 4, "2002:db8:1:2:3:4:5:6": 0, "::1": 4, "2001:db8::1": 0b1100, "2001:db8:1::abc": 0b1100,
             "2001:db8::2": 4}
    assert {a: A.bl_mask(doc, V6, ip6(a)) for a in want6} == want6


def test_hand_worked():
    """Records, masks and probe paths written out by hand."""
    st = A.step(5)  # five kept ranges in both families
    # handed over last range first: the duplicate pair arrives as records 4, 3 and must stay so
    assert [r[2] for r in st.asn4] == [1, 2, 4, 3, 5] and [r[2] for r in st.asn6] == [101, 102, 104, 103, 105]
    L = A.Lookup
    t = st.asn4  # 20/8 | 20.1.0.0-255 | 20.2.0.0-255 twice | 20.2.1.0-255
    assert A.asn_lookup(t, ip4("20.2.0.9")) == L(4, (2,), True, 2)            # the first of the duplicates
    assert A.asn_lookup(t, ip4("20.2.0.255")) == L(4, (2,), True, 2)          # a range's last address
    assert A.asn_lookup(t, ip4("20.2.1.0")) == L(5, (2, 4), True, 4)          # end + 1: the adjacent range
    assert A.asn_lookup(t, ip4("20.3.0.0")) == L(-1, (2, 4), False, 5)        # 20/8 contains it: never probed
    assert A.asn_lookup(t, ip4("20.1.0.5")) == L(2, (2, 1), True, 1)
    assert A.asn_lookup(t, ip4("20.0.0.1")) == L(1, (2, 1, 0), True, 0)       # a hit at the last possible probe
    assert A.asn_lookup(t, ip4("19.255.255.255")) == L(-1, (2, 1, 0), False, 0)
    t = A.step(7).asn6  # three kept IPv6 ranges: 2001:db8::/32 | 2001:db8:1::-ff | 2001:db8:2::-ff
    assert [r[2] for r in t] == [101, 102, 103]
    assert A.asn_lookup(t, ip6("2001:db8:2::80")) == L(103, (1, 2), True, 2)
    assert A.asn_lookup(t, ip6("2001:db8:1::100")) == L(-1, (1, 2), False, 2)  # the /32 contains it
    assert A.asn_lookup([], 5) == L(-1, (), False, 0)
    # blacklists
    assert A.bl_intervals(A.BL4[2], V4) == ((ip4("8.8.8.0"), 1), (ip4("8.8.9.0"), 0))
    assert A.bl_intervals(A.BL4[1], V4) == ((0, 1 << 63),) and A.bl_intervals(A.BL6[1], V6) == ((A.TOP[V6], 1 << 63),)
    got = [A.bl_mask(A.BL4[3], V4, ip4(a)) for a in ("8.8.7.255", "8.8.8.0", "8.8.8.255", "8.8.9.0", "255.255.255.255")]
    assert got == [0, 0b1100000, 0b1100000, 0, 1 << 63]
    got = [A.bl_mask(A.BL6[3], V6, ip6(a)) for a in ("::", "2001:db8::", "2001:db8:ffff:ffff:ffff:ffff:ffff:ffff", "2001:db9::")]
    assert got == [1, 3, 3, 1]
    assert A.bl_mask(A.BL4[3], V6, ip6("::808:808")) == 0 and A.bl_mask(A.BL6[3], V4, ip4("8.8.8.8")) == 0
    # per flow, step 5: 64 own addresses, 64 lan_v6 prefixes, the deep documents
    f, (a, b) = A.enrich_key(st, (6, V4, ip4("10.1.2.3"), 40001, ip4("20.2.0.9"), 40003))
    assert f == dict(flags=A.LOCAL_SRC, src_asn=-1, dst_asn=4, src_blacklists=0, dst_blacklists=0b11000)
    assert a is None and b.path == (2,)                                       # 10/8 is in list 62: local, so not looked up
    f, (a, b) = A.enrich_key(st, (17, V4, A.OWN4, 40005, ip4("20.3.0.0"), 40007))
    assert f == dict(flags=A.SELF_SRC, src_asn=-1, dst_asn=-1, src_blacklists=0, dst_blacklists=0)
    assert a.path == b.path == (2, 4)
    f, _ = A.enrich_key(st, (6, V6, A.OWN6, 40001, ip6("fc00::1"), 40003))
    assert f["flags"] == A.SELF_SRC | A.LOCAL_DST and f["dst_blacklists"] == 0 and A.step_mask(st, V6, ip6("fc00::1")) == 1 << 62
    f, _ = A.enrich_key(st, (6, V6, A.w6(0, 0, 0, A.OWN4), 40001, ip6("2620:0:0:1::7"), 40003))
    assert f["flags"] == A.SELF_SRC | A.LOCAL_DST                             # an own address from the table's middle; the /127
    f, _ = A.enrich_key(st, (6, V6, A.OWN6 + 1, 40001, ip6("2620:0:0:1::8"), 40003))
    assert f["flags"] == 0                                                    # own under the other family only; behind the /127
    f, _ = A.enrich_key(A.step(4), (6, V4, A.OWN4, 40001, ip4("8.8.8.8"), 40003))
    assert f["flags"] == 0                                                    # step 4 holds the IPv6 own address only


def test_corpus_keys_are_stored_as_sent():
    """Every packet's key survives process_parsed_packet unswapped and unfiltered, so the table holds exactly
    the keys the corpus names: none left out, none merged."""
    keys = A.keys()
    assert len(set(keys)) == len(keys) > 3000
    recs, cls, st = coracle.process_parsed(coracle.make_cfg(2), A.parsed())
    assert len(recs) == len(keys) and int(st[0]["n_session"]) == len(keys)
    assert [A.key_of(r) for r in recs] == list(keys)
    for fam in (V4, V6):
        used = {k[2] for k in keys if k[1] == fam} & {k[4] for k in keys if k[1] == fam}
        assert used == set(A.addresses(fam))  # every address is a source and a destination somewhere


def test_ladder_is_complete():
    steps = A.steps()
    for fam, n, level, docs in ((V4, "n4", "l4", A.BL4), (V6, "n6", "l6", A.BL6)):
        assert sorted(getattr(s, n) for s in steps) == list(A.SIZES)
        assert {getattr(s, level) for s in steps} == {0, 1, 2, 3, 4}
        counts = [len(A.bl_intervals(d, fam)) for d in docs]
        assert tuple(counts[:4]) == A.BL_COUNTS and 900 <= counts[4] <= 1100
        assert any(getattr(s, n) == 0 and getattr(s, level) == 4 for s in steps)           # empty ASN, deep intervals
        assert any(getattr(s, n) == max(A.SIZES) and getattr(s, level) == 0 for s in steps)  # and the reverse
        assert {l for _, l in docs[4]} == set(range(64))
    assert {len(s.own) for s in steps} == {0, 1, N.FB_MAX_OWN_IPS} == {len(s.lan) for s in steps}
    assert N.FB_MAX_OWN_IPS == N.FB_MAX_LAN_V6 == 64
    assert {p for s in steps for _, p in s.lan if len(s.lan) == 1} == {1, 64, 127, 128}
    assert {(s.own[0], s.own[-1]) for s in steps if len(s.own) == 64} == {((V4, A.OWN4), (V6, A.OWN6)), ((V6, A.OWN6), (V4, A.OWN4))}
    assert {s.own for s in steps if len(s.own) == 1} == {((V4, A.OWN4),), ((V6, A.OWN6),)}
    for s in steps:  # start > end rows to drop wherever there is a table, and nothing but them at IPv6 size 0
        assert len(s.rows4) == (s.n4 + 2 if s.n4 else 0) and len(s.rows6) == s.n6 + 2
    assert A.step(A.LARGEST).l4 == A.step(A.LARGEST).l6 == 4
    # the configured prefixes: the last address inside and the first outside are corpus addresses
    core = set(A.core_addresses(V6))
    for net, prefix in (A.P1, A.P64, A.P127, A.P128):
        inside = [v for v in A._prefix_edges(net, prefix) if A.is_lan_v6(v, [(net, prefix)]) and not A.is_lan_v6(v, [])]
        outside = [v for v in A._prefix_edges(net, prefix) if not A.is_lan_v6(v, [(net, prefix)])]
        assert inside and outside and set(inside) | set(outside) <= core, prefix


def test_census():
    c = A.census()
    print({k: c[k] for k in A.census_classes()})
    empty = [k for k in A.census_classes() if c[k] <= 0]
    assert not empty, empty
