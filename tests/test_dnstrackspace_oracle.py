"""CPU checks of the DNS tracker's corpora (tests/dnstrackspace.py): the restated tag functions against the
stand-alone host program over fb_dns_hash.h (g++ with the address and undefined-behaviour sanitizers; nothing
is loaded into Python), the second restatement against DnsResolver on every string both can express, the
census of every claimed home, tag, slot and sorted position, and the bounds of the growth rule."""
import numpy as np
import pytest

import dnstrackgen as T
import dnstrackspace as D
from flodbadd_amd import _native as N
from flodbadd_amd.dns import DnsResolver

MASKS = [D.M64, 0x1F, 0xFF, 1]


@pytest.fixture(scope="module")
def random_keys():
    rng = np.random.default_rng(20250114)
    n = 10000
    rows = rng.integers(0, 256, (n, N.FB_DNS_MAX_NAME), dtype=np.uint8)  # name and garbage alike
    lens = rng.integers(0, 256, n).astype(np.uint16)
    lens[:8] = [0, 1, 3, 4, 5, 252, 254, 255]
    keys = [(int(w[0]), 0, 0, 0, 2) for w in rng.integers(0, 1 << 32, (1000, 1))]
    keys += [tuple(int(x) for x in w) + (10,) for w in rng.integers(0, 1 << 32, (1000, 4))]
    keys += [(0, 0, 0, 0, 2), (0, 0, 0, 0, 10), (0xFFFFFFFF,) * 4 + (10,), (0xFFFFFFFF, 0, 0, 0, 2)]
    return rows, lens, keys


def test_python_tags_equal_the_header_on_random_keys(random_keys):
    rows, lens, keys = random_keys
    full_n = [D.name_tag(r.tobytes(), int(l)) for r, l in zip(rows, lens)]
    full_a = [D.key_tag(k) for k in keys]
    for mask in MASKS:
        got_n, got_a = D.host_tags(rows, lens, keys, mask)
        assert got_n == [(t & mask) | D.TAG_USED for t in full_n]
        assert got_a == [(t & mask) | D.TAG_USED for t in full_a]
        # the restated functions with the mask itself
        assert got_n[:600] == [D.name_tag(r.tobytes(), int(l), mask) for r, l in zip(rows[:600], lens[:600])]
        assert got_a == [D.key_tag(k, mask) for k in keys]
    # the garbage does not count: the same names with other bytes behind them
    other = rows.copy()
    for r, l in zip(other, lens):
        r[int(l):] ^= 0xA5
    assert D.host_tags(other, lens, [], D.M64)[0] == full_n


def test_python_tags_equal_the_header_on_every_corpus_key():
    names, keys = D.corpus_keys()
    assert len(names) > 50 and len(keys) > 700
    lens = np.array([len(nm) for nm in names], dtype=np.uint16)
    for garbage in D.GARBAGE:
        rows = np.full((len(names), N.FB_DNS_MAX_NAME), garbage, dtype=np.uint8)
        for r, nm in zip(rows, names):
            r[:len(nm)] = np.frombuffer(nm, dtype=np.uint8)
        for mask in MASKS:
            got_n, got_a = D.host_tags(rows, lens, keys, mask)
            assert got_n == [D.bname_tag(nm, mask) for nm in names]
            assert got_a == [D.key_tag(k, mask) for k in keys]
            assert {D.home(t) for t in got_n} <= set(range(32))


def against_resolver(model, ref, msgs, names, addrs, ts=None, n_dns=None):
    """One call through the restatement and through DnsResolver: the strings agree."""
    want = T.reference_step(ref, msgs, names, addrs, n_dns=n_dns)
    out = model.track(msgs, names, addrs, ts=ts, n_dns=n_dns)
    got = [model.names[int(t)].decode("ascii") if int(t) else None for t in out["taken"]]
    assert got == want
    assert model.pending_strings() == ref.pending and model.resolution_strings() == ref.resolutions
    assert [i for i, _ in out["new_names"]] == list(range(len(model.names) - len(out["new_names"]), len(model.names)))
    return out


@pytest.mark.parametrize("corpus", D.all_corpora(), ids=repr)
def test_restatement_equals_the_resolver_on_every_corpus_call(corpus):
    model, ref = D.Tracker(corpus.name_capacity, corpus.addr_capacity), DnsResolver()
    for step in corpus.steps:
        if isinstance(step, D.Expire):
            before = set(np.nonzero(model.pend_name)[0])
            dropped = model.expire(step.now)
            gone = before - set(np.nonzero(model.pend_name)[0])
            assert len(gone) == dropped
            ref.expire(int(t) for t in gone)
            assert model.pending_strings() == ref.pending
        else:
            against_resolver(model, ref, *step.arrays(), ts=step.ts, n_dns=step.n_dns)
    for _, k in corpus.absent:
        assert D.ip_of(k) not in ref.resolutions and model.lookup(k) == 0


def hand_cases():
    """The hand cases of tests/test_gpu_dnstrack.py (test_hand_cases, test_stats_n_dns_below_n, the names of
    test_name_edge_cases), as (batch, n_dns)."""
    B = T.Batch
    yield B().query(1, "a.example").response(1, ["192.0.2.1"]), None
    yield B().query(2, "b.example"), None
    yield B().response(2, ["192.0.2.2"]), None
    yield B().response(3, ["192.0.2.3"]), None
    yield B().query(4, "first.example").query(4, "second.example").response(4, ["192.0.2.4"]), None
    yield B().query(5, "c.example").response(5, ["192.0.2.5"]).response(5, ["192.0.2.55"]), None
    yield B().query(6, "d.example").reverse(6).no_question(6).response(6, ["192.0.2.6"]), None
    yield B().query(7, "e.example"), None
    yield B().reverse(7).no_question(7), None
    yield B().response(7, ["192.0.2.7"]), None
    yield B().query(8, "f.example").rejected(8, query=True).rejected(8, query=False, addrs=["192.0.2.80"]) \
        .response(8, ["192.0.2.8"]), None
    yield B().query(9, "g.example").response(9, []).response(9, ["192.0.2.9"]), None
    yield B().query(10, "old.example").query(11, "new.example").response(10, ["192.0.2.10"]).response(11, ["192.0.2.10"]), None
    yield B().query(11, "new.example").query(10, "old.example").response(11, ["192.0.2.10"]).response(10, ["192.0.2.10"]), None
    yield B().query(12, "newest.example").response(12, ["192.0.2.10"]), None
    yield B().query(13, "v4.example").query(14, "v6.example").response(13, ["32.1.13.184"]) \
        .response(14, ["2001:db8::", "2001:db8::1"]), None
    yield B().query(15, "eight.example").response(15, ["198.51.100.%d" % i for i in range(8)]), None
    yield B().query(1, "in.example").response(1, ["192.0.2.1"]).query(2, "in2.example").query(3, "out.example") \
        .response(2, ["192.0.2.2"]), 3
    b = B()
    for i, nm in enumerate(["abcdefg1", "abcdefg2", "abcd", "abcde", "abcdef", "a", "x" * 254 + "a", "x" * 254 + "b",
                            "Case.Example", "case.example"]):
        b.query(20 + i, nm, garbage=0xEE)
    b.query(100, "garbage.example", garbage=0x00).query(101, "garbage.example", garbage=0xFF)
    yield b, None


def test_restatement_equals_the_resolver_on_the_hand_cases():
    model, ref = D.Tracker(1024, 4096), DnsResolver()
    for batch, n_dns in hand_cases():
        against_resolver(model, ref, *batch.arrays(), n_dns=n_dns)
    assert b"out.example" not in model.ids and b"in2.example" in model.ids  # (out.example lies behind n_dns)
    assert model.names[1] == b"a.example" and model.res[D.key_of("192.0.2.10")][0] == model.ids[b"newest.example"]


def test_census():
    c = D.census()
    assert c["id_runs"] == {"sequences": 340, "messages": 1252, "setters": 939, "straddles": {2: 255, 3: 510, 4: 766},
                            "variants": 6}
    assert c["ladder"]["k"] == [1, 2, 3, 4, 5, 6]
    assert c["wrap"]["slots"] == [29, 30, 31, 0, 1, 2, 3, 4] and c["cluster"]["slots"] == list(range(9, 19))
    assert c["cluster"]["pairs"] == ["last_byte", "partial_dword", "prefix", "v4_v6_word0", "v6_word0", "v6_word3"]
    assert set(c["absent"]) == {"wrap-0x1f", "wrap-0xff", "cluster-0x1f", "cluster-0xff"}
    assert c["times"]["dropped"] == [0, 0, 1] and c["grow"]["adds"] == [12, 20, 40, 80, 160]
    assert c["corpora"] == 20


@pytest.mark.parametrize("corpus", D.all_corpora(), ids=repr)
def test_no_corpus_grows_but_grow(corpus):
    """Names held + accepted queries and addresses held + answers stay within the capacities in every call of
    every corpus but GROW (check_bounds asserts it); GROW grows in every call."""
    model = D.check_bounds(corpus)
    grew = (model.name_cap, model.addr_cap) != (corpus.name_capacity, corpus.addr_capacity)
    assert grew == corpus.grows == (corpus.name == "grow")
