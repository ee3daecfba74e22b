"""Flow enrichment on the GPU (fb_flow_enrich_dev: k_flow_enrich / flow_lookups, and fb_ip_lookup_dev:
k_ip_lookup, flodbadd_amd/csrc/fb_enrich.hip) on the enumerated corpora of tests/addrspace.py.

One table of 3,204 hand-placed flows -- every ASN range end and every first address of a blacklist
interval with both neighbours, every is_lan_ip edge, own addresses, lan_v6 prefix edges, IPv6 addresses
decided at each key word -- is swept under a ladder of eleven configurations (ASN tables of 0-17 ranges,
blacklists of 0 to about 930 intervals, own and lan_v6 tables of 0, 1 and 64 entries).  Every field of every flow
must equal the plain-Python restatement and the C oracle; everything is an integer, so nothing is
tolerated.  tests/test_addrspace_oracle.py pins the restatement and the census of classes on the CPU.

A failure names the flow, the field, both values and the restatement's probe paths."""
import numpy as np
import pytest

import addrspace as A
from addrspace import V4, V6
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture, lan_v6_table
from flodbadd_amd.sessions import SessionFilter
from oracle import coracle

pytestmark = pytest.mark.gpu

STEPS = list(range(len(A.SIZES)))


def _capture(capacity=1 << 12, lan=()):
    return FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=capacity, lan_v6=lan)


def _configure(cap, st, only=None):
    """The step's configuration into the context (only: one of 'asn', 'bl', 'own', 'lan')."""
    if only in (None, "asn"):
        cap.set_asn_tables(A.asn_array(st.rows4, V4), A.asn_array(st.rows6, V6))
    if only in (None, "bl"):
        cap.set_blacklists(A.cidr_array(st.doc))
    if only in (None, "own"):
        cap.set_own_ips([A.text(f, v) for f, v in st.own])
    if only in (None, "lan"):
        cap.set_lan_v6(A.lan_pairs(st))


def _load(cap, recs=None):
    """The corpus (or a part of it, renumbered) in one update call -> its keys."""
    recs = A.parsed() if recs is None else recs
    recs = recs.copy()
    recs["pkt_index"] = np.arange(len(recs), dtype=np.uint32)
    g = cap.process_parsed(recs)
    assert g.stats["error"] == 0 and g.stats["n_session"] == g.stats["new_sessions"] == len(recs)
    return [A.key_of(r) for r in recs]


def _by_slot(cap, keys):
    """export_flows joined by slot -> {slot: key}; the table holds exactly `keys`: none left out, none twice."""
    flows = cap.export_flows()
    out = {int(r["slot"]): A.key_of(r) for r in flows}
    assert len(out) == len(flows) == cap.flow_count() == len(keys)
    assert set(out.values()) == set(keys)
    return out, flows


def _check(tag, st, by_slot, e, exp=None):
    """Enrichment records against the restatement under `st`, every field of every flow."""
    slots = [int(s) for s in e["slot"]]
    assert len(set(slots)) == len(slots) and set(slots) <= set(by_slot), tag
    bad = []
    for r in e:
        key = by_slot[int(r["slot"])]
        want, paths = exp[key] if exp is not None else A.enrich_key(st, key)
        for f in A.FIELDS:
            if int(r[f]) != want[f]:
                bad.append("%s: flow %s (slot %d), %s: device %#x, restatement %#x; src %s; dst %s" % (
                    tag, A.describe(key), int(r["slot"]), f, int(r[f]), want[f], A.describe_path(paths[0]),
                    A.describe_path(paths[1])))
    assert not bad, "%d differences\n%s" % (len(bad), "\n".join(bad[:10]))


def _check_c_oracle(tag, st, by_slot, flows, e):
    cfg = coracle.make_cfg(2, lan_v6=lan_v6_table(A.lan_pairs(st)), own_ips=A.ip_array(st.own))
    a4 = coracle.asn_prepare(A.asn_array(st.rows4, V4), V4)
    a6 = coracle.asn_prepare(A.asn_array(st.rows6, V6), V6)
    row = {int(r["slot"]): i for i, r in enumerate(flows)}
    ref = coracle.enrich_keys(cfg, a4, a6, A.cidr_array(st.doc), flows[[row[int(s)] for s in e["slot"]]])
    for f in A.FIELDS:
        d = np.flatnonzero(e[f] != ref[f])
        assert d.size == 0, "%s: flow %s, %s: device %#x, C oracle %#x" % (
            tag, A.describe(by_slot[int(e["slot"][d[0]])]), f, int(e[f][d[0]]), int(ref[f][d[0]]))


def _lookup(cap, arr, n=None, asn=True, lists=True):
    """fb_ip_lookup_dev over fb_ip entries; an output left out is passed as NULL -> (asn, lists), prefilled
    with a pattern the call must overwrite."""
    n = len(arr) if n is None else n
    d_ip = N.DeviceBuffer(max(arr.nbytes, 32))
    if len(arr):
        d_ip.upload(arr)
    d_a, d_l = N.DeviceBuffer(4 * max(len(arr), 1)), N.DeviceBuffer(8 * max(len(arr), 1))
    d_a.upload(np.full(max(len(arr), 1), -77, dtype=np.int32))
    d_l.upload(np.full(max(len(arr), 1), 0xA5A5, dtype=np.uint64))
    N.check(N.gpu_lib().fb_ip_lookup_dev(cap.ctx, d_ip.ptr, n, d_a.ptr if asn else None, d_l.ptr if lists else None, None))
    N.check(N.gpu_lib().fb_stream_sync(None))
    return (d_a.download(np.zeros(max(len(arr), 1), dtype=np.int32))[: len(arr)],
            d_l.download(np.zeros(max(len(arr), 1), dtype=np.uint64))[: len(arr)])


ADDRS = [(fam, v) for fam in (V4, V6) for v in A.addresses(fam)]


# ---- 1. the flow sweep --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", STEPS)
def test_flow_sweep(k):
    """enrich(new_only=False) under ladder step k: every field of every flow equals the restatement and
    the C oracle."""
    st = A.step(k)
    cap = _capture()
    try:
        by_slot, flows = _by_slot(cap, _load(cap))
        _configure(cap, st)
        e = cap.enrich(new_only=False)
        assert sorted(int(s) for s in e["slot"]) == sorted(by_slot)
        _check("step %d" % k, st, by_slot, e, A.expected(k))
        _check_c_oracle("step %d" % k, st, by_slot, flows, e)
    finally:
        cap.close()


# ---- 2. the address lookup ----------------------------------------------------------------------------
def test_address_lookup():
    """Every corpus address through fb_ip_lookup_dev under every ladder step: the restatement without the
    local rule.  Then the call's edges: an unknown family, either output NULL, n = 0."""
    cap = _capture(capacity=1 << 9)
    try:
        arr = A.ip_array(ADDRS)
        for k in STEPS:
            st = A.step(k)
            _configure(cap, st)
            ga, gl = _lookup(cap, arr)
            for (fam, v), x, m in zip(ADDRS, ga, gl):
                lk, mask = A.lookup_ip(st, fam, v)
                assert (int(x), int(m)) == (lk.record, mask), "step %d: address %s: device (%d, %#x), restatement (%d, %#x); %s" % (
                    k, A.text(fam, v), int(x), int(m), lk.record, mask, A.describe_path(lk))
        # step 10 stays configured: 17 IPv4 ranges, the deep IPv6 document
        st = A.step(STEPS[-1])
        probe = [(V4, A.ip4("20.2.0.9")), (V6, A.ip6("a000::5")), (V4, A.ip4("20.2.0.9")), (V6, A.ip6("a000::5"))]
        want = [A.lookup_ip(st, f, v) for f, v in probe[:2]]
        assert want[0][0].record >= 0 and want[1][1] != 0
        odd = A.ip_array(probe)
        odd[2]["family"], odd[3]["family"] = 7, 0   # neither AF_INET nor AF_INET6: None and no list
        ga, gl = _lookup(cap, odd)
        assert ga.tolist() == [want[0][0].record, want[1][0].record, -1, -1]
        assert gl.tolist() == [want[0][1], want[1][1], 0, 0]
        ga2, gl2 = _lookup(cap, odd, asn=False)                      # d_asn NULL: the masks alone
        assert ga2.tolist() == [-77] * 4 and gl2.tolist() == gl.tolist()
        ga2, gl2 = _lookup(cap, odd, lists=False)                    # d_lists NULL: the records alone
        assert ga2.tolist() == ga.tolist() and gl2.tolist() == [0xA5A5] * 4
        ga2, gl2 = _lookup(cap, odd, n=0)                            # n = 0: nothing is written
        assert ga2.tolist() == [-77] * 4 and gl2.tolist() == [0xA5A5] * 4
        assert N.gpu_lib().fb_ip_lookup_dev(cap.ctx, None, 0, None, None, None) == N.FB_OK
        assert N.gpu_lib().fb_ip_lookup_dev(cap.ctx, None, 1, None, None, None) == N.FB_ERR_INVAL
    finally:
        cap.close()


# ---- 3. the two kernels agree -------------------------------------------------------------------------
def test_flow_sweep_agrees_with_address_lookup():
    """flow_lookups against the plain loops of k_ip_lookup, device against device: for every flow address the
    stored key calls public, the sweep's record and mask are the address lookup's; for every local address
    they are -1 and 0 whatever the tables hold."""
    cap = _capture()
    try:
        by_slot, _ = _by_slot(cap, _load(cap))
        arr = A.ip_array(ADDRS)
        n_listed = 0
        for k in STEPS:
            st = A.step(k)
            _configure(cap, st)
            ga, gl = _lookup(cap, arr)
            of = {a: (int(x), int(m)) for a, x, m in zip(ADDRS, ga, gl)}
            n_local = 0
            for r in cap.enrich():
                key = by_slot[int(r["slot"])]
                fam = key[1]
                for ip, fa, fm, bit in ((key[2], "src_asn", "src_blacklists", A.LOCAL_SRC),
                                        (key[4], "dst_asn", "dst_blacklists", A.LOCAL_DST)):
                    got = (int(r[fa]), int(r[fm]))
                    local = A.is_lan(fam, ip, st.lan)
                    assert bool(int(r["flags"]) & bit) is local, (k, A.describe(key), A.text(fam, ip))
                    want = (-1, 0) if local else of[(fam, ip)]
                    assert got == want, "step %d: flow %s, address %s (%s): sweep (%d, %#x), address lookup (%d, %#x)" % (
                        k, A.describe(key), A.text(fam, ip), "local" if local else "public", got[0], got[1], of[(fam, ip)][0],
                        of[(fam, ip)][1])
                    n_local += local
                    n_listed += local and of[(fam, ip)] != (-1, 0)
            assert n_local > 100, k
        assert n_listed > 100  # local addresses that the tables do hold
    finally:
        cap.close()


# ---- 4. agreement with the blacklist pass --------------------------------------------------------------
def test_flow_sweep_agrees_with_blacklist_pass():
    """fb_flow_blacklist shares bl_probe / bl_step with flow_lookups but not the loop: on the largest step its
    mask word per slot is src_blacklists | dst_blacklists.  (The pass reads the local flags stored at insert,
    so the capture has the step's lan_v6 prefixes from the start.)"""
    st = A.step(A.LARGEST)
    cap = _capture(lan=A.lan_pairs(st))
    try:
        by_slot, _ = _by_slot(cap, _load(cap))
        _configure(cap, st)
        e = cap.enrich()
        _check("largest step", st, by_slot, e, A.expected(A.LARGEST))
        stats = cap.update_blacklist(mark_whitelist=False)
        masks = cap.blacklist_masks()
        assert stats["flows"] == len(by_slot)
        for r in e:
            want = int(r["src_blacklists"]) | int(r["dst_blacklists"])
            assert int(masks[int(r["slot"])]) == want, "flow %s: blacklist pass %#x, sweep %#x | %#x" % (
                A.describe(by_slot[int(r["slot"])]), int(masks[int(r["slot"])]), int(r["src_blacklists"]), int(r["dst_blacklists"]))
        # (each of the 880 listed addresses of a family's dense run is in a flow, at most two of them in one)
        assert stats["blacklisted"] == int(((e["src_blacklists"] | e["dst_blacklists"]) != 0).sum()) >= 880
    finally:
        cap.close()


# ---- 5. re-configuration ------------------------------------------------------------------------------
def test_reconfiguration():
    """One setter at a time between two sweeps of the same table: the second sweep reflects the new
    configuration and nothing of the old.  Then empty tables: every record -1, every mask 0, the flags stay."""
    cap = _capture()
    try:
        by_slot, _ = _by_slot(cap, _load(cap))
        st = A.step(5)
        _configure(cap, st)
        _check("step 5", st, by_slot, cap.enrich(), A.expected(5))
        walk = [("own", 4, lambda s, o: s._replace(own=o.own)), ("lan", 4, lambda s, o: s._replace(lan=o.lan)),
                ("asn", 10, A.with_asn), ("bl", 3, A.with_blacklists), ("lan", 7, lambda s, o: s._replace(lan=o.lan)),
                ("own", 2, lambda s, o: s._replace(own=o.own)), ("asn", 2, A.with_asn), ("bl", 5, A.with_blacklists)]
        for what, k, change in walk:
            before = np.sort(cap.enrich(), order="slot")
            st = change(st, A.step(k))
            _configure(cap, st, only=what)
            e = np.sort(cap.enrich(), order="slot")
            _check("after %s of step %d" % (what, k), st, by_slot, e)
            assert e.tobytes() != before.tobytes(), (what, k)  # the change was one the flows can see
        flags = {int(r["slot"]): int(r["flags"]) for r in cap.enrich()}
        st = A.empty_step(st)
        _configure(cap, st, only="asn")
        _configure(cap, st, only="bl")
        e = cap.enrich()
        _check("empty tables", st, by_slot, e)
        assert (e["src_asn"] == -1).all() and (e["dst_asn"] == -1).all()
        assert not e["src_blacklists"].any() and not e["dst_blacklists"].any()
        assert {int(r["slot"]): int(r["flags"]) for r in e} == flags
        for bit in (A.LOCAL_SRC, A.LOCAL_DST, A.SELF_SRC, A.SELF_DST):
            assert 0 < sum(1 for f in flags.values() if f & bit) < len(flags), bit
    finally:
        cap.close()


# ---- 6. new_only through a slot move ------------------------------------------------------------------
def test_new_only_through_a_slot_move():
    """A 2^9-slot table takes flows in two update calls, the second of which makes it grow:
    enrich(new_only=True) returns exactly the second call's flows, at their new slots, with correct contents;
    after clear_all_sessions() and one more update, exactly that update's flows.  (The table grows before a
    call, to hold twice the flows the call before it inserted, so the second call cannot bring the whole
    corpus behind a first one that fits 2^9 slots: every third pair of the corpus, both directions, goes in.)"""
    st = A.step(A.LARGEST)
    cap = _capture(capacity=1 << 9)
    try:
        _configure(cap, st)
        recs = A.parsed()
        rest = recs[(np.arange(len(recs)) // 2) % 3 != 0]
        recs = recs[(np.arange(len(recs)) // 2) % 3 == 0]
        assert len(recs) > 1000
        first = _load(cap, recs[:300])
        slot0 = {key: s for s, key in _by_slot(cap, first)[0].items()}
        e = cap.enrich(new_only=True)
        assert sorted(int(s) for s in e["slot"]) == sorted(slot0.values())
        assert cap.table_info()["capacity"] == 1 << 9
        second = _load(cap, recs[300:])
        assert cap.table_info()["capacity"] > 1 << 9 and cap.table_info()["generation"] > 0
        by_slot, _ = _by_slot(cap, first + second)
        assert any(slot0[key] != s for s, key in by_slot.items() if key in slot0)       # the first call's flows moved
        e = cap.enrich(new_only=True)
        want = sorted(s for s, key in by_slot.items() if key not in slot0)
        assert len(want) == len(second) and sorted(int(s) for s in e["slot"]) == want
        _check("new_only after the growth", st, by_slot, e, A.expected(A.LARGEST))
        _check("all flows after the growth", st, by_slot, cap.enrich(new_only=False), A.expected(A.LARGEST))
        cap.clear_all_sessions()
        assert len(cap.enrich(new_only=False)) == 0
        third = _load(cap, rest[1000:1200])
        by_slot, _ = _by_slot(cap, third)
        e = cap.enrich(new_only=True)
        assert sorted(int(s) for s in e["slot"]) == sorted(by_slot)
        _check("new_only after the clear", st, by_slot, e, A.expected(A.LARGEST))
        fourth = _load(cap, recs[500:600])
        by_slot, _ = _by_slot(cap, third + fourth)
        e = cap.enrich(new_only=True)
        assert sorted(by_slot[int(s)] for s in e["slot"]) == sorted(fourth)
        _check("new_only after one more update", st, by_slot, e, A.expected(A.LARGEST))
    finally:
        cap.close()
