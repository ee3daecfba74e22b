"""The DNS tracker on the device over the enumerated corpora of tests/dnstrackspace.py, against that module's
restatement -- exactly: these are integers and bytes.  After EVERY step of every corpus

  taken                     the name id each response took
  the store                 every id's 256-byte row (the name, then zeros) and length, read from the device
  pending                   all 65,536 name ids and times
  counters, info            fb_dns_track_stats but `rounds`; fb_dns_track_info whole
  raw resolutions           fb_dns_export_resolutions_dev: as many records as info says, no address twice,
                            name_id and order of every address, the reserved fields zero

and per corpus what it was built for: the rounds of LADDER, the lookups of present and absent addresses and the
domain pass over WRAP and CLUSTER, the ids through GROW, the stamp reset behind FB_DEBUG_DNS_LAUNCH, a clear
followed by collisions.  Each test builds its own small context."""
import ipaddress

import numpy as np
import pytest

import dnstrackgen as T
import dnstrackspace as D
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.sessions import Protocol, Session, SessionPacketData

pytestmark = pytest.mark.gpu

COUNTERS = ("messages", "queries", "responses", "matched", "resolutions", "names_new", "addrs_new")


def capture(corpus, **kw):
    return T.new_capture(**dict(corpus.config(), **kw))[0]


def track(cap, call):
    """One fb_dns_track_dev call over the call's arrays -> (the device's counters with "taken", the arrays)."""
    msgs, names, addrs = call.arrays()
    n = len(msgs)
    d_msg = N.DeviceBuffer(max(msgs.nbytes, 16)).upload(msgs)
    d_names = N.DeviceBuffer(max(names.nbytes, 16)).upload(names)
    d_addrs = N.DeviceBuffer(max(addrs.nbytes, 32)).upload(addrs)
    d_ts = N.DeviceBuffer(call.ts.nbytes).upload(call.ts) if call.ts is not None else None
    d_st = None
    if call.n_dns is not None:
        st = np.zeros(1, dtype=N.STATS_DTYPE)
        st[0]["n_dns"] = call.n_dns
        d_st = N.DeviceBuffer(st.nbytes).upload(st)
    return cap.track_dns_parsed_dev(d_msg, d_names, d_addrs, n, d_stats=d_st, d_ts=d_ts, want_taken=True), (msgs, names, addrs)


def raw_resolutions(cap, room):
    d_out, d_n = N.DeviceBuffer(max(room, 1) * N.DNS_RESOLUTION_DTYPE.itemsize), N.DeviceBuffer(8)
    N.check(N.gpu_lib().fb_dns_export_resolutions_dev(cap.ctx, d_out.ptr, max(room, 1), d_n.ptr, None))
    n = int(d_n.download(np.zeros(1, dtype=np.uint64))[0])
    return n, d_out.download(np.zeros(max(room, 1), dtype=N.DNS_RESOLUTION_DTYPE))[:min(n, room)]


def check_state(cap, model):
    info = cap.dns_track_info()
    assert info == model.info()
    # the store, read by id from the device (one id past the last: length 0, a zero row)
    n = info["names"]
    ids = np.arange(1, n + 2, dtype=np.uint32)
    d_ids = N.DeviceBuffer(ids.nbytes).upload(ids)
    d_out, d_len = N.DeviceBuffer(len(ids) * N.FB_DNS_MAX_NAME), N.DeviceBuffer(len(ids) * 2)
    N.check(N.gpu_lib().fb_dns_names_dev(cap.ctx, d_ids.ptr, len(ids), d_out.ptr, d_len.ptr, None))
    rows = d_out.download(np.zeros((len(ids), N.FB_DNS_MAX_NAME), dtype=np.uint8))
    lens = d_len.download(np.zeros(len(ids), dtype=np.uint16))
    want_rows = np.zeros_like(rows)
    for i, nm in enumerate(model.names[1:]):
        want_rows[i, :len(nm)] = np.frombuffer(nm, dtype=np.uint8)
    assert [int(x) for x in lens] == [len(nm) for nm in model.names[1:]] + [0]
    assert np.array_equal(rows, want_rows)
    # pending
    pid, ptime = cap.dns_pending_ids()
    assert np.array_equal(pid, model.pend_name)
    assert np.array_equal(ptime, model.pend_time)
    # the raw export
    cnt, recs = raw_resolutions(cap, info["addrs"] + 8)
    assert cnt == info["addrs"] == len(recs)
    keys = [tuple(int(w) for w in r["ip"]["addr"]) + (int(r["ip"]["family"]),) for r in recs]
    assert len(set(keys)) == len(keys)
    assert {k: (int(r["name_id"]), int(r["order"])) for k, r in zip(keys, recs)} == model.res
    assert not recs["reserved"].any() and not recs["ip"]["reserved"].any()


def step(cap, model, s):
    """One step on the device and in the model, everything compared; returns the device's counters."""
    if isinstance(s, D.Expire):
        assert cap.expire_dns(s.now) == model.expire(s.now)
        check_state(cap, model)
        return None
    out, (msgs, names, addrs) = track(cap, s)
    want = model.track(msgs, names, addrs, ts=s.ts, n_dns=s.n_dns)
    assert np.array_equal(out["taken"], want["taken"])
    assert {f: out[f] for f in COUNTERS} == {f: want[f] for f in COUNTERS}
    check_state(cap, model)
    return out


def lookups(cap, model, keys):
    got = cap.dns_lookup([D.ip_of(k) for k in keys])
    assert [int(x) for x in got] == [model.lookup(k) for k in keys]
    return [int(x) for x in got]


@pytest.mark.parametrize("corpus", D.all_corpora(), ids=repr)
def test_corpus(corpus):
    """Every step of the corpus equals the restatement; a call with predicted rounds takes exactly those (LADDER:
    k equal tags, no duplicate message -- every round publishes one slot of the chain); at the end every address
    the corpus inserted looks up to its last writer and every absent one to 0."""
    cap, model = capture(corpus), D.Tracker(corpus.name_capacity, corpus.addr_capacity)
    try:
        for s in corpus.steps:
            out = step(cap, model, s)
            if isinstance(s, D.Call) and s.rounds is not None:
                assert out["rounds"] == s.rounds
        present = sorted(model.res)
        assert all(lookups(cap, model, present)) or not present
        assert not any(lookups(cap, model, [k for _, k in corpus.absent]))
    finally:
        cap.close()


def pkt(src, dst, sport):
    s = Session(Protocol.TCP, ipaddress.ip_address(src), sport, ipaddress.ip_address(dst), 443)
    return SessionPacketData(s, 100, 140, 0x10)


@pytest.mark.parametrize("corpus", [D.wrap(0x1F), D.wrap(0xFF), D.cluster(0x1F), D.cluster(0xFF)], ids=repr)
def test_probe_geometry_lookup_and_domain_pass(corpus):
    """WRAP / CLUSTER with ABSENT: the same keys sent again add nothing and take the same ids; fb_dns_lookup_dev
    of every present key gives its id and of every absent key 0 (first, middle and last slot of the cluster, slot
    31, the empty slot behind it; both families); the domain pass over flows between those addresses writes what
    the lookup says."""
    cap, model = capture(corpus, flow_capacity=1 << 9), D.Tracker()
    try:
        first = step(cap, model, corpus.steps[0])
        assert first["names_new"] == first["addrs_new"] == len(model.names) - 1 == len(model.res) > 0
        ids = dict(model.ids)
        for s in corpus.steps[1:]:
            out = step(cap, model, s)
            assert out["names_new"] == out["addrs_new"] == 0 and out["matched"] == out["responses"]
        assert model.ids == ids
        present, absent = sorted(model.res), [k for _, k in corpus.absent]
        assert all(lookups(cap, model, present)) and not any(lookups(cap, model, absent))
        p4, p6 = [k for k in present if k[4] == 2], [k for k in present if k[4] == 10]
        a4, a6 = [k for k in absent if k[4] == 2], [k for k in absent if k[4] == 10]
        ends = [(p4[0], a4[0]), (a4[1], p4[1]), (p6[0], a6[0]), (a6[1], p6[1]), (p6[1], p6[2]), (a4[2], a4[3]), (p4[2], p4[0])]
        cap.process_parsed([pkt(D.ip_of(s), D.ip_of(d), 40000 + i) for i, (s, d) in enumerate(ends)])
        st = cap.update_domains()
        flows, plane = cap.export_flows(), cap.domain_ids()
        assert len(flows) == len(ends) == st["flows"]
        seen = set()
        for r in flows:
            fam = int(r["family"])
            src, dst = tuple(int(w) for w in r["src_ip"]) + (fam,), tuple(int(w) for w in r["dst_ip"]) + (fam,)
            got = plane[int(r["slot"])]
            assert (int(got["src_name_id"]), int(got["dst_name_id"])) == (model.lookup(src), model.lookup(dst))
            seen.add(frozenset((src, dst)))
        assert seen == {frozenset(e) for e in ends}
        assert st["with_domain"] == 6 and st["src_set"] + st["dst_set"] == 8
    finally:
        cap.close()


def test_growth_keeps_ids_chains_and_last_writers():
    """GROW: after each of the five growing calls the capacities are what grow_names / grow_addrs define (the
    restatement's), every id ever handed out names the same bytes (check_state reads the whole store), the old
    names queried again took their old ids -- names_new counts the new ones alone --, every address looks up to
    its last writer -- which changed in this call for three old addresses of four, while the fourth was left alone
    and has nothing but what the rebuild carried over --, and the export has no duplicate."""
    corpus = D.grow()
    cap, model = capture(corpus), D.Tracker()
    try:
        held, caps = 0, []
        for call, add in zip(corpus.steps, D.GROW_ADDS):
            old_ids, old_res = dict(model.ids), dict(model.res)
            out = step(cap, model, call)
            assert (out["names_new"], out["addrs_new"]) == (add, 2 * add) and out["queries"] == held + add
            assert all(model.ids[nm] == i for nm, i in old_ids.items())
            alone = {D.key_of(a) for j in range(held) if j % 4 == 3
                     for a in ("172.16.%d.%d" % (j >> 8, j & 255), "2001:db8:9::%x" % j)}
            assert all((model.res[k] == v) == (k in alone) for k, v in old_res.items()) and len(alone) == held // 4 * 2
            held += add
            info = cap.dns_track_info()
            caps.append((info["name_capacity"], info["addr_capacity"]))
            assert all(lookups(cap, model, sorted(model.res)))
            assert sorted(cap.dns_names(range(1, held + 1)).values()) == sorted("grow-%03d.example" % j for j in range(held))
            cap._dns_names = {}
        assert caps == D.GROW_CAPS
    finally:
        cap.close()


def test_stamp_reset():
    """FB_DEBUG_DNS_LAUNCH.  WRAP is inserted under launch numbers just below 0xF0000000, so its slots carry
    stamps no later launch would ever pass; then the number is set past the threshold.  The next call restamps
    both tables first: the same WRAP keys are found where they are (an unrestamped slot would read "not yet"
    for ever), CLUSTER goes in beside them, and ids, pending, lookups and export equal the restatement as if
    nothing had happened.  Afterwards a multi-round call converges and the knob takes a small number again --
    which it refuses while the launch number is large: the reset ran."""
    lib, knob = N.gpu_lib(), N.FB_DEBUG_DNS_LAUNCH
    w, c = D.wrap(0x1F), D.cluster(0x1F)
    cap, model = capture(w), D.Tracker()
    try:
        assert lib.fb_debug_set(cap.ctx, knob, 0xF0000000 - 256) == N.FB_OK
        step(cap, model, w.steps[0])
        assert lib.fb_debug_set(cap.ctx, knob, 1000) == N.FB_ERR_INVAL  # below the current number
        assert lib.fb_debug_set(cap.ctx, knob, 0) == N.FB_ERR_INVAL
        assert lib.fb_debug_set(cap.ctx, knob, 1 << 32) == N.FB_ERR_INVAL
        assert lib.fb_debug_set(cap.ctx, 5, 1) == N.FB_ERR_INVAL  # (the unassigned knob)
        assert lib.fb_debug_set(cap.ctx, knob, 0xF0000000 + 1) == N.FB_OK
        out = step(cap, model, w.steps[1])
        assert out["names_new"] == out["addrs_new"] == 0 and out["matched"] == 8
        rounds = [step(cap, model, s)["rounds"] for s in c.steps]
        assert max(rounds) >= 3
        present = sorted(model.res)
        assert len(present) == 18 and all(lookups(cap, model, present))
        assert not any(lookups(cap, model, [k for _, k in w.absent + c.absent]))
        assert lib.fb_debug_set(cap.ctx, knob, 1000) == N.FB_OK  # small again: the numbers restarted
        assert lib.fb_debug_set(cap.ctx, knob, 999) == N.FB_ERR_INVAL
        for s in D.ladder(4).steps:
            assert step(cap, model, s)["rounds"] >= 2
    finally:
        cap.close()
    off = FlodbaddGpuCapture(0, flow_capacity=0)
    try:
        assert lib.fb_debug_set(off.ctx, knob, 7) == N.FB_ERR_INVAL  # no tracker
    finally:
        off.close()


def test_clear_then_collisions():
    """clear_dns() after CLUSTER, then WRAP: the launch numbers restart at 1 over zeroed stamps, the ids restart at
    1, and everything equals a restatement that was cleared too."""
    c, w = D.cluster(0x1F), D.wrap(0x1F)
    cap, model = capture(c), D.Tracker()
    try:
        for s in c.steps[:2]:
            step(cap, model, s)
        cap.clear_dns()
        model.clear()
        check_state(cap, model)
        out = step(cap, model, w.steps[0])
        assert out["names_new"] == 8 and sorted(model.ids.values()) == list(range(1, 9)) and out["rounds"] >= 3
        fresh = D.Tracker()
        fresh.track(*w.steps[0].arrays())
        assert fresh.names == model.names and fresh.res == model.res
        out = step(cap, model, w.steps[1])
        assert out["names_new"] == out["addrs_new"] == 0
        assert all(lookups(cap, model, sorted(model.res))) and not any(lookups(cap, model, [k for _, k in w.absent]))
    finally:
        cap.close()
