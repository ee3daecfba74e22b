"""The L7 pass on the GPU (fb_flow_l7: k_flow_l7, and fb_l7_lookup_dev: k_l7_lookup, flodbadd_amd/csrc/fb_l7.hip)
on the enumerated corpora of tests/l7space.py.

The flows go in through process_parsed, the sessions come back through the export, and the whole plane
(fb_flow_l7_dev, indexed by fb_flow_rec.slot; unoccupied slots zero) and the counters (fb_l7_stats) must equal the
list-scan restatement run on the exported keys: everything is an integer, the comparison is byte for byte.
tests/test_l7space_oracle.py pins the restatement and the census of classes on the CPU.

The captures use an empty service table, so no key is reversed on its way into the table: the flows under test
are the corpus's own."""
import json

import numpy as np
import pytest

import l7space as L
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.l7 import SocketSnapshot
from flodbadd_amd.sessions import Session, SessionFilter, SessionL7, WhitelistState
from l7space import EXACT, FAILED, FUZZY, NONE, TCP, UDP, V4, Flow, Sock, addr

pytestmark = pytest.mark.gpu

S = 10 ** 9
T0 = 1_700_000_000 * S


def capture(timed=False, capacity=1 << 12):
    return FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=capacity, service_bitmap=bytes(8192),
                              timed=timed)


def install(cap, socks):
    """The socket list as it stands (process ids the corpus's own) through fb_set_l7_sockets."""
    a = L.socket_array(socks)
    N.check(N.gpu_lib().fb_set_l7_sockets(cap.ctx, N.ptr(a) if len(a) else None, len(a)))
    cap._l7_installed = True


def install_snapshot(cap, socks):
    """The same through SocketSnapshot and cap.set_l7_sockets (process pid = the corpus id) -> the list with the
    ids the capture interned, which is what the device stores."""
    snap = SocketSnapshot([(s.proto, L.text(s.local), s.lport, L.text(s.remote), s.rport, (s.pid,)) for s in socks],
                          {s.pid: ("proc%d" % s.pid, "/bin/proc%d" % s.pid, "user%d" % (s.pid % 3)) for s in socks})
    assert cap.set_l7_sockets(snap) == len(socks)
    ids = {l7.pid: i for i, l7 in cap._l7_procs.processes.items()}
    return [s._replace(pid=ids[s.pid]) for s in socks]


def load(cap, flows, ts=None):
    g = cap.process_parsed(L.parsed_array(flows), ts=ts)
    assert g.stats["error"] == 0 and g.stats["n_session"] == g.stats["new_sessions"] == len(flows)


def table(cap):
    """[(slot, Flow)] of the exported sessions, and the set of current ones (None: untimed, all)."""
    rows = [(int(r["slot"]), L.flow_of(r)) for r in cap.export_flows(SessionFilter.All)]
    if not cap.timed:
        return rows, None
    status = cap.status_bytes()
    return rows, {f for s, f in rows if int(status[s]) == 0 or int(status[s]) & N.STATUS_CURRENT}


def want_plane(cap, rows, state):
    want = np.zeros(cap.table_info()["capacity"], dtype=N.L7_REC_DTYPE)
    for slot, f in rows:
        e = state.get(f, (0, NONE, 0))
        want[slot] = (e[0], e[1], e[2], 0)
    return want


def check_pass(cap, socks, state, max_retries=5, tag=""):
    """One pass against the restatement (state {Flow: element} brought forward): the plane byte for byte, the
    counters; -> (counters, the slots the restatement says changed)."""
    rows, current = table(cap)
    before = dict(state)
    want_st = L.run_pass(state, [f for _, f in rows], socks, max_retries, current)
    st = cap.update_l7(max_retries)
    got, want = cap.l7_records(), want_plane(cap, rows, state)
    if got.tobytes() != want.tobytes():
        bad = ["%s: %s (slot %d): device %s, restatement %s" % (tag, L.describe(f), s, got[s], want[s])
               for s, f in rows if got[s] != want[s]]
        occupied = np.zeros(len(got), dtype=bool)
        occupied[[s for s, _ in rows]] = True
        stray = np.flatnonzero(got.view(np.uint64) * ~occupied)
        assert False, "%d differences, %d unoccupied slots written\n%s" % (len(bad), len(stray), "\n".join(bad[:10]))
    assert st == want_st, tag
    changed = {s for s, f in rows if state.get(f, (0, 0, 0))[0] != before.get(f, (0, 0, 0))[0]}
    assert len(changed) == st["changed"]
    return st, changed


# ---- 1. every corpus through the pass and through the lookup ----------------------------------------------
def test_corpora_through_the_pass():
    cap = capture()
    try:
        for c in [L.semantic()] + L.shapes():
            cap.clear_all_sessions()
            assert not cap.l7_records().view(np.uint64).any()
            install(cap, c.socks)
            load(cap, c.flows)
            rows, _ = table(cap)
            assert sorted(f for _, f in rows) == sorted(c.flows), c.name  # the corpus's own keys, none reversed
            state = {}
            st, _ = check_pass(cap, c.socks, state, tag=c.name)
            for label, f, want in c.cases:
                assert state[f][:2] == want, "%s / %s: %s" % (c.name, label, L.describe(f))
            assert st["looked_up"] == st["flows"] == len(c.flows)
    finally:
        cap.close()


def test_corpora_through_the_lookup():
    """fb_l7_lookup_dev: the pass's device function on caller-supplied keys; needs no flow table."""
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=0)
    lib = N.gpu_lib()
    try:
        keys = L.key_array(L.semantic().flows)
        d = N.DeviceBuffer(keys.nbytes).upload(keys)
        o = N.DeviceBuffer(8 * len(keys))
        assert lib.fb_l7_lookup_dev(cap.ctx, d.ptr, len(keys), o.ptr, None) == N.FB_ERR_INVAL  # no snapshot yet
        assert lib.fb_flow_l7(cap.ctx, None, None, None) == N.FB_ERR_INVAL                   # no flow table
        for c in [L.semantic()] + L.shapes():
            install(cap, c.socks)
            got = cap.l7_lookup(L.key_array(c.flows))
            want = np.zeros(len(c.flows), dtype=N.L7_REC_DTYPE)
            for i, f in enumerate(c.flows):
                pid, src = L.resolve(c.socks, f)
                want[i] = (pid, src, 0, 0)
            bad = [i for i in range(len(want)) if got[i] != want[i]]
            assert got.tobytes() == want.tobytes(), "%s: %s: device %s, restatement %s" % (
                c.name, L.describe(c.flows[bad[0]]), got[bad[0]], want[bad[0]])
        assert len(cap.l7_lookup(keys[:0])) == 0
        # an invalid snapshot is refused and the installed one stays
        c = L.shape(9, "pair")
        install(cap, c.socks)
        bad = L.socket_array(c.socks[:2])
        bad[1]["process_id"] = 0
        assert lib.fb_set_l7_sockets(cap.ctx, N.ptr(bad), 2) == N.FB_ERR_INVAL
        got = cap.l7_lookup(L.key_array(c.flows))
        assert [(int(r["process_id"]), int(r["source"])) for r in got] == [L.resolve(c.socks, f) for f in c.flows]
        # the empty snapshot is valid: nothing matches
        install(cap, [])
        assert not cap.l7_lookup(L.key_array(c.flows)).view(np.uint64).any()
        cap.clear_l7()
        assert lib.fb_l7_lookup_dev(cap.ctx, d.ptr, len(keys), o.ptr, None) == N.FB_ERR_INVAL
    finally:
        cap.close()


# ---- 2. pass state --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_retries", [0, 1, 5])
def test_retry_ladder(max_retries):
    """Successive passes under one snapshot: tries counts up, the flow fails once it is above max_retries and is
    not looked up again; then two passes on the unchanged table write identical bytes."""
    flows, c1, c2 = L.ladder()
    cap = capture()
    try:
        install(cap, c1.socks)
        load(cap, flows)
        state = {}
        for k in range(max_retries + 1):
            st, _ = check_pass(cap, c1.socks, state, max_retries, "pass %d" % k)
            assert st["looked_up"] == (24 if k == 0 else 16)
            assert st["failed"] == (16 if k == max_retries else 0) and st["changed"] == (8 if k == 0 else 0)
        assert sorted(e[1:] for e in state.values()) == [(EXACT, 0)] * 8 + [(FAILED, max_retries + 1)] * 16
        before = cap.l7_records().tobytes()
        st, _ = check_pass(cap, c1.socks, state, max_retries, "settled")
        assert st["looked_up"] == st["changed"] == st["failed"] == 0 and st["resolved"] == 8
        assert cap.l7_records().tobytes() == before
        # a later snapshot that would resolve the failed flows, and give the resolved ones another process: neither
        install(cap, c2.socks)
        st, _ = check_pass(cap, c2.socks, state, max_retries, "later snapshot")
        assert st["looked_up"] == 0 and cap.l7_records().tobytes() == before
    finally:
        cap.close()


def test_max_retries_255_never_fails_and_a_later_snapshot_resolves():
    flows, c1, c2 = L.ladder()
    cap = capture()
    lib = N.gpu_lib()
    try:
        install(cap, c1.socks)
        load(cap, flows)
        state = {}
        check_pass(cap, c1.socks, state, 255, "first")
        prm = np.zeros(1, dtype=N.L7_PARAMS_DTYPE)
        prm[0]["max_retries"] = 255
        rows, _ = table(cap)
        for _ in range(258):  # past the count's width
            N.check(lib.fb_flow_l7(cap.ctx, N.ptr(prm), None, None))
            L.run_pass(state, [f for _, f in rows], c1.socks, 255)
        st, _ = check_pass(cap, c1.socks, state, 255, "after 260 passes")
        assert st["looked_up"] == 16 and st["failed"] == 0
        assert sorted(e[1:] for e in state.values()) == [(NONE, 255)] * 16 + [(EXACT, 0)] * 8
        # NULL params are the defaults: 255 tries are above 5
        st = np.zeros(1, dtype=N.L7_STATS_DTYPE)
        N.check(lib.fb_flow_l7(cap.ctx, None, N.ptr(st), None))
        assert int(st[0]["failed"]) == 16
        for bad in ({"max_retries": 256}, {"flags": 1}, {"reserved": (0, 1)}):
            p = np.zeros(1, dtype=N.L7_PARAMS_DTYPE)
            for k, v in bad.items():
                p[0][k] = v
            assert lib.fb_flow_l7(cap.ctx, N.ptr(p), None, None) == N.FB_ERR_INVAL
        # unresolved, not failed flows under a later snapshot: resolved flows keep their process
        cap.clear_l7()
        install(cap, c1.socks)
        state = {}
        check_pass(cap, c1.socks, state, 5, "again")
        first = dict(state)
        install(cap, c2.socks)
        st, _ = check_pass(cap, c2.socks, state, 5, "second snapshot")
        assert st["looked_up"] == 16 and st["fuzzy"] == st["changed"] == 8 and st["resolved"] == 16
        assert all(state[f] == first[f] for f in flows if first[f][0])
        assert all(L.resolve(c2.socks, f)[0] != first[f][0] for f in flows if first[f][0])
    finally:
        cap.close()


def test_stamps_current_only_and_incremental_sessions():
    """A timed capture aged so that half of its sessions are not current: those are not looked up; the flows that
    got a process carry the pass time -- the retry bookkeeping stamps nothing -- and the incremental getter
    returns exactly them, with their process."""
    flows, c1, c2 = L.ladder()
    cap = capture(timed=True)
    try:
        ts = np.array([T0 + (150 * S if i % 2 else 0) + i for i in range(len(flows))], dtype=np.uint64)
        load(cap, flows, ts=ts)
        t1 = T0 + 200 * S
        full = cap.get_sessions(now_ns=t1)  # ages the table and moves the getter's fetch timestamp
        assert len(full) == 24 and all(i.l7 is None for i in full)
        socks = install_snapshot(cap, c2.socks)
        cap.set_pass_time(t1 + S)
        state = {}
        st, changed = check_pass(cap, socks, state, 5, "timed")
        assert st["current"] == st["looked_up"] == 12 and st["changed"] == 8 and st["failed"] == 0
        stamps = cap.modified_stamps()
        assert {int(i) for i in np.nonzero(stamps)[0]} == changed and set(stamps[sorted(changed)].tolist()) == {t1 + S}
        inc = cap.get_sessions(incremental=True)
        rows, _ = table(cap)
        by_slot = dict(rows)
        assert sorted(L.flow_of_session(i.session) for i in inc) == sorted(by_slot[s] for s in changed)
        procs = cap._l7_procs.processes
        for i in inc:
            assert i.l7 == procs[state[L.flow_of_session(i.session)][0]] and i.last_modified_ns == t1 + S
            assert i.l7.process_name == "proc%d" % i.l7.pid
        # a second pass: the four unresolved current flows are retried, nothing is stamped
        cap.set_pass_time(t1 + 2 * S)
        st, changed2 = check_pass(cap, socks, state, 5, "timed, second")
        assert st["looked_up"] == 4 and not changed2 and (cap.modified_stamps() == stamps).all()
        # without a pass time the pass stamps nothing
        cap.set_pass_time(0)
        cap.clear_l7()
        install_snapshot(cap, c2.socks)
        st, _ = check_pass(cap, socks, {}, 5, "unstamped")
        assert st["changed"] == 8 and (cap.modified_stamps() == stamps).all()
    finally:
        cap.close()


def test_plane_follows_growth_and_purge_and_the_clears():
    cap = capture(timed=True, capacity=1 << 9)
    lib = N.gpu_lib()
    try:
        old = [Flow(TCP, addr(V4, 230, i), 42000 + i, addr(V4, 231, i % 8), 443) for i in range(100)]
        new = [Flow(TCP, addr(V4, 232, i), 43000 + i, addr(V4, 231, 8 + i % 8), 443) for i in range(100)]
        socks = [Sock(TCP, f.src, f.sport, f.dst, f.dport, 1000 + i) for i, f in enumerate(old + new) if i % 2 == 0]
        socks.append(Sock(TCP, L.WILD4, 443, L.WILD4, 0, 7))  # the odd ones: fuzzy
        install(cap, socks)
        load(cap, old, ts=np.full(100, T0, dtype=np.uint64))
        load(cap, new, ts=np.full(100, T0 + 1000 * S, dtype=np.uint64))
        state = {}
        st, _ = check_pass(cap, socks, state, 5, "before")
        assert st["exact"] == st["fuzzy"] == 100

        def by_key():
            recs = cap.l7_records()
            return {L.flow_of(r): tuple(int(x) for x in recs[int(r["slot"])]) for r in cap.export_flows(SessionFilter.All)}

        want = by_key()
        cap0 = cap.table_info()["capacity"]
        k = 0
        while cap.table_info()["capacity"] == cap0:  # growth: new flows until the table has grown
            more = [Flow(UDP, addr(V4, 240 + k, i), 44000, addr(V4, 248 + k, i), 5000) for i in range(250)]
            load(cap, more, ts=np.full(250, T0 + 1000 * S, dtype=np.uint64))
            k += 1
            assert k < 8
        got = by_key()
        assert {f: got[f] for f in want} == want and all(v == (0, 0, 0, 0) for f, v in got.items() if f not in want)
        # purge: the first hundred flows (idle since T0) go, the others keep their element at their new slots
        age = cap.update_sessions_status(T0 + 1100 * S, purge=True, retention_s=500)
        assert age["purged"] == 100
        got = by_key()
        assert {f: v for f, v in got.items() if v[0]} == {f: v for f, v in want.items() if f in set(new)}
        for f in old:
            state.pop(f)
        # a purged flow that returns starts unresolved, and the next pass resolves it again
        load(cap, old[:2], ts=np.full(2, T0 + 1100 * S, dtype=np.uint64))
        got = by_key()
        assert got[old[0]] == got[old[1]] == (0, 0, 0, 0)
        st, changed = check_pass(cap, socks, state, 5, "after the purge")
        assert st["changed"] == 2 and st["exact"] == st["fuzzy"] == 1 and st["resolved"] == 102
        # fb_flow_clear zeroes the plane and keeps the snapshot; fb_l7_clear drops the snapshot
        cap.clear_all_sessions()
        assert not cap.l7_records().view(np.uint64).any()
        load(cap, new[:10], ts=np.full(10, T0 + 1200 * S, dtype=np.uint64))
        st, _ = check_pass(cap, socks, {}, 5, "after fb_flow_clear")
        assert st["changed"] == 10
        cap.clear_l7()
        assert not cap.l7_records().view(np.uint64).any()
        assert lib.fb_flow_l7(cap.ctx, None, None, None) == N.FB_ERR_INVAL and b"snapshot" in lib.fb_last_error()
    finally:
        cap.close()


# ---- 3. the Python layer ------------------------------------------------------------------------------------
def _wl(endpoints):
    return json.dumps({"date": "today", "signature": None, "whitelists": [
        {"name": "custom_whitelist", "extends": None, "endpoints": endpoints}]})


def test_update_sessions_order_and_whitelist_process_endpoints():
    """update_sessions runs the L7 pass before the whitelist pass: a process endpoint turns the host-check flows of
    that process Conforming with no process_names argument; an explicit process_names still wins."""
    cap = capture()
    try:
        flows = [Flow(TCP, addr(V4, 210, i), 47000 + i, addr(V4, 211, i), 443) for i in range(6)]
        load(cap, flows)
        out = cap.update_sessions()
        assert set(out) == {"status", "blacklist", "whitelist", "domains"}  # no snapshot: as before
        snap = SocketSnapshot([(6, L.text(f.src), f.sport, L.text(f.dst), f.dport, (900 + i, 10 if i < 4 else 20))
                               for i, f in enumerate(flows)],
                              {10: ("curl", "/usr/bin/curl", "alice"), 20: ("wget", "/usr/bin/wget", "bob")})
        cap.set_l7_sockets(snap)
        cap.set_custom_whitelists(_wl([{"process": "curl", "port": 443, "protocol": "TCP"}]))
        out = cap.update_sessions()
        assert out["l7"]["changed"] == out["l7"]["exact"] == 6 and out["whitelist"]["host_check"] == 6
        infos = {L.flow_of_session(i.session): i for i in cap.get_sessions()}
        for i, f in enumerate(flows):
            assert infos[f].l7 == (SessionL7(10, "curl", "/usr/bin/curl", "alice") if i < 4 else
                                   SessionL7(20, "wget", "/usr/bin/wget", "bob"))
            assert infos[f].is_whitelisted is (WhitelistState.Conforming if i < 4 else WhitelistState.NonConforming)
        assert not cap.get_whitelist_conformance()
        exc = cap.get_whitelist_exceptions()
        assert sorted(L.flow_of_session(i.session) for i in exc) == sorted(flows[4:])
        assert all(i.l7.process_name == "wget" and "wget" in i.whitelist_reason for i in exc)
        assert cap.l7_process_names() == {Session.from_key(r): "curl" if L.flow_of(r) in flows[:4] else "wget"
                                          for r in cap.export_flows(SessionFilter.All)}
        # the learning path takes the attribution too
        doc = json.loads(cap.create_custom_whitelists())
        assert sorted(e["process"] for e in doc["whitelists"][0]["endpoints"]) == ["curl"] * 4 + ["wget"] * 2
        # an explicit argument wins
        names = {Session.from_key(r): "curl" for r in cap.export_flows(SessionFilter.All)}
        cap.update_whitelist(None, names)
        assert cap.get_whitelist_conformance()
    finally:
        cap.close()


def test_session_info_l7_in_all_four_getters():
    cap = capture(timed=True)
    try:
        flows = [Flow(TCP, addr(V4, 212, i), 48000 + i, (V4, (93 << 24) | (184 << 16) | i), 443) for i in range(8)]
        load(cap, flows, ts=np.full(8, T0, dtype=np.uint64))
        assert all(i.l7 is None for i in cap.get_sessions())
        snap = SocketSnapshot([(6, L.text(f.src), f.sport, L.text(f.dst), f.dport, (50 + i,)) for i, f in enumerate(flows[:6])],
                              {50 + i: ("p%d" % i, "/opt/p%d" % i, "u") for i in range(8)})
        cap.set_custom_blacklists(json.dumps({"date": "d", "signature": "s", "blacklists": [
            {"name": "bad", "ip_ranges": ["93.184.0.0/29"]}]}))
        cap.set_custom_whitelists(_wl([{"ip": "93.184.0.6", "port": 443}]))
        cap.set_l7_sockets(snap)
        out = cap.update_sessions(T0 + S)
        assert out["l7"]["changed"] == 6 and out["l7"]["looked_up"] == 8
        want = {f: (SessionL7(50 + i, "p%d" % i, "/opt/p%d" % i, "u") if i < 6 else None) for i, f in enumerate(flows)}
        for name, got, n in (("sessions", cap.get_sessions(), 8), ("current", cap.get_current_sessions(), 8),
                             ("blacklisted", cap.get_blacklisted_sessions(), 8),
                             ("exceptions", cap.get_whitelist_exceptions(), 7)):
            assert len(got) == n, name
            for i in got:
                assert i.l7 == want[L.flow_of_session(i.session)], (name, i.session)
        assert int((cap.l7_records()["process_id"] != 0).sum()) == 6
    finally:
        cap.close()
