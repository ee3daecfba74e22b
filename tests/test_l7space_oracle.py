"""The L7 corpora and their restatement (tests/l7space.py), pinned on the CPU: every outcome class the corpora
claim is populated, the list-scan restatement gives what each case was built to give and what the reference's
lines say on hand-written cases, the snapshot compiler applies the first-pid-found rule with stable ids, and the
/proc/net parser reads the kernel's format.  tests/test_gpu_l7space.py holds the device to this restatement."""
import ipaddress

import l7space as L
from flodbadd_amd import _native as N
from flodbadd_amd.l7 import ProcessInterner, SocketSnapshot, parse_proc_net
from flodbadd_amd.sessions import SessionInfo, SessionL7
from l7space import EXACT, FAILED, FUZZY, NONE, TCP, UDP, V4, V6, Flow, Sock


def test_census_every_class_is_populated():
    c = L.semantic()
    lab = c.labels()
    assert set(lab) == set(L.REQUIRED_SEMANTIC)
    # every rule for both families (the word-wise near misses carry their family in the label)
    for name in L.REQUIRED_SEMANTIC:
        if not name.endswith(("_v4", "_v6")) and not name.startswith("v4_mapped"):
            fams = {f.src[0] for l, f, _ in c.cases if l == name}
            assert fams == {V4, V6}, name
    assert lab["tcp_near_miss_local_ip_word_v6"] == lab["tcp_near_miss_remote_ip_word_v6"] == 4  # one per key word
    outcomes = {w[1] for _, _, w in c.cases}
    assert outcomes == {NONE, EXACT, FUZZY}
    assert len(c.socks) <= 400 and len(c.cases) <= 1500
    # both pair tables and local tables of every size, with hits at both ends and misses on every side
    assert [s.name for s in L.shapes()] == ["%s_%d" % (t, n) for t in ("pair", "local") for n in L.SHAPE_SIZES]
    for s in L.shapes():
        n = int(s.name.split("_")[1])
        assert len(s.socks) == n and len(s.socks) <= 400 and len(s.cases) <= 1500
        assert len({(k.proto, k.local, k.lport, k.remote, k.rport) for k in s.socks}) == n  # distinct keys
        lab = s.labels()
        assert lab["miss_below_the_first_key"] == lab["miss_above_the_last_key"] == 2
        assert lab["hit"] + lab["hit_first_key"] + lab["hit_last_key"] == n
        if n >= 4:
            assert lab["hit_first_key"] == lab["hit_last_key"] == 2 and lab["miss_between_two_keys"] == n - 2


def test_restatement_gives_what_every_case_was_built_to_give():
    for c in [L.semantic()] + L.shapes():
        for label, f, want in c.cases:
            assert L.resolve(c.socks, f) == want, "%s / %s: %s" % (c.name, label, L.describe(f))


def _a(text):
    ip = ipaddress.ip_address(text)
    return (V4 if ip.version == 4 else V6, int(ip))


def test_restatement_on_hand_written_cases():
    S, D, X = _a("192.168.1.10"), _a("93.184.216.34"), _a("10.9.9.9")
    f = Flow(TCP, S, 50000, D, 443)
    # src/l7.rs:1247-1254: both sides compared, addresses and ports; form B is the mirrored socket
    assert L.resolve([Sock(TCP, S, 50000, D, 443, 7)], f) == (7, EXACT)
    assert L.resolve([Sock(TCP, D, 443, S, 50000, 8)], f) == (8, EXACT)
    assert L.resolve([Sock(TCP, S, 50000, D, 444, 9)], f) == (9, FUZZY)  # exact fails on remote_port; 1109-1114 takes it
    # src/l7.rs:1227-1231: the src_port bucket is scanned first -- a form-A socket wins at any index
    assert L.resolve([Sock(TCP, D, 443, S, 50000, 1), Sock(TCP, S, 50000, D, 443, 2)], f) == (2, EXACT)
    # ... and with equal ports there is one bucket: list order decides
    g = Flow(TCP, S, 500, D, 500)
    assert L.resolve([Sock(TCP, D, 500, S, 500, 1), Sock(TCP, S, 500, D, 500, 2)], g) == (1, EXACT)
    # src/l7.rs:1256-1261: UDP compares the local side only
    u = Flow(UDP, S, 5353, D, 53)
    assert L.resolve([Sock(UDP, S, 5353, X, 1, 3)], u) == (3, EXACT)
    assert L.resolve([Sock(UDP, D, 53, X, 1, 4)], u) == (4, EXACT)
    assert L.resolve([Sock(UDP, D, 5353, X, 1, 5)], u) == (5, FUZZY)  # crosswise: fuzzy only (1117-1122)
    # src/l7.rs:1234-1243: the protocol must agree
    assert L.resolve([Sock(UDP, S, 50000, D, 443, 6)], f) == (0, NONE)
    # src/l7.rs:1111: is_unspecified() holds for 0.0.0.0 and for ::, whatever the session's family
    assert L.resolve([Sock(TCP, _a("::"), 443, _a("::"), 0, 11)], f) == (11, FUZZY)
    assert L.resolve([Sock(TCP, _a("0.0.0.0"), 50000, _a("0.0.0.0"), 0, 12)],
                     Flow(TCP, _a("2001:db8::1"), 50000, _a("2001:db8::2"), 443)) == (12, FUZZY)
    # IpAddr equality: ::ffff:192.168.1.10 is not 192.168.1.10
    m = Sock(TCP, _a("::ffff:192.168.1.10"), 50000, _a("::ffff:93.184.216.34"), 443, 13)
    assert L.resolve([m], f) == (0, NONE)
    # try_fuzzy_match walks the whole list in order (1098): a wildcard at dst_port before an address at src_port
    assert L.resolve([Sock(TCP, _a("0.0.0.0"), 443, _a("0.0.0.0"), 0, 14), Sock(TCP, S, 50000, X, 1, 15)], f) == (14, FUZZY)
    # resolve_l7_data (1026-1036): exact first, whatever the index of a fuzzy candidate
    assert L.resolve([Sock(TCP, _a("0.0.0.0"), 50000, _a("0.0.0.0"), 0, 16), Sock(TCP, S, 50000, D, 443, 17)], f) == (17, EXACT)


def test_retry_rule():
    """src/l7.rs:456-470: retry_count += 1, then FailedMaxRetries once it is above the maximum (83-89: 5)."""
    for mr, fails_at in ((0, 1), (1, 2), (5, 6), (255, None)):
        e, seen = (0, NONE, 0), None
        for k in range(1, 300):
            e = L.step(e, (0, NONE), mr)
            assert e[2] == min(k, 255)
            if e[1] == FAILED and seen is None:
                seen = k
        assert seen == fails_at, mr
    assert L.step((0, NONE, 3), (42, FUZZY), 5) == (42, FUZZY, 0)  # src/l7.rs:442-451: retry_count 0
    # the queue rules: a resolved or failed flow is not looked up; a non-current one is left alone
    flows, c1, c2 = L.ladder()
    state = {}
    st = L.run_pass(state, flows, c1.socks, 1, current=set(flows[:12]))
    assert st["flows"] == 24 and st["current"] == st["looked_up"] == 12 and st["changed"] == st["resolved"] == 4
    assert all(f not in state for f in flows[12:])
    before = dict(state)
    st = L.run_pass(state, flows, c2.socks, 1, current=set(flows[:12]))
    assert st["looked_up"] == 8 and st["failed"] == 4 and st["fuzzy"] == 4
    assert all(state[f] == before[f] for f in flows[:12] if before[f][0])  # (c2 would give them another process)
    assert all(L.resolve(c2.socks, f)[0] not in (0, before[f][0]) for f in flows[:12] if before[f][0])


def test_snapshot_compiler():
    procs = {10: ("nginx", "/usr/sbin/nginx", "www"), 20: ("curl", "/usr/bin/curl", "alice")}
    socks = [("tcp", "0.0.0.0", 80, "0.0.0.0", 0, (99, 10, 20)),      # first pid FOUND: 99 is unknown
             (6, "10.0.0.1", 40000, "1.2.3.4", 443, (98, 97)),        # no known pid: dropped
             (17, "::", 5353, None, 0, (20,)),
             (6, "2001:db8::1", 40001, "2001:db8::2", 443, (20, 10))]
    snap = SocketSnapshot(socks, procs)
    rows = snap.resolved()
    assert [r[5].pid for r in rows] == [10, 20, 20]
    assert rows[0][5] == SessionL7(10, "nginx", "/usr/sbin/nginx", "www")
    it = ProcessInterner()
    a = snap.compile(it)
    assert a.dtype == N.L7_SOCKET_DTYPE and len(a) == 3
    assert a["process_id"].tolist() == [1, 2, 2] and it.processes[2].process_name == "curl"
    assert a["protocol"].tolist() == [6, 17, 6] and a["local_family"].tolist() == [2, 10, 10]
    assert a["remote_family"].tolist() == [2, 0, 10] and a["local_port"].tolist() == [80, 5353, 40001]
    assert a[2]["local_ip"].tolist() == [0x20010DB8, 0, 0, 1] and not a["reserved0"].any() and not a["reserved1"].any()
    assert N.gpu_lib().fb_l7_validate(N.ptr(a), len(a)) == 0
    # the ids are stable across snapshots: a new process gets the next id, a known one keeps its own
    procs2 = {30: ("sshd", "/usr/sbin/sshd", "root"), 20: ("curl", "/usr/bin/curl", "alice")}
    b = SocketSnapshot([(6, "0.0.0.0", 22, "0.0.0.0", 0, (30,)), (17, "0.0.0.0", 68, None, 0, (20,))], procs2).compile(it)
    assert b["process_id"].tolist() == [3, 2] and sorted(it.processes) == [1, 2, 3]
    # SessionInfo.l7 is no dataclass field: the field list and equality are what they were
    import ipaddress as ipa
    from flodbadd_amd.sessions import Protocol, Session
    s = Session(Protocol.TCP, ipa.ip_address("192.168.1.1"), 12345, ipa.ip_address("8.8.8.8"), 80)
    x, y = SessionInfo(s), SessionInfo(s)
    assert "l7" not in SessionInfo.__dataclass_fields__ and x.l7 is None
    x.l7 = rows[0][5]
    assert x.l7 == SessionL7(10, "nginx", "/usr/sbin/nginx", "www") and x == y and y.l7 is None
    x.l7 = None
    assert x.l7 is None and x.__dict__ == y.__dict__


PROC_TCP = """  sl  local_address rem_address   st tx_queue rx_queue tr tm->when retrnsmt   uid  timeout inode
   0: 0100007F:0035 00000000:0000 0A 00000000:00000000 00:00000000 00000000   101        0 23456 1 0000000000000000 100 0 0 10 0
   1: 0A01A8C0:C350 22D8B85D:01BB 01 00000000:00000000 02:000004B1 00000000  1000        0 34567 2 0000000000000000 20 4 30 10 -1
garbage line
"""
PROC_UDP6 = """  sl  local_address                         remote_address                        st tx_queue rx_queue tr tm->when retrnsmt   uid  timeout inode ref pointer drops
 2233: 00000000000000000000000000000000:14E9 00000000000000000000000000000000:0000 07 00000000:00000000 00:00000000 00000000   108        0 4567 2 0000000000000000 0
 2234: B80D01200000000000000000010000FF:0222 00000000000000000000000000000000:0000 07 00000000:00000000 00:00000000 00000000     0        0 4568 2 0000000000000000 0
"""


def test_proc_net_parser():
    ip = ipaddress.ip_address
    assert parse_proc_net(PROC_TCP, "tcp", False) == [
        (6, ip("127.0.0.1"), 53, ip("0.0.0.0"), 0, 23456),
        (6, ip("192.168.1.10"), 50000, ip("93.184.216.34"), 443, 34567)]
    assert parse_proc_net(PROC_UDP6, 17, True) == [
        (17, ip("::"), 5353, ip("::"), 0, 4567),
        (17, ip("2001:db8::ff00:1"), 546, ip("::"), 0, 4568)]
    assert parse_proc_net("", 6, False) == [] and parse_proc_net(PROC_TCP, 6, True) == []
