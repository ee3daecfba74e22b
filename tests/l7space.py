"""The L7 pass's input space: enumerated socket snapshots and flows, and a second restatement of the
reference's matching (src/l7.rs) as literal loops over the socket list -- nothing here looks at the index
fb_set_l7_sockets builds (flodbadd_amd/csrc/fb_l7_index.h).

Restated:
  exact_scan   try_exact_match_from_index (src/l7.rs:1220-1279): the (src_port, protocol) bucket, then the
               (dst_port, protocol) bucket, each in list order; the first socket that equals the session in
               form A or form B.  A bucket of the reference's port index is the sockets with that local port
               (src/l7.rs:300-330), in list order.
  fuzzy_scan   try_fuzzy_match (src/l7.rs:1091-1135): the whole list in order.
  resolve      resolve_l7_data (src/l7.rs:1020-1044): exact, else fuzzy.
  step         one resolver cycle's outcome for one queued session (src/l7.rs:429-470): a match stores the
               process with retry_count 0; a miss raises retry_count and fails the session once it is above
               max_retries.  (The count is a byte here and stays at 255.)
  run_pass     populate_l7's queue rule (src/capture.rs:1452: only sessions whose l7 is None; src/l7.rs:919-922:
               never one already resolved or failed) over the current sessions, with the pass's counters.

Addresses are (family, int) with family 2 / 10, as IpAddr equality needs both.  A socket is a Sock tuple; every
socket of a corpus carries its own process id (PID0 + list index), so an outcome names the socket that won.

A case is (label, flow, want), want = (process id, source) written down by hand when the case was built: the
CPU test holds the restatement to it, the GPU tests hold the device to the restatement.
"""
import collections
import functools
import ipaddress
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

V4, V6 = 2, 10
TCP, UDP = 6, 17
NONE, EXACT, FUZZY, FAILED = 0, 1, 2, 3
PID0 = 100

Sock = collections.namedtuple("Sock", "proto local lport remote rport pid")   # local / remote: (family, int)
Flow = collections.namedtuple("Flow", "proto src sport dst dport")            # src / dst: (family, int), one family
WILD4, WILD6 = (V4, 0), (V6, 0)


# ---- the restatement -------------------------------------------------------------------------------------
def _is_match(s, f):
    if s.proto != f.proto:  # proto_ok
        return False
    if f.proto == TCP:
        return ((s.local == f.src and s.lport == f.sport and s.remote == f.dst and s.rport == f.dport) or
                (s.local == f.dst and s.lport == f.dport and s.remote == f.src and s.rport == f.sport))
    return (s.local == f.src and s.lport == f.sport) or (s.local == f.dst and s.lport == f.dport)


def exact_scan(socks, f):
    """-> the list index of the socket try_exact_match_from_index returns, or None."""
    for port in (f.sport, f.dport):
        for i, s in enumerate(socks):
            if s.lport != port or s.proto != f.proto:  # (the bucket of (port, protocol))
                continue
            if _is_match(s, f):
                return i
    return None


def fuzzy_scan(socks, f):
    for i, s in enumerate(socks):
        if s.proto != f.proto:
            continue
        port_match = s.lport == f.sport or s.lport == f.dport
        wildcard = s.local[1] == 0  # is_unspecified: 0.0.0.0 or ::
        addr_match = s.local == f.src or s.local == f.dst
        if port_match and (wildcard or addr_match):
            return i
    return None


def resolve(socks, f):
    """-> (process id, source): (0, NONE) when nothing matches."""
    i = exact_scan(socks, f)
    if i is not None:
        return socks[i].pid, EXACT
    i = fuzzy_scan(socks, f)
    if i is not None:
        return socks[i].pid, FUZZY
    return 0, NONE


def step(elem, match, max_retries):
    """elem = (process id, source, tries) of a session the cycle looked up -> its element afterwards."""
    pid, source = match
    if pid:
        return (pid, source, 0)
    tries = min(elem[2] + 1, 255)
    return (0, FAILED if tries > max_retries else NONE, tries)


STATS = ("flows", "current", "looked_up", "exact", "fuzzy", "failed", "resolved", "changed")


def run_pass(state, flows, socks, max_retries=5, current=None):
    """One pass over `flows` (state: {flow: element}, missing = (0, NONE, 0), updated in place); current: the
    set of current flows (None: all).  -> the pass's counters."""
    st = dict.fromkeys(STATS, 0)
    for f in flows:
        st["flows"] += 1
        e = state.get(f, (0, NONE, 0))
        cur = current is None or f in current
        st["current"] += cur
        if cur and e[0] == 0 and e[1] != FAILED:
            st["looked_up"] += 1
            m = resolve(socks, f)
            e = step(e, m, max_retries)
            st["exact"] += m[1] == EXACT
            st["fuzzy"] += m[1] == FUZZY
            st["failed"] += e[1] == FAILED
            st["changed"] += m[0] != 0
            state[f] = e
        st["resolved"] += e[0] != 0
    return st


# ---- corpora -----------------------------------------------------------------------------------------------
class Corpus:
    def __init__(self, name, pid0=PID0):
        self.name, self.socks, self.cases, self.pid0 = name, [], [], pid0

    def sock(self, proto, local, lport, remote=None, rport=0):
        """Append a socket (remote None: the unspecified address of the local family) -> its process id."""
        remote = (local[0], 0) if remote is None else remote
        self.socks.append(Sock(proto, local, lport, remote, rport, self.pid0 + len(self.socks)))
        return self.socks[-1].pid

    def case(self, label, flow, pid=0, source=NONE):
        self.cases.append((label, flow, (pid, source)))

    @property
    def flows(self):
        return [c[1] for c in self.cases]

    def labels(self):
        return collections.Counter(c[0] for c in self.cases)


def addr(fam, case, j):
    """Address j of case `case`: 10.<case>.<j> / 2001:db8:<case>::<j>, every key word in use for IPv6."""
    if fam == V4:
        return (V4, (10 << 24) | (case << 8) | j)
    return (V6, (0x20010DB8 << 96) | (case << 80) | (0x5EED << 48) | (0xABCD << 32) | (0x77 << 16) | j)


def _ports(case):
    return 2000 + 8 * case, 2000 + 8 * case + 1, 2000 + 8 * case + 2


def _flip_word(a, w):
    """The address with one bit of key word w (0 = most significant) flipped."""
    fam, v = a
    return (fam, v ^ (1 << 3)) if fam == V4 else (fam, v ^ (1 << (32 * (3 - w) + 9)))


@functools.lru_cache(maxsize=None)
def semantic():
    """Every rule of the two scans, for TCP and UDP, IPv4 and IPv6; cases are kept apart by their ports."""
    c = Corpus("semantic")
    n = [0]

    def new():
        n[0] += 1
        return n[0]

    for fam in (V4, V6):
        tag = "v4" if fam == V4 else "v6"
        other_wild = WILD6 if fam == V4 else WILD4
        # ---- exact, TCP
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
        p = c.sock(TCP, S, sp, D, dp)
        c.case("tcp_form_a_only", Flow(TCP, S, sp, D, dp), p, EXACT)
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
        p = c.sock(TCP, D, dp, S, sp)
        c.case("tcp_form_b_only", Flow(TCP, S, sp, D, dp), p, EXACT)
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
        c.sock(TCP, D, dp, S, sp)
        p = c.sock(TCP, S, sp, D, dp)
        c.case("tcp_both_forms_ports_differ_a_wins_at_higher_index", Flow(TCP, S, sp, D, dp), p, EXACT)
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, _, _ = _ports(k)
        p = c.sock(TCP, D, sp, S, sp)
        c.sock(TCP, S, sp, D, sp)
        c.case("tcp_both_forms_ports_equal_lower_index_wins", Flow(TCP, S, sp, D, sp), p, EXACT)
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, _, _ = _ports(k)
        p = c.sock(TCP, S, sp, D, sp)
        c.sock(TCP, D, sp, S, sp)
        c.case("tcp_both_forms_ports_equal_lower_index_wins", Flow(TCP, S, sp, D, sp), p, EXACT)
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
        p = c.sock(TCP, S, sp, D, dp)
        c.sock(TCP, S, sp, D, dp)
        c.sock(TCP, S, sp, D, dp)
        c.case("tcp_duplicates_lowest_index_wins", Flow(TCP, S, sp, D, dp), p, EXACT)
        # a pair that differs from the flow in exactly one key word.  A wrong remote side leaves the local side
        # equal to the source: the fuzzy phase then takes that socket; a wrong local side matches nothing.
        words = range(1) if fam == V4 else range(4)
        for w in words:
            k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
            c.sock(TCP, _flip_word(S, w), sp, D, dp)
            c.case("tcp_near_miss_local_ip_word_%s" % tag, Flow(TCP, S, sp, D, dp))
            k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
            p = c.sock(TCP, S, sp, _flip_word(D, w), dp)
            c.case("tcp_near_miss_remote_ip_word_%s" % tag, Flow(TCP, S, sp, D, dp), p, FUZZY)
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, xp = _ports(k)
        c.sock(TCP, S, xp, D, dp)
        c.case("tcp_near_miss_local_port", Flow(TCP, S, sp, D, dp))
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, xp = _ports(k)
        p = c.sock(TCP, S, sp, D, xp)
        c.case("tcp_near_miss_remote_port", Flow(TCP, S, sp, D, dp), p, FUZZY)
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
        c.sock(UDP, S, sp, D, dp)
        c.case("protocol_mismatch", Flow(TCP, S, sp, D, dp))
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
        c.sock(TCP, S, sp, D, dp)
        c.case("protocol_mismatch", Flow(UDP, S, sp, D, dp))
        # ---- exact, UDP: the local side only
        k = new(); S, D, X = addr(fam, k, 1), addr(fam, k, 2), addr(fam, k, 3); sp, dp, xp = _ports(k)
        p = c.sock(UDP, S, sp, X, xp)
        c.case("udp_local_side_only_any_remote", Flow(UDP, S, sp, D, dp), p, EXACT)
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
        p = c.sock(UDP, D, dp)
        c.case("udp_form_b_only", Flow(UDP, S, sp, D, dp), p, EXACT)
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
        c.sock(UDP, D, dp)
        p = c.sock(UDP, S, sp)
        c.case("udp_both_forms_ports_differ_a_wins_at_higher_index", Flow(UDP, S, sp, D, dp), p, EXACT)
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, _, _ = _ports(k)
        p = c.sock(UDP, D, sp)
        c.sock(UDP, S, sp)
        c.case("udp_both_forms_ports_equal_lower_index_wins", Flow(UDP, S, sp, D, sp), p, EXACT)
        k = new(); S, D, X = addr(fam, k, 1), addr(fam, k, 2), addr(fam, k, 3); sp, dp, _ = _ports(k)
        p = c.sock(UDP, S, sp, X, 1)
        c.sock(UDP, S, sp, X, 2)
        c.case("udp_duplicates_lowest_index_wins", Flow(UDP, S, sp, D, dp), p, EXACT)
        k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
        c.sock(UDP, _flip_word(S, 0), sp)
        c.case("udp_near_miss_local_ip", Flow(UDP, S, sp, D, dp))
        # ---- fuzzy
        for proto in (TCP, UDP):
            k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
            p = c.sock(proto, other_wild, sp)
            c.case("fuzzy_wildcard_of_the_other_family_%s" % tag, Flow(proto, S, sp, D, dp), p, FUZZY)
            k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
            p = c.sock(proto, (fam, 0), dp)
            c.case("fuzzy_wildcard_of_the_own_family", Flow(proto, S, sp, D, dp), p, FUZZY)
            k = new(); S, D, X = addr(fam, k, 1), addr(fam, k, 2), addr(fam, k, 3); sp, dp, xp = _ports(k)
            p = c.sock(proto, D, sp, X, xp)
            c.case("fuzzy_cross_pairing_dst_ip_at_src_port", Flow(proto, S, sp, D, dp), p, FUZZY)
            k = new(); S, D, X = addr(fam, k, 1), addr(fam, k, 2), addr(fam, k, 3); sp, dp, xp = _ports(k)
            p = c.sock(proto, S, dp, X, xp)
            c.case("fuzzy_cross_pairing_src_ip_at_dst_port", Flow(proto, S, sp, D, dp), p, FUZZY)
            k = new(); S, D, X = addr(fam, k, 1), addr(fam, k, 2), addr(fam, k, 3); sp, dp, xp = _ports(k)
            p = c.sock(proto, other_wild, dp)
            c.sock(proto, D, sp, X, xp)  # (an address match at src_port that is not an exact match)
            c.case("fuzzy_lower_wildcard_at_dst_port_beats_higher_address_at_src_port", Flow(proto, S, sp, D, dp), p, FUZZY)
            k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, _ = _ports(k)
            c.sock(proto, (fam, 0), sp)
            p = c.sock(proto, S, sp, D, dp)
            c.case("exact_beats_lower_index_fuzzy", Flow(proto, S, sp, D, dp), p, EXACT)
            k = new(); S, D = addr(fam, k, 1), addr(fam, k, 2); sp, dp, xp = _ports(k)
            c.sock(proto, (fam, 0), xp)
            c.case("fuzzy_wildcard_at_another_port", Flow(proto, S, sp, D, dp))
    # an IPv4-mapped IPv6 socket does not equal the IPv4 session (IpAddr equality), exact or fuzzy
    for proto in (TCP, UDP):
        k = new(); S, D = addr(V4, k, 1), addr(V4, k, 2); sp, dp, _ = _ports(k)
        m = lambda a: (V6, (0xFFFF << 32) | a[1])  # noqa: E731
        c.sock(proto, m(S), sp, m(D), dp)
        c.case("v4_mapped_v6_socket_does_not_match_v4_flow", Flow(proto, S, sp, D, dp))
    assert len({f for f in c.flows}) == len(c.flows)
    return c


SHAPE_SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def shape(n, table):
    """n distinct keys in one table -- 'pair': n TCP sockets (both tables then hold n keys, the exact phase reads
    the pair table); 'local': n UDP sockets (the pair table is empty) -- whose keys differ in the local address
    alone, two apart: a hit at every key (the first and the last among them) and a miss below the first, between
    every two neighbours and above the last.  Every other socket is IPv6, so every key word is compared."""
    c = Corpus("%s_%d" % (table, n))
    proto = TCP if table == "pair" else UDP
    sp, dp = 4000, 4001
    for fam in (V4, V6):
        base = addr(fam, 200, 100)
        far = addr(fam, 201, 1)
        at = lambda j: (fam, base[1] + j)  # noqa: E731
        m = (n + 1) // 2 if fam == V4 else n // 2   # the keys of this family
        pids = [c.sock(proto, at(2 * j), sp, far, dp) for j in range(m)]
        for j in range(m):
            lab = "hit_first_key" if j == 0 else "hit_last_key" if j == m - 1 else "hit"
            c.case(lab, Flow(proto, at(2 * j), sp, far, dp), pids[j], EXACT)
            if j + 1 < m:
                c.case("miss_between_two_keys", Flow(proto, at(2 * j + 1), sp, far, dp))
        c.case("miss_below_the_first_key", Flow(proto, (fam, base[1] - 1), sp, far, dp))
        c.case("miss_above_the_last_key", Flow(proto, at(2 * m), sp, far, dp))
    return c


def shapes():
    return [shape(n, t) for t in ("pair", "local") for n in SHAPE_SIZES]


@functools.lru_cache(maxsize=None)
def ladder():
    """The pass-state corpus: flows that resolve at once, flows that never do, and flows that only a second
    snapshot resolves -> (flows, first snapshot, second snapshot).  Under the second snapshot the flows the
    first one resolved would get another process (a socket of theirs at a lower index)."""
    c1, c2 = Corpus("ladder_first"), Corpus("ladder_second", pid0=5000)
    flows = []
    for j in range(24):
        fam = V4 if j % 2 == 0 else V6
        proto = TCP if j % 4 < 2 else UDP
        S, D = addr(fam, 220 + j, 1), addr(fam, 220 + j, 2)
        sp, dp, _ = _ports(300 + j)
        f = Flow(proto, S, sp, D, dp)
        flows.append(f)
        kind = j % 3  # 0: resolved by both snapshots (differently), 1: by the second alone, 2: by neither
        if kind == 0:
            c2.sock(proto, S, sp, D, dp)  # (another process id than the first snapshot's: the list index differs)
            c2.sock(proto, S, sp, D, dp)
            c1.sock(UDP, addr(V4, 250, j + 1), 9)  # (shifts the first snapshot's indices)
            c1.sock(proto, S, sp, D, dp)
        elif kind == 1:
            c2.sock(proto, (fam, 0), dp)
    return flows, c1, c2


# ---- arrays ----------------------------------------------------------------------------------------------
def words(a):
    fam, v = a
    if fam == V4:
        return [v, 0, 0, 0]
    return [(v >> 96) & 0xFFFFFFFF, (v >> 64) & 0xFFFFFFFF, (v >> 32) & 0xFFFFFFFF, v & 0xFFFFFFFF]


def from_words(fam, w):
    w = [int(x) for x in w]
    return (fam, w[0]) if fam == V4 else (fam, (w[0] << 96) | (w[1] << 64) | (w[2] << 32) | w[3])


def text(a):
    return str(ipaddress.IPv4Address(a[1]) if a[0] == V4 else ipaddress.IPv6Address(a[1]))


def socket_array(socks, udp_remote_family=True):
    """fb_l7_socket records of a socket list.  A UDP socket keeps its remote side (the device must ignore it)."""
    from flodbadd_amd import _native as N
    a = np.zeros(len(socks), dtype=N.L7_SOCKET_DTYPE)
    for i, s in enumerate(socks):
        a[i]["local_ip"], a[i]["remote_ip"] = words(s.local), words(s.remote)
        a[i]["local_port"], a[i]["remote_port"], a[i]["protocol"] = s.lport, s.rport, s.proto
        a[i]["local_family"], a[i]["remote_family"] = s.local[0], s.remote[0]
        a[i]["process_id"] = s.pid
    return a


def _fill_key(rec, f):
    rec["src_ip"], rec["dst_ip"] = words(f.src), words(f.dst)
    rec["src_port"], rec["dst_port"], rec["protocol"], rec["family"] = f.sport, f.dport, f.proto, f.src[0]


def parsed_array(flows):
    """One fb_parsed_pkt per flow (a UDP-like packet without flags), pkt_index = position."""
    from flodbadd_amd import _native as N
    a = np.zeros(len(flows), dtype=N.PARSED_DTYPE)
    for i, f in enumerate(flows):
        _fill_key(a[i], f)
        a[i]["packet_length"], a[i]["ip_packet_length"], a[i]["pkt_index"] = 10, 38, i
    return a


def key_array(flows):
    """fb_session_key records (40 bytes) of the flows."""
    from flodbadd_amd import _native as N
    a = np.zeros(len(flows), dtype=np.dtype(N.KEY_FIELDS))
    for i, f in enumerate(flows):
        _fill_key(a[i], f)
    return a


def flow_of(rec):
    """A record's key fields (fb_flow_rec, fb_pkt_out) as a Flow."""
    fam = int(rec["family"])
    return Flow(int(rec["protocol"]), from_words(fam, rec["src_ip"]), int(rec["src_port"]),
                from_words(fam, rec["dst_ip"]), int(rec["dst_port"]))


def flow_of_session(s):
    """A flodbadd_amd.sessions.Session as a Flow."""
    fam = lambda ip: (V4 if ip.version == 4 else V6, int(ip))  # noqa: E731
    return Flow(int(s.protocol), fam(s.src_ip), s.src_port, fam(s.dst_ip), s.dst_port)


def describe(f):
    return "%s %s:%d -> %s:%d" % ("tcp" if f.proto == TCP else "udp", text(f.src), f.sport, text(f.dst), f.dport)


@functools.lru_cache(maxsize=None)
def host_program():
    """tests/l7_index_host.cpp, built once per run with the sanitizers (host code with its own main)."""
    d = tempfile.mkdtemp(prefix="l7index")
    exe = os.path.join(d, "l7_index_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "l7_index_host.cpp")], check=True)
    return exe


def host_match(sock_arr, flows):
    """The host program over fb_l7_socket records and flows -> (status, pair keys, local keys, [(process id,
    source)] per flow); status 1: the program's build_l7_index refused the snapshot."""
    d = tempfile.mkdtemp(prefix="l7indexrun")
    src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    keys = key_array(flows)
    with open(src, "wb") as f:
        f.write(np.array([len(sock_arr), len(keys)], dtype=np.uint64).tobytes())
        f.write(sock_arr.tobytes())
        f.write(keys.tobytes())
    subprocess.run([host_program(), src, dst], check=True)
    out = np.fromfile(dst, dtype=np.uint64)
    return (int(out[0]), int(out[1]), int(out[2]),
            [(int(w) & 0xFFFFFFFF, int(w) >> 32) for w in out[3:]])


REQUIRED_SEMANTIC = (
    "tcp_form_a_only", "tcp_form_b_only", "tcp_both_forms_ports_differ_a_wins_at_higher_index",
    "tcp_both_forms_ports_equal_lower_index_wins", "tcp_duplicates_lowest_index_wins",
    "tcp_near_miss_local_ip_word_v4", "tcp_near_miss_remote_ip_word_v4", "tcp_near_miss_local_ip_word_v6",
    "tcp_near_miss_remote_ip_word_v6", "tcp_near_miss_local_port", "tcp_near_miss_remote_port", "protocol_mismatch",
    "udp_local_side_only_any_remote", "udp_form_b_only", "udp_both_forms_ports_differ_a_wins_at_higher_index",
    "udp_both_forms_ports_equal_lower_index_wins", "udp_duplicates_lowest_index_wins", "udp_near_miss_local_ip",
    "fuzzy_wildcard_of_the_other_family_v4", "fuzzy_wildcard_of_the_other_family_v6", "fuzzy_wildcard_of_the_own_family",
    "fuzzy_cross_pairing_dst_ip_at_src_port", "fuzzy_cross_pairing_src_ip_at_dst_port",
    "fuzzy_lower_wildcard_at_dst_port_beats_higher_address_at_src_port", "exact_beats_lower_index_fuzzy",
    "fuzzy_wildcard_at_another_port", "v4_mapped_v6_socket_does_not_match_v4_flow")
