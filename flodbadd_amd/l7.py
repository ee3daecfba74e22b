"""The host side of the L7 pass: the socket snapshot the device matches sessions against.

The reference's resolver task (src/l7.rs:208-500) reads the OS -- netstat2's socket list and sysinfo's process
table -- and then matches each queued session against that list (resolve_l7_data, src/l7.rs:1020-1135).  Only
the reading is I/O; the matching is a function of the session and the ordered list, and runs on the device
(fb_flow_l7).  This module is the hand-over:

  SocketSnapshot     the ordered socket list and the process table, as the reference's two reads give them
  ProcessInterner    SessionL7 <-> the ids the device stores, stable for the life of a capture
  ProcessNameInterner  process names <-> the ids the whitelist check and the endpoint learning compare on the device
  parse_proc_net     /proc/net/{tcp,tcp6,udp,udp6} text -> sockets with their inodes (pure)
  snapshot_from_proc a snapshot of this machine (Linux)
"""
import ipaddress
import os

import numpy as np

from . import _native as N
from .sessions import Protocol, SessionL7, ip_to_words


def _protocol(p):
    if isinstance(p, str):
        return {"tcp": 6, "udp": 17}[p.lower()]
    p = int(p)
    if p not in (6, 17):
        raise ValueError("protocol %r: TCP (6) or UDP (17)" % (p,))
    return p


class ProcessInterner:
    """The processes a capture has handed the device, each under one id >= 1 for as long as the capture lives:
    a session resolved under an earlier snapshot still decodes after later ones."""

    def __init__(self):
        self._ids = {}
        self.processes = {}  # id -> SessionL7

    def intern(self, l7):
        i = self._ids.get(l7)
        if i is None:
            i = self._ids[l7] = len(self._ids) + 1
            self.processes[i] = l7
        return i


def ascii_lower(s):
    """Lower-case A-Z only: two strings are eq_ignore_ascii_case iff their ascii_lower are equal."""
    return "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in s)


class ProcessNameInterner:
    """Process names under the two ids fb_set_l7_process_names takes, each >= 1 and stable for as long as the
    capture lives: name_id names the string verbatim (new_from_sessions' fingerprint compares the string itself,
    src/whitelists.rs:144-153), match_id its ASCII-lower-cased form (process_matches is eq_ignore_ascii_case,
    src/whitelists.rs:716-724).  The whitelist compiler and the table upload share one, so an endpoint compiled
    before any process of its name was seen already carries the id that process will get."""

    def __init__(self):
        self._match = {}
        self._name = {}
        self.names = {}  # name_id -> the name verbatim

    def match_id(self, name):
        return self._match.setdefault(ascii_lower(name), len(self._match) + 1)

    def name_id(self, name):
        i = self._name.get(name)
        if i is None:
            i = self._name[name] = len(self._name) + 1
            self.names[i] = name
        return i

    def table(self, processes):
        """The (match_id, name_id) arrays of fb_set_l7_process_names for a ProcessInterner's `processes`
        {id: SessionL7}: entry p names process id p, entry 0 is 0."""
        n = max(processes, default=0) + 1
        m, v = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        for p, l7 in processes.items():
            m[p], v[p] = self.match_id(l7.process_name), self.name_id(l7.process_name)
        return m, v


class SocketSnapshot:
    """One read of the OS, in the reference's terms: `sockets`, the ordered list of (protocol, local_addr,
    local_port, remote_addr, remote_port, pids) -- the order is part of the input, every scan of the reference
    returns the first match --, and `processes` {pid: (name, path, username)}.  A UDP socket's remote side may be
    (None, 0)."""

    def __init__(self, sockets, processes):
        self.sockets = [(_protocol(p), ipaddress.ip_address(la), int(lp),
                         None if ra is None else ipaddress.ip_address(ra), int(rp), tuple(int(x) for x in pids))
                        for p, la, lp, ra, rp, pids in sockets]
        self.processes = {int(pid): tuple(v) for pid, v in processes.items()}

    def resolved(self):
        """extract_l7_from_socket (src/l7.rs:1137-1199) per socket: the first of its pids that is in the process
        table names its process; a socket with none makes the reference's scans continue, so it is dropped.
        -> [(protocol, local_addr, local_port, remote_addr, remote_port, SessionL7)] in list order."""
        out = []
        for p, la, lp, ra, rp, pids in self.sockets:
            pid = next((x for x in pids if x in self.processes), None)
            if pid is not None:
                name, path, user = self.processes[pid]
                out.append((p, la, lp, ra, rp, SessionL7(pid, name, path, user)))
        return out

    def compile(self, interner):
        """The fb_l7_socket array of fb_set_l7_sockets, process ids drawn from `interner`."""
        rows = self.resolved()
        a = np.zeros(len(rows), dtype=N.L7_SOCKET_DTYPE)
        for i, (p, la, lp, ra, rp, l7) in enumerate(rows):
            a[i]["local_ip"], a[i]["local_family"] = ip_to_words(la)
            if ra is not None:
                a[i]["remote_ip"], a[i]["remote_family"] = ip_to_words(ra)
            elif p == 6:
                raise ValueError("socket %d: a TCP socket needs a remote address" % i)
            if p == 17:
                a[i]["remote_family"] = 0  # (ignored: a UDP socket matches by its local side)
                a[i]["remote_ip"] = 0
            a[i]["local_port"], a[i]["remote_port"], a[i]["protocol"] = lp, rp, p
            a[i]["process_id"] = interner.intern(l7)
        return a


def _proc_addr(hexaddr, v6):
    """An address of /proc/net/*: the kernel prints each 32-bit word of the network-order address as a
    host-order (little-endian here) hex number."""
    raw = b"".join(bytes.fromhex(hexaddr[k:k + 8])[::-1] for k in range(0, len(hexaddr), 8))
    return ipaddress.IPv6Address(raw) if v6 else ipaddress.IPv4Address(raw)


def parse_proc_net(text, protocol, v6):
    """The rows of one /proc/net/{tcp,tcp6,udp,udp6} file, in file order ->
    [(protocol, local_addr, local_port, remote_addr, remote_port, inode)].  Lines that do not parse (the
    header among them) are skipped."""
    proto, out = _protocol(protocol), []
    want = 32 if v6 else 8
    for line in text.splitlines():
        f = line.split()
        if len(f) < 10 or ":" not in f[1] or ":" not in f[2]:
            continue
        try:
            (la, lp), (ra, rp) = f[1].split(":"), f[2].split(":")
            if len(la) != want or len(ra) != want:
                continue
            out.append((proto, _proc_addr(la, v6), int(lp, 16), _proc_addr(ra, v6), int(rp, 16), int(f[9])))
        except ValueError:
            continue
    return out


def snapshot_from_proc(proc="/proc"):
    """This machine's sockets and processes (Linux): /proc/net/{tcp,tcp6,udp,udp6} in that order, the pids of
    each socket from the /proc/<pid>/fd links to its inode (ascending pid), the process table from comm, exe
    and the owner of /proc/<pid>.  What cannot be read (another user's fds) is left out, as netstat2 leaves it."""
    import pwd
    inode_pids, processes = {}, {}
    for d in sorted((d for d in os.listdir(proc) if d.isdigit()), key=int):
        pid, base = int(d), os.path.join(proc, d)
        try:
            with open(os.path.join(base, "comm")) as f:
                name = f.read().rstrip("\n")
            uid = os.stat(base).st_uid
        except OSError:
            continue
        try:
            path = os.readlink(os.path.join(base, "exe"))
        except OSError:
            path = ""
        try:
            user = pwd.getpwuid(uid).pw_name
        except KeyError:
            user = ""
        processes[pid] = (name, path, user)
        try:
            fds = os.listdir(os.path.join(base, "fd"))
        except OSError:
            continue
        for fd in fds:
            try:
                t = os.readlink(os.path.join(base, "fd", fd))
            except OSError:
                continue
            if t.startswith("socket:[") and t.endswith("]"):
                inode_pids.setdefault(int(t[8:-1]), []).append(pid)
    sockets = []
    for fname, proto, v6 in (("tcp", 6, False), ("tcp6", 6, True), ("udp", 17, False), ("udp6", 17, True)):
        try:
            with open(os.path.join(proc, "net", fname)) as f:
                text = f.read()
        except OSError:
            continue
        for p, la, lp, ra, rp, inode in parse_proc_net(text, proto, v6):
            sockets.append((p, la, lp, ra, rp, inode_pids.get(inode, ())))
    return SocketSnapshot(sockets, processes)


__all__ = ["SessionL7", "SocketSnapshot", "ProcessInterner", "ProcessNameInterner", "parse_proc_net", "snapshot_from_proc", "Protocol"]
