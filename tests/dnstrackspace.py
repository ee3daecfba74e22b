"""The DNS tracker's enumerated corpora and their expectations ("Enumerated corpora").

Three things live here, none of them a test:

* name_tag / addr_tag / home -- the two tag functions of flodbadd_amd/csrc/fb_dns_hash.h restated with Python
  integers (64-bit arithmetic by masking), and host_tags(), which runs the stand-alone host program
  (tests/dns_hash_host.cpp: the header itself under g++ with the address and undefined-behaviour sanitizers).
* Tracker -- a second sequential restatement of DnsPacketProcessor, independent of flodbadd_amd.dns.DnsResolver
  (nothing of flodbadd_amd/dns.py is imported): written from src/dns.rs:16-121 of the reference and from
  DESIGN.md 3.14, and exact where DnsResolver compares strings -- name ids, the order of the last writer, the
  pending times, the counters, the capacities.
* the corpora -- ID-RUNS, LADDER, WRAP, CLUSTER (with ABSENT), LAST-WRITER, TIMES and GROW --, every key found
  by searching candidate strings and addresses with the restated tags, and census(), which recomputes every
  home, tag, slot and sorted position the corpora claim.

A corpus is a list of steps (Call: one tracking call; Expire: one expiry) for one context.  Tables are
name capacity 16 and address capacity 16 -- 32 slots each -- unless the corpus says otherwise; under hash_mask
0x1F a tag equals its home slot, so every same-home pair is compared on its bytes, and under 0xFF keys of one
home mostly have different tags and are passed without a compare.
"""
import functools
import ipaddress
import itertools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from flodbadd_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
M64 = (1 << 64) - 1
TAG_USED = 1 << 63
NO_TIME = N.FB_DNS_NO_TIME
S = 10 ** 9
T0 = 1_700_000_000 * S
SLOTS = 32  # of a 16/16 context
MASKS = (0x1F, 0xFF)
MAX_ADDR_CAP = 1 << 28


# ---- a. the tag functions -----------------------------------------------------------------------------------
def _mix(h, w):
    h = ((h ^ w) * 0xBF58476D1CE4E5B9) & M64
    return h ^ (h >> 31)


def _fin(h, mask):
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    return (h & mask) | TAG_USED


def name_tag(row, length, mask=M64):
    """name_tag of the first `length` bytes of `row`; whatever follows them in the row does not count."""
    row = bytes(row)
    h = 0x9E3779B97F4A7C15 ^ length
    for k in range(0, length, 4):
        h = _mix(h, int.from_bytes(row[k:min(k + 4, length)].ljust(4, b"\0"), "little"))
    return _fin(h, mask)


def addr_tag(words, family, mask=M64):
    h = 0x9E3779B97F4A7C15 ^ family
    h = _mix(h, int(words[0]) | int(words[1]) << 32)
    h = _mix(h, int(words[2]) | int(words[3]) << 32)
    return _fin(h, mask)


def home(tag, slots=SLOTS):
    return tag & (slots - 1)


def key_of(ip):
    """(w0, w1, w2, w3, family) of an address: IPv4 numeric in word 0, IPv6 as four big-endian words.  A tuple
    of five integers is taken as it is."""
    if isinstance(ip, tuple):
        return tuple(int(x) for x in ip)
    ip = ipaddress.ip_address(ip)
    if ip.version == 4:
        return (int(ip), 0, 0, 0, 2)
    v = int(ip)
    return tuple((v >> (96 - 32 * k)) & 0xFFFFFFFF for k in range(4)) + (10,)


def ip_of(key):
    if key[4] == 2:
        return ipaddress.IPv4Address(key[0])
    return ipaddress.IPv6Address(key[0] << 96 | key[1] << 64 | key[2] << 32 | key[3])


def key_tag(key, mask=M64):
    return addr_tag(key[:4], key[4], mask)


def bname_tag(name, mask=M64):
    return name_tag(name, len(name), mask)


@functools.lru_cache(maxsize=None)
def host_program():
    """tests/dns_hash_host.cpp, built once per run with the sanitizers (host code with its own main)."""
    d = tempfile.mkdtemp(prefix="dnshash")
    exe = os.path.join(d, "dns_hash_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "dns_hash_host.cpp")], check=True)
    return exe


def host_tags(rows, lens, keys, mask):
    """The host program over name rows ([n, 256] uint8 with their lengths) and address keys -> (name tags,
    address tags) as lists of Python integers."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, N.FB_DNS_MAX_NAME)
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    ka = np.array([list(k) for k in keys], dtype=np.uint32).reshape(-1, 5)
    d = tempfile.mkdtemp(prefix="dnshashrun")
    src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    try:
        with open(src, "wb") as f:
            np.array([len(lens), len(ka), mask & M64], dtype=np.uint64).tofile(f)
            lens.tofile(f)
            rows.tofile(f)
            ka.tofile(f)
        subprocess.run([host_program(), src, dst], check=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        out = np.fromfile(dst, dtype=np.uint64)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    assert len(out) == len(lens) + len(ka)
    return [int(x) for x in out[:len(lens)]], [int(x) for x in out[len(lens):]]


# ---- the steps of a corpus ----------------------------------------------------------------------------------
class Call:
    """One tracking call: messages in packet order, as fb_dns_parse_dev leaves them.  garbage: the byte a name
    row is filled with past name_len.  ts / pkt: frame times and the frame each message came from (default:
    message i came from frame i).  n_dns: the batch statistics' count, when it is below the message count."""

    def __init__(self, ts=None, pkt=None, n_dns=None, rounds=None):
        self.rows, self.ts, self.pkt, self.n_dns, self.rounds = [], ts, pkt, n_dns, rounds

    def _add(self, tx, flags, name=b"", addrs=(), status=0, garbage=0):
        name = name.encode("ascii") if isinstance(name, str) else bytes(name)
        self.rows.append((tx, flags, name, [key_of(a) for a in addrs], status, garbage))
        return self

    def query(self, tx, name, garbage=0):
        return self._add(tx, N.DNS_QUERY | N.DNS_HAS_QUESTION, name, garbage=garbage)

    def reverse(self, tx):
        return self._add(tx, N.DNS_QUERY | N.DNS_HAS_QUESTION | N.DNS_REVERSE, b"4.3.2.1.in-addr.arpa", garbage=0x5A)

    def no_question(self, tx):
        return self._add(tx, N.DNS_QUERY)

    def response(self, tx, addrs=()):
        return self._add(tx, 0, b"", addrs)

    def rejected(self, tx, query=True, addrs=()):
        return self._add(tx, (N.DNS_QUERY if query else 0) | N.DNS_HAS_QUESTION, b"bad.example", addrs, status=2)

    def arrays(self):
        n = len(self.rows)
        msgs = np.zeros(n, dtype=N.DNS_MSG_DTYPE)
        names = np.zeros((n, N.FB_DNS_MAX_NAME), dtype=np.uint8)
        addrs = np.zeros((n, N.FB_DNS_MAX_ADDRS), dtype=N.FB_IP_DTYPE)
        for i, (tx, flags, name, ads, status, garbage) in enumerate(self.rows):
            assert len(name) < N.FB_DNS_MAX_NAME and len(ads) <= N.FB_DNS_MAX_ADDRS
            msgs[i]["pkt_index"] = self.pkt[i] if self.pkt is not None else i
            msgs[i]["id"], msgs[i]["status"], msgs[i]["flags"] = tx, status, flags
            msgs[i]["questions"], msgs[i]["answers"] = 1 if name else 0, len(ads)
            msgs[i]["name_len"], msgs[i]["n_addrs"] = len(name), len(ads)
            names[i, :] = garbage
            names[i, :len(name)] = np.frombuffer(name, dtype=np.uint8)
            for j, k in enumerate(ads):
                addrs[i, j]["addr"], addrs[i, j]["family"] = k[:4], k[4]
        return msgs, names, addrs

    def query_names(self):
        return [r[2] for r in self.rows if r[1] & N.DNS_QUERY and r[1] & N.DNS_HAS_QUESTION and not r[1] & N.DNS_REVERSE
                and r[4] == 0]

    def answer_keys(self):
        return [k for r in self.rows if not r[1] & N.DNS_QUERY and r[4] == 0 for k in r[3]]


class Expire:
    def __init__(self, now):
        self.now = now


class Corpus:
    """name; hash_mask; the steps; the two capacities; grows: whether a call may grow the tables (else every
    call stays within the bounds of the growth rule, which check_bounds asserts); present / absent: address keys
    to look up after the last step."""

    def __init__(self, name, mask, steps, name_capacity=16, addr_capacity=16, grows=False, absent=()):
        self.name, self.mask, self.steps = name, mask, steps
        self.name_capacity, self.addr_capacity, self.grows, self.absent = name_capacity, addr_capacity, grows, list(absent)

    def config(self):
        return {"dns_name_capacity": self.name_capacity, "dns_addr_capacity": self.addr_capacity,
                "dns_hash_mask": self.mask}

    def calls(self):
        return [s for s in self.steps if isinstance(s, Call)]

    def __repr__(self):
        return self.name


# ---- b. the second restatement ------------------------------------------------------------------------------
def _pow2_at_least(v):
    p = 1
    while p < v:
        p <<= 1
    return p


class Tracker:
    """DnsPacketProcessor (src/dns.rs:16-121) over parsed messages, with the ids, orders, times, counters and
    capacities DESIGN.md 3.14 defines.

      pend_name[tx], pend_time[tx]   pending_dns_queries (src/dns.rs:17): the name id (0: none) and the
                                     query's frame time, NO_TIME where the call had no times
      res[key] = (name id, order)    dns_resolutions (src/dns.rs:18); order = messages handed in before the
                                     call + the message's index ("Resolutions")
      names[id]                      the store: ids are 1-based and numbered in the order of the names' first
                                     message ("Deterministic ids")
    """

    def __init__(self, name_capacity=16, addr_capacity=16):
        self.name_cap, self.addr_cap = name_capacity, addr_capacity
        self.clear(count=False)

    def clear(self, count=True):
        self.names, self.ids, self.res = [None], {}, {}
        self.pend_name = np.zeros(N.FB_DNS_IDS, dtype=np.uint32)
        self.pend_time = np.full(N.FB_DNS_IDS, NO_TIME, dtype=np.uint64)
        self.messages = 0
        self.writes = self.writes + 1 if count else 0  # (a clear invalidates what a reader exported)

    def bounds(self, msgs, n_dns=None):
        """(accepted queries, answers of all responses) of a call: what the growth rule adds up before
        anything is written ("Growth")."""
        cnt = len(msgs) if n_dns is None else min(n_dns, len(msgs))
        q = a = 0
        for m in msgs[:cnt]:
            if int(m["status"]) != 0:
                continue
            f = int(m["flags"])
            if f & N.DNS_QUERY:
                q += bool(f & N.DNS_HAS_QUESTION and not f & N.DNS_REVERSE)
            else:
                a += min(int(m["n_addrs"]), N.FB_DNS_MAX_ADDRS)
        return q, a

    def would_grow(self, msgs, n_dns=None):
        q, a = self.bounds(msgs, n_dns)
        return len(self.names) - 1 + q > self.name_cap or len(self.res) + a > self.addr_cap

    def track(self, msgs, names, addrs, ts=None, n_dns=None):
        n = len(msgs)
        out = dict.fromkeys(("messages", "queries", "responses", "matched", "resolutions", "names_new", "addrs_new"), 0)
        out["taken"], out["new_names"] = np.zeros(n, dtype=np.uint32), []
        if n == 0:
            return out
        cnt = n if n_dns is None else min(n_dns, n)
        if self.would_grow(msgs, n_dns):  # both tables, each to the larger of twice itself and the power of two
            q, a = self.bounds(msgs, n_dns)
            want = len(self.names) - 1 + q
            if want > self.name_cap:
                self.name_cap = min(N.FB_DNS_MAX_NAMES, max(2 * self.name_cap, _pow2_at_least(want)))
            want = len(self.res) + a
            if want > self.addr_cap:
                self.addr_cap = min(MAX_ADDR_CAP, max(2 * self.addr_cap, _pow2_at_least(want)))
        out["messages"] = cnt
        for i in range(cnt):
            m = msgs[i]
            if int(m["status"]) != 0:
                continue  # src/dns.rs:94-96: a packet DnsPacket::parse rejects is logged and skipped
            tx, f = int(m["id"]), int(m["flags"])  # src/dns.rs:40
            if f & N.DNS_QUERY:  # src/dns.rs:41
                if not f & N.DNS_HAS_QUESTION or f & N.DNS_REVERSE:
                    continue  # src/dns.rs:43 (no first question), 46-50 (reverse lookups excluded)
                nm = bytes(names[i][:min(int(m["name_len"]), N.FB_DNS_MAX_NAME - 1)])
                nid = self.ids.get(nm)
                if nid is None:
                    nid = self.ids[nm] = len(self.names)
                    self.names.append(nm)
                    out["new_names"].append((nid, nm))
                    out["names_new"] += 1
                self.pend_name[tx] = nid  # src/dns.rs:52-60: insert replaces an earlier query of the id
                self.pend_time[tx] = int(ts[int(m["pkt_index"])]) if ts is not None else NO_TIME
                out["queries"] += 1
            else:  # src/dns.rs:62-91
                out["responses"] += 1
                nid = int(self.pend_name[tx])  # src/dns.rs:65-68: remove, whether or not there are answers
                self.pend_name[tx], self.pend_time[tx] = 0, NO_TIME
                out["taken"][i] = nid
                if not nid:
                    continue  # src/dns.rs:69
                out["matched"] += 1
                for a in addrs[i][:min(int(m["n_addrs"]), N.FB_DNS_MAX_ADDRS)]:  # src/dns.rs:76-90
                    key = tuple(int(w) for w in a["addr"]) + (int(a["family"]),)
                    out["addrs_new"] += key not in self.res
                    self.res[key] = (nid, self.messages + i)  # insert: the later packet replaces
                    out["resolutions"] += 1
        self.messages += n
        if out["resolutions"]:
            self.writes += 1
        return out

    def expire(self, now):
        """The cleanup task (src/dns.rs:112-117): a query stays while now - timestamp < 30 s.  One stored without
        a time never goes, and neither does one whose time is ahead of `now`."""
        dropped = 0
        for tx in np.nonzero(self.pend_name)[0]:
            t = int(self.pend_time[tx])
            if t != NO_TIME and now >= t and now - t >= N.FB_DNS_EXPIRY_NS:
                self.pend_name[tx], self.pend_time[tx] = 0, NO_TIME
                dropped += 1
        return dropped

    def info(self):
        return {"names": len(self.names) - 1, "addrs": len(self.res), "name_capacity": self.name_cap,
                "addr_capacity": self.addr_cap, "pending": int(np.count_nonzero(self.pend_name)),
                "messages": self.messages, "writes": self.writes}

    def lookup(self, key):
        return self.res.get(key_of(key), (0, 0))[0]

    # strings, for the comparison with DnsResolver
    def pending_strings(self):
        return {int(tx): self.names[int(self.pend_name[tx])].decode("ascii") for tx in np.nonzero(self.pend_name)[0]}

    def resolution_strings(self):
        return {ip_of(k): self.names[v[0]].decode("ascii") for k, v in self.res.items()}


def check_bounds(corpus):
    """Every call of a non-growing corpus stays within both bounds of the growth rule; returns the model after
    the last step."""
    model = Tracker(corpus.name_capacity, corpus.addr_capacity)
    for k, step in enumerate(corpus.steps):
        if isinstance(step, Expire):
            model.expire(step.now)
            continue
        msgs, names, addrs = step.arrays()
        assert corpus.grows or not model.would_grow(msgs, step.n_dns), (corpus.name, k)
        model.track(msgs, names, addrs, ts=step.ts, n_dns=step.n_dns)
    return model


# ---- c. key search ------------------------------------------------------------------------------------------
def _names(prefix):
    return (("%s%d.example" % (prefix, i)).encode("ascii") for i in itertools.count())


def _v4s(net):
    return (key_of("10.%d.%d.%d" % (net, i >> 8 & 255, i & 255)) for i in itertools.count(1))


def _v6s(net):
    return (key_of("2001:db8:%x::%x" % (net, i)) for i in itertools.count(1))


def find(gen, tagf, want_home, count, want_tag8=None, skip=()):
    """The first `count` candidates of `gen` whose home (of 32 slots) is want_home -- and whose tag under 0xFF
    is want_tag8, if given."""
    out = []
    for c in gen:
        t = tagf(c, 0xFF)
        if home(t) == want_home and (want_tag8 is None or t == want_tag8) and c not in skip:
            out.append(c)
            if len(out) == count:
                return out


def mixed_addrs(net, want_home, count):
    """`count` addresses of one home, IPv4 and IPv6 alternating."""
    v4, v6 = find(_v4s(net), key_tag, want_home, (count + 1) // 2), find(_v6s(net), key_tag, want_home, count // 2)
    return [(v4 if k % 2 == 0 else v6)[k // 2] for k in range(count)]


def occupied(keys, tagf, mask, slots=SLOTS):
    """{key: slot} of a sequential insert in the given order.  WHICH key sits in which slot of a cluster depends
    on the order -- on the device, on who wins a claim --, the SET of occupied slots does not."""
    used, out = set(), {}
    for k in keys:
        p = home(tagf(k, mask), slots)
        while p in used:
            p = (p + 1) % slots
        used.add(p)
        out[k] = p
    return out


LADDER_HOME = 13
WRAP_HOMES = ((29, 3), (30, 3), (31, 2))
CLUSTER_HOMES = ((9, 4), (10, 3), (11, 3))
GARBAGE = (0x00, 0xFF, 0x41)


@functools.lru_cache(maxsize=None)
def wrap_keys():
    """Eight names and eight addresses with homes 29, 30, 31 (3 + 3 + 2): five of each land in slots 0..4."""
    names, addrs = [], []
    for h, c in WRAP_HOMES:
        names += find(_names("wrap-"), bname_tag, h, c)
        addrs += mixed_addrs(0x29, h, c)
    return names, addrs


@functools.lru_cache(maxsize=None)
def cluster_keys():
    """Ten names and ten addresses on the adjacent homes 9, 10, 11 (4 + 3 + 3).  Among them, each pair with one
    home and one tag under 0xFF (hence under 0x1F too):
      names      a name and the same name plus one byte (a proper prefix); two names differing only in the last
                 byte; two names of length 4m + 3 differing only in the first byte of the last, partial dword
      addresses  an IPv4 and an IPv6 key with equal word 0; IPv6 keys differing only in word 3; IPv6 keys differing
                 only in word 0
    Returns (names, addresses, {claim: (key, key)})."""
    (h0, _), (h1, _), (h2, _) = CLUSTER_HOMES
    pairs = {}
    for nm in _names("cl-prefix-"):
        if home(bname_tag(nm, 0xFF)) == h0 and bname_tag(nm + b"x", 0xFF) == bname_tag(nm, 0xFF):
            pairs["prefix"] = (nm, nm + b"x")
            break
    for i in itertools.count():
        a, b = b"cl-last-%d.example-a" % i, b"cl-last-%d.example-b" % i
        if home(bname_tag(a, 0xFF)) == h1 and bname_tag(a, 0xFF) == bname_tag(b, 0xFF):
            pairs["last_byte"] = (a, b)
            break
    for i in itertools.count():
        stem = b"cl-part-%d.example" % i
        stem += b"." * ((-len(stem)) % 4)  # 4m bytes, then a partial dword of three
        a, b = stem + b"pzz", stem + b"qzz"
        if home(bname_tag(a, 0xFF)) == h2 and bname_tag(a, 0xFF) == bname_tag(b, 0xFF):
            pairs["partial_dword"] = (a, b)
            break
    names = list(pairs["prefix"]) + find(_names("cl-a-"), bname_tag, h0, 2)
    names += list(pairs["last_byte"]) + find(_names("cl-b-"), bname_tag, h1, 1)
    names += list(pairs["partial_dword"]) + find(_names("cl-c-"), bname_tag, h2, 1)
    # addresses
    for v4 in find(_v4s(0xC1), key_tag, h0, 16):
        t = key_tag(v4, 0xFF)
        v6 = next((k for k in ((v4[0], 0, 0, j, 10) for j in range(1, 2048)) if key_tag(k, 0xFF) == t), None)
        if v6:
            pairs["v4_v6_word0"] = (v4, v6)
            break
    a = find(_v6s(0xC2), key_tag, h1, 1)[0]
    b = find(((a[0], a[1], a[2], j, 10) for j in itertools.count(0x1000)), key_tag, h1, 1, key_tag(a, 0xFF))[0]
    pairs["v6_word3"] = (a, b)
    a = find(_v6s(0xC3), key_tag, h2, 1)[0]
    b = find(((0x20010DB9 + j, a[1], a[2], a[3], 10) for j in itertools.count()), key_tag, h2, 1, key_tag(a, 0xFF))[0]
    pairs["v6_word0"] = (a, b)
    addrs = list(pairs["v4_v6_word0"]) + mixed_addrs(0xC4, h0, 2)
    addrs += list(pairs["v6_word3"]) + find(_v4s(0xC5), key_tag, h1, 1)
    addrs += list(pairs["v6_word0"]) + find(_v4s(0xC6), key_tag, h2, 1)
    return names, addrs, pairs


def absent_keys(present, mask):
    """Addresses never inserted, both families, for the cluster the `present` keys make in a 32-slot table:
    homes = its first, a middle and its last slot, slot 31, and the empty slot behind it.  Under 0x1F every one
    whose home has a present key shares that key's tag.  -> [(claim, key)]"""
    slots = sorted(occupied(present, key_tag, mask).values())
    run = [s for s in slots if s >= 16] + [s for s in slots if s < 16] if 0 in slots and 31 in slots else slots
    targets = (("first", run[0]), ("middle", run[len(run) // 2]), ("last", run[-1]), ("slot31", 31),
               ("behind", (run[-1] + 1) % SLOTS))
    out = []
    for claim, h in targets:
        out.append((claim + "-v4", find(_v4s(0xAB), key_tag, h, 1, skip=present)[0]))
        out.append((claim + "-v6", find(_v6s(0xAB), key_tag, h, 1, skip=present)[0]))
    return out


# ---- c. the corpora -----------------------------------------------------------------------------------------
def _pairs_call(names, addrs, tx0, garbage=lambda i: 0, order=None):
    """One query per name on its own transaction id, then one response per id carrying one address."""
    c = Call()
    idx = list(range(len(names))) if order is None else order
    for i in idx:
        c.query(tx0 + i, names[i], garbage=garbage(i))
    for i in idx:
        c.response(tx0 + i, [addrs[i]])
    return c


@functools.lru_cache(maxsize=None)
def wrap(mask):
    """WRAP: the eight keys in one call, then the identical call again (8 + 8 is exactly the capacity)."""
    names, addrs = wrap_keys()
    return Corpus("wrap-%#x" % mask, mask, [_pairs_call(names, addrs, 300), _pairs_call(names, addrs, 300)],
                  absent=absent_keys(addrs, mask))


@functools.lru_cache(maxsize=None)
def cluster(mask):
    """CLUSTER: the ten keys in one call with the garbage bytes rotating over the names; then the same keys again
    in four calls of five (ten more queries would pass the growth bound), with the other two garbage bytes."""
    names, addrs, _ = cluster_keys()
    steps = [_pairs_call(names, addrs, 100, garbage=lambda i: GARBAGE[i % 3])]
    for g in (1, 2):
        for half in (range(0, 5), range(5, 10)):
            steps.append(_pairs_call(names, addrs, 100, garbage=lambda i, g=g: GARBAGE[(i + g) % 3], order=list(half)))
    return Corpus("cluster-%#x" % mask, mask, steps, absent=absent_keys(addrs, mask))


@functools.lru_cache(maxsize=None)
def ladder_keys():
    return find(_names("ladder-"), bname_tag, LADDER_HOME, 6), mixed_addrs(0x1A, LADDER_HOME, 6)


@functools.lru_cache(maxsize=None)
def ladder(k):
    """LADDER: k distinct names of one home and tag, each in one message, in call 1; k distinct addresses of one
    home and tag in call 2.  Every round publishes exactly one slot of the chain -- the claim of a slot is won
    by one item, the others of the tag stop there until the next launch, compare, differ and move on together
    --, so each call takes k rounds, and each call's rounds belong to one table."""
    names, addrs = ladder_keys()
    q, r = Call(rounds=k), Call(rounds=k)
    for i in range(k):
        q.query(40 + i, names[i])
        r.response(40 + i, [addrs[i]])
    return Corpus("ladder-%d" % k, 0x1F, [q, r])


@functools.lru_cache(maxsize=None)
def last_writer(mask=0x1F):
    """LAST-WRITER: X written at i < j in one call by two names, and again in the next call; an 8-answer
    response that carries X twice; W written in call 1 and left alone in call 2."""
    x, w = key_of("198.51.100.7"), key_of("2001:db8:77::7")
    fill = [key_of("198.51.100.%d" % (20 + i)) for i in range(3)] + [key_of("2001:db8:77::%x" % (20 + i)) for i in range(3)]
    c1 = Call().query(1, "lw-a.example").query(2, "lw-b.example").response(1, [x]).query(3, "lw-a.example") \
        .response(2, [x]).response(3, [w])
    c2 = Call().query(4, "lw-b.example").query(5, "lw-a.example").response(5, [x]).no_question(9) \
        .response(4, [fill[0], x] + fill[1:] + [x])
    return Corpus("last-writer", mask, [c1, c2])


@functools.lru_cache(maxsize=None)
def crowd():
    """LAST-WRITER, many writers: 2048 responses to two alternating names all carry one address, across 64
    workgroups of the resolve kernel; the largest order is the last response's.  (Larger tables: the growth rule
    counts every answer.)"""
    c = Call()
    for i in range(2048):
        c.query(i, "crowd-%d.example" % (i % 2))
    for i in range(2048):
        c.response((i * 5) % 2048, ["203.0.113.9"])
    return Corpus("crowd", 0x1F, [c], name_capacity=4096, addr_capacity=4096)


@functools.lru_cache(maxsize=None)
def times():
    """TIMES: 64 frame times, not monotone; message i came from frame 3i + 1.  Call 1: id 1 queried twice (the
    later query's time stays), id 2 queried and answered (time cleared), ids 3..6 left pending.  Call 2 has no
    times: id 3 is queried again and loses its time.  Then the expiry around id 4's time t4: at t4 + 30 s - 1 it
    stays, at t4 + 30 s it goes, and id 6, whose time is ahead of both, stays; a last expiry before every time."""
    ts = np.array([T0 + ((k * 37) % 64) * S + k for k in range(64)], dtype=np.uint64)
    pkt = [3 * i + 1 for i in range(21)]
    c1 = Call(ts=ts, pkt=pkt[:9]).query(1, "t-a.example").query(2, "t-b.example").query(3, "t-a.example") \
        .query(1, "t-b.example").response(2, ["192.0.2.1"]).query(4, "t-a.example").query(5, "t-b.example") \
        .query(6, "t-a.example").reverse(5)
    c2 = Call().query(3, "t-b.example")
    t4 = int(ts[pkt[5]])
    return Corpus("times", 0x1F, [c1, c2, Expire(T0 - 1), Expire(t4 + 30 * S - 1), Expire(t4 + 30 * S),
                                  Expire(T0 + 10 ** 6 * S)])


GROW_ADDS = (12, 20, 40, 80, 160)
GROW_CAPS = [(16, 32), (64, 128), (128, 256), (256, 512), (512, 1024)]  # (12 names fit the first 16)


@functools.lru_cache(maxsize=None)
def grow():
    """GROW: from 16/16 under 0x1F, five calls add 12, 20, 40, 80 and 160 new names with one new IPv4 and one new
    IPv6 address each.  Every call also queries every old name again -- from other transaction ids, other garbage
    -- and answers the old addresses again, from the NEXT old name, so an old address changes its writer -- but
    the addresses of every fourth name (j % 4 == 3) are left alone: what the rebuild carried over for them is
    all there is (an address answered again in the growing call has its value rewritten right after it)."""
    steps, n_old = [], 0
    name = lambda j: "grow-%03d.example" % j  # noqa: E731
    pair = lambda j: ["172.16.%d.%d" % (j >> 8, j & 255), "2001:db8:9::%x" % j]  # noqa: E731
    for c, add in enumerate(GROW_ADDS):
        call = Call()
        for j in range(n_old + add):
            call.query(1000 * c + j, name(j), garbage=GARBAGE[(c + j) % 3])
        for j in range(n_old + add):
            if j >= n_old:
                call.response(1000 * c + j, pair(j))
            else:
                call.response(1000 * c + j, pair((j + 1) % n_old) if (j + 1) % n_old % 4 != 3 else [])
        steps.append(call)
        n_old += add
    return Corpus("grow", 0x1F, steps, grows=True)


# ID-RUNS
SYMBOLS = "abrx"  # query of name a, query of name b, response with one address, non-setter
RUN_NAMES = {"a": "run-a.example", "b": "run-b.example"}
RUN_ADDRS = 61
STRADDLE = {2: ("ar", 256, 255), 3: ("abr", 512, 510), 4: ("barr", 768, 766)}  # length: sequence, boundary, start
RUN_FIRST, RUN_LAST = "abrr", "rab"


def _setters(seq):
    return sum(ch != "x" for ch in seq)


@functools.lru_cache(maxsize=None)
def run_sequences():
    """The 340 sequences of length 1..4 in the order of their transaction ids -> [(id, sequence)].  The ids
    ascend, from 0 to 65535, and the order is arranged so that in the one-call variant's sorted order (setters by
    id, then by index) RUN_FIRST starts at position 0, RUN_LAST ends at the last setter position, and for each
    length L of STRADDLE that sequence starts where its run straddles the multiple of 256, a response sitting ON
    the multiple with its predecessor -- the message whose name it must take -- in the workgroup before."""
    seqs = ["".join(p) for L in range(1, 5) for p in itertools.product(SYMBOLS, repeat=L)]
    special = {RUN_FIRST, RUN_LAST} | {s for s, _, _ in STRADDLE.values()}
    pool = {c: [s for s in seqs if _setters(s) == c and s not in special] for c in range(5)}
    order, pos = [RUN_FIRST], _setters(RUN_FIRST)
    order += pool[0]  # (no setter: they take ids and no sorted position)
    pool[0] = []
    for L in sorted(STRADDLE):
        seq, _, start = STRADDLE[L]
        while pos < start:
            c = next(c for c in (4, 3, 2, 1) if c <= start - pos and pool[c])
            order.append(pool[c].pop(0))
            pos += c
        order.append(seq)
        pos += L
    for c in (4, 3, 2, 1):
        order += pool[c]
    order.append(RUN_LAST)
    assert sorted(order) == sorted(seqs) and len(order) == 340
    ids = [0] + [1 + 191 * k for k in range(1, 339)] + [65535]
    return list(zip(ids, order))


def _run_addr(s, p):
    k = (s * 4 + p) % RUN_ADDRS
    return "10.77.0.%d" % k if k % 2 == 0 else "2001:db8:77::%x" % k


def _run_call(lo, hi, n_dns=None):
    """Positions lo..hi-1 of every sequence, round-robin over the ids: all first messages, then all second ones,
    ..., so no id's run is contiguous in packet order."""
    c = Call(n_dns=n_dns)
    for p in range(lo, hi):
        for s, (tx, seq) in enumerate(run_sequences()):
            if p >= len(seq):
                continue
            ch = seq[p]
            if ch in RUN_NAMES:
                c.query(tx, RUN_NAMES[ch], garbage=GARBAGE[(s + p) % 3])
            elif ch == "r":
                c.response(tx, [_run_addr(s, p)])
            else:  # the non-setter rotates
                k = (s + p) % 4
                if k == 0:
                    c.reverse(tx)
                elif k == 1:
                    c.no_question(tx)
                else:
                    c.rejected(tx, query=k == 2, addrs=[] if k == 2 else ["10.77.9.9"])
    return c


@functools.lru_cache(maxsize=None)
def id_runs(cut=None, n_dns=None):
    """ID-RUNS as one call (cut None), or as two calls split after the first `cut` messages of every run.  Both
    capacities are 1024: there are two names and 61 addresses, but the growth rule counts every accepted query,
    626 of them, and the answer of every response, 313, matched or not."""
    steps = [_run_call(0, 4, n_dns)] if cut is None else [_run_call(0, cut), _run_call(cut, 4)]
    name = "id-runs" + ("" if cut is None else "-cut%d" % cut) + ("" if n_dns is None else "-ndns%d" % n_dns)
    return Corpus(name, M64, steps, name_capacity=1024, addr_capacity=1024)


def sorted_setters(call):
    """[(id, index)] of a call's setters in the order the sort leaves them."""
    msgs, _, _ = call.arrays()
    cnt = len(msgs) if call.n_dns is None else min(call.n_dns, len(msgs))
    out = []
    for i in range(cnt):
        f = int(msgs[i]["flags"])
        if int(msgs[i]["status"]) == 0 and (not f & N.DNS_QUERY or (f & N.DNS_HAS_QUESTION and not f & N.DNS_REVERSE)):
            out.append((int(msgs[i]["id"]), i))
    return sorted(out)


ID_RUN_NDNS = (500, 1252 - 128)  # inside the second messages; inside the fourth ones


@functools.lru_cache(maxsize=None)
def all_corpora():
    out = [id_runs()] + [id_runs(cut=c) for c in (1, 2, 3)] + [id_runs(n_dns=v) for v in ID_RUN_NDNS]
    out += [ladder(k) for k in range(1, 7)]
    out += [wrap(m) for m in MASKS] + [cluster(m) for m in MASKS]
    out += [last_writer(), crowd(), times(), grow()]
    return out


def corpus_keys():
    """Every name and address key of every corpus, ABSENT included (for the tag comparison)."""
    names, keys = set(), set()
    for c in all_corpora():
        for call in c.calls():
            names.update(r[2] for r in call.rows)
            keys.update(k for r in call.rows for k in r[3])
        keys.update(k for _, k in c.absent)
    return sorted(names), sorted(keys)


# ---- the census ---------------------------------------------------------------------------------------------
def census():
    """Recomputes every claim of the corpora from the restated tags and the restated classification, asserts
    it, and returns the counts of each case class."""
    out = {}
    # ID-RUNS: the sequences, the ids, the sorted positions
    seqs = run_sequences()
    assert len(seqs) == 340 and len({s for _, s in seqs}) == 340 and [t for t, _ in seqs] == sorted({t for t, _ in seqs})
    assert seqs[0] == (0, RUN_FIRST) and seqs[-1] == (65535, RUN_LAST)
    one = id_runs().steps[0]
    order = sorted_setters(one)
    by_tx = dict(seqs)
    assert len(one.rows) == 1252 and len(order) == sum(_setters(s) for _, s in seqs) == 939
    kinds = [r[1] for r in one.rows]
    is_resp = lambda i: not kinds[i] & N.DNS_QUERY  # noqa: E731
    starts = {}
    for p, (tx, _) in enumerate(order):
        starts.setdefault(tx, p)
    assert starts[0] == 0 and order[-1][0] == 65535 and starts[65535] == len(order) - _setters(RUN_LAST)
    for L, (seq, bound, start) in STRADDLE.items():
        tx = next(t for t, s in seqs if s == seq)
        assert starts[tx] == start and _setters(seq) == L and start < bound <= start + L - 1
        assert order[bound][0] == tx == order[bound - 1][0] and is_resp(order[bound][1])  # the read across the edge
    for tx, p in starts.items():  # no run is contiguous in packet order (runs of one message aside)
        idx = [i for t, i in order if t == tx]
        assert all(b - a > 1 for a, b in zip(idx, idx[1:])), by_tx[tx]
    out["id_runs"] = {"sequences": 340, "messages": 1252, "setters": 939,
                      "straddles": {L: v[2] for L, v in STRADDLE.items()}, "variants": 1 + 3 + len(ID_RUN_NDNS)}
    for cut in (1, 2, 3):
        c1, c2 = id_runs(cut=cut).steps
        assert len(c1.rows) + len(c2.rows) == 1252
    for v in ID_RUN_NDNS:  # the count cuts runs: some id has setters on both sides of it
        call = id_runs(n_dns=v).steps[0]
        kept = {t for t, _ in sorted_setters(call)}
        lost = {r[0] for r in call.rows[v:]}
        assert kept & lost
    # LADDER
    names, addrs = ladder_keys()
    assert len(set(names)) == 6 and len(set(addrs)) == 6 and {a[4] for a in addrs} == {2, 10}
    assert {bname_tag(nm, 0x1F) for nm in names} == {TAG_USED | LADDER_HOME} == {key_tag(a, 0x1F) for a in addrs}
    out["ladder"] = {"k": list(range(1, 7)), "home": LADDER_HOME, "rounds": {k: [c.rounds for c in ladder(k).steps] for k in range(1, 7)}}
    assert all(v == [k, k] for k, v in out["ladder"]["rounds"].items())
    # WRAP
    names, addrs = wrap_keys()
    for keys, tagf in ((names, bname_tag), (addrs, key_tag)):
        assert [home(tagf(k, 0xFF)) for k in keys] == [h for h, c in WRAP_HOMES for _ in range(c)]
        for m in MASKS:
            assert sorted(occupied(keys, tagf, m).values()) == [0, 1, 2, 3, 4, 29, 30, 31]
        assert len({tagf(k, 0xFF) for k in keys}) > len({tagf(k, 0x1F) for k in keys}) == 3
    out["wrap"] = {"keys": 8, "homes": [h for h, _ in WRAP_HOMES], "slots": [29, 30, 31, 0, 1, 2, 3, 4]}
    # CLUSTER
    names, addrs, pairs = cluster_keys()
    for keys, tagf in ((names, bname_tag), (addrs, key_tag)):
        assert len(set(keys)) == 10
        assert [home(tagf(k, 0xFF)) for k in keys] == [h for h, c in CLUSTER_HOMES for _ in range(c)]
        for m in MASKS:
            assert sorted(occupied(keys, tagf, m).values()) == list(range(9, 19))
        # under 0xFF a later key walks past slots of other tags: more tags than homes, fewer than keys
        assert 3 < len({tagf(k, 0xFF) for k in keys}) < 10
    a, b = pairs["prefix"]
    assert b[:len(a)] == a and len(b) == len(a) + 1
    a, b = pairs["last_byte"]
    assert len(a) == len(b) and a[:-1] == b[:-1] and a[-1] != b[-1]
    a, b = pairs["partial_dword"]
    assert len(a) == len(b) and len(a) % 4 == 3 and a[:-3] == b[:-3] and a[-3] != b[-3] and a[-2:] == b[-2:]
    for k in ("prefix", "last_byte", "partial_dword"):
        assert bname_tag(pairs[k][0], 0xFF) == bname_tag(pairs[k][1], 0xFF) and pairs[k][0] in names and pairs[k][1] in names
    a, b = pairs["v4_v6_word0"]
    assert a[0] == b[0] and (a[4], b[4]) == (2, 10)
    a, b = pairs["v6_word3"]
    assert a[:3] == b[:3] and a[3] != b[3] and a[4] == b[4] == 10
    a, b = pairs["v6_word0"]
    assert a[1:] == b[1:] and a[0] != b[0] and a[4] == 10
    for k in ("v4_v6_word0", "v6_word3", "v6_word0"):
        assert key_tag(pairs[k][0], 0xFF) == key_tag(pairs[k][1], 0xFF) and pairs[k][0] in addrs and pairs[k][1] in addrs
    garbage = {(r[2], r[5]) for c in cluster(0x1F).calls() for r in c.rows if r[1] & N.DNS_QUERY}
    assert garbage == {(nm, g) for nm in names for g in GARBAGE}
    out["cluster"] = {"keys": 10, "homes": [h for h, _ in CLUSTER_HOMES], "slots": list(range(9, 19)), "pairs": sorted(pairs)}
    # ABSENT
    out["absent"] = {}
    for corp, present in [(wrap(m), wrap_keys()[1]) for m in MASKS] + [(cluster(m), cluster_keys()[1]) for m in MASKS]:
        slots = set(occupied(present, key_tag, corp.mask).values())
        claims = dict(corp.absent)
        assert len(claims) == 10 and not set(claims.values()) & set(present)
        homes = {c: home(key_tag(k, corp.mask)) for c, k in claims.items()}
        for fam, v in (("v4", 2), ("v6", 10)):
            assert claims["first-" + fam][4] == v
            first, last = homes["first-" + fam], homes["last-" + fam]
            assert first in slots and (first - 1) % SLOTS not in slots and last in slots and (last + 1) % SLOTS not in slots
            assert homes["behind-" + fam] == (last + 1) % SLOTS and homes["slot31-" + fam] == 31
            assert homes["middle-" + fam] in slots and homes["middle-" + fam] not in (first, last)
            if corp.mask == 0x1F:  # an equal tag: the lookup has to compare the key, and differ
                assert key_tag(claims["first-" + fam], 0x1F) in {key_tag(k, 0x1F) for k in present}
        out["absent"][corp.name] = homes
    # LAST-WRITER, TIMES, GROW: what the restatement says of them
    model = check_bounds(last_writer())
    x, w = key_of("198.51.100.7"), key_of("2001:db8:77::7")
    assert model.res[x] == (model.ids[b"lw-b.example"], 6 + 4) and model.res[w] == (model.ids[b"lw-a.example"], 5)
    m1 = Tracker()
    m1.track(*last_writer().steps[0].arrays())
    assert m1.res[x] == (m1.ids[b"lw-b.example"], 4)  # written at 2 and at 4 in call 1
    assert sum(k == x for k in last_writer().steps[1].rows[4][3]) == 2 and len(last_writer().steps[1].rows[4][3]) == 8
    model = check_bounds(crowd())
    assert model.res[key_of("203.0.113.9")] == (model.ids[b"crowd-%d.example" % ((2047 * 5) % 2048 % 2)], 4095)
    out["last_writer"] = {"one_call": 1, "two_calls": 1, "twice_in_one_response": 1, "left_alone": 1, "crowd": 2048}
    t = times()
    model = Tracker()
    ts, c1 = t.steps[0].ts, t.steps[0]
    model.track(*c1.arrays(), ts=ts)
    assert int(model.pend_time[1]) == int(ts[10]) != int(ts[1]) and int(model.pend_time[2]) == NO_TIME
    assert not (np.diff(ts.astype(np.int64)) > 0).all() and [int(x) for x in c1.arrays()[0]["pkt_index"]] == c1.pkt
    t4, t6 = int(model.pend_time[4]), int(model.pend_time[6])
    model.track(*t.steps[1].arrays())
    assert int(model.pend_time[3]) == NO_TIME and int(model.pend_name[3]) == model.ids[b"t-b.example"]
    assert model.expire(t.steps[2].now) == 0
    before = model.expire(t.steps[3].now)
    assert int(model.pend_name[4]) and t.steps[3].now == t4 + 30 * S - 1 < t6
    assert model.expire(t.steps[4].now) == 1 and not int(model.pend_name[4]) and int(model.pend_name[6])
    assert model.expire(t.steps[5].now) >= 1 and model.pending_strings() == {3: "t-b.example"}
    out["times"] = {"dropped": [0, before, 1]}
    g = grow()
    model, caps, held = Tracker(), [], 0
    for call, add in zip(g.steps, GROW_ADDS):
        msgs = call.arrays()
        assert model.would_grow(msgs[0])
        r = model.track(*msgs)
        held += add
        assert r["names_new"] == add and r["addrs_new"] == 2 * add and r["queries"] == held
        caps.append((model.name_cap, model.addr_cap))
    assert caps == GROW_CAPS, caps
    out["grow"] = {"adds": list(GROW_ADDS), "capacities": caps}
    out["corpora"] = len(all_corpora())
    return out
