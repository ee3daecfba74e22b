"""Corpora for the device-side domain matching of the whitelist check (fb_set_whitelist_dom, fb_wl_name_matches_dev,
fb_flow_whitelist) and what each name and each flow must come out as.

The expectation is the literal scan of flodbadd_amd/whitelists.py -- domain_matches / endpoint_matches, which never
look at an index -- called with the name or the flow's domain STRING; the device sees name ids and pattern ids only.
What the device leaves to the host is restated as a literal scan too (expected()): an endpoint whose pattern has no
id never matches by domain and asks for the host, and a name that matches more than FB_WL_NAME_MATCHES patterns is
decided by the least ones alone and asks for the host.

  exhaustive_names / _patterns   every name over {a,b,.,*} up to 5 bytes, every pattern over {a,.,*} up to 4
  dot_candidate_matches          the four "dot-candidate" forms the device evaluates, restated in Python
  name_cases()                   (label, pattern list) per corpus; NAMES the names they are matched against
  expected_rows()                the row and the flags byte of every name under a pattern list
  flow_cases() / expected()      endpoint lists over the flows of a World, and every flow's state byte
  write_corpus()                 names and patterns for tests/wl_domain_host.cpp
"""
import collections
import functools
import itertools
import struct

import numpy as np

import wlprocspace as P
from flodbadd_amd import _native as N
from flodbadd_amd.whitelists import WhitelistEndpoint, Whitelists, classify_domain_pattern, domain_matches, endpoint_matches

ROW = N.FB_WL_NAME_MATCHES
KINDS = ("exact", "suffix", "prefix", "general", "never")
MASKS = (0, 0xF, 1 << 63)  # FB_DEBUG_WL_NAME_HASH_MASK: all bits, four bits, the top bit alone


# ---- the space the matching forms were settled on -------------------------------------------------------------
def _strings(alphabet, upto):
    return ["".join(t) for n in range(upto + 1) for t in itertools.product(alphabet, repeat=n)]


@functools.lru_cache(maxsize=None)
def exhaustive_names():
    return tuple(_strings("ab.*", 5))  # 1,365, the empty name first


@functools.lru_cache(maxsize=None)
def exhaustive_patterns():
    return tuple(_strings("a.*", 4))  # 121, the empty pattern first


def dot_candidate_matches(n, p):
    """domain_matches as the device evaluates it: the pattern's kind, then equality of a whole name, of what
    follows a dot or of what precedes one -- or the two ends of an a*b pattern.  n and p lower-cased."""
    kind = classify_domain_pattern(p)
    dots = [i for i, c in enumerate(n) if c == "."]
    if kind == "exact":
        return n == p
    if kind == "suffix":
        return any(n[i + 1:] == p[2:] for i in dots)
    if kind == "prefix":
        return n == p[:-2] or any(n[:i] == p[:-2] for i in dots)
    if kind == "general":
        a, b = p.split("*")
        return n.startswith(a) and n.endswith(b) and len(n) > len(a) + len(b)
    return False


# ---- names ------------------------------------------------------------------------------------------------------
def _label_name(length, dots=()):
    """A name of `length` bytes, letters except for dots at the given positions."""
    s = [chr(ord("a") + (i * 7) % 26) for i in range(length)]
    for d in dots:
        s[d] = "."
    return "".join(s)


def geometry_names():
    out = [_label_name(n) for n in (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 252, 253, 254, 255)]
    out += [_label_name(n, (n // 2,)) for n in (3, 4, 5, 63, 64, 65, 127, 128, 129, 252, 253, 254, 255)]
    out += [_label_name(70, (0,)), _label_name(70, (69,)), _label_name(255, (0, 254)), _label_name(255, (254,))]
    # dots on dword and lane edges (bytes 3 | 4, 63 | 64, 127 | 128, 251 | 252), and doubled
    out += [_label_name(255, (d,)) for d in (3, 4, 63, 64, 127, 128, 191, 192, 251, 252)]
    out += [_label_name(200, (63, 64)), _label_name(200, (64, 65)), _label_name(9, (4, 5)), "a..b", "..", "."]
    out += [".".join("x" * 1 for _ in range(127)),  # 127 labels, 253 bytes, 126 dots: more than a wavefront's lanes
            ".".join(["y"] * 100 + ["zz"])]
    out += ["WWW.Example.COM", "www.example.com", "API.example.org", "a*b.example.com", "*.example.com", "x*"]
    return out


EDGE_NAMES = ["example.com", "a.example.com", "com", "x.com", "example", "example.org", "example.co.uk", "examples.com",
              "www.example.org", "aba", "abba", "abxba", "ab", "a.x.b", "a..b", "a.b", "x.a.y", "x.a.*", "a.", ".a", "a", "cafe.fr", "k.com"]
EDGE_PATTERNS = ["example.com", "*.example.com", "*.com", "example.*", "example.com.*", "ab*ba", "*", "*.", ".*", "**", "*.*",
                 "a.*.b", "*.a.*", "café.fr", "*.café.fr", "K.com", "a", "*a", "a*", "a.x.b", "*.x.b", "a.x.*"]


def _numbered(kind, j):
    """Pattern j of a table of one kind, and a name only it (of its table) matches."""
    return {"exact": ("h%03d.ex" % j, "h%03d.ex" % j), "suffix": ("*.s%03d.ex" % j, "x.s%03d.ex" % j),
            "prefix": ("p%03d.*" % j, "p%03d.com" % j), "general": ("g%03d*z" % j, "g%03d-z" % j)}[kind]


TABLE_SIZES = (0, 1, 2, 255, 256, 257)
# m.o.example.com matches nine of these (ids 2 .. 10), and exactly the eight of OVERFLOW_PATTERNS[2:10]
OVERFLOW_PATTERNS = ["zz.nope", "m.o.example.com", "*.o.example.com", "*.example.com", "*.com", "m.*", "m.o.*", "m.o.example.*",
                     "m*m", "m.o*.com", "*.example.org"]
OVERFLOW_NAMES = ["m.o.example.co", "m.o.example.com", "m.o.example.org"]


def name_cases():
    """(label, patterns): every pattern list the name-match kernel is run under."""
    pats = exhaustive_patterns()
    out = [("exhaustive_%02d" % k, list(pats[k:k + ROW])) for k in range(0, len(pats), ROW)]  # rows cannot overflow
    geo = []
    for n in geometry_names():
        low = n.lower()
        dots = [i for i, c in enumerate(low) if c == "."]
        geo.append(low)
        for i in (dots[:1] + dots[-1:]):
            geo += ["*." + low[i + 1:], low[:i] + ".*"]
        if len(low) >= 3:
            geo.append(low[0] + "*" + low[-1])
    out.append(("geometry", list(dict.fromkeys(geo))))
    out.append(("edges", list(EDGE_PATTERNS)))
    for kind in KINDS[:4]:
        for size in TABLE_SIZES:
            out.append(("table_%s_%d" % (kind, size), [_numbered(kind, j)[0] for j in range(size)]))
    out.append(("overflow", list(OVERFLOW_PATTERNS)))
    out.append(("overflow_8", OVERFLOW_PATTERNS[2:10] + ["zz.nope"]))
    out.append(("duplicates", ["*.com"] * 12 + ["x.com"]))  # one string under many ids: the C ABI allows it
    return out


@functools.lru_cache(maxsize=None)
def all_names():
    """Every name of the corpora, the order the tracker meets them in (the empty name is the host program's alone)."""
    names = [n for n in exhaustive_names() if n] + geometry_names() + EDGE_NAMES + OVERFLOW_NAMES
    names += [_numbered(kind, j)[1] for kind in KINDS[:4] for j in range(max(TABLE_SIZES))]
    return tuple(dict.fromkeys(names))


def case_names(label):
    """The names a case is checked with on the CPU (the device matches every stored name under every list)."""
    if label.startswith("exhaustive"):
        return list(exhaustive_names())
    if label.startswith("table_"):
        kind = label.split("_")[1]
        return [_numbered(kind, j)[1] for j in range(max(TABLE_SIZES))] + EDGE_NAMES
    return geometry_names() + EDGE_NAMES + OVERFLOW_NAMES + [""]


def expected_row(name, patterns):
    """(row, flags) of one name: the 1-based ids of the patterns domain_matches accepts, the least ROW of them
    ascending and zero-padded; flags bit 0: there were more."""
    hits = [k + 1 for k, p in enumerate(patterns) if domain_matches(name, p)]
    return hits[:ROW] + [0] * (ROW - len(hits[:ROW])), 1 if len(hits) > ROW else 0


def expected_rows(names, patterns):
    rows = [expected_row(n, patterns) for n in names]
    return np.array([r for r, _ in rows], dtype=np.uint32).reshape(len(names), ROW), np.array([f for _, f in rows], dtype=np.uint8)


def pattern_arrays(patterns):
    """pattern_bytes / pattern_off of fb_set_whitelist_dom: the lower-cased patterns' UTF-8 bytes."""
    blobs = [p.lower().encode("utf-8") for p in patterns]
    return (np.frombuffer(b"".join(blobs), dtype=np.uint8).copy(),
            np.cumsum([0] + [len(b) for b in blobs], dtype=np.uint64))


def write_corpus(path, names, patterns):
    """The input of tests/wl_domain_host.cpp: u64 n_patterns, n_names; pattern_off[n_patterns + 1] (u64); the
    pattern bytes; per name u32 length and FB_DNS_MAX_NAME bytes (the name as stored: its own case, zero-filled)."""
    blob, off = pattern_arrays(patterns)
    parts = [struct.pack("<2Q", len(patterns), len(names)), off.tobytes(), blob.tobytes()]
    for n in names:
        b = n.encode("latin-1")
        assert len(b) <= N.FB_DNS_MAX_NAME
        parts.append(struct.pack("<I", len(b)) + b + bytes(N.FB_DNS_MAX_NAME - len(b)))
    with open(path, "wb") as fh:
        fh.write(b"".join(parts))


# ---- flows ------------------------------------------------------------------------------------------------------
# destination -> the name it resolves to (None: no resolution, name id 0)
A4, B4, A6, B6 = P.A4, P.B4, P.A6, P.B6
DOMAINS = collections.OrderedDict([(A4, "WWW.Example.com"), (B4, "api.other.org"), (A6, "m.o.example.com"), (B6, None)])
LATE_DST = "93.184.216.35"  # resolves too, but its flows are inserted after the last domain pass: no domain
LATE_NAME = "late.example.com"


def world():
    """wlprocspace's semantic flows -- every process state x {hit candidates, near misses} -- whose destinations
    resolve as DOMAINS says, and per process state one flow the domain pass never saw."""
    return P.World("domains", P.semantic_flows())


def late_flows():
    return [P.Flow(P.TCP, "192.168.77.%d" % (k + 1), 62000 + k, LATE_DST, 443, "unresolved") for k in range(3)]


class Case:
    """One endpoint list.  no_id: the endpoints the device gets no process id for; no_pat: those it gets no pattern
    id for."""

    def __init__(self, name, endpoints, no_id=(), no_pat=(), label=None):
        self.name, self.endpoints, self.no_id, self.no_pat, self.label = name, list(endpoints), set(no_id), set(no_pat), label

    def compile(self, interner):
        m = {"date": "", "signature": None,
             "whitelists": [{"name": "custom_whitelist", "extends": None, "endpoints": self.endpoints}]}
        comp = Whitelists(m).compile("custom_whitelist", P.ASN_RECORDS, process_ids=interner, domain_patterns=True)
        for k in self.no_id:
            comp.rows[k]["reserved2"] = 0
        for k in self.no_pat:
            comp.ep_pattern[k] = 0
        return comp

    def pattern_ids(self):
        """The 1-based pattern id of every endpoint as Whitelists.compile numbers them (first appearance of the
        lower-cased string), 0 without a domain or in no_pat."""
        ids, out = {}, []
        for k, e in enumerate(self.endpoints):
            d = e.get("domain")
            if d is not None:
                ids.setdefault(d.lower(), len(ids) + 1)
            out.append(0 if (d is None or k in self.no_pat) else ids[d.lower()])
        return out, list(ids)


def _key_matches(ep, f):
    return (ep.get("protocol") is None or ep["protocol"].lower() == f.proto.lower()) and \
        (ep.get("port") is None or ep["port"] == f.dport)


def expected(flows, domains, wld, case, n_names):
    """(state bytes, dom_overflow) of `flows` (domains[f]: the flow's dst_domain string or None) under `case` with
    a process-name table of n_names entries (0: none)."""
    installed = n_names > 0
    pids, patterns = case.pattern_ids()
    out, over_n = [], 0
    for f in flows:
        dom = domains.get(f)
        row, flag = expected_row(dom, patterns) if dom is not None else ([0] * ROW, 0)
        rec = P.asn_of(f.dst)
        a = P.ASN_RECORDS[rec] if rec is not None else (None, None, None)
        proc = wld.process(f, n_names)
        ok = hc = over = False
        for k, e in enumerate(case.endpoints):
            ep = WhitelistEndpoint.from_dict(e)
            over |= bool(flag) and pids[k] != 0 and _key_matches(e, f)  # the row is not all the name matches
            if ep.process is not None and (k in case.no_id or not installed):
                hc |= _key_matches(e, f)  # the device cannot compare the process
                continue
            if ep.domain is not None and pids[k] == 0:
                hc |= _key_matches(e, f)  # ... nor the domain: the endpoint without it (never by domain)
                ok |= ep.ip is not None and endpoint_matches(ep, None, f.dst, f.dport, f.proto, a[0], a[1], a[2], proc)[0]
                continue
            if ep.domain is not None:  # decided by the ids the row holds
                d = dom if pids[k] in row else None
                ok |= endpoint_matches(ep, d, f.dst, f.dport, f.proto, a[0], a[1], a[2], proc)[0]
                continue
            ok |= endpoint_matches(ep, dom, f.dst, f.dport, f.proto, a[0], a[1], a[2], proc)[0]
        b = P.CONFORMING if ok else P.NONCONFORMING | (P.HOST_CHECK if (hc or over) else 0)
        over_n += (not ok) and over
        out.append(b)
    return out, over_n


SHAPES = collections.OrderedDict([("domain_only", {}), ("domain_ip", {"ip": A4}), ("domain_other_ip", {"ip": B4})])
# the pattern -> which of DOMAINS' names it matches
PATTERNS = collections.OrderedDict([
    ("exact", "www.example.com"), ("exact_case", "WWW.EXAMPLE.COM"), ("suffix", "*.example.com"), ("prefix", "www.*"),
    ("general", "w*m"), ("miss", "*.example.net"), ("never", "w**m")])
EP_PROCS = collections.OrderedDict([("none", (None, True)), ("same", ("curl", True)), ("another", ("nginx", True)),
                                    ("id0", ("curl", False))])


def semantic():
    out = []
    for sn, shape in SHAPES.items():
        for kn, key in P.KEY_FORMS.items():
            for pn, pat in PATTERNS.items():
                for en, (proc, has_id) in EP_PROCS.items():
                    if en != "none" and kn not in ("any", "proto_port"):
                        continue
                    for no_pat in ((), (0,)) if (pn == "suffix" and en in ("none", "same")) else ((),):
                        ep = dict(shape, domain=pat, **key)
                        if proc is not None:
                            ep["process"] = proc
                        out.append(Case("%s/%s/%s/%s%s" % (sn, kn, pn, en, "/nopat" if no_pat else ""), [ep],
                                        () if has_id else (0,), no_pat, (sn, kn, pn, en, bool(no_pat))))
    return out


RUN_SIZES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257)


def runs():
    """One pattern's run of the domain table holding n (key, process) entries: decoys under ports no flow has, then
    the entry that decides at the run's start (port None sorts first), inside it, or at its end (UDP 65535)."""
    out = []
    for n in RUN_SIZES:
        for where in ("none", "first", "inside", "last"):
            eps = [{"domain": "*.example.com", "protocol": "TCP", "port": 1000 + j} for j in range(n if where == "none" else max(n - 1, 0))]
            if where != "none" and n:
                eps.append({"first": {"domain": "*.example.com"}, "inside": {"domain": "*.example.com", "protocol": "TCP", "port": 443},
                            "last": {"domain": "*.example.com", "protocol": "UDP", "port": 443, "process": "curl"}}[where])
            elif where != "none":
                continue
            out.append(Case("run_%d_%s" % (n, where), eps))
    return out


def overflows():
    """A6's name matches 9 of OVERFLOW_PATTERNS; B-side names match fewer.  The endpoint of the greatest matched id
    alone has the flows' key: the device cannot see it -- NonConforming, host check, counted --; with the first
    pattern removed the name matches exactly 8 and the same endpoint decides on the device."""
    def eps(pats):
        return [{"domain": p, "protocol": "UDP", "port": 9} for p in pats[:-2]] + \
               [{"domain": pats[-2], "protocol": "TCP", "port": 443}, {"domain": pats[-1], "port": 1}]
    nine = OVERFLOW_PATTERNS[1:10] + ["*.example.org"]
    return [Case("overflow_9", eps(nine)), Case("overflow_8", eps(nine[1:])),
            Case("overflow_9_other_key", [{"domain": p, "protocol": "UDP", "port": 9} for p in nine])]


def mixed():
    """Domain endpoints beside every other route of the index: an address, a net, an AS rule, a process rule."""
    return [Case("mixed", [{"domain": "*.other.org", "port": 443}, {"ip": A6, "protocol": "TCP", "port": 443},
                           {"ip": "93.184.0.0/16", "port": 80}, {"as_number": 64500, "protocol": "UDP"},
                           {"domain": "late.example.com"}, {"domain": "*.example.com", "process": "sshd", "port": 443}]),
            Case("no_domain_endpoints", [{"ip": A4, "port": 443}]), Case("empty", [])]


def flow_cases():
    return semantic() + runs() + overflows() + mixed()


def counters(states, prev=None):
    return P.counters(states, prev)


# ---- putting names and patterns on the device (the GPU tests) -----------------------------------------------
def track(cap, call):
    msgs, names, addrs = call.arrays()
    d_msg = N.DeviceBuffer(max(msgs.nbytes, 16)).upload(msgs)
    d_names = N.DeviceBuffer(max(names.nbytes, 16)).upload(names)
    d_addrs = N.DeviceBuffer(max(addrs.nbytes, 32)).upload(addrs)
    return cap.track_dns_parsed_dev(d_msg, d_names, d_addrs, len(msgs))


def track_names(cap, names, tx0=1):
    """One query per name, 500 a call."""
    for k in range(0, len(names), 500):
        import dnstrackspace as T
        call = T.Call()
        for j, n in enumerate(names[k:k + 500]):
            call.query(tx0 + k + j, n.encode("latin-1"))
        track(cap, call)


def stored_names(cap):
    """{id: the stored string} of every name of the tracker."""
    n = cap.dns_track_info()["names"]
    return cap.dns_names(range(1, n + 1))


def install_patterns(cap, patterns):
    """A list of no endpoints with the given patterns."""
    blob, off = pattern_arrays(patterns)
    N.check(N.gpu_lib().fb_set_whitelist_dom(cap.ctx, None, 0, None, N.ptr(blob) if len(blob) else None, N.ptr(off),
                                             len(patterns), None, None, 0))
