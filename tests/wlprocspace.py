"""Corpora for the process-aware whitelist check (fb_set_l7_process_names, fb_flow_whitelist)
and what each flow must come out as.

The expectation is `is_session_in_whitelist` of flodbadd_amd/whitelists.py -- the literal scan over the endpoint
list that never looks at an index -- called with the flow's process STRING; the device sees ids only.  The
FB_WL_HOST_CHECK bit is restated as a literal scan too (host_check below).  What the device cannot decide stays as
include/flodbadd_gpu.h states it: a domain never matches, and an endpoint whose process the device has no id
for (process_match_id 0), or any process endpoint while no name table is installed, never matches either.

  World      the flows of a table with their processes, the process names and the ASN table
  Case       one endpoint list over a World, with the endpoints the device has no process id for
  semantic() endpoint shape x key form x endpoint process, one list each, over flows of every process state
  runs()     one address's run of the exact index holding 0-9 and 255-257 (key, process) entries
  staging()  lists at the staging thresholds: 512 / 513 groups and rules
  expected() the state byte of every flow;  write_corpus() the same inputs for tests/wl_match_host.cpp
"""
import collections
import ipaddress
import struct

import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.l7 import ProcessNameInterner
from flodbadd_amd.sessions import ip_to_words, is_lan_ip
from flodbadd_amd.whitelists import Whitelists, WhitelistEndpoint, is_session_in_whitelist

TCP, UDP = "TCP", "UDP"
CONFORMING, NONCONFORMING, HOST_CHECK = 1, 2, 4

# process id -> name (id 0: none).  1 and 2 share a name, 3 has it in other case; the name table of the
# corpora has N_NAMES entries, so id N_NAMES - 1 is the last it names and id N_NAMES is beyond it.
PROCS = [None, "curl", "curl", "CURL", "nginx", "sshd"]
N_NAMES = 5
# the process state of a flow -> (how the L7 plane gets it, its process id)
FLOW_PROCS = collections.OrderedDict([
    ("unresolved", ("late", 0)),     # inserted after the L7 pass: a zero element
    ("failed", ("nosock", 0)),       # looked up, no socket: FB_L7_FAILED with max_retries 0
    ("resolved", ("sock", 1)),
    ("second_id", ("sock", 2)),      # another process id of the same name
    ("other_case", ("sock", 3)),     # the same name in other case
    ("last_id", ("sock", N_NAMES - 1)),
    ("beyond", ("sock", N_NAMES)),   # an id the table does not name: no process
])
A4, B4, A6, B6 = "93.184.216.34", "8.8.8.8", "2001:db8::1", "3001:db8::1"
# the ASN table: 93.0.0.0/8 alone -> AS 64500, record 0
ASN_RECORDS = [(64500, "US", "Alpha Net")]
ASN_V4 = [(93 << 24, (93 << 24) | 0xFFFFFF, 0)]

Flow = collections.namedtuple("Flow", "proto src sport dst dport state")  # state: a FLOW_PROCS key


def asn_of(dst):
    """SessionInfo.dst_asn over ASN_V4: the record index or None (a LAN destination has none)."""
    ip = ipaddress.ip_address(dst)
    if ip.version != 4 or is_lan_ip(ip, ()):
        return None
    return next((r for s, e, r in ASN_V4 if s <= int(ip) <= e), None)


class World:
    """flows: the table's flows.  plane: whether an L7 pass has run (False: every flow is without a process)."""

    def __init__(self, name, flows, plane=True):
        self.name, self.flows, self.plane = name, list(flows), plane

    def process_id(self, f):
        return FLOW_PROCS[f.state][1] if self.plane else 0

    def process(self, f, n_names):
        """The flow's process name as the device defines it: x names one when x != 0 and x < n."""
        x = self.process_id(f)
        return PROCS[x] if (x != 0 and x < n_names) else None


def semantic_flows():
    """Per process state: a hit candidate of every address shape, and a near miss in address, port and protocol."""
    out = []
    for c, state in enumerate(FLOW_PROCS):
        for k, (proto, dst, dport) in enumerate([(TCP, A4, 443), (TCP, A4, 80), (UDP, A4, 443), (TCP, B4, 443),
                                                 (TCP, A6, 443), (TCP, B6, 443)]):
            v6 = ":" in dst
            src = "fd00::%x:%x" % (c + 1, k + 1) if v6 else "192.168.%d.%d" % (c + 1, k + 1)
            out.append(Flow(proto, src, 61000 + 16 * c + k, dst, dport, state))
    return out


SHAPES = collections.OrderedDict([
    ("exact_v4", {"ip": A4}), ("exact_v6", {"ip": A6}), ("net", {"ip": "93.184.0.0/16"}),
    ("as_only", {"as_number": 64500}), ("nothing", {}),
    ("domain_ip", {"domain": "x.example.com", "ip": A4}), ("domain_only", {"domain": "x.example.com"}),
])
KEY_FORMS = collections.OrderedDict([("any", {}), ("port", {"port": 443}), ("proto", {"protocol": "tcp"}),
                                     ("proto_port", {"protocol": "TCP", "port": 443})])
# the endpoint's process -> (the string, whether the device gets an id for it)
EP_PROCS = collections.OrderedDict([
    ("none", (None, True)), ("same", ("curl", True)), ("same_other_case", ("CuRl", True)),
    ("another", ("nginx", True)), ("nobody", ("ghost", True)), ("id0", ("curl", False)),
])


class Case:
    def __init__(self, name, endpoints, no_id=(), label=None):
        self.name, self.endpoints, self.no_id, self.label = name, list(endpoints), set(no_id), label

    def model(self):
        return {"date": "", "signature": None,
                "whitelists": [{"name": "custom_whitelist", "extends": None, "endpoints": self.endpoints}]}

    def compile(self, interner, zero_ids=False):
        """The fb_wl_endpoint rows (Whitelists.compile with process ids), the no_id endpoints' ids zeroed."""
        comp = Whitelists(self.model()).compile("custom_whitelist", ASN_RECORDS, process_ids=interner)
        rows = comp.rows.copy()
        for k in range(len(rows)):
            if zero_ids or k in self.no_id:
                rows[k]["reserved2"] = 0
        return comp, rows


def semantic():
    out = []
    for sn, shape in SHAPES.items():
        for kn, key in KEY_FORMS.items():
            for pn, (proc, has_id) in EP_PROCS.items():
                ep = dict(shape, **key)
                if proc is not None:
                    ep["process"] = proc
                out.append(Case("%s/%s/%s" % (sn, kn, pn), [ep], () if has_id else (0,), (sn, kn, pn)))
    return out


def rule_allows_conforming(shape, ep_proc, flow_state, names_installed=True):
    """Hand-written: can a flow of this process state conform to an endpoint of this class at all?"""
    if shape == "domain_only":
        return False
    if ep_proc == "none":
        return True
    if not names_installed or ep_proc in ("nobody", "id0"):
        return False
    return flow_state in {"same": ("resolved", "second_id", "other_case"),
                          "same_other_case": ("resolved", "second_id", "other_case"),
                          "another": ("last_id",)}[ep_proc]


RUN_SIZES = list(range(10)) + [255, 256, 257]
RUN_PROCS = ("curl", "nginx", None)


def run_entry(j):
    """Entry j of a run at A4: (key, process) pairs that ascend with j -- three processes per port."""
    ep = {"ip": A4, "protocol": "TCP", "port": 2000 + 2 * (j // 3)}
    if RUN_PROCS[j % 3] is not None:
        ep["process"] = RUN_PROCS[j % 3]
    return ep


def run_flows():
    """Flows at A4 around the first and the last key of every run size (hit first, hit last, absent below,
    between and above), each as a curl, an nginx and a process-less flow."""
    ports = sorted({1999, 2000, 2001} | {2000 + 2 * ((k - 1) // 3) + d for k in RUN_SIZES if k for d in (-1, 0, 1, 2)})
    out = []
    for c, state in enumerate(("resolved", "last_id", "unresolved")):
        for k, p in enumerate(ports):
            out.append(Flow(TCP, "192.168.%d.%d" % (40 + c, k + 1), 61000 + k, A4, p, state))
    return out


def runs():
    # (the entries come in descending order: the index has to sort them)
    return [Case("run_%d" % k, [run_entry(j) for j in reversed(range(k))]) for k in RUN_SIZES]


def staging():
    """(groups, rules) at and past kWlLdsGroups / kWlLdsRules: decoy nets under UDP ports no flow has (one group
    and one rule each), decoy domain-only endpoints (a group without a rule), and the live endpoints of three
    groups -- a net for curl, a net for anyone at another port, a match-all for nginx -- among them."""
    live = [{"ip": "93.184.0.0/16", "protocol": "TCP", "port": 443, "process": "curl"},
            {"ip": "93.184.0.0/16", "protocol": "TCP", "port": 80},
            {"protocol": "UDP", "port": 443, "process": "NGINX"}]
    out = []
    for groups, rules in ((N.WL_LDS_GROUPS, N.WL_LDS_RULES), (N.WL_LDS_GROUPS + 1, N.WL_LDS_RULES + 1),
                          (N.WL_LDS_GROUPS, N.WL_LDS_RULES + 1), (N.WL_LDS_GROUPS + 1, N.WL_LDS_RULES)):
        eps = list(live)
        n_groups, n_rules = 3, 3
        while n_groups < groups and n_rules < rules:   # one group, one rule
            eps.append({"ip": "10.0.0.0/8", "protocol": "UDP", "port": 10000 + n_groups})
            n_groups, n_rules = n_groups + 1, n_rules + 1
        while n_rules < rules:                          # a rule in an existing group
            eps.append({"ip": "10.%d.0.0/16" % (n_rules % 200), "protocol": "UDP", "port": 10003})
            n_rules += 1
        while n_groups < groups:                        # a group without a rule
            eps.append({"domain": "d%d.example.com" % n_groups, "protocol": "UDP", "port": 20000 + n_groups})
            n_groups += 1
        eps = eps[3:] + eps[:3]
        out.append(Case("staging_%dg_%dr" % (groups, rules), eps, label=(groups, rules)))
    return out


def host_check(endpoints, no_id, names_installed, port, protocol):
    """The FB_WL_HOST_CHECK condition as a literal scan: some endpoint the device cannot decide -- one with a
    domain, or with a process it has no id for, or with any process while no name table is installed -- has
    the flow's protocol and port."""
    for k, ep in enumerate(endpoints):
        left = ep.get("domain") is not None or (ep.get("process") is not None and (k in no_id or not names_installed))
        if left and (ep.get("protocol") is None or ep["protocol"].lower() == protocol.lower()) and \
                (ep.get("port") is None or ep["port"] == port):
            return True
    return False


def expected(world, case, n_names, zero_ids=False):
    """The state byte of every flow of `world` under `case` with a name table of n_names entries (0: none
    installed).  zero_ids: every endpoint's process id is zeroed (the list as it was compiled before the device
    knew processes)."""
    no_id = set(range(len(case.endpoints))) if zero_ids else case.no_id
    installed = n_names > 0
    # the endpoints the device can match: not those whose process it cannot compare
    eps = [WhitelistEndpoint.from_dict(e) for k, e in enumerate(case.endpoints)
           if e.get("process") is None or (installed and k not in no_id)]
    out = []
    for f in world.flows:
        rec = asn_of(f.dst)
        a = ASN_RECORDS[rec] if rec is not None else (None, None, None)
        ok = bool(eps) and is_session_in_whitelist(eps, "custom_whitelist", None, f.dst, f.dport, f.proto, a[0], a[1], a[2],
                                                   world.process(f, n_names))[0]
        b = CONFORMING if ok else NONCONFORMING
        if not ok and host_check(case.endpoints, no_id, installed, f.dport, f.proto):
            b |= HOST_CHECK
        out.append(b)
    return out


def counters(states, prev=None):
    return dict(flows=len(states), conforming=sum(1 for b in states if b & 1), nonconforming=sum(1 for b in states if b & 2),
                host_check=sum(1 for b in states if b & 4),
                changed=len(states) if prev is None else sum(1 for x, y in zip(states, prev) if x != y))


def name_table(interner, n_names):
    """The (match_id, name_id) arrays of the first n_names process ids of PROCS."""
    m, v = np.zeros(n_names, dtype=np.uint32), np.zeros(n_names, dtype=np.uint32)
    for p in range(1, n_names):
        m[p], v[p] = interner.match_id(PROCS[p]), interner.name_id(PROCS[p])
    return m, v


def flow_key(f):
    """The ten session_key words of a flow."""
    s, fam = ip_to_words(ipaddress.ip_address(f.src))
    d, _ = ip_to_words(ipaddress.ip_address(f.dst))
    return list(s) + list(d) + [f.sport | f.dport << 16, {TCP: 6, UDP: 17}[f.proto] | fam << 8]


def write_corpus(path, world, case, n_names, interner=None):
    """The inputs of tests/wl_match_host.cpp: the compiled rows, the name table, and per flow its key, its L7
    element's process id and its dst_asn (as the ids Whitelists.compile interned)."""
    interner = interner or ProcessNameInterner()
    comp, rows = case.compile(interner)
    m, v = name_table(interner, n_names)
    blob = [struct.pack("<4Q", len(rows), n_names, 1 if world.plane else 0, len(world.flows)), rows.tobytes(),
            m.tobytes(), v.tobytes()]
    for f in world.flows:
        rec = asn_of(f.dst)
        asn = (0, 0, 0xFFFFFFFF, 0xFFFFFFFF) if rec is None else \
            (1, ASN_RECORDS[rec][0], int(comp.rec_owner_id[rec]), int(comp.rec_country_id[rec]))
        blob.append(struct.pack("<16I", *(flow_key(f) + [world.process_id(f)] + list(asn) + [0])))
    with open(path, "wb") as fh:
        fh.write(b"".join(blob))


WORLDS = {
    "semantic": lambda: World("semantic", semantic_flows()),
    "semantic_no_plane": lambda: World("semantic_no_plane", semantic_flows(), plane=False),
    "runs": lambda: World("runs", run_flows()),
}


def corpora():
    """Every (world name, case, n_names) the tests run."""
    out = [("semantic", c, N_NAMES) for c in semantic()]
    out += [("semantic_no_plane", c, N_NAMES) for c in semantic() if c.label[1] == "proto_port"]
    out += [("runs", c, N_NAMES) for c in runs()]
    out += [("semantic", c, N_NAMES) for c in staging()]
    # table sizes 0 (none), 1 (entry 0 alone: no flow has a process) and 2
    out += [("semantic", c, n) for n in (0, 1, 2) for c in semantic() if c.label[:2] == ("exact_v4", "proto_port")]
    return out


# ---- hand-written expectations: one case of each rule (endpoint, the flow's process, names installed, byte) ----
HAND = [
    # process_matches (src/whitelists.rs:716-724): None matches any process
    ({"ip": A4}, "curl", True, CONFORMING), ({"ip": A4}, None, True, CONFORMING),
    # ... Some(p): the session's must be Some and equal ignoring ASCII case
    ({"ip": A4, "process": "curl"}, "curl", True, CONFORMING), ({"ip": A4, "process": "Curl"}, "cURL", True, CONFORMING),
    ({"ip": A4, "process": "curl"}, "nginx", True, NONCONFORMING), ({"ip": A4, "process": "curl"}, None, True, NONCONFORMING),
    # the process gates every shape: a net, AS fields, match-all, domain + ip by the address
    ({"ip": "93.184.0.0/16", "process": "curl"}, "curl", True, CONFORMING),
    ({"ip": "93.184.0.0/16", "process": "curl"}, "wget", True, NONCONFORMING),
    ({"as_number": 64500, "process": "curl"}, "curl", True, CONFORMING),
    ({"as_number": 64500, "process": "curl"}, None, True, NONCONFORMING),
    ({"process": "curl"}, "curl", True, CONFORMING), ({"process": "curl"}, "nginx", True, NONCONFORMING),
    ({"domain": "x.example.com", "ip": A4, "process": "curl"}, "curl", True, CONFORMING),
    ({"domain": "x.example.com", "ip": A4, "process": "curl"}, "nginx", True, NONCONFORMING | HOST_CHECK),  # (the domain)
    ({"domain": "x.example.com", "process": "curl"}, "curl", True, NONCONFORMING | HOST_CHECK),
    # without a name table a process endpoint is the host's
    ({"ip": A4, "process": "curl"}, "curl", False, NONCONFORMING | HOST_CHECK),
    ({"ip": A4, "process": "curl", "port": 80}, "curl", False, NONCONFORMING),  # (not the flow's port: nothing to check)
]
HAND_FLOW = Flow(TCP, "192.168.1.1", 61000, A4, 443, "resolved")


class HandWorld(World):
    def __init__(self, proc):
        super().__init__("hand", [HAND_FLOW])
        self.proc = proc

    def process(self, f, n_names):
        return self.proc if n_names else None


# ---- putting a World on the device (the GPU tests) ----------------------------------------------------------
def l7_flow(f):
    """The flow in tests/l7space.py's terms (its loaders and socket arrays are reused)."""
    import l7space as L
    a = lambda t: (L.V6 if ":" in t else L.V4, int(ipaddress.ip_address(t)))  # noqa: E731
    return L.Flow({TCP: 6, UDP: 17}[f.proto], a(f.src), f.sport, a(f.dst), f.dport)


def load_world(cap, world):
    """The world's flows into the capture's table with the L7 elements FLOW_PROCS describes: the flows a socket
    or no socket is to decide go in first, one snapshot with an exact socket per 'sock' flow (process_id = the
    corpus's own), one pass with max_retries 0 -- whoever finds no socket fails at once --, then the 'late' flows,
    which no pass has seen.  -> {Flow: table slot}; the plane is checked against the corpus here."""
    import l7space as L
    how = {f: FLOW_PROCS[f.state][0] for f in world.flows}

    def load(part):
        g = cap.process_parsed(L.parsed_array([l7_flow(f) for f in part]))
        assert g.stats["error"] == 0 and g.stats["new_sessions"] == len(part)

    if not world.plane:
        load(world.flows)
    else:
        first = [f for f in world.flows if how[f] != "late"]
        load(first)
        socks = [L.Sock(l7_flow(f).proto, l7_flow(f).src, f.sport, l7_flow(f).dst, f.dport, FLOW_PROCS[f.state][1])
                 for f in first if how[f] == "sock"]
        arr = L.socket_array(socks)
        N.check(N.gpu_lib().fb_set_l7_sockets(cap.ctx, N.ptr(arr), len(arr)))
        st = cap.update_l7(max_retries=0)
        assert st["exact"] == len(socks) and st["fuzzy"] == 0 and st["failed"] == len(first) - len(socks)
        load([f for f in world.flows if how[f] == "late"])
    slots = {L.flow_of(r): int(r["slot"]) for r in cap.export_flows()}
    out = {f: slots[l7_flow(f)] for f in world.flows}
    assert len(out) == len(world.flows) == len(slots)
    if world.plane:
        plane = cap.l7_records()
        for f, s in out.items():
            want = {"sock": (FLOW_PROCS[f.state][1], N.FB_L7_EXACT), "nosock": (0, N.FB_L7_FAILED), "late": (0, 0)}[how[f]]
            assert (int(plane[s]["process_id"]), int(plane[s]["source"])) == want, f
    return out


def asn_arrays():
    v4 = np.zeros(len(ASN_V4), dtype=N.ASN_RANGE_DTYPE)
    for i, (s, e, r) in enumerate(ASN_V4):
        v4[i]["start"], v4[i]["end"], v4[i]["as_number"], v4[i]["record"] = (s, 0, 0, 0), (e, 0, 0, 0), ASN_RECORDS[r][0], r
    return v4, np.zeros(0, dtype=N.ASN_RANGE_DTYPE)
