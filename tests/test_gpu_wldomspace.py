"""Domain endpoints of the whitelist decided on the GPU (fb_set_whitelist_dom, fb_wl_name_matches_dev, fb_flow_whitelist;
DESIGN.md 3.20) against tests/wldomspace.py: the name-match kernel's rows and flags byte for byte under three hash
masks, and every flow corpus through the staged and the global-memory instances, with and without stamps, with and
without a process-name table -- the state byte of every flow including FB_WL_HOST_CHECK, all six counters and the
stamp plane; no tolerance applies.  The expectation is the literal scan with the name or the flow's domain string
(tests/test_wldomspace_oracle.py pins it, and the kernels' own header, on the CPU)."""
import functools

import numpy as np
import pytest

import dnstrackspace as T
import l7space as L
import wldomspace as D
import wlprocspace as P
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.l7 import ProcessNameInterner
from flodbadd_amd.sessions import SessionFilter
from flodbadd_amd.whitelists import Whitelists

pytestmark = pytest.mark.gpu

S = 10 ** 9
T0 = 1_700_000_000 * S


track, track_names, stored_names, install_patterns = D.track, D.track_names, D.stored_names, D.install_patterns


def pass_stats(cap):
    """fb_flow_whitelist -> (the five counters, dom_overflow)."""
    st = np.zeros(1, dtype=N.WL_STATS_DOM_DTYPE)
    N.check(N.gpu_lib().fb_flow_whitelist(cap.ctx, 0, N.ptr(st), None))
    assert not st[0]["reserved"].any()
    return {f: int(st[0][f]) for f in N.WL_STATS_FIELDS}, int(st[0]["dom_overflow"])


@pytest.fixture(scope="module")
def namedev():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9, service_bitmap=bytes(8192),
                             track_dns=True, dns_name_capacity=4)  # (the store grows many times on the way)
    track_names(cap, list(D.all_names()))
    ids = {s: i for i, s in stored_names(cap).items()}
    assert set(ids) == set(D.all_names()) and len(ids) == len(D.all_names())
    yield cap, ids
    cap.close()


@functools.lru_cache(maxsize=None)
def name_expectation(k):
    label, pats = D.name_cases()[k]
    names = [n for n in D.case_names(label) if n]
    return names, D.expected_rows(names, pats)


@pytest.mark.parametrize("mask", D.MASKS, ids=["all_bits", "four_bits", "top_bit"])
def test_name_rows_byte_for_byte(namedev, mask):
    cap, ids = namedev
    lib = N.gpu_lib()
    N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_WL_NAME_HASH_MASK, mask))
    try:
        n_all = len(ids)
        for k, (label, pats) in enumerate(D.name_cases()):
            install_patterns(cap, pats)
            names, (rows, flags) = name_expectation(k)
            ask = np.array([ids[n] for n in names] + [0, n_all + 1, 0xFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
            got_rows, got_flags = cap.whitelist_name_matches(ask)
            want_rows = np.concatenate([rows, np.zeros((4, D.ROW), dtype=np.uint32)])
            want_flags = np.concatenate([flags, np.zeros(4, dtype=np.uint8)])
            bad = np.nonzero((got_rows != want_rows).any(axis=1) | (got_flags != want_flags))[0]
            assert len(bad) == 0, (label, mask, [((names + ["-"] * 4)[i], got_rows[i].tolist(), want_rows[i].tolist()) for i in bad[:4]])
            info = cap.whitelist_domain_info()
            kinds = [D.classify_domain_pattern(p.lower()) for p in pats]
            assert [info[kd] for kd in D.KINDS] == [kinds.count(kd) for kd in D.KINDS], label
            assert info["names_done"] == (n_all if pats else 0), label
            if label in ("overflow", "duplicates"):
                assert info["names_overflowed"] >= 1
            if label.startswith("exhaustive"):
                assert info["names_overflowed"] == 0  # no pair of the space is left out
    finally:
        N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_WL_NAME_HASH_MASK, 0))


def test_incremental_matching_growth_clear_and_reinstall():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9, service_bitmap=bytes(8192),
                             track_dns=True, dns_name_capacity=4)
    lib = N.gpu_lib()
    try:
        pats = ["*.example.com", "m.*", "x.com"]
        # no list: the call is refused; a list, no names: nothing to do
        d = N.DeviceBuffer(64)
        assert lib.fb_wl_name_matches_dev(cap.ctx, d.ptr, 1, d.ptr, d.ptr, None) == N.FB_ERR_INVAL
        install_patterns(cap, pats)
        assert cap.whitelist_domain_info()["names_done"] == 0
        first = ["a.example.com", "x.com", "nothing.org"]
        track_names(cap, first)
        ids = {s: i for i, s in stored_names(cap).items()}
        rows, flags = cap.whitelist_name_matches([ids[n] for n in first])
        assert rows.tolist() == [D.expected_row(n, pats)[0] for n in first] and not flags.any()
        assert cap.whitelist_domain_info()["names_done"] == 3 and cap.whitelist_domain_info()["names_matched"] == 2
        # names added after the install, past the store's capacity of 4 and past the rows' first allocation
        more = ["m.o.example.com", "M.Example.Org"] + ["n%04d.example.com" % j for j in range(1100)]
        track_names(cap, more, tx0=100)
        ids = {s: i for i, s in stored_names(cap).items()}
        assert cap.dns_track_info()["name_capacity"] > 1024
        rows, flags = cap.whitelist_name_matches([ids[n] for n in first + more])
        assert rows.tolist() == [D.expected_row(n, pats)[0] for n in first + more]
        info = cap.whitelist_domain_info()
        assert info["names_done"] == len(first) + len(more) and info["names_matched"] == 2 + 2 + 1100
        # another list: every name is matched again
        install_patterns(cap, ["nothing.*"])
        assert cap.whitelist_domain_info()["names_done"] == 0
        rows, _ = cap.whitelist_name_matches([ids["nothing.org"], ids["x.com"]])
        assert rows[:, 0].tolist() == [1, 0] and cap.whitelist_domain_info()["names_matched"] == 1
        # fb_dns_track_clear: the ids died with the store
        cap.clear_dns()
        assert cap.whitelist_domain_info()["names_done"] == 0
        rows, _ = cap.whitelist_name_matches([1, 2, 3])
        assert not rows.any()
        track_names(cap, ["nothing.net"])
        rows, _ = cap.whitelist_name_matches([1])
        assert rows[0].tolist() == [1] + [0] * 7
        # fb_clear_whitelist forgets the rows too
        cap.reset_whitelist()
        assert cap.whitelist_domain_info()["names_done"] == 0
    finally:
        cap.close()


# ---- the per-flow pass ------------------------------------------------------------------------------------------
class Dev:
    """A capture holding wldomspace's world: the flows with their processes, the resolutions, the domain plane."""

    def __init__(self):
        self.world = D.world()
        self.cap = cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 11,
                                            service_bitmap=bytes(8192), track_dns=True)
        self.names = ProcessNameInterner()
        self.n_names = None
        slots = P.load_world(cap, self.world)
        cap.set_asn_tables(*P.asn_arrays(), P.ASN_RECORDS)
        call = T.Call()
        res = [(ip, nm) for ip, nm in D.DOMAINS.items() if nm] + [(D.LATE_DST, D.LATE_NAME)]
        for j, (ip, nm) in enumerate(res):
            call.query(10 + j, nm)
        for j, (ip, nm) in enumerate(res):
            call.response(10 + j, [ip])
        track(cap, call)
        st = cap.update_domains()
        assert st["dst_set"] == sum(1 for f in self.world.flows if D.DOMAINS[f.dst])
        late = D.late_flows()  # after the last domain pass: their plane element is zero
        g = cap.process_parsed(L.parsed_array([P.l7_flow(f) for f in late]))
        assert g.stats["new_sessions"] == len(late)
        self.flows = self.world.flows + late
        by_flow = {L.flow_of(r): int(r["slot"]) for r in cap.export_flows()}
        self.slots = {f: by_flow[P.l7_flow(f)] for f in self.flows}
        assert all(self.slots[f] == s for f, s in slots.items())
        self.domains = {f: D.DOMAINS[f.dst] for f in self.world.flows}
        dom = cap.domain_ids()["dst_name_id"]
        stored = stored_names(cap)
        for f in self.flows:  # the plane is what the corpus says
            assert (stored[int(dom[self.slots[f]])] if dom[self.slots[f]] else None) == self.domains.get(f), f

    def set_names(self, n):
        m, v = P.name_table(self.names, n)
        N.check(N.gpu_lib().fb_set_l7_process_names(self.cap.ctx, N.ptr(m) if n else None, N.ptr(v) if n else None, n))
        self.n_names = n

    def install(self, case, extra=None):
        comp = case.compile(self.names)
        if extra is not None:
            comp.rows = np.concatenate([comp.rows, extra])
            comp.ep_pattern = np.concatenate([comp.ep_pattern, np.zeros(len(extra), dtype=np.uint32)])
        self.cap.install_whitelist(comp)

    def states(self):
        sb = self.cap.whitelist_bytes()
        assert int((sb != 0).sum()) == len(self.flows)
        return [int(sb[self.slots[f]]) for f in self.flows]


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.cap.close()


@functools.lru_cache(maxsize=None)
def decoys():
    """513 nets under UDP ports no flow has: past both staging thresholds, the global-memory instances run."""
    eps = [{"ip": "10.0.0.0/8", "protocol": "UDP", "port": 30000 + j} for j in range(N.WL_LDS_GROUPS + 1)]
    m = {"date": "", "signature": None, "whitelists": [{"name": "w", "extends": None, "endpoints": eps}]}
    return Whitelists(m).compile("w").rows


_WANT = {}


def want(d, k, n_names):
    if (k, n_names) not in _WANT:
        _WANT[(k, n_names)] = D.expected(d.flows, d.domains, d.world, D.flow_cases()[k], n_names)
    return _WANT[(k, n_names)]


@pytest.mark.parametrize("n_names", [P.N_NAMES, 0], ids=["names", "no_names"])
@pytest.mark.parametrize("staged,stamped", [(True, False), (False, False), (True, True), (False, True)],
                         ids=["staged", "global", "staged_stamped", "global_stamped"])
def test_every_corpus_through_the_pass(dev, staged, stamped, n_names):
    d, lib = dev, N.gpu_lib()
    d.cap.reset_whitelist()
    d.set_names(n_names)
    prev, now = None, T0
    stamps = d.cap.modified_stamps().copy() if stamped else None
    seen_over = 0
    try:
        for k, case in enumerate(D.flow_cases()):
            now += S
            N.check(lib.fb_set_pass_time(d.cap.ctx, now if stamped else 0))
            d.install(case, None if staged else decoys())
            stats, over = pass_stats(d.cap)
            got, (exp, exp_over) = d.states(), want(d, k, n_names)
            assert got == exp, (case.name, n_names, [(f, g, e) for f, g, e in zip(d.flows, got, exp) if g != e][:4])
            assert stats == D.counters(exp, prev) and over == exp_over, (case.name, n_names, stats, over, exp_over)
            seen_over += over
            if stamped:
                for j, f in enumerate(d.flows):
                    if prev is None or prev[j] != exp[j]:
                        stamps[d.slots[f]] = now
                assert d.cap.modified_stamps().tobytes() == stamps.tobytes(), (case.name, n_names)
            prev = exp
        assert seen_over > 0
    finally:
        N.check(lib.fb_set_pass_time(d.cap.ctx, 0))


def test_a_list_without_pattern_ids_is_the_list_of_before(dev):
    """fb_set_whitelist, and fb_set_whitelist_dom with every id 0, give the bytes the pass gave before it knew
    domains: a domain never matches and its key asks for the host."""
    d = dev
    d.set_names(P.N_NAMES)
    for case in [c for c in D.semantic() if c.label[1] in ("any", "proto_port") and c.label[2] in ("suffix", "miss")] + D.mixed():
        comp = case.compile(d.names)
        none = D.Case(case.name, case.endpoints, case.no_id, set(range(len(case.endpoints))))
        exp, over = D.expected(d.flows, d.domains, d.world, none, P.N_NAMES)
        out = []
        for how in ("plain", "zero_ids"):
            d.cap.reset_whitelist()
            if how == "plain":
                d.cap.install_whitelist(comp.rows)
            else:
                comp.ep_pattern[:] = 0
                d.cap.install_whitelist(comp)
            out.append((pass_stats(d.cap), d.states()))
        assert out[0] == out[1] and out[0][1] == exp and out[0][0] == (D.counters(exp), 0) and over == 0, case.name


def test_domain_verdicts_follow_growth_and_purge():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9, service_bitmap=bytes(8192),
                             timed=True, track_dns=True)
    try:
        A = (L.V4, int(__import__("ipaddress").ip_address(D.A4)))
        B = (L.V4, int(__import__("ipaddress").ip_address(D.B4)))
        old = [L.Flow(L.TCP, L.addr(L.V4, 230, i), 42000 + i, A if i % 2 else B, 443) for i in range(60)]
        new = [L.Flow(L.TCP, L.addr(L.V4, 232, i), 43000 + i, A if i % 2 else B, 443) for i in range(60)]
        for part, t in ((old, T0), (new, T0 + 1000 * S)):
            g = cap.process_parsed(L.parsed_array(part), ts=np.full(len(part), t, dtype=np.uint64))
            assert g.stats["new_sessions"] == len(part)
        track(cap, T.Call().query(1, "www.example.com").query(2, "api.other.org").response(1, [D.A4]).response(2, [D.B4]))
        assert cap.update_domains()["dst_set"] == 120
        case = D.Case("g", [{"domain": "*.example.com", "protocol": "TCP", "port": 443}])
        cap.install_whitelist(case.compile(ProcessNameInterner()))

        def check(flows, others=0):
            st, over = pass_stats(cap)
            sb = cap.whitelist_bytes()
            got = {L.flow_of(r): int(sb[int(r["slot"])]) for r in cap.export_flows()}
            assert {f: got[f] for f in flows} == {f: (P.CONFORMING if f.dst == A else P.NONCONFORMING) for f in flows}
            assert len(got) == len(flows) + others and st["conforming"] == sum(1 for f in flows if f.dst == A)
            assert st["host_check"] == 0 and over == 0

        check(old + new)
        cap0, k, extra = cap.table_info()["capacity"], 0, 0
        while cap.table_info()["capacity"] == cap0:  # growth: the plane's ids move with their flows
            more = [L.Flow(L.UDP, L.addr(L.V4, 240 + k, i), 44000, L.addr(L.V4, 248 + k, i), 5000) for i in range(250)]
            cap.process_parsed(L.parsed_array(more), ts=np.full(250, T0 + 1000 * S, dtype=np.uint64))
            k, extra = k + 1, extra + 250
            assert k < 8
        check(old + new, extra)
        age = cap.update_sessions_status(T0 + 1100 * S, purge=True, retention_s=500)
        assert age["purged"] == 60
        check(new, extra)
    finally:
        cap.close()
