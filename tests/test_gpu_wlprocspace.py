"""The process-aware whitelist pass on the GPU (fb_set_l7_process_names, fb_flow_whitelist) against
tests/wlprocspace.py: every corpus through the staged and the global-memory instances, with and without stamps --
the state byte of every flow including FB_WL_HOST_CHECK, the five counters and the stamp plane, byte for byte; no
tolerance applies.  The expectation is the literal endpoint scan with the flow's process string
(tests/test_wlprocspace_oracle.py pins it, and the kernels' own header, on the CPU)."""
import functools
import ipaddress

import numpy as np
import pytest

import l7space as L
import wlprocspace as W
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.l7 import ProcessNameInterner
from flodbadd_amd.sessions import SessionFilter
from flodbadd_amd.whitelists import Whitelists

pytestmark = pytest.mark.gpu

S = 10 ** 9
T0 = 1_700_000_000 * S


class Dev:
    """A capture holding one World, and the interner its lists and its name table share."""

    def __init__(self, world, timed=False, capacity=1 << 11):
        self.world = world
        self.cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=capacity,
                                      service_bitmap=bytes(8192), timed=timed)
        self.names = ProcessNameInterner()
        self.n_names = None  # what the device holds (None: the install call was never made)
        if not timed:
            self.slots = W.load_world(self.cap, world)
            self.cap.set_asn_tables(*W.asn_arrays(), W.ASN_RECORDS)

    def set_names(self, n):
        m, v = W.name_table(self.names, n)
        N.check(N.gpu_lib().fb_set_l7_process_names(self.cap.ctx, N.ptr(m) if n else None, N.ptr(v) if n else None, n))
        self.n_names = n

    def install(self, case, extra=None, zero_ids=False):
        comp, rows = case.compile(self.names, zero_ids)
        comp.rows = rows if extra is None else np.concatenate([rows, extra])
        self.cap.install_whitelist(comp)

    def states(self):
        sb = self.cap.whitelist_bytes()
        assert int((sb != 0).sum()) == len(self.world.flows)  # no byte outside the occupied slots
        return [int(sb[self.slots[f]]) for f in self.world.flows]


@pytest.fixture(scope="module")
def devs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Dev(W.WORLDS[name]())
        return made[name]

    yield get
    for d in made.values():
        d.cap.close()


@functools.lru_cache(maxsize=None)
def decoys():
    """513 nets under UDP ports no flow has, one group and one rule each: a list with them is past both staging
    thresholds and runs the global-memory instances."""
    eps = [{"ip": "10.0.0.0/8", "protocol": "UDP", "port": 30000 + j} for j in range(N.WL_LDS_GROUPS + 1)]
    m = {"date": "", "signature": None, "whitelists": [{"name": "w", "extends": None, "endpoints": eps}]}
    return Whitelists(m).compile("w").rows


@functools.lru_cache(maxsize=None)
def want(k, zero_ids=False):
    wname, case, n = W.corpora()[k]
    return W.expected(W.WORLDS[wname](), case, n, zero_ids)


@pytest.mark.parametrize("staged,stamped", [(True, False), (False, False), (True, True), (False, True)],
                         ids=["staged", "global", "staged_stamped", "global_stamped"])
def test_every_corpus_through_the_pass(devs, staged, stamped):
    lib = N.gpu_lib()
    prev, stamps, now, ran = {}, {}, T0, 0
    for k, (wname, case, n) in enumerate(W.corpora()):
        if case.name.startswith("staging_") and not staged:
            continue  # (these choose their instance themselves)
        d = devs(wname)
        if wname not in prev:
            d.cap.reset_whitelist()  # every byte Unknown: the first pass changes every flow
            prev[wname] = None
            stamps[wname] = d.cap.modified_stamps().copy() if stamped else None
        if d.n_names != n:
            d.set_names(n)
        now += S
        N.check(lib.fb_set_pass_time(d.cap.ctx, now if stamped else 0))
        d.install(case, None if (staged or case.name.startswith("staging_")) else decoys())
        stats = d.cap.whitelist_pass()
        got, exp = d.states(), want(k)
        assert got == exp, (wname, case.name, n, [(f, g, e) for f, g, e in zip(d.world.flows, got, exp) if g != e][:4])
        assert stats == W.counters(exp, prev[wname]), (wname, case.name, n)
        if stamped:  # exactly the flows whose byte changed carry this pass's time
            for j, f in enumerate(d.world.flows):
                if prev[wname] is None or prev[wname][j] != exp[j]:
                    stamps[wname][d.slots[f]] = now
            assert d.cap.modified_stamps().tobytes() == stamps[wname].tobytes(), (wname, case.name, n)
        prev[wname] = exp
        ran += 1
    print("corpora through the pass:", ran)
    assert ran >= len(W.semantic()) + len(W.runs())
    for wname in prev:
        N.check(lib.fb_set_pass_time(devs(wname).cap.ctx, 0))


def test_default_mode_identity_and_install_order(devs):
    """With no name table installed the state bytes and the counters are those of the same list with its process
    ids zeroed; and whether the list or the table is installed first does not matter."""
    lib = N.gpu_lib()
    d = devs("semantic")
    d.set_names(0)
    cases = [c for c in W.semantic() if c.label[1] in ("any", "proto_port")] + W.staging()[:2]
    for case in cases:
        out = []
        for zero in (False, True):
            d.cap.reset_whitelist()
            d.install(case, zero_ids=zero)
            out.append((d.cap.whitelist_pass(), d.states()))
        assert out[0] == out[1], case.name
        exp = W.expected(d.world, case, 0, zero_ids=True)
        assert out[0][1] == exp == W.expected(d.world, case, 0) and out[0][0] == W.counters(exp), case.name
    # the list first, then the table; the table first, then the list; then the table taken away again
    for case in [c for c in W.semantic() if c.label[1:] == ("proto_port", "same")] + W.runs()[-1:]:
        dd = d if case.label else devs("runs")
        exp_on, exp_off = W.expected(dd.world, case, W.N_NAMES), W.expected(dd.world, case, 0)
        dd.set_names(0)
        dd.install(case)
        dd.set_names(W.N_NAMES)
        dd.cap.whitelist_pass()
        assert dd.states() == exp_on, case.name
        dd.install(case)
        dd.cap.whitelist_pass()
        assert dd.states() == exp_on, case.name
        dd.set_names(0)
        dd.cap.whitelist_pass()
        assert dd.states() == exp_off, case.name
        assert exp_on != exp_off or case.label[0] == "domain_only"  # (the table decides something in every other)
    # an invalid call leaves the installed table as it was
    case = next(c for c in W.semantic() if c.label == ("exact_v4", "proto_port", "same"))
    d.set_names(W.N_NAMES)
    d.install(case)
    m, v = W.name_table(d.names, W.N_NAMES)
    bad = m.copy()
    bad[2] = 0
    assert lib.fb_set_l7_process_names(d.cap.ctx, N.ptr(bad), N.ptr(v), len(bad)) == N.FB_ERR_INVAL
    assert lib.fb_set_l7_process_names(d.cap.ctx, N.ptr(m), N.ptr(bad), len(bad)) == N.FB_ERR_INVAL
    assert lib.fb_set_l7_process_names(d.cap.ctx, None, N.ptr(v), len(v)) == N.FB_ERR_INVAL
    assert lib.fb_set_l7_process_names(d.cap.ctx, N.ptr(m), None, len(v)) == N.FB_ERR_INVAL
    d.cap.whitelist_pass()
    assert d.states() == W.expected(d.world, case, W.N_NAMES)
    # entry 0 is "no process" whatever the caller wrote there; fb_l7_clear leaves the table
    m2 = m.copy()
    m2[0] = m[1]
    N.check(lib.fb_set_l7_process_names(d.cap.ctx, N.ptr(m2), N.ptr(v), len(m2)))
    d.cap.whitelist_pass()
    assert d.states() == W.expected(d.world, case, W.N_NAMES)


def test_plane_and_verdicts_follow_growth_and_purge():
    """The process a flow was resolved to decides its verdict at whatever slot a growth or a purge moves it to;
    fb_l7_clear zeroes the plane and leaves the name table."""
    d = Dev(None, timed=True, capacity=1 << 9)
    cap, lib = d.cap, N.gpu_lib()
    A4 = (L.V4, int(ipaddress.ip_address(W.A4)))
    try:
        old = [L.Flow(L.TCP, L.addr(L.V4, 230, i), 42000 + i, A4, 443) for i in range(60)]
        new = [L.Flow(L.TCP, L.addr(L.V4, 232, i), 43000 + i, A4, 443) for i in range(60)]
        socks = [L.Sock(L.TCP, f.src, f.sport, f.dst, f.dport, 1 + i % 4) for i, f in enumerate(old + new)]
        arr = L.socket_array(socks)
        N.check(lib.fb_set_l7_sockets(cap.ctx, N.ptr(arr), len(arr)))
        for part, t in ((old, T0), (new, T0 + 1000 * S)):
            g = cap.process_parsed(L.parsed_array(part), ts=np.full(len(part), t, dtype=np.uint64))
            assert g.stats["new_sessions"] == len(part)
        assert cap.update_l7()["exact"] == 120
        d.set_names(W.N_NAMES)  # ids 1-3 are curl in some case, 4 is nginx
        d.install(W.Case("g", [{"ip": W.A4, "port": 443, "protocol": "TCP", "process": "curl"}]))
        pid = {f: 1 + i % 4 for i, f in enumerate(old + new)}

        def check(flows, others=0):
            st = cap.whitelist_pass()
            sb = cap.whitelist_bytes()
            got = {L.flow_of(r): int(sb[int(r["slot"])]) for r in cap.export_flows()}
            assert {f: got[f] for f in flows} == {f: (W.CONFORMING if pid[f] != 4 else W.NONCONFORMING) for f in flows}
            assert len(got) == len(flows) + others and st["conforming"] == sum(1 for f in flows if pid[f] != 4)
            assert st["host_check"] == 0

        check(old + new)
        cap0, k, extra = cap.table_info()["capacity"], 0, 0
        while cap.table_info()["capacity"] == cap0:  # growth: new flows until the table has grown
            more = [L.Flow(L.UDP, L.addr(L.V4, 240 + k, i), 44000, L.addr(L.V4, 248 + k, i), 5000) for i in range(250)]
            cap.process_parsed(L.parsed_array(more), ts=np.full(250, T0 + 1000 * S, dtype=np.uint64))
            k, extra = k + 1, extra + 250
            assert k < 8
        check(old + new, extra)
        age = cap.update_sessions_status(T0 + 1100 * S, purge=True, retention_s=500)
        assert age["purged"] == 60
        check(new, extra)
        cap.clear_l7()  # every flow is without a process again; the names stay
        st = cap.whitelist_pass()
        assert st["conforming"] == 0 and st["host_check"] == 0 and st["changed"] == sum(1 for f in new if pid[f] != 4)
    finally:
        cap.close()
