"""FlodbaddGpuCapture(processes_on_device=True) against the default (the host decides every process endpoint) on the
same input of a few hundred flows: the same conformance, exceptions and reasons, the same learned and augmented
documents -- and what only the device mode gives: no host-check flows on account of a process, a learned list that
makes its own table Conforming on the device alone, and stamps for the verdicts a process decides."""
import json

import numpy as np
import pytest

import l7space as L
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.l7 import SocketSnapshot
from flodbadd_amd.sessions import SessionFilter, WhitelistState

pytestmark = pytest.mark.gpu

S = 10 ** 9
T0 = 1_700_000_000 * S
PROCESSES = {10: ("curl", "/usr/bin/curl", "alice"), 11: ("curl", "/opt/curl", "bob"), 12: ("Curl", "/usr/bin/Curl", "alice"),
             13: ("nginx", "/usr/sbin/nginx", "www"), 14: ("sshd", "/usr/sbin/sshd", "root")}
N_FLOWS = 300


def flows():
    """300 TCP / UDP flows to 12 destinations (two IPv6) on three ports."""
    out = []
    for i in range(N_FLOWS):
        fam = L.V6 if i % 6 == 5 else L.V4
        out.append(L.Flow(L.UDP if i % 7 == 3 else L.TCP, L.addr(fam, 200, i), 45000 + i, L.addr(fam, 201, i % 12),
                          (443, 80, 8443)[i % 3]))
    return out


def snapshot(fl):
    """An exact socket for four flows of five (every fifth stays unresolved), the processes in turn."""
    pids = sorted(PROCESSES)
    socks = [(f.proto, L.text(f.src), f.sport, L.text(f.dst), f.dport, (pids[(i // 2) % len(pids)],))
             for i, f in enumerate(fl) if i % 5 != 4]
    return SocketSnapshot(socks, PROCESSES)


def whitelist(fl):
    d = [L.text(L.addr(L.V4, 201, j)) for j in range(12)]
    eps = [{"ip": d[0], "port": 443, "protocol": "TCP", "process": "curl"},
           {"ip": d[1], "process": "CURL"}, {"ip": d[1], "port": 80, "process": "nginx"}, {"ip": d[2]},
           {"process": "nginx", "port": 8443}, {"ip": "10.201.0.0/16", "protocol": "UDP", "process": "sshd"},
           {"domain": "*.example.com", "port": 443, "process": "Curl"}, {"domain": "cdn.example.org"},
           {"ip": L.text(L.addr(L.V6, 201, 5)), "process": "wget"}, {"ip": L.text(L.addr(L.V6, 201, 11)), "process": "curl"}]
    return json.dumps({"date": "today", "signature": None,
                       "whitelists": [{"name": "custom_whitelist", "extends": None, "endpoints": eps}]})


DNS = {L.text(L.addr(L.V4, 201, 3)): "a.example.com", L.text(L.addr(L.V4, 201, 4)): "cdn.example.org",
       L.text(L.addr(L.V4, 201, 6)): "Unknown"}


def make(on_device):
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 10, service_bitmap=bytes(8192),
                             timed=True, processes_on_device=on_device)
    fl = flows()
    g = cap.process_parsed(L.parsed_array(fl), ts=np.full(len(fl), T0, dtype=np.uint64))
    assert g.stats["new_sessions"] == len(fl)
    cap.set_l7_sockets(snapshot(fl))
    assert cap.update_l7()["exact"] == len(fl) - len(fl) // 5
    return cap, fl


@pytest.fixture(scope="module")
def pair():
    host, fl = make(False)
    dev, _ = make(True)
    yield host, dev, fl
    host.close()
    dev.close()


def verdicts(cap):
    return {i.session: i.is_whitelisted for i in cap.get_sessions()}


def test_same_conformance_exceptions_reasons_and_documents(pair):
    host, dev, fl = pair
    wl = whitelist(fl)
    for cap in (host, dev):
        cap.set_custom_whitelists(wl)
    sh, sd = host.update_whitelist(DNS), dev.update_whitelist(DNS)
    print("host mode:", sh, "device mode:", sd)
    # the host mode leaves every flow a process endpoint's key names to the host; the device mode only the domains'
    assert sh["flows"] == sd["flows"] == N_FLOWS and sd["host_check"] < sh["host_check"]
    assert sd["conforming"] > sh["conforming"] > 0  # (the process endpoints the device now decides itself)
    vh, vd = verdicts(host), verdicts(dev)
    assert vh == vd and set(vd.values()) == {WhitelistState.Conforming, WhitelistState.NonConforming}
    assert sum(1 for v in vd.values() if v is WhitelistState.Conforming) == sd["conforming"]  # no host overlay needed
    assert host.get_whitelist_conformance() is dev.get_whitelist_conformance() is False
    eh, ed = host.get_whitelist_exceptions(), dev.get_whitelist_exceptions()
    assert [i.session for i in eh] == [i.session for i in ed] and 0 < len(ed) < N_FLOWS
    assert [i.whitelist_reason for i in eh] == [i.whitelist_reason for i in ed]
    assert any('process: Some("' in i.whitelist_reason for i in ed) and any("process: None" in i.whitelist_reason for i in ed)
    # learning: the device path of the one, the host path of the other, one document
    lh, ld = host.create_custom_whitelists(DNS, on_device=True), dev.create_custom_whitelists(DNS, on_device=True)
    assert lh == ld
    procs = [e["process"] for e in json.loads(ld)["whitelists"][0]["endpoints"]]
    assert {"curl", "Curl", "nginx", "sshd", None} == set(procs)
    assert dev.create_custom_whitelists(DNS, on_device=False) == ld
    assert host.augment_custom_whitelists(dns_resolutions=DNS) == dev.augment_custom_whitelists(dns_resolutions=DNS)
    # a caller who passes process_names keeps the host path, in both modes
    names = host.l7_process_names()
    rh, rd = host.update_whitelist(DNS, names), dev.update_whitelist(DNS, names)
    assert all(rh[k] == rd[k] == sh[k] for k in ("flows", "conforming", "nonconforming", "host_check"))
    assert verdicts(dev) == vd


def test_a_learned_list_makes_its_own_table_conforming_on_the_device(pair):
    host, dev, fl = pair
    doc = dev.create_custom_whitelists(on_device=True)
    assert sum(1 for e in json.loads(doc)["whitelists"][0]["endpoints"] if e["process"]) > 10
    st = dev.set_custom_whitelists(doc)
    assert (st["conforming"], st["nonconforming"], st["host_check"]) == (N_FLOWS, 0, 0)
    assert dev.get_whitelist_conformance() is True and dev.get_whitelist_exceptions() == []
    assert not dev._wl_host_ok  # the device's verdicts alone
    # the default mode needs the host for the same list: every flow with a process comes back marked
    st = host.set_custom_whitelists(doc)
    assert st["host_check"] == st["nonconforming"] > 0 and host.get_whitelist_conformance() is True


def test_incremental_exceptions_report_a_verdict_the_process_changed(pair):
    host, dev, fl = pair
    wl = json.dumps({"date": "today", "signature": None, "whitelists": [
        {"name": "custom_whitelist", "extends": None, "endpoints": [{"process": "nginx"}, {"port": 80}]}]})
    dev.set_custom_whitelists(wl)
    t1, t2 = T0 + 100 * S, T0 + 200 * S
    before = dev.get_whitelist_exceptions(now_ns=t1)  # a full fetch: the getter's timestamp moves to t1
    assert dev.get_whitelist_exceptions(now_ns=t1 + S, incremental=True) == []  # nothing changed since
    nginx = {i.session for i in dev.get_sessions() if i.l7 is not None and i.l7.process_name == "nginx" and i.session.dst_port != 80}
    assert nginx and not nginx & {i.session for i in before}
    dev.clear_l7()  # every flow is without a process again: the nginx flows lose what made them Conforming
    inc = dev.get_whitelist_exceptions(now_ns=t2, incremental=True)
    assert {i.session for i in inc} == nginx
    assert all(i.is_whitelisted is WhitelistState.NonConforming and "process: None" in i.whitelist_reason for i in inc)
    stamps = dev.modified_stamps()
    slots = {L.flow_of(r): int(r["slot"]) for r in dev.export_flows()}
    assert all(int(stamps[slots[L.flow_of_session(s)]]) == t2 for s in nginx)
