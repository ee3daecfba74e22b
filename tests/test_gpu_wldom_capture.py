"""A capture that decides domain endpoints on the device (FlodbaddGpuCapture(domains_on_device=True))
end to end from DNS frames: learn -> install -> update_sessions leaves the table Conforming with no flow for the
host, a new resolution installs nothing, the domain verdicts show up in an incremental fetch, and every result is
the default mode's."""
import json

import numpy as np
import pytest

import dnsgen as G
import framegen as fg
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.sessions import SessionFilter, WhitelistState

pytestmark = pytest.mark.gpu

S = 10 ** 9
T0 = 1_700_000_000 * S


def dns_pair(tx, name, addr, port):
    q, r = G.query(tx, name), G.response(tx, name, [("A", addr)])
    return [fg.eth(0x0800, fg.ipv4("10.0.0.2", "8.8.8.8", 17, fg.udp(port, 53, q))),
            fg.eth(0x0800, fg.ipv4("8.8.8.8", "10.0.0.2", 17, fg.udp(53, port, r)))]


def feed(cap, frames, t):
    buf, offs = fg.pack(frames)
    return cap.process(buf, offs, ts=np.full(len(frames), t, dtype=np.uint64))


def verdicts(st):
    """The counters both modes must agree on (host_check is what the default mode leaves to its host loop)."""
    return {k: st[k] for k in ("flows", "conforming", "nonconforming")}


def states(cap):
    return {(str(i.session.dst_ip), i.session.dst_port): (i.is_whitelisted, i.dst_domain) for i in cap.get_sessions()}


def test_learn_install_update_and_a_new_resolution():
    caps = {m: FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9, timed=True, track_dns=True,
                                  domains_on_device=(m == "device")) for m in ("device", "default")}
    try:
        with pytest.raises(ValueError):
            FlodbaddGpuCapture(0, flow_capacity=1 << 9, domains_on_device=True)
        frames = dns_pair(0x42, "video.example.com", "198.51.100.7", 5353) + dns_pair(0x43, "cdn.example.org", "203.0.113.9", 5354) + [
            fg.tcp_frame("10.0.0.3", 44000, "1.1.1.1", 443, fg.ACK, 20),
            fg.tcp_frame("10.0.0.2", 45000, "198.51.100.7", 443, fg.ACK, 64),
            fg.tcp_frame("10.0.0.2", 45001, "203.0.113.9", 443, fg.ACK, 64)]
        out = {}
        for m, cap in caps.items():
            feed(cap, frames, T0)
            cap.update_sessions(T0 + S)
            learned = cap.create_custom_whitelists(on_device=True)
            cap.set_custom_whitelists(learned)
            st = cap.update_sessions(T0 + 2 * S)["whitelist"]
            out[m] = (json.loads(learned)["whitelists"], verdicts(st), states(cap), cap.get_whitelist_conformance())
            if m == "device":
                assert st["host_check"] == 0
        dev = caps["device"]
        assert out["device"] == out["default"]
        lists, st, sessions, conf = out["device"]
        assert any(e["domain"] for e in lists[0]["endpoints"])  # the list was learned with domains
        assert st["conforming"] == st["flows"] == len(sessions) and conf
        assert dev._wl_host_ok == set() and dev.wl_installs == 1
        assert all(w is WhitelistState.Conforming for w, _ in sessions.values())
        info = dev.whitelist_domain_info()
        assert info["exact"] == 2 and info["names_done"] == dev.dns_track_info()["names"] and info["names_overflowed"] == 0

        # a list that only the domains can satisfy, then a new resolution and a flow to it
        wl = {"date": "today", "signature": None, "whitelists": [
            {"name": "custom_whitelist", "extends": None,
             "endpoints": [{"domain": "*.example.com", "port": 443}, {"domain": "CDN.example.*", "protocol": "TCP"},
                           {"ip": "1.1.1.1", "port": 443}, {"ip": "8.8.8.8"}, {"ip": "10.0.0.2"}]}]}
        more = dns_pair(0x44, "new.example.com", "198.51.100.99", 5355) + dns_pair(0x45, "other.example.net", "198.51.100.100", 5356) + [
            fg.tcp_frame("10.0.0.2", 45002, "198.51.100.99", 443, fg.ACK, 64),
            fg.tcp_frame("10.0.0.2", 45003, "198.51.100.100", 443, fg.ACK, 64)]
        out = {}
        for m, cap in caps.items():
            cap.set_custom_whitelists(json.dumps(wl))
            a = cap.update_sessions(T0 + 3 * S)["whitelist"]
            installs = cap.wl_installs
            cap.get_sessions(T0 + 3 * S)  # a full fetch: the increments below start here
            feed(cap, more, T0 + 4 * S)
            b = cap.update_sessions(T0 + 5 * S)["whitelist"]
            inc = {(str(i.session.dst_ip), i.session.dst_port): i.is_whitelisted for i in cap.get_sessions(incremental=True)}
            exc = [(str(i.session.dst_ip), i.whitelist_reason) for i in cap.get_whitelist_exceptions()]
            out[m] = (verdicts(a), verdicts(b), states(cap), inc, exc, cap.get_whitelist_conformance())
            if m == "device":
                assert a["host_check"] == 0 and b["host_check"] == 0
                assert cap.wl_installs == installs  # the new resolutions installed nothing
                assert cap._wl_host_ok == set()
            else:
                assert cap.wl_installs > installs
        assert out["device"] == out["default"]
        a, b, sessions, inc, exc, conf = out["device"]
        assert a["conforming"] == a["flows"]
        assert b["nonconforming"] == 1 and not conf
        assert sessions[("198.51.100.99", 443)] == (WhitelistState.Conforming, "new.example.com")
        assert sessions[("198.51.100.100", 443)] == (WhitelistState.NonConforming, "other.example.net")
        assert sessions[("198.51.100.7", 443)] == (WhitelistState.Conforming, "video.example.com")
        assert inc[("198.51.100.99", 443)] is WhitelistState.Conforming  # a device verdict: stamped, so fetched
        assert [ip for ip, _ in exc] == ["198.51.100.100"] and 'domain: Some("other.example.net")' in exc[0][1]
    finally:
        for cap in caps.values():
            cap.close()
