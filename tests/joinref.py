"""The session getters restated over the separate exports: the independent side of the getter tests.

FlodbaddGpuCapture's getters read the table through one fused view export (fb_flow_export_view) and
views_to_sessions.  sessions(cap, getter) builds the same SessionInfo list the way the getters did before that:
flow records, time records and the status / whitelist / blacklist / stamp / domain planes, each downloaded at whole
table capacity, joined by slot in flows_to_sessions, and the anomaly merge fed from anomaly_records().  It calls
neither export_view nor views_to_sessions and runs no pass: it reads the state the getter's own passes left, so it
is called after the getter it is compared with."""
import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.sessions import Session, WhitelistState, flows_to_sessions
from flodbadd_amd.whitelists import no_match_reason

GETTERS = ("sessions", "current", "blacklisted", "exceptions", "anomalous")


def _domains(cap):
    if not (cap.track_dns and cap._dom_ran):
        return None
    ids = cap.domain_ids()
    pairs = np.stack([ids["src_name_id"], ids["dst_name_id"]], axis=1)
    return pairs, cap.dns_names(np.unique(pairs))


def _join(cap, flows, whitelist, blacklist):
    """flows_to_sessions over the whole-capacity planes: status and times on a timed capture only, the whitelist
    bytes and the blacklist masks as the getter decodes them, then the anomaly tags of the plane's records."""
    out = flows_to_sessions(flows, cap.histories if cap.track_history else None,
                            times=cap.export_times() if cap.timed else None,
                            status=cap.status_bytes() if cap.timed else None,
                            whitelist=cap.whitelist_bytes() if whitelist else None,
                            blacklist=(cap.blacklist_masks(), cap._bl_names) if blacklist else None,
                            modified=cap.modified_stamps(), domains=_domains(cap))
    return cap._merge_anomaly(out, flows, cap.anomaly_records()[flows["slot"]])


def sessions(cap, getter):
    wl = bool(cap._wl_name or cap._bl_marked)
    if getter == "sessions":
        out = _join(cap, cap.export_flows(cap.filter), wl, cap._bl_ran)
        for info in out:          # the host's verdict for the flows the whitelist pass left to it
            if info.session in cap._wl_host_ok and info.is_whitelisted is WhitelistState.NonConforming:
                info.is_whitelisted = WhitelistState.Conforming
        return out
    if getter == "current":
        if not cap.timed:
            raise ValueError("current sessions need a timed capture (timed=True)")
        flows = cap.export_flows(cap.filter)
        b = cap.status_bytes()[flows["slot"]]
        return _join(cap, flows[(b == 0) | ((b & N.STATUS_CURRENT) != 0)], False, cap._bl_ran)
    if getter == "blacklisted":
        flows, masks = cap.export_blacklisted_flows()
        assert (cap.blacklist_masks()[flows["slot"]] == masks).all()
        return _join(cap, flows, wl, True)
    if getter == "anomalous":
        if cap._an_mode != "model":
            return []
        return _join(cap, cap.export_anomalous_flows(N.FB_AN_SUSPICIOUS)[0], wl, cap._bl_ran)
    assert getter == "exceptions", getter
    if not cap._wl_name:
        return []
    exc = cap.export_whitelist_flows(N.FB_WL_NONCONFORMING)
    exc = exc[np.array([Session.from_key(r) not in cap._wl_host_ok for r in exc], dtype=bool)]
    out = _join(cap, exc, False, False)
    proc = cap._wl_inputs[1] or {}
    comp, dns = cap._wl_installed  # (the resolutions the installed list was compiled with)
    keys = [Session.from_key(r) for r in exc]
    asn = dict(zip(keys, cap._dst_asn([k.dst_ip for k in keys])))
    for info in out:
        s, a = info.session, asn[info.session] or (None, None, None)
        info.is_whitelisted = WhitelistState.NonConforming
        info.whitelist_reason = no_match_reason(comp.endpoints, comp.name, dns.get(str(s.dst_ip)), str(s.dst_ip), s.dst_port,
                                                s.protocol.name, a[0], a[1], a[2], proc.get(s))
    return out


def info_fields(i):
    """Every field of a SessionInfo as plain values, for field-by-field comparison."""
    d = dict(i.__dict__)
    d["stats"] = dict(i.stats.__dict__)
    d["status"] = None if i.status is None else dict(i.status.__dict__)
    return d


def assert_same(got, want, what=None):
    assert [i.session for i in got] == [i.session for i in want], what
    for g, w in zip(got, want):
        assert info_fields(g) == info_fields(w), (what, g.session)
