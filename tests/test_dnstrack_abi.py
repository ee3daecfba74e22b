"""CPU-side checks of the DNS tracker's and the domain pass's C ABI: every new struct as the header lays it
out against the numpy dtypes of flodbadd_amd/_native.py, the constants, and the new entry points' argument
checks (no device is needed for a NULL context)."""
import os
import subprocess

import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.sessions import Protocol, Session, SessionInfo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "fb_dns_track_config": (N.DNS_TRACK_CONFIG_DTYPE, 32,
                            {"name_capacity": 0, "addr_capacity": 8, "hash_mask": 16, "flags": 24, "reserved": 28}),
    "fb_dns_track_stats": (N.DNS_TRACK_STATS_DTYPE, 64,
                           {"messages": 0, "queries": 8, "responses": 16, "matched": 24, "resolutions": 32,
                            "names_new": 40, "addrs_new": 48, "rounds": 56}),
    "fb_dns_track_info": (N.DNS_TRACK_INFO_DTYPE, 64,
                          {"names": 0, "addrs": 8, "name_capacity": 16, "addr_capacity": 24, "pending": 32,
                           "messages": 40, "writes": 48, "reserved": 56}),
    "fb_dns_resolution": (N.DNS_RESOLUTION_DTYPE, 48, {"ip": 0, "name_id": 32, "reserved": 36, "order": 40}),
    "fb_flow_domain": (N.FLOW_DOMAIN_DTYPE, 8, {"src_name_id": 0, "dst_name_id": 4}),
    "fb_dom_stats": (N.DOM_STATS_DTYPE, 64,
                     {"flows": 0, "current": 8, "src_set": 16, "dst_set": 24, "changed": 32, "with_domain": 40,
                      "reserved": 48}),
}
NEW_SYMBOLS = ["fb_dns_track_enable", "fb_dns_track_clear", "fb_dns_track_dev", "fb_dns_expire", "fb_dns_track_info_get",
               "fb_dns_export_resolutions_dev", "fb_dns_export_pending_dev", "fb_dns_names_dev", "fb_dns_lookup_dev",
               "fb_flow_domains", "fb_flow_domains_dev"]


def test_structs_and_constants_match_the_header(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s/include/flodbadd_gpu.h"' % ROOT, "int main(void) {"]
    want = []
    for struct, (dt, size, offsets) in STRUCTS.items():
        assert list(dt.names) == list(offsets) and dt.itemsize == size, struct
        src.append('printf("%%zu\\n", sizeof(%s));' % struct)
        want.append(size)
        for f in dt.names:
            assert dt.fields[f][1] == offsets[f], (struct, f)
            src.append('printf("%%zu\\n", offsetof(%s, %s));' % (struct, f))
            want.append(offsets[f])
    consts = {"FB_ABI_VERSION": N.FB_ABI_VERSION, "FB_DNS_MAX_NAMES": N.FB_DNS_MAX_NAMES, "FB_DNS_MAX_NAME": N.FB_DNS_MAX_NAME,
              "FB_DNS_MAX_ADDRS": N.FB_DNS_MAX_ADDRS, "FB_DEBUG_DNS_LAUNCH": N.FB_DEBUG_DNS_LAUNCH,
              "FB_DEBUG_LEARN_HASH_MASK": N.FB_DEBUG_LEARN_HASH_MASK}
    for c, v in consts.items():
        src.append('printf("%%llu\\n", (unsigned long long)%s);' % c)
        want.append(v)
    src.append('printf("%llu\\n", (unsigned long long)FB_DNS_EXPIRY_NS);')
    want.append(N.FB_DNS_EXPIRY_NS)
    # the view record did not change: 256 bytes with its 14 reserved bytes
    src.append('printf("%zu %zu\\n", sizeof(fb_flow_view), sizeof(((fb_flow_view*)0)->reserved)); return 0; }')
    want += [256, 14]
    c = tmp_path / "dnstrack.c"
    c.write_text("\n".join(src) + "\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "dnstrack"), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "dnstrack")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert N.FB_ABI_VERSION == 4 and N.FB_DNS_EXPIRY_NS == 30 * 10**9
    assert (N.FB_DEBUG_LEARN_HASH_MASK, N.FB_DEBUG_DNS_LAUNCH) == (6, 7)  # (5 stays unassigned)
    assert N.DNS_RESOLUTION_DTYPE.fields["ip"][0] == N.FB_IP_DTYPE


def test_symbols_are_bound_and_reject_a_null_context():
    lib = N.gpu_lib()
    bound = {n for n, _, _ in N.GPU_SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and hasattr(lib, name), name
    st = np.zeros(1, dtype=N.DNS_TRACK_STATS_DTYPE)
    info = np.zeros(1, dtype=N.DNS_TRACK_INFO_DTYPE)
    dom = np.zeros(1, dtype=N.DOM_STATS_DTYPE)
    assert lib.fb_dns_track_enable(None, None) == N.FB_ERR_INVAL
    assert b"NULL" in lib.fb_last_error()
    assert lib.fb_dns_track_clear(None) == N.FB_ERR_INVAL
    assert lib.fb_dns_track_dev(None, None, None, None, 0, None, None, None, N.ptr(st), None) == N.FB_ERR_INVAL
    assert lib.fb_dns_expire(None, 0, None) == N.FB_ERR_INVAL
    assert lib.fb_dns_track_info_get(None, N.ptr(info)) == N.FB_ERR_INVAL
    assert lib.fb_dns_export_resolutions_dev(None, None, 0, None, None) == N.FB_ERR_INVAL
    assert lib.fb_dns_export_pending_dev(None, None, None, None) == N.FB_ERR_INVAL
    assert lib.fb_dns_names_dev(None, None, 0, None, None, None) == N.FB_ERR_INVAL
    assert lib.fb_dns_lookup_dev(None, None, 0, None, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_domains(None, 0, N.ptr(dom), None) == N.FB_ERR_INVAL
    assert lib.fb_flow_domains_dev(None, None, 0, None) == N.FB_ERR_INVAL


def test_session_info_gains_defaulted_domains_at_the_end():
    names = list(SessionInfo.__dataclass_fields__)
    assert names[-2:] == ["src_domain", "dst_domain"]
    import ipaddress
    info = SessionInfo(Session(Protocol.TCP, ipaddress.ip_address("192.168.1.1"), 12345, ipaddress.ip_address("8.8.8.8"), 80))
    assert info.src_domain is None and info.dst_domain is None


def test_domains_are_joined_by_slot():
    """flows_to_sessions / views_to_sessions fill the domains from the plane's id pairs and the id -> string map."""
    from flodbadd_amd.sessions import flows_to_sessions, views_to_sessions
    flows = np.zeros(2, dtype=N.FLOW_REC_DTYPE)
    for i, (dst, slot) in enumerate(((0x08080808, 5), (0x01010101, 9))):
        flows[i]["src_ip"][0], flows[i]["dst_ip"][0] = 0xC0A80101, dst
        flows[i]["src_port"], flows[i]["dst_port"], flows[i]["protocol"], flows[i]["family"] = 12345, 80, 6, 2
        flows[i]["slot"], flows[i]["end_seen"] = slot, N.FB_SEEN_NONE
    plane = np.zeros((16, 2), dtype=np.uint32)
    plane[5] = (0, 3)
    plane[9] = (4, 0)
    names = {3: "dns.google", 4: "lan.example"}
    by_dst = {str(s.session.dst_ip): s for s in flows_to_sessions(flows, domains=(plane, names))}
    assert (by_dst["8.8.8.8"].src_domain, by_dst["8.8.8.8"].dst_domain) == (None, "dns.google")
    assert (by_dst["1.1.1.1"].src_domain, by_dst["1.1.1.1"].dst_domain) == ("lan.example", None)
    assert all(s.dst_domain is None for s in flows_to_sessions(flows))
    views = np.zeros(2, dtype=N.FLOW_VIEW_DTYPE)
    views["rec"] = flows
    by_dst = {str(s.session.dst_ip): s for s in views_to_sessions(views, timed=False, domains=(plane, names))}
    assert by_dst["8.8.8.8"].dst_domain == "dns.google" and by_dst["1.1.1.1"].src_domain == "lan.example"
