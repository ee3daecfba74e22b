"""CPU-side checks of the whitelist feature: the C-ABI structs and symbols, the host compiler's
encodings (flodbadd_amd/whitelists.py: Whitelists.compile), domain expansion, `extends` flattening,
new_from_sessions' de-duplication and the reason strings -- each against the restatement in
tests/wlref.py (written from src/whitelists.rs, independent of the product's host code)."""
import ipaddress
import json
import os
import subprocess

import numpy as np
import pytest

import wlref
from flodbadd_amd import _native as N
from flodbadd_amd.sessions import Protocol, Session, SessionInfo, WhitelistState, flows_to_sessions
from flodbadd_amd.whitelists import (Whitelists, WhitelistEndpoint, domain_matches, endpoint_matches, ip_matches,
                                     is_session_in_whitelist, rows_from_flows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "whitelist_kats.json")))["cases"]


def model(*lists):
    return {"date": "d", "signature": None,
            "whitelists": [{"name": n, "extends": ext, "endpoints": eps} for n, ext, eps in lists]}


def test_struct_sizes_match_the_header(tmp_path):
    checks = [("fb_wl_endpoint", N.WL_ENDPOINT_DTYPE), ("fb_wl_stats", N.WL_STATS_DTYPE)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s/include/flodbadd_gpu.h"' % ROOT, "int main(void) {"]
    want = []
    for st, dt in checks:
        src.append('printf("%%zu\\n", sizeof(%s));' % st)
        want.append(dt.itemsize)
        for f in dt.names:
            src.append('printf("%%zu\\n", offsetof(%s, %s));' % (st, f))
            want.append(dt.fields[f][1])
    for c in ("FB_WL_NEVER", "FB_WL_HAS_PORT", "FB_WL_HAS_ASN", "FB_WL_HAS_OWNER", "FB_WL_HAS_COUNTRY", "FB_WL_HAS_DOMAIN",
              "FB_WL_HAS_PROCESS", "FB_WL_CONFORMING", "FB_WL_NONCONFORMING", "FB_WL_HOST_CHECK", "FB_WL_MASK_UNKNOWN",
              "FB_WL_MAX_EXACT", "FB_WL_MAX_OTHER"):
        src.append('printf("%%u\\n", (unsigned)%s);' % c)
        want.append(getattr(N, c))
    src.append("return 0; }")
    c = tmp_path / "wl.c"
    c.write_text("\n".join(src) + "\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "wl"), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "wl")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert N.FB_WL_MAX_EXACT >= 1 << 20 and N.FB_WL_MAX_OTHER >= 4096


def test_symbols_are_exported_and_reject_a_null_context():
    lib = N.gpu_lib()
    for name in ("fb_set_whitelist", "fb_clear_whitelist", "fb_flow_whitelist", "fb_flow_whitelist_dev",
                 "fb_flow_export_whitelist_dev"):
        assert hasattr(lib, name), name
    assert lib.fb_set_whitelist(None, None, 0, None, None, 0) == N.FB_ERR_INVAL
    assert lib.fb_clear_whitelist(None) == N.FB_ERR_INVAL
    assert lib.fb_flow_whitelist(None, 0, None, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_whitelist_dev(None, None, 0, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_export_whitelist_dev(None, 0, None, 0, None, None) == N.FB_ERR_INVAL


def test_compile_encodings():
    eps = [
        {"ip": "1.2.3.4"},                                            # 0: a plain v4 address is a /32
        {"ip": "2001:db8::1", "protocol": "tcp", "port": 443},        # 1: /128, protocol folded
        {"ip": "10.1.2.3/8", "protocol": "Udp"},                      # 2: host bits kept as written
        {"ip": "not-an-ip", "protocol": "TCP"},                       # 3: never
        {"ip": "1.2.3.4/33"},                                         # 4: never
        {"ip": "fe80::1%eth0"},                                       # 5: never (IpAddr has no zone)
        {"protocol": "ICMP", "port": 0},                              # 6: protocol never; port 0 is a port
        {"as_number": 64500, "as_owner": "Example NET", "as_country": "us"},          # 7
        {"as_owner": "example net", "as_country": "US"},              # 8: same ids as 7 (case folded)
        {"as_owner": "EXAMPLE NÉT"},                                  # 9: non-ASCII is not folded
        {"domain": "x.example.com", "process": "curl"},               # 10
        {},                                                           # 11: nothing specified
    ]
    recs = [(64500, "US", "Example Net"), (64501, "FR", "Autre")]
    c = Whitelists(model(("w", None, eps))).compile("w", recs)
    r = c.rows
    assert len(r) == len(eps) and r.dtype == N.WL_ENDPOINT_DTYPE
    assert (r[0]["family"], r[0]["prefix"], int(r[0]["addr"][0]), r[0]["protocol"], r[0]["flags"]) == (2, 32, 0x01020304, 0, 0)
    assert (r[1]["family"], r[1]["prefix"], r[1]["protocol"], r[1]["port"], r[1]["flags"]) == (10, 128, 6, 443, N.FB_WL_HAS_PORT)
    assert r[1]["addr"].tolist() == [0x20010DB8, 0, 0, 1]
    assert (r[2]["family"], r[2]["prefix"], int(r[2]["addr"][0]), r[2]["protocol"]) == (2, 8, 0x0A010203, 17)
    for k in (3, 4, 5):
        assert r[k]["family"] == N.FB_WL_NEVER, k
    assert r[3]["protocol"] == 6
    assert r[6]["protocol"] == N.FB_WL_NEVER and r[6]["flags"] == N.FB_WL_HAS_PORT and r[6]["port"] == 0
    assert r[7]["flags"] == N.FB_WL_HAS_ASN | N.FB_WL_HAS_OWNER | N.FB_WL_HAS_COUNTRY and r[7]["as_number"] == 64500
    assert r[8]["flags"] == N.FB_WL_HAS_OWNER | N.FB_WL_HAS_COUNTRY
    assert (r[7]["owner_id"], r[7]["country_id"]) == (r[8]["owner_id"], r[8]["country_id"])
    assert r[9]["owner_id"] != r[7]["owner_id"]
    assert r[10]["flags"] == N.FB_WL_HAS_DOMAIN | N.FB_WL_HAS_PROCESS and r[10]["family"] == 0
    assert r[11].tobytes() == bytes(40)
    # the records' interned strings: record 0 is 7's owner and country, record 1 is nobody's
    assert c.rec_owner_id.dtype == np.uint32 and len(c.rec_owner_id) == 2
    assert (c.rec_owner_id[0], c.rec_country_id[0]) == (r[7]["owner_id"], r[7]["country_id"])
    assert c.rec_owner_id[1] not in (r[7]["owner_id"], r[9]["owner_id"])
    assert len(set(c.strings.values())) == len(c.strings)


DOMAIN_CASES = [  # (pattern, domain, matches) -- src/whitelists.rs:602-679
    ("example.com", "example.com", True), ("Example.COM", "example.com", True), ("example.com", "a.example.com", False),
    ("*.example.com", "a.example.com", True), ("*.example.com", "example.com", False),
    ("*.example.com", "a.b.EXAMPLE.com", True), ("*.example.com", "badexample.com", False),
    ("example.*", "example.org", True), ("example.*", "example", True), ("example.*", "example.co.uk", True),
    ("example.*", "examples.org", False), ("example.*", "www.example.org", False),
    ("api*.example.com", "api1.example.com", True), ("api*.example.com", "api.example.com", False),
    ("a*b*c", "aXbXc", False), ("*", "anything", True), ("*", "", False),
]


@pytest.mark.parametrize("pattern,domain,want", DOMAIN_CASES)
def test_domain_matches(pattern, domain, want):
    assert wlref.domain_matches(domain, pattern) is want
    assert domain_matches(domain, pattern) is want
    assert domain_matches(None, pattern) is False and domain_matches(domain, None) is True


def test_ip_matches_agrees_with_the_restatement():
    ips = ["1.2.3.4", "1.2.3.5", "129.0.0.1", "2001:db8::1", "2001:db8:0:1::", "::1", "bad"]
    pats = ["1.2.3.4", "1.2.3.4/32", "1.2.3.4/31", "1.2.3.4/0", "128.0.0.0/1", "2001:db8::/33", "2001:db8::ffff/64",
            "::/0", "2001:db8::1/128", "2001:db8::1/129", "1.2.3.4/", "1.2.3.4/255.255.255.0", "x", "01.2.3.4"]
    for ip in ips:
        for p in pats:
            assert ip_matches(ip, p) == wlref.ip_matches(ip, p), (ip, p)
    assert ip_matches("1.2.3.5", "1.2.3.4/31") and not ip_matches("1.2.3.6", "1.2.3.4/31")
    assert not ip_matches("1.2.3.4", "::/0") and not ip_matches("::1", "0.0.0.0/0")


def test_domain_expansion():
    eps = [{"domain": "example.com", "port": 443, "protocol": "TCP"},
           {"domain": "*.example.com", "process": "curl"},
           {"domain": "cdn.*", "as_number": 5},
           {"domain": "api*.example.net", "ip": "9.9.9.9"}]
    dns = {"1.1.1.1": "example.com", "2.2.2.2": "www.Example.com", "2001:db8::2": "cdn.org", "3.3.3.3": "api7.example.net",
           "4.4.4.4": "other.test"}
    rows = Whitelists(model(("w", None, eps))).compile("w", None, dns).rows
    exp = [r for r in rows if not (r["flags"] & N.FB_WL_HAS_DOMAIN)]
    keep = [r for r in rows if r["flags"] & N.FB_WL_HAS_DOMAIN]
    assert len(keep) == 4 and len(exp) == 4  # example.com against *.example.com does not match
    got = sorted((r["family"], tuple(r["addr"].tolist()), r["prefix"], r["protocol"], r["port"], r["flags"],
                  r["as_number"]) for r in exp)
    want = sorted([(2, (0x01010101, 0, 0, 0), 32, 6, 443, N.FB_WL_HAS_PORT, 0),
                   (2, (0x02020202, 0, 0, 0), 32, 0, 0, N.FB_WL_HAS_PROCESS, 0),
                   (10, (0x20010DB8, 0, 0, 2), 128, 0, 0, 0, 0),       # the AS field is not carried over
                   (2, (0x03030303, 0, 0, 0), 32, 0, 0, 0, 0)])
    assert got == want
    assert keep[3]["family"] == 2 and int(keep[3]["addr"][0]) == 0x09090909  # the original keeps its own ip


def test_extends_flattening_cycle_and_missing_parent():
    m = model(("a", ["b", "c"], [{"port": 1}]), ("b", ["a", "c"], [{"port": 2}]), ("c", ["a"], [{"port": 3}]),
              ("d", ["nope"], [{"port": 4}]), ("e", ["b", "d"], [{"port": 5}]))
    w = Whitelists(json.dumps(m))
    for name in "abcde":
        assert [e.port for e in w.get_all_endpoints(name)] == [e["port"] for e in wlref.flatten(m, name)], name
    assert [e.port for e in w.get_all_endpoints("a")] == [1, 2, 3]   # own first, then depth-first, each once
    assert w.get_all_endpoints("d") == [] and w.get_all_endpoints("e") == []  # a missing parent voids the list
    assert w.get_all_endpoints("unknown") == []
    assert len(w.compile("unknown").rows) == 0


def sess(proto, src, sport, dst, dport):
    return Session(Protocol[proto], ipaddress.ip_address(src), sport, ipaddress.ip_address(dst), dport)


def test_new_from_sessions_deduplicates_by_fingerprint():
    ss = [SessionInfo(sess("TCP", "10.0.0.1", 1000, "8.8.8.8", 443)), SessionInfo(sess("TCP", "10.0.0.2", 1001, "8.8.8.8", 443)),
          SessionInfo(sess("UDP", "10.0.0.1", 1000, "8.8.8.8", 443)), SessionInfo(sess("TCP", "10.0.0.1", 1000, "8.8.8.8", 80)),
          SessionInfo(sess("TCP", "fd00::1", 1000, "2001:db8::1", 443))]
    w = Whitelists.new_from_sessions(ss)
    assert list(w.whitelists) == ["custom_whitelist"] and w.signature is None
    eps = w.whitelists["custom_whitelist"].endpoints
    assert [(e.ip, e.port, e.protocol) for e in eps] == [("8.8.8.8", 443, "TCP"), ("8.8.8.8", 443, "UDP"),
                                                          ("8.8.8.8", 80, "TCP"), ("2001:db8::1", 443, "TCP")]
    assert eps[0].description == "Auto-generated from session: 10.0.0.1:1000 -> 8.8.8.8:443"  # the first one's
    assert all(e.domain is None and e.process is None and e.as_number is None for e in eps)
    # a domain or a process is part of the fingerprint; "Unknown" / "Resolving" are no domains
    w2 = Whitelists.new_from_sessions(ss[:2], {"8.8.8.8": "Resolving"}, {ss[1].session: "dig"})
    e2 = w2.whitelists["custom_whitelist"].endpoints
    assert [(e.domain, e.process) for e in e2] == [(None, None), (None, "dig")]
    w3 = Whitelists.new_from_sessions(ss[:2], {"8.8.8.8": "dns.google"})
    assert [e.domain for e in w3.whitelists["custom_whitelist"].endpoints] == ["dns.google"]
    again = Whitelists(w3.to_json())  # the JSON round trip keeps the model
    assert again.to_dict() == w3.to_dict()
    # the array fast path gives the rows the compiled learned list gives
    flows = np.zeros(len(ss), dtype=N.FLOW_REC_DTYPE)
    for f, i in zip(flows, ss):
        s, d, fam = i.session.key_fields()
        f["src_ip"], f["dst_ip"], f["family"], f["protocol"] = s, d, fam, int(i.session.protocol)
        f["src_port"], f["dst_port"] = i.session.src_port, i.session.dst_port
    assert [x.session for x in flows_to_sessions(flows)] == sorted((i.session for i in ss), key=Session.sort_key)
    a = sorted(r.tobytes() for r in rows_from_flows(flows))
    assert a == sorted(r.tobytes() for r in w.compile("custom_whitelist").rows)


def test_reason_strings():
    eps = [WhitelistEndpoint(ip="1.2.3.4", port=443, protocol="TCP")]
    ok, why = is_session_in_whitelist(eps, "lst", None, "8.8.8.8", 443, "TCP")
    assert not ok and why == ("No matching endpoint found in whitelist 'lst' for domain: None, ip: Some(\"8.8.8.8\"), "
                              "port: 443, protocol: TCP, ASN: None, country: None, owner: None, process: None")
    ok, why = is_session_in_whitelist(eps, "lst", "a.b", "8.8.8.8", 53, "UDP", 15169, "US", 'Goo"gle', "dig")
    assert why == ("No matching endpoint found in whitelist 'lst' for domain: Some(\"a.b\"), ip: Some(\"8.8.8.8\"), "
                   "port: 53, protocol: UDP, ASN: Some(15169), country: Some(\"US\"), owner: Some(\"Goo\\\"gle\"), "
                   "process: Some(\"dig\")")
    assert why == wlref.in_whitelist([{"ip": "1.2.3.4", "port": 443, "protocol": "TCP"}], "lst", "a.b", "8.8.8.8", 53,
                                     "UDP", (15169, "US", 'Goo"gle'), "dig")[1]
    assert is_session_in_whitelist([], "e", None, "1.1.1.1", 1, "TCP") == (False, "Whitelist 'e' contains no endpoints")
    assert is_session_in_whitelist(eps, "lst", None, "1.2.3.4", 443, "tcp") == (True, None)
    # per-endpoint reasons (src/whitelists.rs:469-491, 516-531, 541-593)
    assert endpoint_matches(eps[0], None, "1.2.3.4", 80, "UDP")[1] == \
        "Protocol mismatch: UDP not matching Some(\"TCP\"), Port mismatch: 80 not matching Some(443)"
    assert endpoint_matches(WhitelistEndpoint(process="curl"), None, "1.2.3.4", 80, "UDP")[1] == \
        "Process mismatch: None not matching Some(\"curl\")"
    assert endpoint_matches(WhitelistEndpoint(domain="x.y", ip="9.9.9.9"), "q.r", "1.2.3.4", 80, "UDP")[1] == \
        "Domain mismatch: Some(\"q.r\") not matching Some(\"x.y\"), IP mismatch: Some(\"1.2.3.4\") not matching Some(\"9.9.9.9\")"
    assert endpoint_matches(WhitelistEndpoint(as_number=5), None, "1.2.3.4", 80, "UDP", 6)[1] == \
        "AS number mismatch: Some(6) not matching Some(5)"
    assert endpoint_matches(WhitelistEndpoint(as_owner="a"), None, "1.2.3.4", 80, "UDP", 6, "US", "b")[1] == \
        "Owner mismatch: Some(\"b\") not matching Some(\"a\")"
    assert endpoint_matches(WhitelistEndpoint(as_country="FR"), None, "1.2.3.4", 80, "UDP", 6, "US", "b")[1] == \
        "Country mismatch: Some(\"US\") not matching Some(\"FR\")"


def test_endpoint_matches_agrees_with_the_restatement():
    """Every combination of a small field alphabet through both implementations."""
    import itertools
    doms, ips = [None, "a.example.com", "*.example.com"], [None, "1.2.3.4", "1.2.0.0/16", "bad"]
    asns, procs = [None, (5, "US", "Own")], [None, "Curl"]
    n = 0
    for d, i, port, proto, num, own, cty, pr in itertools.product(doms, ips, [None, 443], [None, "tcp", "x"], [None, 5, 6],
                                                                 [None, "OWN", "z"], [None, "us"], [None, "curl"]):
        ep = dict(domain=d, ip=i, port=port, protocol=proto, as_number=num, as_owner=own, as_country=cty, process=pr)
        for sd in (None, "a.example.com"):
            for sip in ("1.2.3.4", "9.9.9.9"):
                for asn in asns:
                    for sp in procs:
                        a = asn or (None, None, None)
                        got = endpoint_matches(WhitelistEndpoint(**ep), sd, sip, 443, "TCP", a[0], a[1], a[2], sp)[0]
                        assert got == wlref.endpoint_matches(ep, sd, sip, 443, "TCP", asn, sp), (ep, sd, sip, asn, sp)
                        n += 1
    assert n > 10000


@pytest.mark.parametrize("case", KATS, ids=[c["from"].split()[1] for c in KATS])
def test_reference_kats_host_side(case):
    """The reference's own examples through the restatement and the product's host function."""
    w = Whitelists(case["whitelists"])
    eps = w.get_all_endpoints(case["name"])
    for s in case["sessions"]:
        want = s["conforming"]
        assert wlref.in_whitelist(wlref.flatten(case["whitelists"], case["name"]), case["name"], None, s["dst_ip"],
                                  s["dst_port"], s["protocol"], None, None)[0] is want
        assert is_session_in_whitelist(eps, case["name"], None, s["dst_ip"], s["dst_port"], s["protocol"])[0] is want


def test_whitelist_state_decoding():
    assert WhitelistState.from_byte(0) is WhitelistState.Unknown
    assert WhitelistState.from_byte(N.FB_WL_CONFORMING) is WhitelistState.Conforming
    assert WhitelistState.from_byte(N.FB_WL_NONCONFORMING | N.FB_WL_HOST_CHECK) is WhitelistState.NonConforming
    assert SessionInfo(sess("TCP", "10.0.0.1", 1, "8.8.8.8", 2)).is_whitelisted is WhitelistState.Unknown
