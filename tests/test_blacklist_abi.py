"""CPU-side checks of the blacklist pass: the C-ABI struct, constants and symbols, the restatement in
tests/blref.py against the reference's own examples (tests/golden/blacklist_kats.json), the
criticality strings and the host model behind set_custom_blacklists / get_blacklists."""
import ipaddress
import json
import os
import subprocess

import pytest

import blref
from flodbadd_amd import _native as N
from flodbadd_amd.enrich import Blacklists, blacklists_from_json, criticality_of, mask_names
from flodbadd_amd.sessions import Protocol, Session, SessionInfo, WhitelistState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "blacklist_kats.json")))["cases"]


def kat_id(c):
    return c["from"].split()[1]


def info_of(s):
    return SessionInfo(Session(Protocol[s["protocol"]], ipaddress.ip_address(s["src_ip"]), s["src_port"],
                               ipaddress.ip_address(s["dst_ip"]), s["dst_port"]),
                       is_local_src=s["is_local_src"], is_local_dst=s["is_local_dst"])


def test_struct_and_constants_match_the_header(tmp_path):
    dt = N.BL_STATS_DTYPE
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s/include/flodbadd_gpu.h"' % ROOT, "int main(void) {",
           'printf("%zu\\n", sizeof(fb_bl_stats));']
    want = [64]
    assert dt.itemsize == 64
    for f in dt.names:
        src.append('printf("%%zu\\n", offsetof(fb_bl_stats, %s));' % f)
        want.append(dt.fields[f][1])
    for c, v in (("FB_BL_MARK_WHITELIST", 1), ("FB_WL_BLACKLISTED", 8), ("FB_ABI_VERSION", 4), ("FB_MAX_BLACKLISTS", 64)):
        src.append('printf("%%u\\n", (unsigned)%s);' % c)
        want.append(v)
        assert getattr(N, c) == v
    src.append("return 0; }")
    c = tmp_path / "bl.c"
    c.write_text("\n".join(src) + "\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "bl"), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "bl")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert list(dt.names[:6]) == N.BL_STATS_FIELDS == ["flows", "blacklisted", "changed", "newly_blacklisted", "cleared",
                                                        "wl_marked"]
    # the new whitelist bit is none of the existing ones
    assert N.FB_WL_BLACKLISTED & (N.FB_WL_CONFORMING | N.FB_WL_NONCONFORMING | N.FB_WL_HOST_CHECK | N.FB_WL_MASK_UNKNOWN) == 0
    assert WhitelistState.from_byte(N.FB_WL_NONCONFORMING | N.FB_WL_BLACKLISTED) is WhitelistState.NonConforming


def test_symbols_are_exported_and_reject_a_null_context():
    lib = N.gpu_lib()
    for name in ("fb_flow_blacklist", "fb_flow_blacklist_dev", "fb_flow_export_blacklisted_dev"):
        assert hasattr(lib, name), name
    assert lib.fb_flow_blacklist(None, 0, None, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_blacklist(None, N.FB_BL_MARK_WHITELIST, None, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_blacklist_dev(None, None, 0, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_export_blacklisted_dev(None, None, None, 0, None, None) == N.FB_ERR_INVAL


@pytest.mark.parametrize("case", [c for c in KATS if c["kind"] == "ip"], ids=kat_id)
def test_blref_reproduces_the_address_kats(case):
    ref = blref.BlRef()
    ref.set_lists(case["blacklists"], case["filter_local_ranges"])
    for name, want in case.get("remaining", {}).items():
        assert ref.ranges(name) == want
    for x in case["ips"]:
        got = ref.ip_lists(x["ip"])
        assert bool(got) is x["blacklisted"], x
        for l in x.get("lists", []):
            assert l in got
    # the host flattening for fb_set_blacklists keeps the same ranges as the restatement
    arr, names = blacklists_from_json(case["blacklists"], case["filter_local_ranges"])
    assert names == [i["name"] for i in case["blacklists"]["blacklists"]]
    for l, name in enumerate(names):
        assert int((arr["list"] == l).sum()) == len(ref.lists[name])


@pytest.mark.parametrize("case", [c for c in KATS if c["kind"] == "sessions"], ids=kat_id)
def test_blref_reproduces_the_session_kats(case):
    ref = blref.BlRef()
    infos = {}
    for step in case["steps"]:
        if "blacklists" in step:
            ref.set_lists(step["blacklists"])
        cur = []
        for s in step["sessions"]:
            i = info_of(s)
            cur.append(infos.setdefault(i.session, i))  # a session keeps its SessionInfo across the steps
        res = ref.run(cur)
        for s, i in zip(step["sessions"], cur):
            if "criticality" in s:
                assert i.criticality == s["criticality"] == res["criticality"][i.session]
            if "contains" in s:
                assert s["contains"] in i.criticality
            if s.get("not_unknown"):
                assert i.is_whitelisted is not WhitelistState.Unknown
        want = sorted((cur[k].session for k in step["blacklisted"]), key=Session.sort_key)
        assert res["blacklisted"] == want == ref.blacklisted
        assert bool(res["blacklisted"]) is step["status"]
        assert res["n_blacklisted"] == len(want)


def test_blref_counts_across_successive_runs():
    a, b, c = (info_of(dict(protocol="TCP", src_ip="10.0.0.1", src_port=40001 + k, dst_ip=d, dst_port=443,
                            is_local_src=True, is_local_dst=False)) for k, d in enumerate(("8.8.8.8", "9.9.9.9", "1.1.1.1")))
    ref = blref.BlRef()
    ref.set_lists({"blacklists": [{"name": "x", "ip_ranges": ["8.8.8.8", "9.9.9.0/24"]}]})
    r = ref.run([a, b, c])
    assert blref.stats_of(r) == dict(flows=3, blacklisted=2, changed=2, newly_blacklisted=2, cleared=0, wl_marked=2)
    assert (a.whitelist_reason, c.whitelist_reason) == (blref.REASON, None)
    r = ref.run([a, b, c])
    assert blref.stats_of(r) == dict(flows=3, blacklisted=2, changed=0, newly_blacklisted=0, cleared=0, wl_marked=0)
    ref.set_lists({"blacklists": [{"name": "x", "ip_ranges": ["9.9.9.9"]}, {"name": "y", "ip_ranges": ["1.0.0.0/8", "9.9.9.9"]}]})
    r = ref.run([a, b, c])
    assert blref.stats_of(r) == dict(flows=3, blacklisted=2, changed=3, newly_blacklisted=1, cleared=1, wl_marked=1)
    assert (a.criticality, b.criticality, c.criticality) == ("", "blacklist:x,blacklist:y", "blacklist:y")
    assert a.is_whitelisted is WhitelistState.NonConforming  # the fallback is never taken back by this pass
    ref.set_lists("")
    r = ref.run([a, b, c])
    assert blref.stats_of(r) == dict(flows=3, blacklisted=0, changed=2, newly_blacklisted=0, cleared=2, wl_marked=0)
    assert ref.blacklisted == []


def test_criticality_strings():
    names = ["zeta", "alpha", "Beta", "alpha2"]
    assert criticality_of(0, names) == ""
    assert criticality_of(0b0001, names) == "blacklist:zeta"
    # sorted by the tag text (bytewise: upper case first), not by list number
    assert criticality_of(0b1111, names) == "blacklist:Beta,blacklist:alpha,blacklist:alpha2,blacklist:zeta"
    assert mask_names(0b0101, names) == ["zeta", "Beta"]
    # the same list matching both ends appears once: the union of the two masks, and blref's dedup
    src_mask, dst_mask = 0b0010, 0b0010
    assert criticality_of(src_mask | dst_mask, names) == "blacklist:alpha"
    ref = blref.BlRef()
    ref.set_lists({"blacklists": [{"name": n, "ip_ranges": r} for n, r in
                                  (("zeta", ["8.8.8.8"]), ("alpha", ["8.0.0.0/8", "9.9.9.9"]), ("Beta", ["9.9.9.9"]),
                                   ("alpha2", []))]})
    i = info_of(dict(protocol="UDP", src_ip="8.8.8.8", src_port=40001, dst_ip="9.9.9.9", dst_port=53,
                     is_local_src=False, is_local_dst=False))
    r = ref.run([i])
    assert r["names"][i.session] == ["Beta", "alpha", "zeta"]
    assert i.criticality == "blacklist:Beta,blacklist:alpha,blacklist:zeta" == criticality_of(0b0111, names)
    # bit 63
    many = ["l%02d" % k for k in range(64)]
    assert criticality_of((1 << 63) | 1, many) == "blacklist:l00,blacklist:l63"


@pytest.mark.parametrize("case", [c for c in KATS if c["kind"] == "model"], ids=kat_id)
def test_model_round_trip(case):
    m = Blacklists(json.dumps(case["blacklists"]))
    back = json.loads(m.to_json())
    assert set(back) == {"date", "signature", "blacklists"}
    assert {i["name"]: i["ip_ranges"] for i in back["blacklists"]} == case["lists"]
    assert m.names == list(case["lists"]) and len(m.cidrs) == sum(len(v) for v in case["lists"].values())
    assert Blacklists(m.to_json()).to_json() == m.to_json()
    # custom lists are not filtered: the local /32s stay
    assert len(blacklists_from_json(case["blacklists"], filter_local_ranges=True)[0]) < len(m.cidrs)


def test_model_empty_and_invalid_text():
    e = Blacklists("")
    assert e.names == [] and len(e.cidrs) == 0
    assert json.loads(e.to_json()) == {"date": "", "signature": "", "blacklists": []}
    good = {"date": "d", "signature": "s", "blacklists": [{"name": "a", "ip_ranges": ["1.2.3.4", "bogus", "::1/200"]}]}
    m = Blacklists(json.dumps(good))
    assert m.names == ["a"] and len(m.cidrs) == 1          # unparsable ranges are skipped, not refused
    assert json.loads(m.to_json())["blacklists"][0]["ip_ranges"] == ["1.2.3.4", "bogus", "::1/200"]
    bad = ["{", "[]", json.dumps({"date": "d", "blacklists": []}),                       # a missing field
           json.dumps(dict(good, extra=1)),                                              # deny_unknown_fields
           json.dumps(dict(good, blacklists=[{"name": "a"}])),                           # ip_ranges missing
           json.dumps(dict(good, blacklists=[{"name": "a", "ip_ranges": [], "x": 1}])),
           json.dumps(dict(good, blacklists=[{"name": "a", "ip_ranges": [1]}])),
           json.dumps(dict(good, date=None))]
    for text in bad:
        with pytest.raises(ValueError):
            Blacklists(text)
    with pytest.raises(ValueError):                                                       # more lists than mask bits
        Blacklists(json.dumps(dict(good, blacklists=[{"name": "n%d" % k, "ip_ranges": []} for k in range(65)])))
    # a repeated name replaces the earlier list (the reference keeps the lists in a map by name)
    twice = dict(good, blacklists=[{"name": "a", "ip_ranges": ["1.1.1.1"]}, {"name": "a", "ip_ranges": ["2.2.2.2", "3.3.3.3"]}])
    m = Blacklists(json.dumps(twice))
    assert m.names == ["a"] and len(m.cidrs) == 2
