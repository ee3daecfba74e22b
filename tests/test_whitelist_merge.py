"""Whitelists.merge_custom_whitelists (src/whitelists.rs:223-299) against the inputs and expectations of the
reference's own two merge tests (tests/golden/whitelist_merge_kats.json), and the rules they leave open."""
import json
import os

import pytest

from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.whitelists import Whitelists

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "whitelist_merge_kats.json")))["cases"]


def doc(lists, date="d", signature=None):
    return json.dumps({"date": date, "signature": signature, "whitelists": lists})


def wl(name, eps, extends=None):
    return {"name": name, "extends": extends, "endpoints": eps}


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
@pytest.mark.parametrize("entry", [Whitelists.merge_custom_whitelists, FlodbaddGpuCapture.merge_custom_whitelists],
                         ids=["model", "capture"])
def test_reference_cases(case, entry):
    text = entry(json.dumps(case["a"]), json.dumps(case["b"]))
    exp = case["expect"]
    for needle in exp["contains"]:
        assert needle in text
    assert "\n" not in text and text == json.dumps(json.loads(text), separators=(",", ":"))  # compact
    got = json.loads(text)
    assert isinstance(got["whitelists"], list) and len(got["whitelists"]) == exp["lists"]  # one merged list
    info = got["whitelists"][0]
    assert info["name"] == exp["name"]
    assert info["extends"] == exp["extends"]           # from the second document: the first has none
    assert len(info["endpoints"]) == exp["endpoints"]  # two unique endpoints
    assert (got["date"], got["signature"]) == (exp["date"], exp["signature"])  # metadata from the first
    assert set(got) == {"date", "signature", "whitelists"}
    Whitelists(text)  # and the model reads it back


def test_omitted_fields_read_as_none_and_are_written_out():
    a = doc([wl("custom_whitelist", [{"domain": "a.com", "port": 80}])])
    b = doc([wl("custom_whitelist", [{"domain": "a.com", "port": 80, "ip": None, "description": "again"},
                                     {"domain": "a.com", "port": 80, "protocol": "TCP"}])])
    eps = json.loads(Whitelists.merge_custom_whitelists(a, b))["whitelists"][0]["endpoints"]
    # an omitted field is None: the second document's first endpoint has the first's fingerprint (the description
    # is no part of it) and goes; the first occurrence keeps its (absent) description
    assert eps == [{"domain": "a.com", "ip": None, "port": 80, "protocol": None, "as_number": None, "as_country": None,
                    "as_owner": None, "process": None, "description": None},
                   {"domain": "a.com", "ip": None, "port": 80, "protocol": "TCP", "as_number": None, "as_country": None,
                    "as_owner": None, "process": None, "description": None}]


def test_order_extends_and_per_list_dedup():
    e1, e2, e3 = {"ip": "1.1.1.1", "port": 1}, {"ip": "2.2.2.2", "port": 2}, {"ip": "3.3.3.3", "port": 3}
    a = doc([wl("x", [e1, e2], ["p"]), wl("y", [e1])], date="first", signature="sig")
    b = doc([wl("z", [e3]), wl("y", [e2, e1], ["q"]), wl("x", [e3, e1], ["other"])], date="second")
    got = json.loads(Whitelists.merge_custom_whitelists(a, b))
    lists = got["whitelists"]
    assert [i["name"] for i in lists] == ["x", "y", "z"]  # first appearance
    ips = lambda i: [e["ip"] for e in i["endpoints"]]
    assert ips(lists[0]) == ["1.1.1.1", "2.2.2.2", "3.3.3.3"]  # a's endpoints, then b's new ones
    assert ips(lists[1]) == ["1.1.1.1", "2.2.2.2"] and ips(lists[2]) == ["3.3.3.3"]  # the same endpoint in two lists stays in both
    assert [i["extends"] for i in lists] == [["p"], ["q"], None]  # the first source that has one
    assert (got["date"], got["signature"]) == ("first", "sig")


@pytest.mark.parametrize("bad", ["", "not json", "[]", "null", json.dumps({"date": "d", "whitelists": "x"}),
                                 json.dumps({"signature": None, "whitelists": []}),
                                 json.dumps({"date": "d", "signature": None, "whitelists": [], "extra": 1}),
                                 doc([{"name": "x", "endpoints": [], "color": "red"}]), doc([{"endpoints": []}]),
                                 doc([wl("x", [{"domain": "a.com", "prot": "TCP"}])])],
                         ids=["empty", "text", "array", "null", "lists-not-a-list", "no-date", "unknown-top-field",
                              "unknown-list-field", "no-name", "unknown-endpoint-field"])
def test_parse_failure_on_either_side(bad):
    good = doc([wl("custom_whitelist", [{"domain": "a.com", "port": 80}])])
    with pytest.raises(ValueError, match="first"):
        Whitelists.merge_custom_whitelists(bad, good)
    with pytest.raises(ValueError, match="second"):
        Whitelists.merge_custom_whitelists(good, bad)
    assert json.loads(Whitelists.merge_custom_whitelists(good, good))["whitelists"][0]["endpoints"][0]["domain"] == "a.com"
