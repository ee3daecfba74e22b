"""tests/domref.py (populate_domain_names restated, src/capture.rs:1307-1411) against the known answers of
tests/golden/domain_kats.json: the reference's own test_populate_domain_names transcribed as data (case 0,
pinned), the rest hand-derived from the code (restated, not reference-pinned)."""
import ipaddress
import json
import os

import pytest

import domref

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "domain_kats.json")))["cases"]


def run_case(case, now=7):
    sessions, current = {}, []
    for k, (proto, sip, sport, dip, dport, cur, sdom, ddom) in enumerate(case["sessions"]):
        sessions[k] = {"src_ip": ipaddress.ip_address(sip), "dst_ip": ipaddress.ip_address(dip), "src_domain": sdom,
                       "dst_domain": ddom, "last_modified": 0}
        if cur:
            current.append(k)
    res = {ipaddress.ip_address(ip): name for ip, name in case["resolutions"].items()}
    modified = domref.populate_domain_names(sessions, current, res, now=now)
    return sessions, modified


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_known_answers(case):
    sessions, modified = run_case(case)
    for k, (sdom, ddom, mod) in enumerate(case["expect"]):
        assert (sessions[k]["src_domain"], sessions[k]["dst_domain"]) == (sdom, ddom), k
        assert (k in modified) == mod and sessions[k]["last_modified"] == (7 if mod else 0), k


def test_fixture_shape():
    assert KATS[0]["pinned"] and KATS[0]["name"] == "reference_test_populate_domain_names"
    assert KATS[0]["sessions"] == [["TCP", "192.168.1.1", 12345, "8.8.8.8", 80, True, None, None]]
    assert KATS[0]["resolutions"] == {"8.8.8.8": "dns.google"} and KATS[0]["expect"] == [[None, "dns.google", True]]
    assert not any(c["pinned"] for c in KATS[1:])


def test_a_second_pass_changes_nothing():
    for case in KATS:
        sessions, _ = run_case(case)
        cur = [k for k, s in enumerate(case["sessions"]) if s[5]]
        res = {ipaddress.ip_address(ip): name for ip, name in case["resolutions"].items()}
        assert domref.populate_domain_names(sessions, cur, res, now=9) == []


def test_current_predicate():
    assert domref.is_current(0) and domref.is_current(16 | 128) and not domref.is_current(128) and not domref.is_current(1 | 128)
