"""tests/learnref.py -- the restatement the GPU learning tests compare the device with -- against
Whitelists.new_from_sessions (src/whitelists.rs:103-177) fed the sessions in Session's derived Ord: the first
occurrence of a fingerprint is then the group's least session, so both must give the same endpoints field for
field, descriptions included.  No GPU: the flow records are made here, at shuffled slots."""
import ipaddress
import json
import random
from dataclasses import asdict

import numpy as np
import pytest

import learncorpus as LC
import learnref
from flodbadd_amd import _native as N
from flodbadd_amd.sessions import Protocol, Session, SessionInfo
from flodbadd_amd.whitelists import Whitelists


def world(name):
    """The corpus as (sessions, flow records at shuffled slots, the dst name id per slot, {id: name}, {ip: domain})."""
    corpus = LC.ALL[name]()
    dns = LC.dns_for(corpus)
    ids = {n: k + 1 for k, n in enumerate(sorted(set(dns.values()) - {"Unknown", "Resolving"}))}
    sessions = [Session(Protocol[p], ipaddress.ip_address(s), sp, ipaddress.ip_address(d), dp) for p, s, sp, d, dp in corpus]
    assert len(set(sessions)) == len(sessions)
    slots = list(range(2 * len(sessions) + 3))
    random.Random(len(sessions)).shuffle(slots)
    flows = np.zeros(len(sessions), dtype=N.FLOW_REC_DTYPE)
    dom = np.zeros(len(slots), dtype=np.uint32)
    for r, s, slot in zip(flows, sessions, slots):
        r["src_ip"], r["dst_ip"], r["family"] = s.key_fields()
        r["src_port"], r["dst_port"], r["protocol"], r["slot"] = s.src_port, s.dst_port, int(s.protocol), slot
        dom[slot] = ids.get(dns.get(str(s.dst_ip)), 0)
    return sessions, flows, dom, {v: k for k, v in ids.items()}, dns


def by_fingerprint(eps):
    return sorted(eps, key=lambda e: json.dumps([e[f] for f in e if f != "description"]))


@pytest.mark.parametrize("name", sorted(LC.ALL))
def test_learnref_equals_new_from_sessions(name):
    sessions, flows, dom, names, dns = world(name)
    res = learnref.learn(flows, dom)
    ordered = [SessionInfo(session=s) for s in sorted(sessions, key=Session.sort_key)]
    want = Whitelists.new_from_sessions(ordered, dns).whitelists["custom_whitelist"].endpoints
    assert by_fingerprint(learnref.endpoints(res, names)) == by_fingerprint([asdict(e) for e in want])
    assert sum(c for _, _, c in res) == len(sessions)
    # a selection mask: the restatement over the selected flows alone
    mask = np.arange(len(flows)) % 3 != 1
    sub = learnref.learn(flows, dom, mask)
    ordered = [SessionInfo(session=s) for s in sorted((s for s, m in zip(sessions, mask) if m), key=Session.sort_key)]
    want = Whitelists.new_from_sessions(ordered, dns).whitelists["custom_whitelist"].endpoints
    assert by_fingerprint(learnref.endpoints(sub, names)) == by_fingerprint([asdict(e) for e in want])


def test_records_are_in_ascending_rep_slot_order():
    _, flows, dom, _, _ = world("representatives")
    recs = learnref.records(flows, dom)
    assert len(recs) == len(learnref.learn(flows, dom)) and (np.diff(recs["rep_slot"].astype(np.int64)) > 0).all()
    assert int(recs["sessions"].sum()) == len(flows)


@pytest.mark.parametrize("name", ["one_field_apart", "representatives", "mixed_local"])
def test_from_learned_round_trips(name):
    _, flows, dom, names, _ = world(name)
    recs = learnref.records(flows, dom)
    w = Whitelists.from_learned(recs, names)
    info = w.whitelists["custom_whitelist"]
    assert list(w.whitelists) == ["custom_whitelist"] and info.extends is None and w.signature is None
    res = sorted(learnref.learn(flows, dom), key=lambda t: t[1][2])
    assert [asdict(e) for e in info.endpoints] == learnref.endpoints(res, names)  # the records' order
    for text in (w.to_json(), w.to_json(compact=True)):
        back = Whitelists(text)
        assert back.to_dict() == w.to_dict()
    assert "\n" in w.to_json() and "\n" not in w.to_json(compact=True) and '{"date":"' in w.to_json(compact=True)
    day = w.date.split()  # "%B %dth %Y"
    assert len(day) == 3 and day[1].endswith("th") and len(day[1]) == 4 and day[2].isdigit()
