"""Endpoint learning with the process in the fingerprint (fb_set_l7_process_names, fb_flow_learn_endpoints_dev;
DESIGN.md 3.19): flows that share (destination, port, protocol, domain) over several process names -- two process
ids of one name, "curl" / "CURL", and no process for unresolved, failed and unnamed ids -- against
Whitelists.new_from_sessions(..., process_names=...) and, byte for byte, against tests/learnref.py run once per
process name.  Without a name table the records are the bytes they were: reserved2 all zero."""
import collections

import numpy as np
import pytest

import learnref
import wlprocspace as W
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.l7 import ProcessNameInterner
from flodbadd_amd.sessions import Session, SessionFilter, flows_to_sessions
from flodbadd_amd.whitelists import Whitelists

pytestmark = pytest.mark.gpu


def world():
    """Per process state three sources to each of two destinations (one IPv6), and one destination only
    process-less flows reach."""
    flows = []
    for c, state in enumerate(W.FLOW_PROCS):
        for k in range(3):
            flows.append(W.Flow(W.TCP, "192.168.%d.%d" % (c + 1, 9 - k), 61000 + 8 * c + k, "8.8.8.8", 443, state))
            flows.append(W.Flow(W.TCP, "fd00::%x:%x" % (c + 1, 9 - k), 61100 + 8 * c + k, W.A6, 443, state))
    flows += [W.Flow(W.UDP, "192.168.9.%d" % (k + 1), 61200 + k, "9.9.9.9", 53, "unresolved") for k in range(2)]
    return W.World("learn", flows)


@pytest.fixture(scope="module")
def dev():
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9, service_bitmap=bytes(8192))
    w = world()
    slots = W.load_world(cap, w)
    yield cap, w, slots
    cap.close()


def set_names(cap, interner, n):
    m, v = W.name_table(interner, n)
    N.check(N.gpu_lib().fb_set_l7_process_names(cap.ctx, N.ptr(m) if n else None, N.ptr(v) if n else None, n))


def test_without_a_name_table_the_records_are_what_they_were(dev):
    cap, w, slots = dev
    set_names(cap, ProcessNameInterner(), 0)
    recs, st = cap.learn_endpoints()
    flows = cap.export_flows(SessionFilter.All)
    want = learnref.records(flows, cap.domain_ids()["dst_name_id"], None)
    assert recs.tobytes() == want.tobytes() and not recs["reserved2"].any() and not recs["reserved"].any()
    assert (st["selected"], st["endpoints"]) == (len(w.flows), 3)
    again, st2 = cap.learn_endpoints()
    assert again.tobytes() == recs.tobytes() and st2 == st


def test_process_in_the_fingerprint(dev):
    cap, w, slots = dev
    it = ProcessNameInterner()
    set_names(cap, it, W.N_NAMES)
    recs, st = cap.learn_endpoints()
    again, st2 = cap.learn_endpoints()
    assert again.tobytes() == recs.tobytes() and st2 == st  # two calls, identical bytes
    # byte for byte: learnref over the flows of each process name, the name's id written in, in slot order
    flows = cap.export_flows(SessionFilter.All)
    by_slot = {s: f for f, s in slots.items()}
    name_of = [w.process(by_slot[int(r["slot"])], W.N_NAMES) for r in flows]
    parts = []
    for name in (None, "curl", "CURL", "nginx"):
        part = learnref.records(flows, cap.domain_ids()["dst_name_id"], np.array([x == name for x in name_of]))
        part["reserved2"][:, 0] = 0 if name is None else it.name_id(name)
        parts.append(part)
    want = np.concatenate(parts)
    want = want[np.argsort(want["rep_slot"], kind="stable")]
    assert recs.tobytes() == want.tobytes()
    assert (np.diff(recs["rep_slot"].astype(np.int64)) > 0).all()  # slot order
    assert (st["selected"], st["endpoints"], st["written"]) == (len(w.flows), len(want), len(want))
    # per destination: curl (two process ids, one endpoint), CURL (its own endpoint), nginx, and no process
    pv = recs.view(N.LEARNED_ENDPOINT_PROC_DTYPE)
    google = [(it.names.get(int(r["proc_name_id"])), int(r["sessions"])) for r in pv if int(r["dst_ip"][0]) == 0x08080808]
    assert sorted(google, key=str) == sorted([("curl", 6), ("CURL", 3), ("nginx", 3), (None, 9)], key=str)
    assert len(recs) == 9 and int(recs["sessions"].sum()) == len(w.flows)
    # against the reference's own loop: endpoints, representatives (the descriptions) and counts
    sessions = flows_to_sessions(flows)
    names = {Session.from_key(r): n for r, n in zip(flows, name_of) if n is not None}
    ref = Whitelists.new_from_sessions(sessions, None, names).whitelists["custom_whitelist"].endpoints
    got = Whitelists.from_learned(recs, None, it.names).whitelists["custom_whitelist"].endpoints
    assert sorted(((e.fingerprint(), e.description) for e in got), key=repr) == \
        sorted(((e.fingerprint(), e.description) for e in ref), key=repr)
    count = collections.Counter((str(i.session.dst_ip), i.session.dst_port, i.session.protocol.name, names.get(i.session))
                                for i in sessions)
    assert {(e.ip, e.port, e.protocol, e.process): int(r["sessions"]) for e, r in zip(got, recs)} == dict(count)
    # a name table of two entries names process 1 alone: every other flow is process-less
    set_names(cap, it, 2)
    small, _ = cap.learn_endpoints()
    assert sorted(small.view(N.LEARNED_ENDPOINT_PROC_DTYPE)["proc_name_id"].tolist()) == [0, 0, 0, 1, 1]
    set_names(cap, it, 0)
