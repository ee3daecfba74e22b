"""Parsed DNS batches for the tracker tests, built as fb_dns_parse_dev leaves them (fb_dns_msg, names,
answers), and the comparison of a tracking call with DnsResolver.process over the same arrays."""
import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.dns import DnsResolver
from flodbadd_amd.sessions import ip_to_words


class Batch:
    """Messages in packet order.  garbage: the byte the name row is filled with past name_len (the parse
    leaves those bytes unspecified)."""

    def __init__(self):
        self.rows = []

    def _add(self, tx, flags, name=b"", addrs=(), status=0, garbage=0):
        name = name.encode("ascii") if isinstance(name, str) else bytes(name)
        self.rows.append((tx, flags, name, list(addrs), status, garbage))
        return self

    def query(self, tx, name, garbage=0):
        return self._add(tx, N.DNS_QUERY | N.DNS_HAS_QUESTION, name, garbage=garbage)

    def reverse(self, tx, name="4.3.2.1.in-addr.arpa"):
        return self._add(tx, N.DNS_QUERY | N.DNS_HAS_QUESTION | N.DNS_REVERSE, name)

    def no_question(self, tx):
        return self._add(tx, N.DNS_QUERY)

    def response(self, tx, addrs=(), name=b"", garbage=0):
        return self._add(tx, N.DNS_HAS_QUESTION if name else 0, name, addrs, garbage=garbage)

    def rejected(self, tx, status=2, query=True, name=b"bad.example", addrs=()):
        return self._add(tx, (N.DNS_QUERY if query else 0) | N.DNS_HAS_QUESTION, name, addrs, status=status)

    def arrays(self):
        n = len(self.rows)
        msgs = np.zeros(n, dtype=N.DNS_MSG_DTYPE)
        names = np.zeros((n, N.FB_DNS_MAX_NAME), dtype=np.uint8)
        addrs = np.zeros((n, N.FB_DNS_MAX_ADDRS), dtype=N.FB_IP_DTYPE)
        for i, (tx, flags, name, ads, status, garbage) in enumerate(self.rows):
            assert len(name) < N.FB_DNS_MAX_NAME and len(ads) <= N.FB_DNS_MAX_ADDRS
            msgs[i]["pkt_index"], msgs[i]["id"], msgs[i]["status"], msgs[i]["flags"] = i, tx, status, flags
            msgs[i]["questions"], msgs[i]["answers"] = 1 if name else 0, len(ads)
            msgs[i]["name_len"], msgs[i]["n_addrs"] = len(name), len(ads)
            names[i, :] = garbage
            names[i, : len(name)] = np.frombuffer(name, dtype=np.uint8)
            for j, ip in enumerate(ads):
                w, fam = ip_to_words(ip)
                addrs[i, j]["addr"], addrs[i, j]["family"] = w, fam
        return msgs, names, addrs


def track(cap, msgs, names, addrs, ts=None, n_dns=None):
    """One fb_dns_track_dev call over host arrays; returns its counters with "taken"."""
    n = len(msgs)
    d_msg = N.DeviceBuffer(max(msgs.nbytes, 16))
    d_names = N.DeviceBuffer(max(names.nbytes, 16))
    d_addrs = N.DeviceBuffer(max(addrs.nbytes, 32))
    if n:
        d_msg.upload(msgs)
        d_names.upload(names)
        d_addrs.upload(addrs)
    d_ts = N.DeviceBuffer(max(n, 1) * 8).upload(np.ascontiguousarray(ts, dtype=np.uint64)) if ts is not None else None
    d_st = None
    if n_dns is not None:
        st = np.zeros(1, dtype=N.STATS_DTYPE)
        st[0]["n_dns"] = n_dns
        d_st = N.DeviceBuffer(st.nbytes).upload(st)
    return cap.track_dns_parsed_dev(d_msg, d_names, d_addrs, n, d_stats=d_st, d_ts=d_ts, want_taken=True)


def reference_step(ref, msgs, names, addrs, n_dns=None):
    """DnsResolver.process over the same arrays, one message at a time so that the name each response took
    is known: returns the list of taken names (None: none, or no response)."""
    taken = []
    cnt = len(msgs) if n_dns is None else min(n_dns, len(msgs))
    for i in range(len(msgs)):
        m = msgs[i]
        is_resp = i < cnt and int(m["status"]) == 0 and not int(m["flags"]) & N.DNS_QUERY
        taken.append(ref.pending.get(int(m["id"])) if is_resp else None)
        if i < cnt:
            ref.process(msgs[i: i + 1], names[i: i + 1], addrs[i: i + 1])
    return taken


def check_state(cap, ref):
    assert cap.dns_pending() == ref.pending
    assert cap.dns_resolutions() == ref.resolutions


def step(cap, ref, batch, ts=None, n_dns=None):
    """Track a batch (a Batch or the three arrays) on the device and in `ref`; compare pending, resolutions
    and d_taken; returns the call's counters."""
    msgs, names, addrs = batch.arrays() if isinstance(batch, Batch) else batch
    out = track(cap, msgs, names, addrs, ts=ts, n_dns=n_dns)
    want = reference_step(ref, msgs, names, addrs, n_dns=n_dns)
    ids = out["taken"]
    got_names = cap.dns_names(ids)
    got = [got_names[int(i)] if int(i) else None for i in ids]
    assert got == want
    check_state(cap, ref)
    return out


def new_capture(**kw):
    from flodbadd_amd.capture import FlodbaddGpuCapture
    from flodbadd_amd.sessions import SessionFilter
    kw.setdefault("flow_capacity", 0)
    kw.setdefault("dns_name_capacity", 1024)
    kw.setdefault("dns_addr_capacity", 4096)
    return FlodbaddGpuCapture(0, session_filter=SessionFilter.All, track_dns=True, **kw), DnsResolver()
