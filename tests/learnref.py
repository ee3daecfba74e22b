"""Plain-Python restatement of the endpoint learning pass (fb_flow_learn_endpoints_dev) over exported arrays:
flow records, the domain-id plane and a selection mask in; the distinct endpoints, each with its least
session and the number of its flows, out.

  learn(flows, dom, mask)    the sorted list of (fingerprint, representative, count):
                               fingerprint    (family, dst_ip words, dst_port, protocol, dst name id)
                               representative (src_ip words, src_port, slot) of the group's least session under
                                              Session's derived Ord -- inside a group protocol and destination are
                                              equal, so the order of (src_ip, src_port); sources of one group have
                                              one family, and the words compare as the addresses do
  records(flows, dom, mask)  the same as the LEARNED_ENDPOINT_DTYPE array the device writes: ascending rep_slot
  endpoints(result, names)   ... as WhitelistEndpoint field dicts, for the comparison with new_from_sessions
"""
import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.sessions import words_to_ip


def learn(flows, dom=None, mask=None):
    groups = {}
    for k, r in enumerate(flows):
        if mask is not None and not mask[k]:
            continue
        slot = int(r["slot"])
        fp = (int(r["family"]), tuple(int(w) for w in r["dst_ip"]), int(r["dst_port"]), int(r["protocol"]),
              int(dom[slot]) if dom is not None else 0)
        rep = (tuple(int(w) for w in r["src_ip"]), int(r["src_port"]), slot)
        g = groups.setdefault(fp, [rep, 0])
        if rep[:2] < g[0][:2]:
            g[0] = rep
        g[1] += 1
    return sorted((fp, g[0], g[1]) for fp, g in groups.items())


def records(flows, dom=None, mask=None):
    res = sorted(learn(flows, dom, mask), key=lambda t: t[1][2])
    out = np.zeros(len(res), dtype=N.LEARNED_ENDPOINT_DTYPE)
    for o, ((fam, dst, dport, proto, nid), (src, sport, slot), cnt) in zip(out, res):
        o["dst_ip"], o["rep_src_ip"], o["dst_port"], o["rep_src_port"] = dst, src, dport, sport
        o["protocol"], o["family"], o["dst_name_id"], o["rep_slot"], o["sessions"] = proto, fam, nid, slot, cnt
    return out


def endpoints(result, names=None):
    out = []
    for (fam, dst, dport, proto, nid), (src, sport, _), _ in result:
        d = words_to_ip(dst, fam)
        out.append({"domain": (names or {})[nid] if nid else None, "ip": str(d), "port": dport,
                    "protocol": {6: "TCP", 17: "UDP"}[proto], "as_number": None, "as_country": None, "as_owner": None,
                    "process": None,
                    "description": "Auto-generated from session: %s:%d -> %s:%d" % (words_to_ip(src, fam), sport, d, dport)})
    return out
