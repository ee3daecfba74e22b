"""Host side of the new-session enrichment: the reference's table loaders
restated for the C ABI's fb_asn_range / fb_cidr tables, and the capture-level calls.

  asn_tables_from_tsv   Db::from_tsv (src/asn_db.rs:82-140): IPtoASN TSV rows
                        `range_start range_end as_number country owner`; rows with < 5 fields or
                        owner "Not routed" / "None" skipped, mismatched families or start > end
                        skipped (the sort happens in fb_set_asn_tables, stable like Vec::sort).
  blacklists_from_json  Blacklists::new_from_json (src/blacklists.rs:111-186): a plain IP becomes
                        /32 or /128, unparsable ranges are skipped, and with filter_local_ranges
                        a range entirely inside a known local range is dropped
                        (is_range_local_to_filter, src/blacklists.rs:70-105).
  Blacklists            the BlacklistsJSON model behind set_custom_blacklists / get_blacklists
                        (src/blacklists.rs:20-36, 782-815): date, signature and the lists.
  criticality_of        a flow's blacklist mask as the reference's criticality string
                        (src/blacklists.rs:608-631).
"""
import ipaddress
import json

import numpy as np

from . import _native as N
from .sessions import ip_to_words

LOCAL_V4_TO_FILTER = [ipaddress.ip_network(x) for x in ("0.0.0.0/8", "10.0.0.0/8", "127.0.0.0/8", "169.254.0.0/16",
                                                        "172.16.0.0/12", "192.168.0.0/16")]
LOCAL_V6_TO_FILTER = [ipaddress.ip_network(x) for x in ("::/128", "::1/128", "fc00::/7", "fe80::/10")]


def asn_tables_from_tsv(text):
    """-> (v4 ASN_RANGE_DTYPE array, v6 array, records [(as_number, country, owner)]), file order."""
    v4, v6, recs = [], [], []
    for line in text.splitlines():
        f = line.split("\t")
        if len(f) < 5:
            continue
        owner = f[4]
        if owner in ("Not routed", "None"):
            continue
        a, b = ipaddress.ip_address(f[0]), ipaddress.ip_address(f[1])  # parse errors abort, like `?`
        asn = int(f[2])
        if a.version != b.version or a > b:
            continue
        r = np.zeros(1, dtype=N.ASN_RANGE_DTYPE)[0]
        r["start"] = ip_to_words(a)[0]
        r["end"] = ip_to_words(b)[0]
        r["as_number"] = asn
        r["record"] = len(recs)
        recs.append((asn, f[3], owner))
        (v4 if a.version == 4 else v6).append(r)
    mk = lambda rows: np.array(rows, dtype=N.ASN_RANGE_DTYPE) if rows else np.zeros(0, dtype=N.ASN_RANGE_DTYPE)
    return mk(v4), mk(v6), recs


def _is_range_local(net):
    return any(net.version == l.version and net.subnet_of(l)
               for l in (LOCAL_V4_TO_FILTER if net.version == 4 else LOCAL_V6_TO_FILTER))


def blacklists_from_json(obj, filter_local_ranges=False):
    """{"blacklists": [{"name": ..., "ip_ranges": [...]}, ...]} -> (CIDR_DTYPE array, [names])."""
    names, rows = [], []
    for info in obj["blacklists"]:
        if len(names) >= N.FB_MAX_BLACKLISTS:
            raise ValueError("at most %d blacklists" % N.FB_MAX_BLACKLISTS)
        lid = len(names)
        names.append(info["name"])
        for s in info.get("ip_ranges", []):
            try:
                ip = ipaddress.ip_address(s)
                s = "%s/%d" % (s, 32 if ip.version == 4 else 128)
            except ValueError:
                pass
            try:
                net = ipaddress.ip_network(s, strict=False)
                addr = ipaddress.ip_address(s.split("/")[0])
            except ValueError:
                continue  # "Failed to parse IP range" (src/blacklists.rs:151-157)
            if filter_local_ranges and _is_range_local(net):
                continue
            r = np.zeros(1, dtype=N.CIDR_DTYPE)[0]
            r["addr"], r["family"] = ip_to_words(addr)
            r["prefix"] = net.prefixlen
            r["list"] = lid
            rows.append(r)
    arr = np.array(rows, dtype=N.CIDR_DTYPE) if rows else np.zeros(0, dtype=N.CIDR_DTYPE)
    return arr, names


def mask_names(mask, names):
    """The list names of a blacklist bit mask (is_ip_blacklisted's Vec<String>)."""
    return [n for i, n in enumerate(names) if (int(mask) >> i) & 1]


def criticality_of(mask, names):
    """SessionInfo.criticality of a blacklist mask: the matching names sorted and de-duplicated, as
    "blacklist:<name>" tags, sorted and de-duplicated again, joined by "," (src/blacklists.rs:608-631;
    there are no non-blacklist tags to keep: the analyzer is not part of this package)."""
    if not int(mask):
        return ""
    return ",".join(sorted({"blacklist:" + n for n in mask_names(mask, names)}))


class Blacklists:
    """The custom blacklist model (BlacklistsJSON, src/blacklists.rs:20-36): parsed with the
    reference's strictness -- `date`, `signature`, `blacklists` required, each list a `name` and
    `ip_ranges` plus optional description / last_updated / source_url, unknown fields refused
    (deny_unknown_fields) -- and flattened for fb_set_blacklists WITHOUT the local-range filter, as
    set_custom_blacklists does (Blacklists::new_from_json(json, false), src/blacklists.rs:790-800).
    The reference keeps the lists in a map by name: a repeated name replaces the earlier list."""
    _INFO_REQUIRED = ("name", "ip_ranges")
    _INFO_OPTIONAL = ("description", "last_updated", "source_url")

    def __init__(self, doc=None):
        self.date, self.signature, self.infos = "", "", []
        self.cidrs, self.names = np.zeros(0, dtype=N.CIDR_DTYPE), []
        if doc is None or doc == "":
            return
        obj = json.loads(doc) if isinstance(doc, (str, bytes)) else doc
        if not isinstance(obj, dict) or set(obj) != {"date", "signature", "blacklists"}:
            raise ValueError("BlacklistsJSON needs exactly date, signature and blacklists")
        if not isinstance(obj["date"], str) or not isinstance(obj["signature"], str) or \
                not isinstance(obj["blacklists"], list):
            raise ValueError("BlacklistsJSON: date and signature are strings, blacklists a list")
        by_name = {}
        for info in obj["blacklists"]:
            if not isinstance(info, dict) or any(k not in info for k in self._INFO_REQUIRED) or \
                    any(k not in self._INFO_REQUIRED + self._INFO_OPTIONAL for k in info):
                raise ValueError("BlacklistInfo: missing or unknown field")
            if not isinstance(info["name"], str) or not isinstance(info["ip_ranges"], list) or \
                    not all(isinstance(x, str) for x in info["ip_ranges"]) or \
                    not all(info.get(k) is None or isinstance(info[k], str) for k in self._INFO_OPTIONAL):
                raise ValueError("BlacklistInfo: bad field type")
            by_name[info["name"]] = dict(info)
        self.date, self.signature, self.infos = obj["date"], obj["signature"], list(by_name.values())
        self.cidrs, self.names = blacklists_from_json({"blacklists": self.infos}, filter_local_ranges=False)

    def to_json(self):
        """get_blacklists (src/blacklists.rs:802-815): the model as BlacklistsJSON text."""
        infos = [{"name": i["name"], "description": i.get("description"), "last_updated": i.get("last_updated"),
                  "source_url": i.get("source_url"), "ip_ranges": list(i["ip_ranges"])} for i in self.infos]
        return json.dumps({"date": self.date, "signature": self.signature, "blacklists": infos})
