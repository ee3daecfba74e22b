"""Host side of the whitelist conformance pass (src/whitelists.rs).

  Whitelists              the WhitelistsJSON model (src/whitelists.rs:22-57): named lists of endpoints that
                          may extend each other; get_all_endpoints flattens one (180-211),
                          new_from_sessions learns one from a session list (103-177).  There are no
                          built-in lists: the reference's default database is not part of this package.
  Whitelists.from_learned the same list from the distinct endpoints the device found (fb_flow_learn_endpoints_dev);
  Whitelists.merge_custom_whitelists  two documents merged by list name (223-299).
  Whitelists.compile      the flattened list as fb_wl_endpoint rows for fb_set_whitelist.  The device
                          sees neither a session's dst_domain nor its process, so the domains the host
                          has resolved are expanded here: dst_domain is a function of dst_ip, hence a
                          domain endpoint whose pattern matches the domain of a resolved address equals
                          an exact-address endpoint for that address.
  endpoint_matches        the full endpoint_matches_with_reason (453-599), with domain and process, for
                          the flows the device marks FB_WL_HOST_CHECK; is_session_in_whitelist builds
                          the reference's whitelist_reason strings (413-449).
"""
import ipaddress
import json
import logging
import time
from dataclasses import asdict, dataclass, field
from typing import List, Optional

import numpy as np

from . import _native as N
from .sessions import ip_to_words, words_to_ip

log = logging.getLogger(__name__)

ENDPOINT_FIELDS = ("domain", "ip", "port", "protocol", "as_number", "as_country", "as_owner", "process", "description")


@dataclass
class WhitelistEndpoint:
    """src/whitelists.rs:24-34."""
    domain: Optional[str] = None
    ip: Optional[str] = None
    port: Optional[int] = None
    protocol: Optional[str] = None
    as_number: Optional[int] = None
    as_country: Optional[str] = None
    as_owner: Optional[str] = None
    process: Optional[str] = None
    description: Optional[str] = None

    @staticmethod
    def from_dict(d):
        unknown = set(d) - set(ENDPOINT_FIELDS)
        if unknown:  # serde(deny_unknown_fields)
            raise ValueError("unknown endpoint field(s): %s" % ", ".join(sorted(unknown)))
        return WhitelistEndpoint(**d)

    def fingerprint(self):
        """The de-duplication key of new_from_sessions (src/whitelists.rs:144-153): all but description."""
        return (self.domain, self.ip, self.port, self.protocol, self.as_number, self.as_country, self.as_owner,
                self.process)


@dataclass
class WhitelistInfo:
    """src/whitelists.rs:38-42."""
    name: str
    extends: Optional[List[str]] = None
    endpoints: List[WhitelistEndpoint] = field(default_factory=list)


def dedup_endpoints(endpoints):
    """The endpoints without those whose fingerprint an earlier one has (the first occurrence stays)."""
    seen, out = set(), []
    for ep in endpoints:
        if ep.fingerprint() not in seen:
            seen.add(ep.fingerprint())
            out.append(ep)
    return out


def ascii_lower(s):
    """Lower-case A-Z only: two strings are eq_ignore_ascii_case iff their ascii_lower are equal."""
    return "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in s)


def rust_debug(v):
    """Rust's {:?} of an Option<&str> / Option<u32>: None, Some("x"), Some(5)."""
    if v is None:
        return "None"
    if isinstance(v, str):
        esc = v.replace("\\", "\\\\").replace('"', '\\"').replace("\n", "\\n").replace("\r", "\\r").replace("\t", "\\t")
        return 'Some("%s")' % esc
    return "Some(%d)" % int(v)


def parse_ip(s):
    """str::parse::<IpAddr>: an address and nothing else (no zone id), or None."""
    if "%" in s or "/" in s:
        return None
    try:
        return ipaddress.ip_address(s)
    except ValueError:
        return None


def parse_net(s):
    """str::parse::<IpNet> (ipnet): address '/' decimal prefix length, host bits allowed, or None."""
    addr, _, pfx = s.partition("/")
    ip = parse_ip(addr)
    if ip is None or not pfx.isascii() or not pfx.isdigit() or len(pfx) > 3:
        return None
    if int(pfx) > (32 if ip.version == 4 else 128):
        return None
    return ipaddress.ip_network("%s/%d" % (ip, int(pfx)), strict=False)


def domain_matches(session_domain, pattern):
    """src/whitelists.rs:602-679."""
    if pattern is None:
        return True
    if session_domain is None:
        return False
    domain, pattern = session_domain.lower(), pattern.lower()
    if "*" in pattern:
        if pattern.startswith("*."):  # *.example.com: a subdomain, not the suffix itself
            suffix = pattern[2:]
            if domain == suffix:
                return False
            return domain.endswith(suffix) and len(domain) > len(suffix) and domain[len(domain) - len(suffix) - 1] == "."
        if pattern.endswith(".*"):    # example.*: the prefix alone, or followed by a dot
            prefix = pattern[:-2]
            if domain.startswith(prefix):
                if len(domain) == len(prefix):
                    return True
                if domain[len(prefix)] == ".":
                    return True
            return False
        parts = pattern.split("*")
        if len(parts) == 2:           # a*b
            return domain.startswith(parts[0]) and domain.endswith(parts[1]) and len(domain) > len(parts[0]) + len(parts[1])
        return False
    return domain == pattern


def classify_domain_pattern(pattern):
    """The kind of a lower-cased pattern as domain_matches tells them apart, in its order: "exact" (no '*'),
    "suffix" ("*.s"), "prefix" ("q.*"), "general" (one '*': a*b) or "never" -- what fb_set_whitelist_dom
    classifies the pattern's bytes as."""
    if "*" not in pattern:
        return "exact"
    if pattern.startswith("*."):
        return "suffix"
    if pattern.endswith(".*"):
        return "prefix"
    return "general" if pattern.count("*") == 1 else "never"


def ip_matches(session_ip, pattern):
    """src/whitelists.rs:682-709."""
    if pattern is None:
        return True
    if session_ip is None:
        return False
    ip = parse_ip(str(session_ip))
    if ip is None:
        return False
    if "/" in pattern:
        net = parse_net(pattern)
        return net is not None and net.version == ip.version and ip in net
    p = parse_ip(pattern)
    return p is not None and p == ip


def endpoint_matches(ep, session_domain, session_ip, port, protocol, as_number=None, as_country=None, as_owner=None,
                     process=None):
    """endpoint_matches_with_reason (src/whitelists.rs:453-599) -> (matches, reason)."""
    protocol_match = ep.protocol is None or ascii_lower(protocol) == ascii_lower(ep.protocol)
    port_match = ep.port is None or ep.port == port
    process_match = ep.process is None or (process is not None and ascii_lower(process) == ascii_lower(ep.process))
    if not (protocol_match and port_match and process_match):
        reasons = []
        if not protocol_match:
            reasons.append("Protocol mismatch: %s not matching %s" % (protocol, rust_debug(ep.protocol)))
        if not port_match:
            reasons.append("Port mismatch: %d not matching %s" % (port, rust_debug(ep.port)))
        if not process_match:
            reasons.append("Process mismatch: %s not matching %s" % (rust_debug(process), rust_debug(ep.process)))
        return False, ", ".join(reasons)
    domain_specified, ip_specified = ep.domain is not None, ep.ip is not None
    if domain_specified and domain_matches(session_domain, ep.domain):
        return True, None
    if ip_specified and ip_matches(session_ip, ep.ip):
        return True, None
    if domain_specified or ip_specified:
        reasons = []
        if domain_specified:
            reasons.append("Domain mismatch: %s not matching %s" % (rust_debug(session_domain), rust_debug(ep.domain)))
        if ip_specified:
            reasons.append("IP mismatch: %s not matching %s" % (rust_debug(session_ip), rust_debug(ep.ip)))
        return False, ", ".join(reasons)
    if ep.as_number is not None and as_number != ep.as_number:
        return False, "AS number mismatch: %s not matching %s" % (rust_debug(as_number), rust_debug(ep.as_number))
    if ep.as_owner is not None and (as_owner is None or ascii_lower(as_owner) != ascii_lower(ep.as_owner)):
        return False, "Owner mismatch: %s not matching %s" % (rust_debug(as_owner), rust_debug(ep.as_owner))
    if ep.as_country is not None and (as_country is None or ascii_lower(as_country) != ascii_lower(ep.as_country)):
        return False, "Country mismatch: %s not matching %s" % (rust_debug(as_country), rust_debug(ep.as_country))
    return True, None


def is_session_in_whitelist(endpoints, whitelist_name, session_domain, session_ip, port, protocol, as_number=None,
                            as_country=None, as_owner=None, process=None):
    """is_session_in_whitelist (src/whitelists.rs:341-450) over an already flattened list."""
    for ep in endpoints:
        if endpoint_matches(ep, session_domain, session_ip, port, protocol, as_number, as_country, as_owner, process)[0]:
            return True, None
    return False, no_match_reason(endpoints, whitelist_name, session_domain, session_ip, port, protocol, as_number,
                                  as_country, as_owner, process)


def no_match_reason(endpoints, whitelist_name, session_domain, session_ip, port, protocol, as_number=None,
                    as_country=None, as_owner=None, process=None):
    """The whitelist_reason of a session no endpoint matches (src/whitelists.rs:413-421, 444-447)."""
    if not endpoints:
        return "Whitelist '%s' contains no endpoints" % whitelist_name
    return ("No matching endpoint found in whitelist '%s' for domain: %s, ip: %s, port: %d, protocol: %s, "
            "ASN: %s, country: %s, owner: %s, process: %s"
            % (whitelist_name, rust_debug(session_domain), rust_debug(session_ip), port, protocol,
               rust_debug(as_number), rust_debug(as_country), rust_debug(as_owner), rust_debug(process)))


@dataclass
class CompiledWhitelist:
    """Whitelists.compile's result: the fb_set_whitelist arguments and the list they were made from."""
    name: str
    endpoints: List[WhitelistEndpoint]  # flattened (get_all_endpoints), without the expansion
    rows: np.ndarray                    # WL_ENDPOINT_DTYPE
    rec_owner_id: np.ndarray            # uint32 per ASN record
    rec_country_id: np.ndarray
    strings: dict                       # lower-cased string -> id
    # compile(domain_patterns=True), the further fb_set_whitelist_dom arguments: the distinct lower-cased domain
    # patterns (id = index + 1), their UTF-8 bytes and offsets, and the pattern id of every row (0: none)
    patterns: Optional[List[str]] = None
    ep_pattern: Optional[np.ndarray] = None
    pattern_bytes: Optional[np.ndarray] = None
    pattern_off: Optional[np.ndarray] = None


def _ip_fields(row, text):
    """`ip` -> (addr, family, prefix); a string that does not parse -> family FB_WL_NEVER."""
    net = parse_net(text) if "/" in text else None
    ip = None if "/" in text else parse_ip(text)
    if net is None and ip is None:
        row["family"] = N.FB_WL_NEVER
        return
    if net is not None:
        ip, pfx = parse_ip(text.partition("/")[0]), net.prefixlen  # the address as written: host bits kept
    else:
        pfx = 32 if ip.version == 4 else 128
    row["addr"], row["family"] = ip_to_words(ip)
    row["prefix"] = pfx


class Whitelists:
    """The WhitelistsJSON model: {"date", "signature", "whitelists": [{"name", "extends", "endpoints"}]}."""

    def __init__(self, data=None):
        if isinstance(data, (str, bytes)):
            data = json.loads(data)
        data = data or {"date": "", "signature": None, "whitelists": []}
        unknown = set(data) - {"date", "signature", "whitelists"}
        if unknown or "date" not in data or "whitelists" not in data:
            raise ValueError("not a WhitelistsJSON object")
        self.date = data["date"]
        self.signature = data.get("signature")
        self.whitelists = {}
        for info in data["whitelists"]:
            if set(info) - {"name", "extends", "endpoints"} or "name" not in info or "endpoints" not in info:
                raise ValueError("not a WhitelistInfo object")
            self.whitelists[info["name"]] = WhitelistInfo(
                info["name"], None if info.get("extends") is None else list(info["extends"]),
                [WhitelistEndpoint.from_dict(e) for e in info["endpoints"]])

    def to_dict(self):
        return {"date": self.date, "signature": self.signature,
                "whitelists": [{"name": w.name, "extends": w.extends, "endpoints": [asdict(e) for e in w.endpoints]}
                               for w in self.whitelists.values()]}

    def to_json(self, compact=False):
        """Pretty-printed (serde_json::to_string_pretty), or compact (to_string)."""
        return json.dumps(self.to_dict(), separators=(",", ":")) if compact else json.dumps(self.to_dict(), indent=2)

    def _flatten(self, name, visited):
        info = self.whitelists.get(name)
        if info is None:
            raise KeyError("Whitelist not found: %s" % name)
        out = list(info.endpoints)  # own endpoints first, then each unvisited parent, depth first
        for parent in info.extends or []:
            if parent not in visited:
                visited.add(parent)
                out.extend(self._flatten(parent, visited))
        return out

    def get_all_endpoints(self, name):
        """src/whitelists.rs:180-211 as is_session_in_whitelist calls it (365-396): the visited set
        starts with the list itself, and an unknown name (the list's, or a parent's) gives an empty
        list with a warning."""
        try:
            return self._flatten(name, {name})
        except KeyError as e:
            log.warning("Error retrieving endpoints for whitelist '%s': %s", name, e.args[0])
            return []

    @staticmethod
    def new_from_sessions(sessions, dns_resolutions=None, process_names=None):
        """src/whitelists.rs:103-177: one endpoint per session -- its domain unless "Unknown" /
        "Resolving", always ip, port and protocol, no AS fields, the process when known -- de-duplicated
        by fingerprint, in a list named custom_whitelist.  dns_resolutions {ip: domain} and
        process_names {Session: name} stand for SessionInfo.dst_domain / l7."""
        w = Whitelists()
        endpoints, seen = [], set()
        for info in sessions:  # (de-duplicated as it goes: a table-sized list has millions of sessions)
            s = info.session
            dom = (dns_resolutions or {}).get(str(s.dst_ip))
            ep = WhitelistEndpoint(
                domain=None if dom in ("Unknown", "Resolving") else dom, ip=str(s.dst_ip), port=s.dst_port,
                protocol=s.protocol.name, process=(process_names or {}).get(s),
                description="Auto-generated from session: %s:%d -> %s:%d" % (s.src_ip, s.src_port, s.dst_ip, s.dst_port))
            if ep.fingerprint() not in seen:
                seen.add(ep.fingerprint())
                endpoints.append(ep)
        return w.as_custom(endpoints)

    def as_custom(self, endpoints, extends=None):
        """This model as new_from_sessions leaves it: one list named custom_whitelist, today's date."""
        self.whitelists["custom_whitelist"] = WhitelistInfo("custom_whitelist", extends, endpoints)
        t = time.localtime()
        self.date = "%s %02dth %d" % (time.strftime("%B", t), t.tm_mday, t.tm_year)  # "%B %dth %Y"
        return self

    @staticmethod
    def from_learned(records, names=None, process_names=None):
        """new_from_sessions from fb_learned_endpoint records (FlodbaddGpuCapture.learn_endpoints): one
        endpoint per record, in the records' order -- domain = names[dst_name_id] ({id: str} from
        FlodbaddGpuCapture.dns_names; id 0: None), ip, port, protocol, and the description of the record's
        representative session.  process_names {id: str} (l7.ProcessNameInterner.names): process =
        process_names[proc_name_id] (id 0: None) of records learned while a process-name table was installed;
        without it no endpoint has a process."""
        names = names or {}
        endpoints = []
        pids = np.asarray(records).view(N.LEARNED_ENDPOINT_PROC_DTYPE)["proc_name_id"] if process_names is not None else None
        for j, r in enumerate(records):
            fam, dst = int(r["family"]), words_to_ip(r["dst_ip"], int(r["family"]))
            nid = int(r["dst_name_id"])
            endpoints.append(WhitelistEndpoint(
                domain=names[nid] if nid else None, ip=str(dst), port=int(r["dst_port"]),
                protocol={6: "TCP", 17: "UDP"}[int(r["protocol"])],
                process=process_names[int(pids[j])] if (pids is not None and int(pids[j])) else None,
                description="Auto-generated from session: %s:%d -> %s:%d" % (
                    words_to_ip(r["rep_src_ip"], fam), int(r["rep_src_port"]), dst, int(r["dst_port"]))))
        return Whitelists().as_custom(endpoints)

    @staticmethod
    def merge_custom_whitelists(json_a, json_b):
        """src/whitelists.rs:223-299: the lists of two WhitelistsJSON documents merged by name -- a's
        endpoints, then b's, de-duplicated per list by fingerprint (the first occurrence stays); extends
        from the first source that has one; date and signature from a.  The lists appear in the order of
        their first appearance (the reference collects a HashMap: unspecified).  Compact JSON; ValueError
        when either document does not parse."""
        merged = {}
        for which, text in (("first", json_a), ("second", json_b)):
            try:
                data = json.loads(text) if isinstance(text, (str, bytes)) else text
                if not isinstance(data, dict):
                    raise ValueError("not a WhitelistsJSON object")
                model = Whitelists(data)  # the model's checks: unknown or missing fields
                infos = [WhitelistInfo(i["name"], None if i.get("extends") is None else list(i["extends"]),
                                       [WhitelistEndpoint.from_dict(e) for e in i["endpoints"]])
                         for i in data["whitelists"]]
            except (ValueError, TypeError, KeyError, AttributeError) as e:
                raise ValueError("Failed to parse %s whitelist JSON: %s" % (which, e)) from e
            if which == "first":
                date, signature = model.date, model.signature
            for info in infos:  # (a name that repeats inside one document merges too)
                entry = merged.setdefault(info.name, WhitelistInfo(info.name, info.extends, []))
                if entry.extends is None:
                    entry.extends = info.extends
                entry.endpoints.extend(info.endpoints)
        out = Whitelists()
        out.date, out.signature = date, signature
        for info in merged.values():
            info.endpoints = dedup_endpoints(info.endpoints)
        out.whitelists = merged
        return out.to_json(compact=True)

    def compile(self, name, asn_records=None, dns_resolutions=None, process_ids=None, domain_patterns=False):
        """The flattened list `name` as fb_wl_endpoint rows.  asn_records: the (as_number, country,
        owner) of every fb_asn_range.record (asn_tables_from_tsv's third result), for the interned
        owner / country ids.  dns_resolutions {ip: domain}: every domain endpoint whose pattern matches
        the domain of a resolved address also yields an exact-address row for that address with the same
        protocol, port and process flag and no AS fields (a matching domain returns true at once); the
        domain endpoint itself keeps FB_WL_HAS_DOMAIN for the host-check bit.  process_ids: an
        l7.ProcessNameInterner -- every endpoint with a process then carries its process_match_id (the
        word `reserved2` of the rows, N.WL_ENDPOINT_PROC_DTYPE), expanded rows included, and the device
        matches it against the flows' processes (fb_set_l7_process_names); without it the word stays 0
        and such an endpoint is the host's to decide.  domain_patterns: no expansion (dns_resolutions must be
        None) -- the result carries the distinct lower-cased patterns and every row's pattern id for
        fb_set_whitelist_dom, which matches them against the names the device tracks; the general (a*b)
        patterns past the FB_WL_MAX_GENERAL-th distinct one, in list order, get id 0 and stay the host's."""
        if domain_patterns and dns_resolutions:
            raise ValueError("domain_patterns compiles no resolutions into the list")
        eps = self.get_all_endpoints(name)
        strings = {}
        pattern_ids, patterns, ep_pattern, generals = {}, [], [], 0

        def intern(s):
            return strings.setdefault(ascii_lower(s), len(strings))

        resolved = []
        for ip, dom in (dns_resolutions or {}).items():
            a = parse_ip(str(ip))
            if a is not None and dom is not None:
                resolved.append((a, dom))
        rows = []
        for ep in eps:
            r = np.zeros(1, dtype=N.WL_ENDPOINT_DTYPE)[0]
            flags = 0
            if ep.protocol is not None:
                r["protocol"] = {"tcp": 6, "udp": 17}.get(ascii_lower(ep.protocol), N.FB_WL_NEVER)
            if ep.port is not None:
                flags |= N.FB_WL_HAS_PORT
                r["port"] = ep.port
            if ep.process is not None:
                flags |= N.FB_WL_HAS_PROCESS
                if process_ids is not None:
                    r["reserved2"] = process_ids.match_id(ep.process)
            base = r.copy()
            base["flags"] = flags  # protocol, port and the process flag: what an expanded row shares
            if ep.ip is not None:
                _ip_fields(r, ep.ip)
            if ep.as_number is not None:
                flags |= N.FB_WL_HAS_ASN
                r["as_number"] = ep.as_number
            if ep.as_owner is not None:
                flags |= N.FB_WL_HAS_OWNER
                r["owner_id"] = intern(ep.as_owner)
            if ep.as_country is not None:
                flags |= N.FB_WL_HAS_COUNTRY
                r["country_id"] = intern(ep.as_country)
            if ep.domain is not None:
                flags |= N.FB_WL_HAS_DOMAIN
                if domain_patterns:
                    pat = ep.domain.lower()
                    if pat not in pattern_ids:
                        general = classify_domain_pattern(pat) == "general"
                        generals += general
                        if general and generals > N.FB_WL_MAX_GENERAL:
                            pattern_ids[pat] = 0
                        else:
                            patterns.append(pat)
                            pattern_ids[pat] = len(patterns)
                    ep_pattern.append(pattern_ids[pat])
                for a, dom in resolved:
                    if domain_matches(dom, ep.domain):
                        x = base.copy()
                        x["addr"], x["family"] = ip_to_words(a)
                        x["prefix"] = 32 if a.version == 4 else 128
                        rows.append(x)
            r["flags"] = flags
            rows.append(r)
            if domain_patterns and ep.domain is None:
                ep_pattern.append(0)
        recs = list(asn_records or [])
        owner = np.array([intern(o) for _, _, o in recs], dtype=np.uint32)
        country = np.array([intern(c) for _, c, _ in recs], dtype=np.uint32)
        arr = np.array(rows, dtype=N.WL_ENDPOINT_DTYPE) if rows else np.zeros(0, dtype=N.WL_ENDPOINT_DTYPE)
        comp = CompiledWhitelist(name, eps, arr, owner, country, strings)
        if domain_patterns:
            blobs = [p.encode("utf-8") for p in patterns]
            comp.patterns = patterns
            comp.ep_pattern = np.array(ep_pattern, dtype=np.uint32)
            comp.pattern_bytes = np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()
            comp.pattern_off = np.cumsum([0] + [len(b) for b in blobs], dtype=np.uint64)
        return comp


def rows_from_flows(flows):
    """The fb_wl_endpoint rows Whitelists.new_from_sessions(...).compile(...) gives for fb_flow_rec
    records without domains or processes -- one exact-address row per distinct (dst_ip, dst_port,
    protocol) -- built with array operations (a table-sized list is millions of rows)."""
    rows = np.zeros(len(flows), dtype=N.WL_ENDPOINT_DTYPE)
    rows["addr"] = flows["dst_ip"]
    rows["family"] = flows["family"]
    rows["prefix"] = np.where(flows["family"] == 2, 32, 128)
    rows["protocol"] = flows["protocol"]
    rows["flags"] = N.FB_WL_HAS_PORT
    rows["port"] = flows["dst_port"]
    if len(rows) == 0:
        return rows
    u = np.unique(rows.view(np.uint64).reshape(len(rows), 5), axis=0)
    return np.ascontiguousarray(u).view(N.WL_ENDPOINT_DTYPE).reshape(-1)


__all__ = ["WhitelistEndpoint", "WhitelistInfo", "Whitelists", "CompiledWhitelist", "domain_matches", "ip_matches",
           "classify_domain_pattern", "endpoint_matches", "is_session_in_whitelist", "no_match_reason", "rows_from_flows", "dedup_endpoints", "ascii_lower", "rust_debug", "parse_ip", "parse_net"]
