"""A plain restatement of the reference's blacklist pass, for the tests: Blacklists::new_from_json and
is_ip_in_blacklist (src/blacklists.rs:70-266), is_ip_blacklisted (every list whose ranges contain the
address), recompute_blacklist_for_sessions (src/blacklists.rs:456-731) and the "Session is blacklisted"
fallback of update_sessions_internal (src/capture.rs:1858-1871), over a list of SessionInfo.

Every lookup is the reference's linear scan of every range of every list (`ipaddress` networks); nothing
here comes from the package's interval index or its masks.  The reference's incremental selection
(sessions modified since the last run, or all after a list change) only skips sessions whose result
cannot have changed -- the tags are a pure function of (addresses, stored local flags, lists) --, so
every run here evaluates every session.
"""
import ipaddress
import json

LOCAL_V4 = [ipaddress.ip_network(x) for x in ("0.0.0.0/8", "10.0.0.0/8", "127.0.0.0/8", "169.254.0.0/16",
                                              "172.16.0.0/12", "192.168.0.0/16")]
LOCAL_V6 = [ipaddress.ip_network(x) for x in ("::/128", "::1/128", "fc00::/7", "fe80::/10")]
REASON = "Session is blacklisted"


def parse_range(text):
    """src/blacklists.rs:127-157: a plain address becomes /32 or /128; an IpNet keeps its host bits
    (contains() masks them); None for text that is neither."""
    try:
        ip = ipaddress.ip_address(text)
        text = "%s/%d" % (text, 32 if ip.version == 4 else 128)
    except ValueError:
        pass
    try:
        return ipaddress.ip_network(text, strict=False)
    except ValueError:
        return None


def is_range_local(net):
    """is_range_local_to_filter (src/blacklists.rs:88-106): entirely inside a known local range."""
    return any(net.version == l.version and net.subnet_of(l) for l in (LOCAL_V4 if net.version == 4 else LOCAL_V6))


class BlRef:
    def __init__(self):
        self.lists = {}        # name -> [network]; the reference's map by name (a repeated name replaces)
        self.blacklisted = []  # blacklisted_sessions: Session keys, sorted after every run

    def set_lists(self, doc, filter_local_ranges=False):
        """doc: BlacklistsJSON text or object; "" / None: no lists."""
        self.lists = {}
        if not doc:
            return
        obj = json.loads(doc) if isinstance(doc, (str, bytes)) else doc
        for info in obj["blacklists"]:
            nets = []
            for s in info["ip_ranges"]:
                net = parse_range(s)
                if net is None or (filter_local_ranges and is_range_local(net)):
                    continue
                nets.append(net)
            self.lists[info["name"]] = nets

    def ranges(self, name):
        return [str(n) for n in self.lists[name]]

    def ip_lists(self, ip):
        """is_ip_blacklisted's Vec<String>: every list one of whose ranges contains ip (a linear scan)."""
        ip = ipaddress.ip_address(ip)
        out = []
        for name, nets in self.lists.items():
            for net in nets:
                if net.version == ip.version and ip in net:
                    out.append(name)
                    break
        return out

    def run(self, sessions, mark_whitelist=True):
        """One recompute over `sessions` (objects with .session, .is_local_src, .is_local_dst,
        .criticality, .is_whitelisted, .whitelist_reason; updated in place like the DashMap entries).
        Returns the run's figures: names {Session: sorted name list}, criticality {Session: str},
        blacklisted (the sorted list), and the counts flows / blacklisted / changed / newly_blacklisted /
        cleared / wl_marked."""
        present = {i.session for i in sessions}
        new_list = [s for s in self.blacklisted if s in present]  # existing, still in the map
        names, crit = {}, {}
        changed = newly = cleared = 0
        for i in sessions:
            match = []
            if not i.is_local_src:
                match += self.ip_lists(i.session.src_ip)
            if not i.is_local_dst:
                match += self.ip_lists(i.session.dst_ip)
            match = sorted(set(match))
            tags = [t for t in i.criticality.split(",") if t and not t.startswith("blacklist:")]
            tags += ["blacklist:" + n for n in match]
            new = ",".join(sorted(set(tags)))
            if match:
                if i.session not in new_list:
                    new_list.append(i.session)
            else:
                new_list = [s for s in new_list if s != i.session]
            old_bl = any(t.startswith("blacklist:") for t in i.criticality.split(","))
            if new != i.criticality:
                changed += 1
                i.criticality = new
            newly += 1 if (match and not old_bl) else 0
            cleared += 1 if (old_bl and not match) else 0
            names[i.session], crit[i.session] = match, new
        new_list = sorted(set(new_list), key=lambda s: s.sort_key())
        self.blacklisted = new_list
        marked = 0
        if mark_whitelist:  # src/capture.rs:1858-1871
            listed = set(new_list)
            for i in sessions:
                if i.session in listed and i.is_whitelisted.name == "Unknown":
                    i.is_whitelisted = type(i.is_whitelisted)["NonConforming"]
                    if i.whitelist_reason is None:
                        i.whitelist_reason = REASON
                    marked += 1
        return dict(names=names, criticality=crit, blacklisted=list(new_list), flows=len(sessions),
                    n_blacklisted=len(new_list), changed=changed, newly_blacklisted=newly, cleared=cleared,
                    wl_marked=marked)


def stats_of(res):
    """A run's counts under fb_bl_stats' field names."""
    return dict(flows=res["flows"], blacklisted=res["n_blacklisted"], changed=res["changed"],
                newly_blacklisted=res["newly_blacklisted"], cleared=res["cleared"], wl_marked=res["wl_marked"])
