"""Plain-Python restatement of the incremental query surface (reference src/capture.rs:411-426, 1578-1760):
a session's last_modified, the four getters' fetch timestamps and the rules of the view export's sets.

    last_modified = max(last_activity, stamp)      stamp: the pass time of the last pass that changed the
                                                   session (0: none); the packet path sets last_activity
    a pass stamps   blacklist: mask changed, or the Unknown -> "Session is blacklisted" fallback marked it
                    whitelist: state changed       anomaly: level or diagnostic codes changed
                    aging: never                   pass time 0: never
    a getter        full fetch with a now: fetch_ts[getter] = now; without: unchanged; incremental: the
                    sessions of the getter's set with last_modified > fetch_ts[getter] (strict), fetch_ts
                    unchanged; the initial fetch_ts is 0, and reset_fetch_timestamps puts it back

Everything is keyed by an opaque session key; times are integers on one clock (ns in the product)."""

SETS = ("all", "current", "blacklisted", "exceptions", "anomalous")
GETTER_SET = {"sessions": "all", "current": "current", "blacklisted": "blacklisted", "exceptions": "exceptions"}

# status byte bits (fb_flow_status_dev), whitelist state bits (fb_flow_whitelist_dev)
ST_ACTIVE, ST_ADDED, ST_ACTIVATED, ST_DEACTIVATED, ST_CURRENT, ST_AGED = 1, 2, 4, 8, 16, 128
WL_CONFORMING, WL_NONCONFORMING, WL_HOST_CHECK, WL_BLACKLISTED = 1, 2, 4, 8


class Sess:
    def __init__(self, t):
        self.start = t          # None on an untimed table
        self.last_activity = t
        self.stamp = 0
        self.status = 0         # 0: never aged since insert (= current)
        self.bl_mask = 0
        self.wl_state = 0
        self.an_level = 0
        self.an_diag = 0

    @property
    def last_modified(self):
        return max(self.last_activity or 0, self.stamp)


class ModRef:
    def __init__(self, timed=True):
        self.timed = timed
        self.s = {}
        self.pass_time = 0
        self.fetch_ts = dict.fromkeys(GETTER_SET, 0)

    # ---- what modifies a session ------------------------------------------------------------------
    def packet(self, key, t=None):
        """src/packets.rs:342 (update) / 524 (insert): last_modified = now = the packet's time."""
        t = t if self.timed else None
        if key in self.s:
            self.s[key].last_activity = t
        else:
            self.s[key] = Sess(t)

    def set_pass_time(self, now):
        self.pass_time = int(now)

    def _stamp(self, key):
        if self.pass_time:
            self.s[key].stamp = self.pass_time

    def blacklist_pass(self, mask_of, mark=True):
        """mask_of(key) -> the new mask.  Returns (changed, wl_marked) keys."""
        changed, marked = [], []
        for k, v in self.s.items():
            nw, hit = int(mask_of(k)), False
            if nw != v.bl_mask:
                v.bl_mask, hit = nw, True
                changed.append(k)
            if mark and nw and v.wl_state == 0:
                v.wl_state, hit = WL_NONCONFORMING | WL_BLACKLISTED, True
                marked.append(k)
            if hit:
                self._stamp(k)
        return changed, marked

    def whitelist_pass(self, state_of):
        changed = []
        for k, v in self.s.items():
            nw = int(state_of(k))
            if nw != v.wl_state:
                v.wl_state = nw
                changed.append(k)
                self._stamp(k)
        return changed

    def anomaly_pass(self, rec_of):
        """rec_of(key) -> (level, diag).  Returns the keys stamped (level or diag changed)."""
        hit = []
        for k, v in self.s.items():
            level, diag = rec_of(k)
            if (level, diag) != (v.an_level, v.an_diag):
                v.an_level, v.an_diag = level, diag
                hit.append(k)
                self._stamp(k)
        return hit

    def age(self, now, activity=60 * 10**9, current=180 * 10**9, retention=86400 * 10**9, purge=True):
        """update_sessions_status (src/capture.rs:1497-1551): never touches last_modified.  Returns purged keys."""
        gone = []
        for k, v in self.s.items():
            if purge and now > v.last_activity + retention:
                gone.append(k)
                continue
            was = True if v.status == 0 else bool(v.status & ST_ACTIVE)
            act = v.last_activity + activity >= now
            v.status = (ST_AGED | (ST_ACTIVE if act else 0) | (ST_ADDED if v.start + activity >= now else 0) |
                        (ST_ACTIVATED if (act and not was) else 0) | (ST_DEACTIVATED if (was and not act) else 0) |
                        (ST_CURRENT if now < v.last_activity + current else 0))
        for k in gone:
            del self.s[k]  # a purged session that returns is inserted afresh: stamp 0
        return gone

    def clear(self):
        self.s = {}

    # ---- the sets and the getters -------------------------------------------------------------------
    def in_set(self, key, which):
        v = self.s[key]
        if which == "all":
            return True
        if which == "current":
            return v.status == 0 or bool(v.status & ST_CURRENT)
        if which == "blacklisted":
            return v.bl_mask != 0
        if which == "exceptions":
            return bool(v.wl_state & WL_NONCONFORMING)
        if which == "anomalous":
            return v.an_level >= 2
        raise ValueError(which)

    def select(self, which="all", since=None, keep=lambda key: True):
        """The view export: the keys of set `which` passing `keep` (the session filter) and, with since, whose
        last_modified is strictly later."""
        if since is not None and not self.timed:
            raise ValueError("no clock")
        return sorted(k for k in self.s
                      if self.in_set(k, which) and keep(k) and (since is None or self.s[k].last_modified > since))

    def get(self, getter, now=None, incremental=False, keep=lambda key: True):
        """One getter call after its update: the keys it returns."""
        which = GETTER_SET[getter]
        if incremental:
            return self.select(which, self.fetch_ts[getter], keep)
        if now is not None:
            self.fetch_ts[getter] = int(now)
        return self.select(which, None, keep)

    def reset_fetch_timestamps(self):
        self.fetch_ts = dict.fromkeys(GETTER_SET, 0)

    def last_modified(self, key):
        return self.s[key].last_modified


# ---- the reference's four incremental known-answer tests (src/capture.rs:2522-3167) ----------------------
# One transcription, run against any "world" that offers packet / set_pass_time / set_blacklists /
# set_whitelist / get / last_modified -- ModRefWorld below, and the GPU capture in tests/test_gpu_view.py.
# Where the reference pokes SessionInfo.last_modified, the session is modified the way the product can: a
# packet at that time (sessions, current, exceptions) or a list change that flips its mask (blacklisted).
import ipaddress  # noqa: E402

S = 10 ** 9
MS = 10 ** 6
T0 = 1_700_000_000 * S
A = ("TCP", "10.0.0.1", 12345, "93.184.216.34", 443)  # the session the scenario modifies
B = ("TCP", "10.0.0.1", 54321, "8.8.8.8", 443)
SCENARIOS = ("sessions", "current", "blacklisted", "exceptions")


class ModRefWorld:
    def __init__(self):
        self.m = ModRef(timed=True)
        self.lists, self.allowed = [], None

    def packet(self, sess, t):
        self.m.packet(sess, t)

    def set_pass_time(self, now):
        self.m.set_pass_time(now)

    def _mask(self, sess):
        hit = 0
        for bit, (_, ranges) in enumerate(self.lists):
            for ip in (sess[1], sess[3]):
                a = ipaddress.ip_address(ip)  # (an address local at insert is not searched: 10.0.0.1 here)
                if a not in ipaddress.ip_network("10.0.0.0/8") and any(a in ipaddress.ip_network(r, strict=False) for r in ranges):
                    hit |= 1 << bit
        return hit

    def _update(self, now, status=True):
        if now is not None:
            self.m.set_pass_time(now)
            if status:
                self.m.age(now)
        self.m.blacklist_pass(self._mask, mark=True)
        self._whitelist()

    def _whitelist(self):
        if self.allowed is not None:
            self.m.whitelist_pass(lambda k: WL_CONFORMING if (k[3], k[4], k[0]) in self.allowed else WL_NONCONFORMING)

    def set_blacklists(self, lists):
        """[(name, [ranges])] replaces the lists; one update without a now follows (set_custom_blacklists)."""
        self.lists = list(lists)
        self._update(None)

    def set_whitelist(self, endpoints):
        """[(ip, port, protocol)]: every state back to Unknown, then one pass (set_custom_whitelists)."""
        self.allowed = set(endpoints)
        for v in self.m.s.values():
            v.wl_state = 0
        self._whitelist()

    def get(self, getter, now=None, incremental=False):
        if getter in ("sessions", "current"):
            if now is not None:
                self.m.age(now)
        elif getter == "blacklisted":
            self._update(now)
        else:
            if now is not None:
                self.m.set_pass_time(now)
            self._whitelist()
        return self.m.get(getter, now, incremental)

    def last_modified(self, sess):
        return self.m.last_modified(sess)


def incremental_scenario(world, getter):
    """full fetch -> modify one session -> the incremental fetch returns exactly it -> a second one still
    does -> full fetch -> the incremental fetch returns nothing.  Returns the modification time."""
    w = world
    w.packet(A, T0 - 10 * S)
    w.packet(B, T0 - 10 * S + 1000)
    if getter == "blacklisted":
        w.set_pass_time(T0 - 5 * S)
        w.set_blacklists([("inc_test", [A[3] + "/32"])])
    if getter == "exceptions":
        w.set_whitelist([(B[3], B[4], B[0])])
    members = [A] if getter in ("blacklisted", "exceptions") else sorted([A, B])
    # before any full fetch the timestamp is the epoch: an incremental fetch is a full one
    assert sorted(w.get(getter, T0 - S, incremental=True)) == members
    assert sorted(w.get(getter, T0)) == members                                # 1. full fetch
    if getter == "exceptions":
        assert w.get(getter, T0 + 10 * MS, incremental=True) == []            # (capture.rs:3116-3125)
    t_mod = T0 + 50 * MS
    if getter == "blacklisted":                                               # 2. modify A
        w.set_pass_time(t_mod)
        w.set_blacklists([("inc_test", [A[3] + "/32"]), ("inc_test2", [A[3] + "/31"])])
    else:
        w.packet(A, t_mod)
    assert w.get(getter, T0 + 100 * MS, incremental=True) == [A]              # 3. exactly A
    assert w.last_modified(A) == t_mod
    assert w.get(getter, T0 + 150 * MS, incremental=True) == [A]              # 4. still A: no timestamp moved
    if getter == "exceptions":
        return t_mod                                                          # (the reference's test ends here)
    assert sorted(w.get(getter, T0 + 200 * MS)) == members                    # 5. full fetch
    assert w.get(getter, T0 + 250 * MS, incremental=True) == []               # 6. nothing
    assert w.last_modified(B) == T0 - 10 * S + 1000
    return t_mod
