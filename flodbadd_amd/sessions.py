"""Host-side session model, mirroring the reference's types (src/sessions.rs).

Only data-model plumbing lives here: converting between the C-ABI `fb_session_key` layout and
Session objects, derived statistics computed from integer counters, and the post-hoc
bucket split `filter_sessions` (src/sessions.rs:678-692), which in the reference runs per
query over the session list, not per packet.  Per-packet work never runs here.
"""
import enum
import ipaddress
import json
import os

import numpy as np
from dataclasses import dataclass, field
from typing import List, Optional

from ._native import (CONN_STATES, FB_FILTER_ALL, FB_FILTER_GLOBAL_ONLY, FB_FILTER_LOCAL_ONLY, FB_SEEN_NONE,
                      FB_WL_BLACKLISTED, FB_WL_CONFORMING, FB_WL_NONCONFORMING,
                      FLOW_REC_DTYPE, FLOW_VIEW_DTYPE, SESSION_DST_SERVICE, SESSION_LOCAL_DST, SESSION_LOCAL_SRC, SESSION_SELF_DST,
                      SESSION_SELF_SRC, STATUS_ACTIVATED, STATUS_ACTIVE, STATUS_ADDED, STATUS_DEACTIVATED,
                      META_DST_SERVICE, META_HAS_FLAGS, META_LOCAL_DST, META_LOCAL_SRC, META_ORIGINATOR,
                      META_SELF_DST, META_SELF_SRC, META_SWAP, PARSED_DTYPE, PKT_OUT_DTYPE, KEY_FIELDS, gpu_lib, ptr)


class Protocol(enum.IntEnum):
    """src/sessions.rs:17-21 (derived Ord: TCP < UDP)."""
    TCP = 6
    UDP = 17


class SessionFilter(enum.IntEnum):
    """src/sessions.rs:173-178 (same discriminant order)."""
    LocalOnly = FB_FILTER_LOCAL_ONLY
    GlobalOnly = FB_FILTER_GLOBAL_ONLY
    All = FB_FILTER_ALL


def ip_to_words(ip):
    """session_to_key word format (src/l7_ebpf.rs:78-104): v4 numeric in word 0; v6 4 BE words."""
    ip = ipaddress.ip_address(ip)
    if ip.version == 4:
        return (int(ip), 0, 0, 0), 2
    v = int(ip)
    return tuple((v >> (96 - 32 * k)) & 0xFFFFFFFF for k in range(4)), 10


def words_to_ip(words, family):
    if family == 2:
        return ipaddress.IPv4Address(int(words[0]))
    v = 0
    for w in words:
        v = (v << 32) | int(w)
    return ipaddress.IPv6Address(v)


@dataclass(frozen=True, order=False)
class Session:
    """The 5-tuple key, src/sessions.rs:23-30."""
    protocol: Protocol
    src_ip: object
    src_port: int
    dst_ip: object
    dst_port: int

    def sort_key(self):
        """Derived Ord: protocol, src_ip (V4 < V6, then octets), src_port, dst_ip, dst_port."""
        return (int(self.protocol), self.src_ip.version, int(self.src_ip), self.src_port,
                self.dst_ip.version, int(self.dst_ip), self.dst_port)

    def __lt__(self, other):
        return self.sort_key() < other.sort_key()

    def reversed(self):
        return Session(self.protocol, self.dst_ip, self.dst_port, self.src_ip, self.src_port)

    @staticmethod
    def from_key(rec):
        fam = int(rec["family"])
        return Session(Protocol(int(rec["protocol"])), words_to_ip(rec["src_ip"], fam), int(rec["src_port"]),
                       words_to_ip(rec["dst_ip"], fam), int(rec["dst_port"]))

    def key_fields(self):
        s, fam = ip_to_words(self.src_ip)
        d, _ = ip_to_words(self.dst_ip)
        return s, d, fam


@dataclass
class SessionPacketData:
    """src/packets.rs:91-98 (per emitted record; raw session = key reversed when swapped)."""
    session: Session
    packet_length: int
    ip_packet_length: int
    flags: Optional[int]


@dataclass
class SessionStats:
    """Integer counters of src/sessions.rs:73-96 + the two derived f64s
    (src/packets.rs:122-135), recomputed from the final counters."""
    inbound_bytes: int = 0
    outbound_bytes: int = 0
    orig_pkts: int = 0
    resp_pkts: int = 0
    orig_ip_bytes: int = 0
    resp_ip_bytes: int = 0
    history: str = ""
    conn_state: Optional[str] = None
    # positions ((flow update call << 32) | pkt_index) standing for start_time / last_activity /
    # end_time (src/sessions.rs:74-76); end None until the first FIN/RST
    first_seen: int = 0
    last_seen: int = 0
    end_seen: Optional[int] = None
    hist_len: int = 0
    # segment detection (src/sessions.rs:88-93; src/packets.rs:137-160, 370-376, 414-420) under the
    # no-timeout model: TCP packets with PSH counted, in a segment unless the latest packet had PSH
    segment_count: int = 0
    in_segment: bool = False
    # timed contexts (fb_flow_time, FB_CFG_TIMED): capture times in ns since the epoch (the
    # reference's DateTime<Utc> start_time / last_activity / end_time / current_segment_start /
    # last_segment_end, src/sessions.rs:74-92) and the exact interarrival sum in ms; None untimed
    start_time_ns: Optional[int] = None
    last_activity_ns: Optional[int] = None
    end_time_ns: Optional[int] = None
    current_segment_start_ns: Optional[int] = None
    last_segment_end_ns: Optional[int] = None
    total_segment_interarrival_ms: int = 0
    segment_interarrival_div: int = 0
    segment_timeout: float = 5.0  # src/packets.rs:379

    @property
    def total_segment_interarrival(self):
        """Seconds (f64), as src/packets.rs:166 accumulates it (from the exact integer ms sum)."""
        return self.total_segment_interarrival_ms / 1000.0

    @property
    def segment_interarrival(self):
        """src/packets.rs:167-171: the total over segment_count - 1 at the last accepted term."""
        d = self.segment_interarrival_div
        return self.total_segment_interarrival / d if d > 0 else 0.0

    @property
    def last_segment_end_set(self):
        """last_segment_end.is_some(): timed, from the capture times; untimed, a segment has ended."""
        if self.start_time_ns is not None:
            return self.last_segment_end_ns is not None
        return self.segment_count > 0

    @property
    def average_packet_size(self):
        tp = self.orig_pkts + self.resp_pkts
        return (self.inbound_bytes + self.outbound_bytes) / tp if tp > 0 else 0.0

    @property
    def inbound_outbound_ratio(self):
        return self.inbound_bytes / self.outbound_bytes if self.outbound_bytes > 0 else 0.0


@dataclass
class SessionStatus:
    """SessionStatus (src/sessions.rs), as update_sessions_status leaves it (src/capture.rs:1514-1528);
    the defaults are the status a session is inserted with (src/packets.rs:497-502)."""
    active: bool = True
    added: bool = True
    activated: bool = True
    deactivated: bool = False

    @staticmethod
    def from_byte(b):
        """A status byte of fb_flow_status_dev; 0 (never aged since insert) is the insert status."""
        b = int(b)
        if b == 0:
            return SessionStatus()
        return SessionStatus(bool(b & STATUS_ACTIVE), bool(b & STATUS_ADDED), bool(b & STATUS_ACTIVATED),
                             bool(b & STATUS_DEACTIVATED))


class WhitelistState(enum.Enum):
    """src/sessions.rs:183-187."""
    Conforming = "Conforming"
    NonConforming = "NonConforming"
    Unknown = "Unknown"

    @staticmethod
    def from_byte(b):
        """A state byte of fb_flow_whitelist_dev; 0 (no pass has seen the flow) is Unknown."""
        b = int(b)
        if b & FB_WL_CONFORMING:
            return WhitelistState.Conforming
        return WhitelistState.NonConforming if b & FB_WL_NONCONFORMING else WhitelistState.Unknown


@dataclass(frozen=True)
class SessionL7:
    """SessionL7 (src/sessions.rs:30-37): the process the L7 pass attributed the session to."""
    pid: int
    process_name: str
    process_path: str
    username: str


@dataclass
class SessionInfo:
    """Subset of src/sessions.rs:40-61 that the GPU path owns.  is_local_* / is_self_* and
    dst_service are the values stored when the session was inserted (src/packets.rs:429-466,
    fb_flow_rec.session_flags); status is None on an untimed capture (no clock to age by);
    is_whitelisted / whitelist_reason are what the last whitelist pass left (Unknown before it), or
    NonConforming / "Session is blacklisted" where the blacklist pass found the session Unknown
    (src/capture.rs:1858-1871); criticality holds the sorted "blacklist:<name>" tags of the last
    blacklist pass (src/blacklists.rs:612-631; "" before it) and, once FlodbaddGpuCapture.analyze_sessions
    has run, the merged "anomaly:<level>[/<diagnostic>]" tag (src/analyzer.rs:630-653).  last_modified_ns
    (src/sessions.rs: last_modified, on the capture clock): the later of the session's last packet (timed
    captures) and the last pass that changed it under a pass time (FlodbaddGpuCapture.set_pass_time); 0 when
    neither exists."""
    session: Session
    stats: SessionStats = field(default_factory=SessionStats)
    is_local_src: bool = False
    is_local_dst: bool = False
    is_self_src: bool = False
    is_self_dst: bool = False
    dst_service: Optional[str] = None
    status: Optional[SessionStatus] = None
    is_whitelisted: WhitelistState = WhitelistState.Unknown
    whitelist_reason: Optional[str] = None
    criticality: str = ""
    last_modified_ns: int = 0
    # populate_domain_names (src/capture.rs:1307-1411): the names the domain pass gave the two addresses from
    # the passively captured DNS resolutions (FlodbaddGpuCapture(track_dns=True)); None before it, and always
    # on a capture that does not track DNS
    src_domain: Optional[str] = None
    dst_domain: Optional[str] = None

    @property
    def l7(self) -> Optional[SessionL7]:
        """SessionInfo.l7 (src/sessions.rs:40-61), populate_l7 (src/capture.rs:1414-1495): the process the L7
        pass matched the session to in the installed socket snapshot (FlodbaddGpuCapture.set_l7_sockets /
        update_l7); None before it and for a session no socket matched.  A property like uid, not a field:
        the field list, equality and the joins are what they were."""
        return self.__dict__.get("_l7")

    @l7.setter
    def l7(self, value):
        if value is None:
            self.__dict__.pop("_l7", None)
        else:
            self.__dict__["_l7"] = value

    @property
    def uid(self):
        """SessionInfo.uid (src/sessions.rs; the reference draws a random UUID v4, src/packets.rs:350): the
        deterministic session_uid of the key and the start time (0 on an untimed capture).  A property, not a
        field: equality and the joins compare what they compared before."""
        return session_uid(self.session, self.stats.start_time_ns or 0)


_SERVICE_NAMES = None


def service_name(port):
    """get_name_from_port (src/port_vulns.rs:213-228) over the reference's built-in port table
    (data/service_names.json, generated by tools/gen_service_bitmap.py with the service bitmap):
    the name, or "" for a port the table does not name."""
    global _SERVICE_NAMES
    if _SERVICE_NAMES is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "service_names.json")) as f:
            _SERVICE_NAMES = {int(k): v for k, v in json.load(f).items()}
    return _SERVICE_NAMES.get(int(port), "")


def is_lan_ip(ip, lan_v6=()):
    """is_lan_ip, src/ip.rs:199-242: the IPv4 fast check (ip.rs:55-91), the IPv6 special ranges
    (ip.rs:112-136) and the interface prefixes of the LAN cache (ip.rs:141-156, 164-191), given as
    [(address, prefix_len)] like FlodbaddGpuCapture's lan_v6.  Host-side: the reference evaluates it
    per query in is_local_session! / filter_sessions (src/sessions.rs:660-692)."""
    ip = ipaddress.ip_address(ip)
    if ip.version == 4:
        v = int(ip)
        return (v in (0, 0xFFFFFFFF) or (v >> 24) in (127, 10) or (v >> 28) == 0xE or (v >> 16) in (0xA9FE, 0xC0A8)
                or ((v >> 24) == 172 and 16 <= ((v >> 16) & 0xFF) <= 31))
    v = int(ip)
    s0 = v >> 112
    if v in (0, 1) or (s0 & 0xFFC0) == 0xFE80 or (s0 & 0xFF00) == 0xFF00 or (s0 & 0xFE00) == 0xFC00:
        return True
    for net, pfx in lan_v6:
        mask = 0 if pfx == 0 else ((1 << 128) - 1) ^ ((1 << (128 - pfx)) - 1)
        if (v & mask) == (int(ipaddress.IPv6Address(net)) & mask):
            return True
    return False


def is_local_session(info, lan_v6=()):
    """is_local_session! (src/sessions.rs:660-666): both key addresses LAN, evaluated now."""
    return is_lan_ip(info.session.src_ip, lan_v6) and is_lan_ip(info.session.dst_ip, lan_v6)


def records_to_packets(recs):
    """fb_pkt_out records -> SessionPacketData (raw direction restored from the SWAP bit)."""
    if recs.dtype != PKT_OUT_DTYPE:
        raise TypeError("expected fb_pkt_out records (PKT_OUT_DTYPE), got %s" % recs.dtype)
    out = []
    for r in recs:
        key = Session.from_key(r)
        raw = key.reversed() if int(r["meta"]) & META_SWAP else key
        flags = int(r["tcp_flags"]) if int(r["meta"]) & META_HAS_FLAGS else None
        out.append(SessionPacketData(raw, int(r["packet_length"]), int(r["ip_packet_length"]), flags))
    return out


def packets_to_parsed(packets):
    """SessionPacketData list -> PARSED_DTYPE array (fb_parsed_pkt), pkt_index = list position."""
    a = np.zeros(len(packets), dtype=PARSED_DTYPE)
    for i, p in enumerate(packets):
        s, d, fam = p.session.key_fields()
        a[i]["src_ip"], a[i]["dst_ip"] = s, d
        a[i]["src_port"], a[i]["dst_port"] = p.session.src_port, p.session.dst_port
        a[i]["protocol"], a[i]["family"] = int(p.session.protocol), fam
        a[i]["packet_length"], a[i]["ip_packet_length"] = p.packet_length, p.ip_packet_length
        a[i]["tcp_flags"] = p.flags or 0
        a[i]["has_flags"] = 0 if p.flags is None else 1
        a[i]["pkt_index"] = i
    return a


def determine_conn_state(history):
    """src/packets.rs:539-559."""
    h = set(history)
    if {"S", "H", "F", "f"} <= h:
        return "SF"
    if "S" in h and "h" not in h and "r" not in h:
        return "S0"
    if "R" in h or "r" in h:
        return "REJ"
    if "S" in h and "H" in h and "F" not in h and "f" not in h:
        return "S1"
    return "-"


def histories_from_records(recs):
    """Per-flow history strings + conn_state from packet-ordered fb_pkt_out records.

    The GPU emits each packet's map_tcp_flags char (src/packets.rs:561-601) in its record; the
    ordered per-flow string (src/packets.rs:187-198, 410-426) is the concatenation in packet order,
    and conn_state is fixed at the first FIN/RST.  Returns {Session: (history, conn_state)}."""
    if recs.dtype != PKT_OUT_DTYPE:
        raise TypeError("expected fb_pkt_out records (PKT_OUT_DTYPE), got %s" % recs.dtype)
    hist, state = {}, {}
    for r in recs[np.argsort(recs["pkt_index"], kind="stable")]:
        if not int(r["meta"]) & META_HAS_FLAGS:
            continue
        k = Session.from_key(r)
        h = hist.get(k, "") + chr(int(r["hist_char"]))
        hist[k] = h
        if int(r["tcp_flags"]) & 0x05 and k not in state:  # FIN | RST
            state[k] = determine_conn_state(h)
    return {k: (h, state.get(k)) for k, h in hist.items()}


def _per_record(plane, slots):
    """A per-slot argument of flows_to_sessions -- an array indexed by slot or {slot: value}; None stays None --
    as one value per record: row k is that of the flow in slots[k]."""
    if plane is None:
        return None
    if isinstance(plane, dict):
        return [plane[s] for s in slots.tolist()]
    return np.asarray(plane)[slots].tolist()


def _join(flows, histories, times=None, status=None, whitelist=None, masks=None, bl_names=(), stamps=None,
          dom_ids=None, dom_names=None, l7_ids=None, l7_procs=None):
    """The join behind flows_to_sessions and views_to_sessions, over per-record columns: row k of every column
    that is not None belongs to flows[k].  times: FLOW_TIME_DTYPE records; status / whitelist: bytes; masks:
    blacklist mask words of the lists bl_names; stamps: fb_flow_modified_dev stamps; dom_ids: (src, dst) name-id
    pairs into dom_names; l7_ids: the L7 plane's process ids into l7_procs ({process id: SessionL7})."""
    from .enrich import criticality_of  # (enrich imports this module)
    none = lambda v: None if int(v) == FB_SEEN_NONE else int(v)  # noqa: E731
    out = []
    for k, r in enumerate(flows):
        st = SessionStats(int(r["inbound_bytes"]), int(r["outbound_bytes"]), int(r["orig_pkts"]),
                          int(r["resp_pkts"]), int(r["orig_ip_bytes"]), int(r["resp_ip_bytes"]),
                          histories.get(int(r["slot"]), "") if histories is not None else "",
                          CONN_STATES[int(r["conn_state"])], int(r["first_seen"]), int(r["last_seen"]),
                          none(r["end_seen"]), int(r["hist_len"]), int(r["segment_count"]), bool(r["in_segment"]))
        if times is not None:
            t = times[k]
            st.start_time_ns, st.last_activity_ns = int(t["start_time_ns"]), int(t["last_activity_ns"])
            st.end_time_ns, st.last_segment_end_ns = none(t["end_time_ns"]), none(t["last_segment_end_ns"])
            st.current_segment_start_ns = int(t["current_segment_start_ns"])
            st.total_segment_interarrival_ms = int(t["total_segment_interarrival_ms"])
            st.segment_interarrival_div = int(t["segment_interarrival_div"])
        s = Session.from_key(r)
        f = int(r["session_flags"])
        svc = (service_name(s.dst_port) or str(s.dst_port)) if f & SESSION_DST_SERVICE else None
        info = SessionInfo(s, st, bool(f & SESSION_LOCAL_SRC), bool(f & SESSION_LOCAL_DST),
                           bool(f & SESSION_SELF_SRC), bool(f & SESSION_SELF_DST), svc)
        if status is not None:
            info.status = SessionStatus.from_byte(status[k])
        if whitelist is not None:
            b = int(whitelist[k])
            info.is_whitelisted = WhitelistState.from_byte(b)
            if b & FB_WL_BLACKLISTED:
                info.whitelist_reason = "Session is blacklisted"
        if masks is not None:
            info.criticality = criticality_of(masks[k], bl_names)
        info.last_modified_ns = max(st.last_activity_ns or 0, int(stamps[k]) if stamps is not None else 0)
        if dom_ids is not None:
            src, dst = int(dom_ids[k][0]), int(dom_ids[k][1])
            info.src_domain = dom_names[src] if src else None
            info.dst_domain = dom_names[dst] if dst else None
        if l7_ids is not None and int(l7_ids[k]):
            info.l7 = l7_procs[int(l7_ids[k])]
        out.append(info)
    out.sort(key=lambda i: i.session.sort_key())
    return out


def flows_to_sessions(flows, histories=None, times=None, status=None, whitelist=None, blacklist=None, modified=None,
                      domains=None, l7=None):
    """fb_flow_rec records -> SessionInfo list sorted by the derived Ord of Session.  `histories`
    ({table slot: str}, FlodbaddGpuCapture.histories) supplies the history strings; the locality
    flags and dst_service come from fb_flow_rec.session_flags (stored at insert, src/packets.rs:
    429-466; dst_service = the key's dst port name, or its number for a port only a service table
    set at run time names).  `times` (timed contexts): FLOW_TIME_DTYPE records, either joined by
    table slot (fb_flow_export_times) or, when every slot field is 0, one per flow in `flows` order.
    `status` (timed contexts): the status byte of every table slot (fb_flow_status_dev), indexed by
    fb_flow_rec.slot, decoded into SessionInfo.status; a zero byte gives the insert status.
    `whitelist`: the whitelist state byte of every table slot (fb_flow_whitelist_dev), decoded into
    SessionInfo.is_whitelisted; without it every session is Unknown.  A byte with FB_WL_BLACKLISTED
    carries the reason "Session is blacklisted".  `blacklist`: (the mask word of every table slot,
    fb_flow_blacklist_dev; the list names), decoded into SessionInfo.criticality.  `modified`: the stamp
    of every table slot (fb_flow_modified_dev); SessionInfo.last_modified_ns is the later of it and the
    flow's last_activity_ns.  `domains`: (the name-id pair of every table slot, fb_flow_domains_dev; {name id:
    str}), decoded into SessionInfo.src_domain / dst_domain (id 0: None).  `l7`: (the process id of every table slot,
    fb_flow_l7_dev's process_id column; {process id: SessionL7}), decoded into SessionInfo.l7 (id 0: None).  The
    per-slot arguments may be arrays
    indexed by slot or {slot: value}.  Each argument's shape is decided here, once; the join itself (_join) runs
    over per-record columns."""
    if flows.dtype != FLOW_REC_DTYPE:
        raise TypeError("expected fb_flow_rec records (FLOW_REC_DTYPE), got %s" % flows.dtype)
    slots = flows["slot"]
    if times is not None and not (len(times) == len(flows) and not times["slot"].any()):
        row = {s: k for k, s in enumerate(times["slot"].tolist())}
        times = times[np.array([row[s] for s in slots.tolist()], dtype=np.intp)]
    bl_masks, bl_names = blacklist if blacklist is not None else (None, ())
    dom_ids, dom_names = domains if domains is not None else (None, None)
    l7_ids, l7_procs = l7 if l7 is not None else (None, None)
    return _join(flows, histories, times, _per_record(status, slots), _per_record(whitelist, slots),
                 _per_record(bl_masks, slots), bl_names, _per_record(modified, slots), _per_record(dom_ids, slots), dom_names,
                 _per_record(l7_ids, slots), l7_procs)


def views_to_sessions(views, histories=None, bl_names=None, timed=True, status=True, whitelist=True, blacklist=True,
                      domains=None, l7=None):
    """fb_flow_view records (fb_flow_export_view) -> the SessionInfo list flows_to_sessions builds from the
    separate exports: each view carries its flow's record, time record and per-slot plane elements -- a view row
    is the per-record join already -- so no other export is needed.  timed: the capture is timed (else the time
    records are zero and left out); status / whitelist / blacklist: decode that plane's element (a getter that
    does not decode a plane passes False here); bl_names: the list names of the blacklist masks; domains: as
    flows_to_sessions takes it, joined by slot (the view record itself carries no domain); l7: likewise."""
    if views.dtype != FLOW_VIEW_DTYPE:
        raise TypeError("expected fb_flow_view records (FLOW_VIEW_DTYPE), got %s" % views.dtype)
    col = lambda f, on=True: views[f].tolist() if on else None  # noqa: E731
    dom_ids, dom_names = domains if domains is not None else (None, None)
    l7_ids, l7_procs = l7 if l7 is not None else (None, None)
    return _join(views["rec"], histories, views["time"] if timed else None, col("status", status and timed),
                 col("wl_state", whitelist), col("bl_mask", blacklist), bl_names or [], col("stamp_ns"),
                 _per_record(dom_ids, views["rec"]["slot"]), dom_names, _per_record(l7_ids, views["rec"]["slot"]), l7_procs)


# ---- Zeek conn.log (format_sessions_zeek, src/sessions.rs:694-774) ------------------------
ZEEK_FIELDS = ["ts", "uid", "id.orig_h", "id.orig_p", "id.resp_h", "id.resp_p", "proto", "service", "duration",
               "orig_bytes", "resp_bytes", "conn_state", "local_orig", "local_resp", "missed_bytes", "history",
               "orig_pkts", "orig_ip_bytes", "resp_pkts", "resp_ip_bytes", "tunnel_parents"]
ZEEK_HEADER = "\t".join(ZEEK_FIELDS)
_MASK64 = (1 << 64) - 1


def _uid_mix(x):
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


def session_uid(session, start_time_ns):
    """The uid of a session: a = fb_flow_hash(key) (the library's host-side hash), b = mix(a ^ start_time_ns),
    the sixteen bytes a then b big-endian as a version-4, variant-1 UUID in lowercase 8-4-4-4-12 hex.  It does
    not depend on the table slot, so it survives growths and purges; a purged flow that returns starts at
    another time and gets another uid, as a new session does in the reference."""
    key = np.zeros(1, dtype=np.dtype(KEY_FIELDS))
    s, d, fam = session.key_fields()
    key[0]["src_ip"], key[0]["dst_ip"], key[0]["family"] = s, d, fam
    key[0]["src_port"], key[0]["dst_port"], key[0]["protocol"] = session.src_port, session.dst_port, int(session.protocol)
    a = int(gpu_lib().fb_flow_hash(ptr(key)))
    b = _uid_mix(a ^ (int(start_time_ns) & _MASK64))
    raw = bytearray(a.to_bytes(8, "big") + b.to_bytes(8, "big"))
    raw[6] = (raw[6] & 0x0F) | 0x40
    raw[8] = (raw[8] & 0x3F) | 0x80
    h = raw.hex()
    return "-".join((h[0:8], h[8:12], h[12:16], h[16:20], h[20:32]))


def rust_ip_str(ip):
    """An address as Rust's Display prints it (std::net): IPv4 dotted; IPv6 lowercase groups without leading
    zeros, the first longest run of two or more zero groups as "::", and an IPv4-mapped address as
    ::ffff:a.b.c.d -- the one form Python's str() printed differently (::ffff:102:304) before 3.13."""
    ip = ipaddress.ip_address(ip)
    if ip.version == 6 and int(ip) >> 32 == 0xFFFF:
        return "::ffff:%s" % ipaddress.IPv4Address(int(ip) & 0xFFFFFFFF)
    return ip.compressed


def format_sessions_zeek(sessions):
    """format_sessions_zeek (src/sessions.rs:694-774): the header, then one conn.log line per session of a
    timed capture, in the order given.  ts and duration take the reference's f64 path on purpose --
    repr(secs + micros / 1e6) is Rust's `{}` of the same sum (shortest round-trip, no exponent in this range,
    no ".0" for an integral value) and '%.6f' its `{:.6}` -- so this is the independent check of the device's
    integer formatting, not a copy of it.  The difference of the two times wraps to 64 bits as the record's
    does.  missed_bytes is 0: the reference never increments it (src/packets.rs)."""
    out = [ZEEK_HEADER]
    for info in sessions:
        st = info.stats
        if st.start_time_ns is None:
            raise ValueError("a Zeek line needs the session's capture times (a timed capture)")
        secs, micros = st.start_time_ns // 10 ** 9, st.start_time_ns % 10 ** 9 // 1000
        ts = repr(float(secs) + float(micros) / 1e6)
        ts = ts[:-2] if ts.endswith(".0") else ts
        if st.end_time_ns is None:
            duration = "-"
        else:
            d = ((st.end_time_ns - st.start_time_ns + (1 << 63)) & _MASK64) - (1 << 63)
            us = abs(d) // 1000 * (-1 if d < 0 else 1)  # num_microseconds truncates toward zero
            duration = "%.6f" % (float(us) / 1e6)
        s = info.session
        out.append("\t".join((
            ts, info.uid, rust_ip_str(s.src_ip), str(s.src_port), rust_ip_str(s.dst_ip), str(s.dst_port),
            "tcp" if s.protocol == Protocol.TCP else "udp", "-", duration, str(st.outbound_bytes),
            str(st.inbound_bytes), st.conn_state or "-", "-", "-", "0", st.history, str(st.orig_pkts),
            str(st.orig_ip_bytes), str(st.resp_pkts), str(st.resp_ip_bytes), "-")))
    return out


def pack_histories(histories, capacity):
    """{table slot: history str} -> (uint8 characters, uint64 off[capacity + 1]): the blob and per-slot offsets
    fb_format_zeek_dev reads (slot s's history is chars[off[s]:off[s + 1]]; a slot without one is empty)."""
    capacity = int(capacity)
    lens = np.zeros(capacity + 1, dtype=np.uint64)
    slots = np.fromiter(histories.keys(), dtype=np.int64, count=len(histories))
    if len(slots) and not (0 <= slots.min() and slots.max() < capacity):
        raise ValueError("history slots %d..%d outside the table (%d slots)" % (slots.min(), slots.max(), capacity))
    lens[slots + 1] = np.fromiter(map(len, histories.values()), dtype=np.uint64, count=len(histories))
    strs = list(histories.values())
    chars = np.frombuffer("".join(strs[k] for k in np.argsort(slots, kind="stable").tolist()).encode("ascii"),
                          dtype=np.uint8)
    return chars, np.cumsum(lens, dtype=np.uint64)


def filter_sessions(sessions: List[SessionInfo], flt: SessionFilter, lan_v6=()) -> List[SessionInfo]:
    """src/sessions.rs:678-692: is_local_session! / is_global_session! evaluate is_lan_ip on the
    session's addresses at call time (src/sessions.rs:660-672), not the flags stored at insert."""
    if flt == SessionFilter.LocalOnly:
        return [s for s in sessions if is_local_session(s, lan_v6)]
    if flt == SessionFilter.GlobalOnly:
        return [s for s in sessions if not is_local_session(s, lan_v6)]
    return list(sessions)


__all__ = ["Protocol", "SessionFilter", "Session", "SessionPacketData", "SessionStats", "SessionStatus", "SessionInfo", "SessionL7",
           "WhitelistState",
           "ip_to_words", "words_to_ip", "service_name", "records_to_packets", "flows_to_sessions", "views_to_sessions",
           "filter_sessions", "ZEEK_FIELDS", "ZEEK_HEADER", "session_uid", "rust_ip_str", "format_sessions_zeek",
           "pack_histories",
           "packets_to_parsed", "determine_conn_state", "histories_from_records", "is_lan_ip", "is_local_session",
           "META_HAS_FLAGS", "META_SWAP", "META_ORIGINATOR", "META_LOCAL_SRC", "META_LOCAL_DST",
           "META_SELF_SRC", "META_SELF_DST", "META_DST_SERVICE"]
