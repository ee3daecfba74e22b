"""ctypes binding of include/flodbadd_gpu.h (libflodbadd_gpu.so) + numpy record dtypes.

The GPU library is the product path: there is no CPU fallback.  `gpu_lib()` raises
NativeLibraryMissing if the in-tree .so is absent, and fb_create fails loudly without a gfx950.
"""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
GPU_LIB_PATH = os.environ.get("FLODBADD_GPU_LIB") or os.path.join(PKG, "libflodbadd_gpu.so")  # override: tools/
SYNTH_LIB_PATH = os.path.join(PKG, "libfb_synth.so")

FB_ABI_VERSION = 4
FB_MAX_BATCH_PACKETS = (1 << 27) - 1
FB_MAX_LAN_V6 = 64
FB_MAX_OWN_IPS = 64

# fb_err
FB_OK, FB_ERR_INVAL, FB_ERR_NOMEM, FB_ERR_HIP, FB_ERR_NODEV, FB_ERR_TABLE_FULL, FB_ERR_INTERNAL = 0, -1, -2, -3, -4, -5, -6
# fb_filter (SessionFilter discriminants, src/sessions.rs:173-178)
FB_FILTER_LOCAL_ONLY, FB_FILTER_GLOBAL_ONLY, FB_FILTER_ALL = 0, 1, 2
# fb_class
FB_CLASS_SESSION, FB_CLASS_DNS, FB_CLASS_DROP, FB_CLASS_FILTERED = 0, 1, 2, 3
# fb_meta_bits
META_HAS_FLAGS, META_SWAP, META_ORIGINATOR = 1, 2, 4
META_LOCAL_SRC, META_LOCAL_DST, META_SELF_SRC, META_SELF_DST, META_DST_SERVICE = 8, 16, 32, 64, 128

KEY_FIELDS = [("src_ip", "<u4", (4,)), ("dst_ip", "<u4", (4,)), ("src_port", "<u2"), ("dst_port", "<u2"),
              ("protocol", "u1"), ("family", "u1"), ("padding", "<u2")]
PKT_OUT_DTYPE = np.dtype(KEY_FIELDS + [
    ("packet_length", "<u4"), ("ip_packet_length", "<u4"), ("tcp_flags", "u1"), ("meta", "u1"),
    ("hist_char", "u1"), ("reserved", "u1"), ("pkt_index", "<u4")])
PARSED_DTYPE = np.dtype(KEY_FIELDS + [
    ("packet_length", "<u4"), ("ip_packet_length", "<u4"), ("tcp_flags", "u1"), ("has_flags", "u1"),
    ("reserved", "<u2"), ("pkt_index", "<u4")])
DNS_OUT_DTYPE = np.dtype([("pkt_index", "<u4"), ("payload_offset", "<u4"), ("payload_length", "<u4"),
                          ("protocol", "u1"), ("family", "u1"), ("reserved", "<u2")])
STATS_FIELDS = ["total_processed", "tcp_processed", "udp_processed", "ipv4_processed", "ipv6_processed",
                "new_sessions", "updated_sessions", "n_session", "n_dns", "n_drop", "n_filtered",
                "bad_offsets", "error", "reserved0", "reserved1", "reserved2"]
STATS_DTYPE = np.dtype([(f, "<u8") for f in STATS_FIELDS])
FLOW_REC_DTYPE = np.dtype(KEY_FIELDS + [
    ("outbound_bytes", "<u8"), ("inbound_bytes", "<u8"), ("orig_pkts", "<u8"), ("resp_pkts", "<u8"),
    ("orig_ip_bytes", "<u8"), ("resp_ip_bytes", "<u8"),
    ("first_seen", "<u8"), ("last_seen", "<u8"), ("end_seen", "<u8"), ("hist_len", "<u4"),
    ("hist_mask", "<u2"), ("conn_state", "u1"), ("end_mask", "u1"), ("slot", "<u4"), ("session_flags", "<u4"),
    ("segment_count", "<u4"), ("in_segment", "u1"), ("reserved", "u1", (3,))])
# fb_flow_mrec: a flow record exported for the multi-GPU merge (positions global, slot = the rank) and
# the update call of the flow's first S, s, H, h (FB_CALL_NONE: none)
FLOW_MREC_DTYPE = np.dtype([("rec", FLOW_REC_DTYPE), ("char_call", "<u4", (4,))])
FB_CALL_NONE = 0xFFFFFFFF
# fb_flow_time: a flow's capture-time state on a timed context (FB_CFG_TIMED)
FLOW_TIME_DTYPE = np.dtype([
    ("start_time_ns", "<u8"), ("last_activity_ns", "<u8"), ("end_time_ns", "<u8"),
    ("current_segment_start_ns", "<u8"), ("last_segment_end_ns", "<u8"),
    ("total_segment_interarrival_ms", "<i8"), ("segment_interarrival_div", "<u4"), ("segment_count", "<u4"),
    ("in_segment", "u1"), ("reserved", "u1", (3,)), ("slot", "<u4")])
assert FLOW_TIME_DTYPE.itemsize == 64
# fb_age_params / fb_age_stats (fb_flow_age: update_sessions_status, src/capture.rs:1497-1551) and the
# per-slot status byte of fb_flow_status_dev (0: never aged since insert = the insert status)
AGE_PARAMS_DTYPE = np.dtype([("activity_ns", "<u8"), ("current_ns", "<u8"), ("retention_ns", "<u8"),
                             ("reserved", "<u8")])
AGE_STATS_FIELDS = ["flows", "active", "added", "activated", "deactivated", "current", "purged", "remaining",
                    "max_partition"]
AGE_STATS_DTYPE = np.dtype([(f, "<u8") for f in AGE_STATS_FIELDS] + [("reserved", "<u8", (7,))])
assert AGE_PARAMS_DTYPE.itemsize == 32 and AGE_STATS_DTYPE.itemsize == 128
FB_AGE_PURGE = 1
STATUS_ACTIVE, STATUS_ADDED, STATUS_ACTIVATED, STATUS_DEACTIVATED, STATUS_CURRENT, STATUS_AGED = 1, 2, 4, 8, 16, 128
# fb_wl_endpoint / fb_wl_stats (fb_set_whitelist, fb_flow_whitelist: recompute_whitelist_for_sessions,
# src/whitelists.rs:810-1023) and the per-slot state byte of fb_flow_whitelist_dev (0: Unknown)
WL_ENDPOINT_DTYPE = np.dtype([("addr", "<u4", (4,)), ("family", "u1"), ("prefix", "u1"), ("protocol", "u1"),
                              ("flags", "u1"), ("port", "<u2"), ("reserved", "<u2"), ("as_number", "<u4"),
                              ("owner_id", "<u4"), ("country_id", "<u4"), ("reserved2", "<u4")])
WL_STATS_FIELDS = ["flows", "conforming", "nonconforming", "host_check", "changed"]
WL_STATS_DTYPE = np.dtype([(f, "<u8") for f in WL_STATS_FIELDS] + [("reserved", "<u8", (3,))])
# the same 40 bytes with the word at offset 36 under its second name: with FB_WL_HAS_PROCESS, the id of the
# endpoint's lower-cased process name (fb_set_l7_process_names' match_id; 0: the device has none).  Rows travel as
# WL_ENDPOINT_DTYPE, where the word is `reserved2`: rows.view(WL_ENDPOINT_PROC_DTYPE) names it.
WL_ENDPOINT_PROC_DTYPE = np.dtype([(n, WL_ENDPOINT_DTYPE.fields[n][0]) if n != "reserved2" else ("process_match_id", "<u4")
                                   for n in WL_ENDPOINT_DTYPE.names])
assert WL_ENDPOINT_DTYPE.itemsize == 40 and WL_STATS_DTYPE.itemsize == 64 and WL_ENDPOINT_PROC_DTYPE.itemsize == 40
FB_WL_NEVER = 0xFF
FB_WL_HAS_PORT, FB_WL_HAS_ASN, FB_WL_HAS_OWNER, FB_WL_HAS_COUNTRY, FB_WL_HAS_DOMAIN, FB_WL_HAS_PROCESS = 1, 2, 4, 8, 16, 32
FB_WL_CONFORMING, FB_WL_NONCONFORMING, FB_WL_HOST_CHECK, FB_WL_MASK_UNKNOWN = 1, 2, 4, 128
FB_WL_MAX_EXACT, FB_WL_MAX_OTHER = 1 << 24, 1 << 16
# domain patterns (fb_set_whitelist_dom): fb_wl_stats with reserved[0] under its second name (the flows left to
# the host because their name's row overflowed), fb_wl_dom_info, the row width and the pattern limits
WL_STATS_DOM_DTYPE = np.dtype([(f, "<u8") for f in WL_STATS_FIELDS] + [("dom_overflow", "<u8"), ("reserved", "<u8", (2,))])
WL_DOM_KINDS = ["exact", "suffix", "prefix", "general", "never"]
WL_DOM_INFO_DTYPE = np.dtype([("patterns", "<u8", (5,)), ("names_done", "<u8"), ("names_matched", "<u8"),
                              ("names_overflowed", "<u8")])
assert WL_STATS_DOM_DTYPE.itemsize == 64 and WL_DOM_INFO_DTYPE.itemsize == 64
FB_WL_MAX_GENERAL, FB_WL_NAME_MATCHES, FB_WL_MAX_PATTERNS = 1024, 8, (1 << 24) - 1
# the kernel's staging thresholds (fb_internal.h: kWlLdsRules, kWlLdsGroups), for the tests at them
WL_LDS_RULES, WL_LDS_GROUPS = 512, 512
# fb_bl_stats (fb_flow_blacklist: recompute_blacklist_for_sessions, src/blacklists.rs:456-731) and the
# whitelist state bit of the "Session is blacklisted" fallback (src/capture.rs:1858-1871)
BL_STATS_FIELDS = ["flows", "blacklisted", "changed", "newly_blacklisted", "cleared", "wl_marked"]
BL_STATS_DTYPE = np.dtype([(f, "<u8") for f in BL_STATS_FIELDS] + [("reserved", "<u8", (2,))])
assert BL_STATS_DTYPE.itemsize == 64
FB_BL_MARK_WHITELIST, FB_WL_BLACKLISTED = 1, 8
# the anomaly pass (fb_flow_anomaly: SessionAnalyzer, src/analyzer.rs): forest nodes, model parameters,
# the per-slot record of fb_flow_anomaly_dev (all zero: no pass has seen the flow) and the counters
FB_AN_FEATURES, FB_IF_MAX_TREES, FB_IF_MAX_TREE_NODES, FB_IF_MAX_DEPTH, FB_IF_LEAF = 10, 64, 255, 12, 0xFFFFFFFF
FB_AN_MAX_SERVICE_CODE = 1000000
IF_NODE_DTYPE = np.dtype([("normal", "<f8", (FB_AN_FEATURES,)), ("value", "<f8"), ("left", "<u4"), ("right", "<u4")])
AN_PARAMS_DTYPE = np.dtype([("mean", "<f8", (FB_AN_FEATURES,)), ("std", "<f8", (FB_AN_FEATURES,)),
                            ("suspicious_cut", "<f8"), ("abnormal_cut", "<f8"), ("has_stats", "<u4"),
                            ("sample_size", "<u4")])
AN_REC_DTYPE = np.dtype([("path_sum", "<f8"), ("diag", "<u4"), ("level", "u1"), ("reserved", "u1", (3,))])
AN_STATS_FIELDS = ["flows", "normal", "suspicious", "abnormal", "changed", "newly_anomalous", "cleared"]
AN_STATS_DTYPE = np.dtype([(f, "<u8") for f in AN_STATS_FIELDS] + [("reserved", "<u8")])
assert (IF_NODE_DTYPE.itemsize, AN_PARAMS_DTYPE.itemsize, AN_REC_DTYPE.itemsize, AN_STATS_DTYPE.itemsize) == (96, 184, 16, 64)
FB_AN_UNSEEN, FB_AN_NORMAL, FB_AN_SUSPICIOUS, FB_AN_ABNORMAL = 0, 1, 2, 3
FB_AN_DIAG_HIGH, FB_AN_DIAG_LOW, FB_AN_DIAG_DEVIATES = 1, 2, 3
# fb_flow_view / fb_view_query (fb_flow_export_view: one joined record per selected flow; the incremental
# getters, src/capture.rs:1578-1760): last_modified_ns = max(time.last_activity_ns, stamp_ns)
FLOW_VIEW_DTYPE = np.dtype([("rec", FLOW_REC_DTYPE), ("time", FLOW_TIME_DTYPE), ("last_modified_ns", "<u8"),
                            ("stamp_ns", "<u8"), ("bl_mask", "<u8"), ("an", AN_REC_DTYPE), ("status", "u1"),
                            ("wl_state", "u1"), ("reserved", "u1", (14,))])
VIEW_QUERY_DTYPE = np.dtype([("since_ns", "<u8"), ("set", "<u4"), ("filter", "<u4"), ("flags", "<u4"),
                             ("reserved", "<u4")])
assert FLOW_VIEW_DTYPE.itemsize == 256 and VIEW_QUERY_DTYPE.itemsize == 24
FB_VIEW_ALL, FB_VIEW_CURRENT, FB_VIEW_BLACKLISTED, FB_VIEW_WL_EXCEPTIONS, FB_VIEW_ANOMALOUS = 0, 1, 2, 3, 4
FB_VIEW_MODIFIED_SINCE = 1
# fb_learned_endpoint / fb_learn_stats (fb_flow_learn_endpoints_dev: the distinct endpoints of the selected flows,
# each with its least session; Whitelists.from_learned builds the custom whitelist from them)
LEARNED_ENDPOINT_DTYPE = np.dtype([("dst_ip", "<u4", (4,)), ("rep_src_ip", "<u4", (4,)), ("dst_port", "<u2"),
                                   ("rep_src_port", "<u2"), ("protocol", "u1"), ("family", "u1"), ("reserved", "<u2"),
                                   ("dst_name_id", "<u4"), ("rep_slot", "<u4"), ("sessions", "<u4"),
                                   ("reserved2", "<u4", (3,))])
LEARN_STATS_FIELDS = ["flows", "selected", "endpoints", "written", "rounds"]
LEARN_STATS_DTYPE = np.dtype([(f, "<u8") for f in LEARN_STATS_FIELDS] + [("reserved", "<u8", (3,))])
# the same 64 bytes with reserved2's first word under its second name: the flow's verbatim process name id
# (fb_set_l7_process_names' name_id; 0: no process, and always 0 while no name table is installed)
LEARNED_ENDPOINT_PROC_DTYPE = np.dtype([("dst_ip", "<u4", (4,)), ("rep_src_ip", "<u4", (4,)), ("dst_port", "<u2"),
                                        ("rep_src_port", "<u2"), ("protocol", "u1"), ("family", "u1"), ("reserved", "<u2"),
                                        ("dst_name_id", "<u4"), ("rep_slot", "<u4"), ("sessions", "<u4"),
                                        ("proc_name_id", "<u4"), ("reserved3", "<u4", (2,))])
assert LEARNED_ENDPOINT_DTYPE.itemsize == 64 and LEARN_STATS_DTYPE.itemsize == 64
assert LEARNED_ENDPOINT_PROC_DTYPE.itemsize == 64
# fb_zeek_stats (fb_format_zeek_dev: one Zeek conn.log line per fb_flow_view, formatted on the device), the
# longest line without its history, and the kernel's thresholds (fb_zeek.hip), for the tests at them: records
# per workgroup step, the step bytes staged in LDS, the history length the wave copies together
ZEEK_STATS_FIELDS = ["lines", "bytes", "lines_written", "ts_inexact", "hist_mismatch"]
ZEEK_STATS_DTYPE = np.dtype([(f, "<u8") for f in ZEEK_STATS_FIELDS] + [("reserved", "<u8", (3,))])
assert ZEEK_STATS_DTYPE.itemsize == 64
FB_ZEEK_FIXED_MAX, FB_ZEEK_STEP, FB_ZEEK_STAGE_BYTES, FB_ZEEK_COOP_HIST = 312, 256, 40000, 64
# device-resident history (fb_hist_store_*, fb_histstore.hip): the config and the counters, the characters of
# a block, and the thresholds from which a wave appends a run / decodes a chain together
HIST_STORE_CONFIG_DTYPE = np.dtype([("block_capacity", "<u8"), ("max_blocks", "<u8"), ("flags", "<u4"),
                                    ("reserved", "<u4", (3,))])
HIST_STORE_INFO_FIELDS = ["blocks_capacity", "blocks_high_water", "blocks_free", "blocks_in_use", "chars", "flows",
                          "appends", "missed_updates"]
HIST_STORE_INFO_DTYPE = np.dtype([(f, "<u8") for f in HIST_STORE_INFO_FIELDS])
assert (HIST_STORE_CONFIG_DTYPE.itemsize, HIST_STORE_INFO_DTYPE.itemsize) == (32, 64)
FB_HIST_BLOCK_CHARS, FB_HIST_COOP_RUN, FB_HIST_COOP_GATHER = 120, 32, 64
FB_SEGMENT_TIMEOUT_MS = 5000
FB_CFG_TIMED = 2
FB_QUEUE_SHARED = 1
# fb_session_flags (fb_flow_rec.session_flags: SessionInfo.is_local_src/dst, is_self_src/dst and
# dst_service is Some, at insert)
SESSION_LOCAL_SRC, SESSION_LOCAL_DST, SESSION_SELF_SRC, SESSION_SELF_DST, SESSION_DST_SERVICE = 1, 2, 4, 8, 16
# fb_flow_rec positions: (update call << 32) | pkt_index; FB_SEEN_NONE = None
FB_SEEN_NONE = (1 << 64) - 1
FB_HIST_CHARS = "SsHhFfRr><Aa-"
# fb_conn_state -> determine_conn_state string (src/packets.rs:539-559); 0 = None
CONN_STATES = {0: None, 1: "SF", 2: "S0", 3: "REJ", 4: "S1", 5: "-"}
ASN_RANGE_DTYPE = np.dtype([("start", "<u4", (4,)), ("end", "<u4", (4,)), ("as_number", "<u4"), ("record", "<u4"),
                            ("reserved", "<u4", (2,))])
CIDR_DTYPE = np.dtype([("addr", "<u4", (4,)), ("family", "<u4"), ("prefix", "<u4"), ("list", "<u4"),
                       ("reserved", "<u4")])
FLOW_ENRICH_DTYPE = np.dtype([("slot", "<u4"), ("flags", "<u4"), ("src_asn", "<i4"), ("dst_asn", "<i4"),
                              ("src_blacklists", "<u8"), ("dst_blacklists", "<u8")])
FB_MAX_BLACKLISTS = 64
# fb_dns_msg + constants (include/flodbadd_gpu.h, DNS divert parse)
DNS_MSG_DTYPE = np.dtype([("pkt_index", "<u4"), ("id", "<u2"), ("status", "u1"), ("flags", "u1"),
                          ("questions", "<u2"), ("answers", "<u2"), ("name_len", "<u2"), ("n_addrs", "u1"),
                          ("reserved", "u1")])
FB_DNS_MAX_NAME, FB_DNS_MAX_ADDRS = 256, 8
DNS_QUERY, DNS_HAS_QUESTION, DNS_REVERSE, DNS_NAME_TRUNCATED, DNS_ADDRS_TRUNCATED = 1, 2, 4, 8, 16
DNS_STATUS = ["ok", "header_too_short", "unexpected_eof", "bad_pointer", "unknown_label_format", "label_not_ascii",
              "invalid_query_type", "invalid_query_class", "invalid_type", "invalid_class", "wrong_rdata_length",
              "additional_opt"]
ENRICH_LOCAL_SRC, ENRICH_LOCAL_DST, ENRICH_SELF_SRC, ENRICH_SELF_DST = 1, 2, 4, 8
LAN_V6_DTYPE = np.dtype([("net", "<u4", (4,)), ("prefix", "<u4"), ("reserved", "<u4", (3,))])
FB_IP_DTYPE = np.dtype([("addr", "<u4", (4,)), ("family", "<u4"), ("reserved", "<u4", (3,))])
# the DNS tracker (fb_dns_track_*: DnsPacketProcessor, src/dns.rs:16-121) and the domain pass
# (fb_flow_domains: populate_domain_names, src/capture.rs:1307-1411)
DNS_TRACK_CONFIG_DTYPE = np.dtype([("name_capacity", "<u8"), ("addr_capacity", "<u8"), ("hash_mask", "<u8"),
                                   ("flags", "<u4"), ("reserved", "<u4")])
DNS_TRACK_STATS_FIELDS = ["messages", "queries", "responses", "matched", "resolutions", "names_new", "addrs_new",
                          "rounds"]
DNS_TRACK_STATS_DTYPE = np.dtype([(f, "<u8") for f in DNS_TRACK_STATS_FIELDS])
DNS_TRACK_INFO_FIELDS = ["names", "addrs", "name_capacity", "addr_capacity", "pending", "messages", "writes"]
DNS_TRACK_INFO_DTYPE = np.dtype([(f, "<u8") for f in DNS_TRACK_INFO_FIELDS] + [("reserved", "<u8")])
DNS_RESOLUTION_DTYPE = np.dtype([("ip", FB_IP_DTYPE), ("name_id", "<u4"), ("reserved", "<u4"), ("order", "<u8")])
FLOW_DOMAIN_DTYPE = np.dtype([("src_name_id", "<u4"), ("dst_name_id", "<u4")])
DOM_STATS_FIELDS = ["flows", "current", "src_set", "dst_set", "changed", "with_domain"]
DOM_STATS_DTYPE = np.dtype([(f, "<u8") for f in DOM_STATS_FIELDS] + [("reserved", "<u8", (2,))])
assert (DNS_TRACK_CONFIG_DTYPE.itemsize, DNS_TRACK_STATS_DTYPE.itemsize, DNS_TRACK_INFO_DTYPE.itemsize,
        DNS_RESOLUTION_DTYPE.itemsize, FLOW_DOMAIN_DTYPE.itemsize, DOM_STATS_DTYPE.itemsize) == (32, 64, 64, 48, 8, 64)
FB_DNS_IDS, FB_DNS_EXPIRY_NS, FB_DNS_MAX_NAMES, FB_DNS_NO_TIME = 65536, 30 * 10**9, (1 << 24) - 1, (1 << 64) - 1
# the L7 pass (fb_set_l7_sockets / fb_flow_l7: src/l7.rs:208-500, 1020-1279)
L7_SOCKET_DTYPE = np.dtype([("local_ip", "<u4", (4,)), ("remote_ip", "<u4", (4,)), ("local_port", "<u2"),
                            ("remote_port", "<u2"), ("protocol", "u1"), ("local_family", "u1"),
                            ("remote_family", "u1"), ("reserved0", "u1"), ("reserved1", "<u4"), ("process_id", "<u4")])
L7_REC_DTYPE = np.dtype([("process_id", "<u4"), ("source", "u1"), ("tries", "u1"), ("reserved", "<u2")])
L7_PARAMS_DTYPE = np.dtype([("max_retries", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (2,))])
L7_STATS_FIELDS = ["flows", "current", "looked_up", "exact", "fuzzy", "failed", "resolved", "changed"]
L7_STATS_DTYPE = np.dtype([(f, "<u8") for f in L7_STATS_FIELDS])
assert (L7_SOCKET_DTYPE.itemsize, L7_REC_DTYPE.itemsize, L7_PARAMS_DTYPE.itemsize, L7_STATS_DTYPE.itemsize) == (48, 8, 16, 64)
FB_L7_NONE, FB_L7_EXACT, FB_L7_FUZZY, FB_L7_FAILED = 0, 1, 2, 3
FB_L7_MAX_SOCKETS, FB_L7_DEFAULT_MAX_RETRIES = 1 << 22, 5

FB_SEG_FRAMES = 64
SEG_BYTES = FB_SEG_FRAMES * 56
FB_MAX_SEG_BATCHES = 32
FB_QUEUE_MAX_DEPTH = 32
# fb_seg_batch: one batch of fb_parse_classify_seg_batches_dev (device pointers as integers)
SEG_BATCH_DTYPE = np.dtype([("d_frames", "<u8"), ("frames_bytes", "<u8"), ("d_offsets", "<u8"), ("n", "<u4"),
                            ("reserved", "<u4"), ("d_out", "<u8"), ("d_seg", "<u8"), ("d_class", "<u8"),
                            ("d_stats", "<u8")])
assert SEG_BATCH_DTYPE.itemsize == 64


def seg_unpack(out_bytes, seg):
    """Densify a segmented batch (fb_parse_classify_seg_dev layout, include/flodbadd_gpu.h):
    returns (SESSION records, DNS records) in packet order, as the dense call would."""
    out_bytes = np.frombuffer(memoryview(out_bytes), dtype=np.uint8)
    seg = np.asarray(seg, dtype=np.uint32)
    recs, dns = [], []
    for s, w in enumerate(seg.tolist()):
        cs, cd = w & 0xFFFF, w >> 16
        base = s * SEG_BYTES
        if cs:
            recs.append(out_bytes[base: base + cs * 56].view(PKT_OUT_DTYPE))
        if cd:
            tail = out_bytes[base + SEG_BYTES - 16 * cd: base + SEG_BYTES].view(DNS_OUT_DTYPE)
            dns.append(tail[::-1])
    r = np.concatenate(recs) if recs else np.zeros(0, dtype=PKT_OUT_DTYPE)
    d = np.concatenate(dns) if dns else np.zeros(0, dtype=DNS_OUT_DTYPE)
    return r, d


assert PKT_OUT_DTYPE.itemsize == 56 and DNS_OUT_DTYPE.itemsize == 16 and PARSED_DTYPE.itemsize == 56
assert STATS_DTYPE.itemsize == 128 and FLOW_REC_DTYPE.itemsize == 136 and FLOW_MREC_DTYPE.itemsize == 152
assert LAN_V6_DTYPE.itemsize == 32 and FB_IP_DTYPE.itemsize == 32
assert ASN_RANGE_DTYPE.itemsize == 48 and CIDR_DTYPE.itemsize == 32 and FLOW_ENRICH_DTYPE.itemsize == 32
assert DNS_MSG_DTYPE.itemsize == 16


class FbConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("filter", C.c_uint32), ("service_bitmap", C.c_void_p),
                ("lan_v6", C.c_void_p), ("n_lan_v6", C.c_uint32), ("n_own_ips", C.c_uint32),
                ("own_ips", C.c_void_p), ("flow_capacity", C.c_uint64), ("max_batch_packets", C.c_uint32),
                ("flags", C.c_uint32), ("max_batch_bytes", C.c_uint64)]


FB_CFG_FIXED_TABLE = 1
FB_MAX_FLOW_CAPACITY = 1 << 25


class FlowTableInfo(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("partitions", C.c_uint64), ("generation", C.c_uint64),
                ("flows", C.c_uint64), ("max_partition", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class FbRingConfig(C.Structure):
    _fields_ = [("slots", C.c_uint32), ("max_packets", C.c_uint32), ("max_bytes", C.c_uint64),
                ("flags", C.c_uint32), ("copy_threads", C.c_uint32)]


FB_RING_NO_FLOW = 1
RING_DNS_DTYPE = np.dtype([("packet_seq", "<u8"), ("payload_offset", "<u8"), ("payload_length", "<u4"),
                           ("protocol", "u1"), ("family", "u1"), ("reserved", "<u2")])
assert RING_DNS_DTYPE.itemsize == 24


class NativeLibraryMissing(RuntimeError):
    pass


class FbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fb error %d: %s" % (code, msg))
        self.code = code


# Every symbol include/flodbadd_gpu.h declares: (name, restype, argtypes).
_P, _U32, _U64, _I = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
_PU32, _PU64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
FB_DEBUG_DENSE_STEAL_POLLS, FB_DEBUG_DENSE_OFFSET_SKEW, FB_DEBUG_VIEW_DIRECT, FB_DEBUG_ZEEK_DIRECT = 1, 2, 3, 4
FB_DEBUG_LEARN_HASH_MASK = 6  # (5 is unassigned)
FB_DEBUG_DNS_LAUNCH = 7
FB_DEBUG_WL_NAME_HASH_MASK = 8

GPU_SYMBOLS = [
    ("fb_abi_version", _U32, []),
    ("fb_last_error", C.c_char_p, []),
    ("fb_create", _P, [_I, C.POINTER(FbConfig)]),
    ("fb_destroy", _I, [_P]),
    ("fb_set_filter", _I, [_P, _U32]),
    ("fb_set_service_bitmap", _I, [_P, _P]),
    ("fb_set_lan_v6", _I, [_P, _P, _U32]),
    ("fb_set_own_ips", _I, [_P, _P, _U32]),
    ("fb_set_stage_event", _I, [_P, _P]),
    ("fb_set_session_records", _I, [_P, C.c_int]),
    ("fb_parse_classify_dev", _I, [_P, _P, _U64, _P, _U32, _P, _P, _P, _P, _P]),
    ("fb_parse_classify", _I, [_P, _P, _U64, _P, _U32, _P, _PU32, _P, _PU32, _P, _P, _P]),
    ("fb_process_parsed_dev", _I, [_P, _P, _U32, _P, _P, _P, _P]),
    ("fb_process_parsed", _I, [_P, _P, _U32, _P, _PU32, _P, _P, _P]),
    ("fb_flow_update_dev", _I, [_P, _P, _P, _P]),
    ("fb_process_dev", _I, [_P, _P, _U64, _P, _U32, _P, _P, _P, _P, _P]),
    ("fb_parse_classify_seg_dev", _I, [_P, _P, _U64, _P, _U32, _P, _P, _P, _P, _P]),
    ("fb_process_parsed_seg_dev", _I, [_P, _P, _U32, _P, _P, _P, _P, _P]),
    ("fb_seg_compact_dev", _I, [_P, _P, _P, _U32, _P, _P, _P]),
    ("fb_parse_classify_seg_batches_dev", _I, [_P, _P, _U32, _P]),
    ("fb_flow_update_seg_dev", _I, [_P, _P, _P, _U32, _P, _P]),
    ("fb_process_seg_dev", _I, [_P, _P, _U64, _P, _U32, _P, _P, _P, _P, _P]),
    ("fb_process_seg_async_dev", _I, [_P, _P, _U64, _P, _U32, _P, _P, _P, _P, _P]),
    ("fb_flow_join", _I, [_P, _P]),
    ("fb_flow_history_dev", _I, [_P, _P, _P, _P, _P]),
    ("fb_set_asn_tables", _I, [_P, _P, _U32, _P, _U32]),
    ("fb_set_blacklists", _I, [_P, _P, _U32]),
    ("fb_ip_lookup_dev", _I, [_P, _P, _U32, _P, _P, _P]),
    ("fb_flow_enrich_dev", _I, [_P, _U32, _P, _U64, _P, _P]),
    ("fb_dns_parse_dev", _I, [_P, _P, _U64, _P, _U32, _P, _P, _P, _P, _P]),
    ("fb_flow_count", _I, [_P, _PU64, _P]),
    ("fb_flow_export", _I, [_P, _P, _U64, _PU64, _P]),
    ("fb_flow_export_dev", _I, [_P, _P, _U64, _P, _P]),
    ("fb_flow_export_sessions", _I, [_P, _U32, _P, _U64, _PU64, _P]),
    ("fb_flow_export_sessions_dev", _I, [_P, _U32, _P, _U64, _P, _P]),
    ("fb_flow_clear", _I, [_P, _P]),
    ("fb_flow_table_info_get", _I, [_P, C.POINTER(FlowTableInfo)]),
    ("fb_flow_slot_remap", _I, [_P, _P, _U64, _PU64]),
    ("fb_flow_hash", _U64, [_P]),
    ("fb_flow_export_merge_dev", _I, [_P, _U32, _U32, _U64, _P, _U64, _P, _P]),
    ("fb_flow_export_merge_map_dev", _I, [_P, _U32, _U32, _P, _U32, _P, _U64, _P, _P]),
    ("fb_flow_merge_dev", _I, [_P, _P, _U64, _P, _P, _P]),
    ("fb_flow_update_records_dev", _I, [_P, _P, _U32, _P, _P]),
    ("fb_route_records_dev", _I, [_P, _P, _P, _U32, _U32, _U64, _P, _P, _P, _P, _P]),
    ("fb_flow_owner", _U32, [_P, _U32]),
    ("fb_ring_create", _P, [_P, C.POINTER(FbRingConfig)]),
    ("fb_ring_destroy", _I, [_P]),
    ("fb_ring_push", _I, [_P, _P, _U32]),
    ("fb_ring_push_block", _I, [_P, _P, _P, _U32]),
    ("fb_ring_reserve", _P, [_P, _U32]),
    ("fb_ring_reserve_block", _P, [_P, _U32, _U64, C.POINTER(C.c_void_p), _PU32]),
    ("fb_ring_submit", _I, [_P]),
    ("fb_ring_sync", _I, [_P]),
    ("fb_ring_stats", _I, [_P, _P, _PU64, _PU64]),
    ("fb_ring_poll_dns", _I, [_P, _P, _U32, _P, _U64, _PU32, _PU64]),
    ("fb_dev_alloc", _I, [C.POINTER(C.c_void_p), _U64]),
    ("fb_dev_free", _I, [_P]),
    ("fb_host_alloc_pinned", _I, [C.POINTER(C.c_void_p), _U64]),
    ("fb_host_free_pinned", _I, [_P]),
    ("fb_memcpy_h2d", _I, [_P, _P, _U64, _P]),
    ("fb_memcpy_d2h", _I, [_P, _P, _U64, _P]),
    ("fb_memset_dev", _I, [_P, _I, _U64, _P]),
    ("fb_stream_create", _I, [C.POINTER(C.c_void_p)]),
    ("fb_stream_destroy", _I, [_P]),
    ("fb_stream_sync", _I, [_P]),
    ("fb_event_create", _I, [C.POINTER(C.c_void_p)]),
    ("fb_event_destroy", _I, [_P]),
    ("fb_event_record", _I, [_P, _P]),
    ("fb_event_elapsed_ms", _I, [C.POINTER(C.c_float), _P, _P]),
    ("fb_event_query", _I, [_P]),
    ("fb_event_spin", _I, [_P]),
    ("fb_device_count", _I, [C.POINTER(C.c_int)]),
    ("fb_set_device", _I, [_I]),
    ("fb_ctx_device", _I, [_P, C.POINTER(C.c_int)]),
    ("fb_seg_queue_create", _P, [_P, _U32, _U32]),
    ("fb_seg_queue_create_ex", _P, [_P, _U32, _U32, _U32]),
    ("fb_seg_queue_submit", _I, [_P, _P, _PU64]),
    ("fb_seg_queue_query", _I, [_P, _U64]),
    ("fb_seg_queue_wait", _I, [_P, _U64]),
    ("fb_seg_queue_destroy", _I, [_P]),
    ("fb_seg_queue_set_limit", _I, [_P, _U64]),
    ("fb_debug_set", _I, [_P, _U32, _U64]),
    ("fb_set_frame_times", _I, [_P, _P]),
    ("fb_flow_export_times_dev", _I, [_P, _P, _U64, _P, _P]),
    ("fb_flow_export_times", _I, [_P, _P, _U64, _PU64, _P]),
    ("fb_flow_age", _I, [_P, _U64, _P, _U32, _P, _P]),
    ("fb_flow_status_dev", _I, [_P, _P, _U64, _P]),
    ("fb_set_whitelist", _I, [_P, _P, _U64, _P, _P, _U32]),
    ("fb_set_whitelist_dom", _I, [_P, _P, _U64, _P, _P, _P, _U64, _P, _P, _U32]),
    ("fb_wl_name_matches_dev", _I, [_P, _P, _U64, _P, _P, _P]),
    ("fb_wl_dom_info_get", _I, [_P, _P]),
    ("fb_clear_whitelist", _I, [_P]),
    ("fb_flow_whitelist", _I, [_P, _U32, _P, _P]),
    ("fb_flow_whitelist_dev", _I, [_P, _P, _U64, _P]),
    ("fb_flow_export_whitelist_dev", _I, [_P, _U32, _P, _U64, _P, _P]),
    ("fb_flow_blacklist", _I, [_P, _U32, _P, _P]),
    ("fb_flow_blacklist_dev", _I, [_P, _P, _U64, _P]),
    ("fb_flow_export_blacklisted_dev", _I, [_P, _P, _P, _U64, _P, _P]),
    ("fb_if_validate", _I, [_P, _U64, _P, _U32]),
    ("fb_set_service_codes", _I, [_P, _P]),
    ("fb_set_anomaly_model", _I, [_P, _P, _U64, _P, _U32, _P, _P]),
    ("fb_clear_anomaly_model", _I, [_P]),
    ("fb_flow_anomaly", _I, [_P, _U32, _P, _P]),
    ("fb_flow_anomaly_dev", _I, [_P, _P, _U64, _P]),
    ("fb_flow_export_anomalous_dev", _I, [_P, _U32, _P, _P, _U64, _P, _P]),
    ("fb_flow_features_dev", _I, [_P, _P, _P, _U64, _P, _P]),
    ("fb_if_score_dev", _I, [_P, _P, _U64, _P, _P]),
    ("fb_set_pass_time", _I, [_P, _U64]),
    ("fb_flow_modified_dev", _I, [_P, _P, _U64, _P]),
    ("fb_flow_export_view_dev", _I, [_P, _P, _P, _U64, _P, _P]),
    ("fb_flow_export_view", _I, [_P, _P, _P, _U64, _PU64, _P]),
    ("fb_flow_learn_endpoints_dev", _I, [_P, _P, _P, _U64, _P, _P, _P]),
    ("fb_format_zeek_dev", _I, [_P, _P, _U64, _P, _P, _U64, _P, _U64, _P, _P, _P]),
    ("fb_format_zeek_hist_dev", _I, [_P, _P, _U64, _P, _P, _P, _U64, _P, _P, _P]),
    ("fb_hist_store_enable", _I, [_P, _P]),
    ("fb_hist_store_append_dev", _I, [_P, _P]),
    ("fb_hist_store_lengths_dev", _I, [_P, _P, _U64, _U64, _P, _P]),
    ("fb_hist_store_gather_dev", _I, [_P, _P, _U64, _U64, _P, _P, _U64, _P]),
    ("fb_hist_store_info_get", _I, [_P, _P]),
    ("fb_dns_track_enable", _I, [_P, _P]),
    ("fb_dns_track_clear", _I, [_P]),
    ("fb_dns_track_dev", _I, [_P, _P, _P, _P, _U32, _P, _P, _P, _P, _P]),
    ("fb_dns_expire", _I, [_P, _U64, _PU64]),
    ("fb_dns_track_info_get", _I, [_P, _P]),
    ("fb_dns_export_resolutions_dev", _I, [_P, _P, _U64, _P, _P]),
    ("fb_dns_export_pending_dev", _I, [_P, _P, _P, _P]),
    ("fb_dns_names_dev", _I, [_P, _P, _U64, _P, _P, _P]),
    ("fb_dns_lookup_dev", _I, [_P, _P, _U64, _P, _P]),
    ("fb_flow_domains", _I, [_P, _U32, _P, _P]),
    ("fb_flow_domains_dev", _I, [_P, _P, _U64, _P]),
    ("fb_l7_validate", _I, [_P, _U64]),
    ("fb_set_l7_sockets", _I, [_P, _P, _U64]),
    ("fb_flow_l7", _I, [_P, _P, _P, _P]),
    ("fb_flow_l7_dev", _I, [_P, _P, _U64, _P]),
    ("fb_l7_clear", _I, [_P]),
    ("fb_l7_lookup_dev", _I, [_P, _P, _U64, _P, _P]),
    ("fb_set_l7_process_names", _I, [_P, _P, _P, _U64]),
]

_gpu = None


def gpu_lib():
    """Load libflodbadd_gpu.so (raises NativeLibraryMissing if it was not built)."""
    global _gpu
    if _gpu is None:
        if not os.path.exists(GPU_LIB_PATH):
            raise NativeLibraryMissing(
                "%s is missing: run `python -m flodbadd_amd.build` (there is no CPU fallback)" % GPU_LIB_PATH)
        lib = C.CDLL(GPU_LIB_PATH)
        for name, res, args in GPU_SYMBOLS:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.fb_abi_version() != FB_ABI_VERSION:
            raise NativeLibraryMissing("ABI version mismatch")
        _gpu = lib
    return _gpu


def check(rc):
    if rc != FB_OK:
        raise FbError(rc, gpu_lib().fb_last_error().decode(errors="replace"))
    return rc


def ptr(a):
    """ctypes void* of a numpy array's buffer (None for None)."""
    if a is None:
        return None
    return C.c_void_p(a.ctypes.data)


# ---- small device buffer / stream helpers ----------------------------------------------
class DeviceBuffer:
    """Raw device allocation (hipMalloc through the C ABI)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(gpu_lib().fb_dev_alloc(C.byref(p), self.nbytes))
        self.ptr = p

    def upload(self, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes > self.nbytes:
            raise ValueError("upload of %d bytes into a %d-byte device buffer" % (arr.nbytes, self.nbytes))
        check(gpu_lib().fb_memcpy_h2d(self.ptr, ptr(arr), arr.nbytes, stream))
        if stream is None:
            check(gpu_lib().fb_stream_sync(None))
        return self

    def download(self, arr, nbytes=None, stream=None):
        nb = arr.nbytes if nbytes is None else int(nbytes)
        check(gpu_lib().fb_memcpy_d2h(ptr(arr), self.ptr, nb, stream))
        check(gpu_lib().fb_stream_sync(stream))
        return arr

    def memset(self, value=0, stream=None):
        check(gpu_lib().fb_memset_dev(self.ptr, value, self.nbytes, stream))

    def free(self):
        if self.ptr:
            gpu_lib().fb_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedBuffer:
    """Page-locked host buffer exposed as a numpy uint8 array."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(gpu_lib().fb_host_alloc_pinned(C.byref(p), max(self.nbytes, 1)))
        self.ptr = p
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(self.nbytes, 1)).from_address(p.value))[: self.nbytes]

    def free(self):
        if self.ptr:
            gpu_lib().fb_host_free_pinned(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Stream:
    def __init__(self):
        p = C.c_void_p()
        check(gpu_lib().fb_stream_create(C.byref(p)))
        self.ptr = p

    def sync(self):
        check(gpu_lib().fb_stream_sync(self.ptr))

    def __del__(self):
        try:
            gpu_lib().fb_stream_destroy(self.ptr)
        except Exception:
            pass


class Event:
    def __init__(self):
        p = C.c_void_p()
        check(gpu_lib().fb_event_create(C.byref(p)))
        self.ptr = p

    def record(self, stream=None):
        check(gpu_lib().fb_event_record(self.ptr, stream.ptr if isinstance(stream, Stream) else stream))

    def wait_spin(self):
        """Poll until the event completed (no blocking wait, no wake-up latency), in C."""
        check(gpu_lib().fb_event_spin(self.ptr))

    def elapsed_ms(self, end):
        ms = C.c_float()
        check(gpu_lib().fb_event_elapsed_ms(C.byref(ms), self.ptr, end.ptr))
        return ms.value

    def __del__(self):
        try:
            gpu_lib().fb_event_destroy(self.ptr)
        except Exception:
            pass


def device_count():
    n = C.c_int(0)
    check(gpu_lib().fb_device_count(C.byref(n)))
    return n.value
