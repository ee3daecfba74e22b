/*
 * flodbadd_gpu.h -- C ABI of the MI355X (gfx950) packet-parse + flow-classification path.
 *
 * Drop-in boundary for edamametechnologies/flodbadd (reference @ 2025-07-18).  The reference
 * calls two Rust functions per captured frame from its capture task:
 *
 *   src/capture.rs:1038  parse_packet_pcap(&data)          -> Option<ParsedPacket>
 *   src/capture.rs:1046  process_parsed_packet(cp, &sessions, &current_sessions,
 *                                              &own_ips, &filter, l7)
 *   (async-capture twin at src/capture.rs:1224-1238)
 *
 * This header replaces that per-packet pair with batched, stream-ordered calls over a packed
 * frame buffer.  Every entry point is plain C (pointers + sizes, no torch/HIP types in the
 * signatures; streams are passed as `void*` = hipStream_t, NULL = the null stream).
 *
 * Conventions (mirroring the reference's error behaviour):
 *   - Every int-returning function returns FB_OK (0) or a negative fb_err; nothing aborts.
 *   - A frame the reference would reject (`parse_packet_pcap` returning None, src/packets.rs:
 *     603-802) is NOT an error: it is classified FB_CLASS_DROP.  A session packet rejected by
 *     the session filter (src/packets.rs:321-327) is FB_CLASS_FILTERED.  Port-53 traffic is
 *     FB_CLASS_DNS (src/packets.rs:638-650, 681-686) and is listed in the DNS side output.
 *   - A context is not thread-safe; use one per capture interface / stream, like the
 *     reference's one processor task per interface (src/capture.rs:1027).
 *   - Frames: `frames[offsets[i] .. offsets[i+1])` is frame i (caplen bytes, as libpcap hands
 *     `packet.data` to the reference, src/capture.rs:1092).  offsets has n+1 entries.
 *     A frame whose offsets are decreasing or exceed frames_bytes is classified DROP and
 *     counted in fb_batch_stats.bad_offsets.  Batches are limited to FB_MAX_BATCH_PACKETS
 *     packets and < 4 GiB of frame bytes (u32 offsets).
 */
#ifndef FLODBADD_GPU_H
#define FLODBADD_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FB_ABI_VERSION 4u /* 4: fb_flow_rec.segment_count / in_segment (136 B); 3: session_flags, error-word
                              bit 16, fb_flow_export_sessions* */
#define FB_MAX_BATCH_PACKETS ((1u << 27) - 1u)
#define FB_MAX_LAN_V6 64u  /* interface IPv6 (prefix, network) pairs, src/ip.rs:164-191 */
#define FB_MAX_OWN_IPS 64u /* per-interface own addresses, src/capture.rs:964-970      */
#define FB_SERVICE_BITMAP_BYTES 8192u
#define FB_MAX_FLOW_CAPACITY (1ull << 25) /* slots: 65,536 partitions of 512 (4 GiB of table)   */
#define FB_CFG_FIXED_TABLE 1u             /* fb_config.flags: never grow the flow table         */
#define FB_CFG_TIMED 2u                   /* fb_config.flags: capture-time state (fb_flow_time);
                                             every update call then needs fb_set_frame_times   */

/* Return codes. */
enum fb_err {
    FB_OK = 0,
    FB_ERR_INVAL = -1,      /* bad argument (NULL, size limits, bad enum)                 */
    FB_ERR_NOMEM = -2,      /* device or host allocation failed                           */
    FB_ERR_HIP = -3,        /* HIP runtime error; fb_last_error() has the text             */
    FB_ERR_NODEV = -4,      /* no gfx950 device / device index out of range                */
    FB_ERR_TABLE_FULL = -5, /* flow table capacity exhausted (some packets not counted)    */
    FB_ERR_INTERNAL = -6    /* kernel-side protocol failure (bounded spin expired)          */
};

/* SessionFilter, src/sessions.rs:173-178 (same discriminant order as the Rust enum). */
enum fb_filter { FB_FILTER_LOCAL_ONLY = 0, FB_FILTER_GLOBAL_ONLY = 1, FB_FILTER_ALL = 2 };

/* Per-packet class (the reference's Option<ParsedPacket> + filter outcome). */
enum fb_class {
    FB_CLASS_SESSION = 0,  /* ParsedPacket::SessionPacket that passed the filter -> out[]   */
    FB_CLASS_DNS = 1,      /* ParsedPacket::DnsPacket -> dns[]                              */
    FB_CLASS_DROP = 2,     /* parse_packet_pcap returned None                               */
    FB_CLASS_FILTERED = 3  /* SessionPacket rejected by the Local/Global filter             */
};

/* fb_pkt_out.meta bits. */
enum fb_meta_bits {
    FB_META_HAS_FLAGS = 1u << 0,  /* SessionPacketData.flags is Some (TCP)                  */
    FB_META_SWAP = 1u << 1,       /* canonical key = reversed raw 5-tuple                    */
    FB_META_ORIGINATOR = 1u << 2, /* is_originator, src/packets.rs:316-319                   */
    FB_META_LOCAL_SRC = 1u << 3,  /* is_lan_ip(key.src_ip), src/packets.rs:430               */
    FB_META_LOCAL_DST = 1u << 4,  /* is_lan_ip(key.dst_ip), src/packets.rs:431               */
    FB_META_SELF_SRC = 1u << 5,   /* own_ips.contains(key.src_ip), src/packets.rs:434        */
    FB_META_SELF_DST = 1u << 6,   /* own_ips.contains(key.dst_ip), src/packets.rs:435        */
    FB_META_DST_SERVICE = 1u << 7 /* dst_service is Some, src/packets.rs:441-464             */
};

/*
 * Session key, byte-identical to the reference's only C-ABI 5-tuple:
 * `struct session_key` (ebpf/l7_ebpf_program/src/l7_ebpf.c:26-34), mirrored by
 * `SessionKey` + `session_to_key` (src/l7_ebpf.rs:33-42, 78-104):
 *   IPv4: ip[0] = u32::from(Ipv4Addr) (numeric value, host byte order), ip[1..3] = 0.
 *   IPv6: ip[k] = u32::from_be_bytes(octets[4k..4k+4]).
 *   family from src_ip: 2 (AF_INET) / 10 (AF_INET6); protocol 6 (TCP) / 17 (UDP).
 */
typedef struct fb_session_key {
    uint32_t src_ip[4];
    uint32_t dst_ip[4];
    uint16_t src_port;
    uint16_t dst_port;
    uint8_t protocol;
    uint8_t family;
    uint16_t padding; /* always 0 */
} fb_session_key;     /* 40 bytes */

/*
 * One emitted session packet (class SESSION), in packet order.  Replaces the
 * SessionPacketData that reaches the DashMap upsert (src/packets.rs:85-98, 329-535).
 * `key` is the CANONICAL session key (src/packets.rs:245-311); the raw 5-tuple is `key`
 * reversed when FB_META_SWAP is set.
 */
typedef struct fb_pkt_out {
    fb_session_key key;        /*  0: canonical Session                                      */
    uint32_t packet_length;    /* 40: L4 payload bytes (SessionPacketData.packet_length)       */
    uint32_t ip_packet_length; /* 44: IPv4 total_length / IPv6 payload_length + 40             */
    uint8_t tcp_flags;         /* 48: TCP flags byte (0 when !HAS_FLAGS)                       */
    uint8_t meta;              /* 49: fb_meta_bits                                             */
    uint8_t hist_char;         /* 50: map_tcp_flags() char (src/packets.rs:561-601), 0 for UDP */
    uint8_t reserved;          /* 51: 0                                                        */
    uint32_t pkt_index;        /* 52: index of the frame in the batch                          */
} fb_pkt_out;                  /* 56 bytes */

/*
 * One SessionPacketData (src/packets.rs:92-98) -- the input of process_parsed_packet
 * (src/packets.rs:202) -- for hosts that keep their own decode and batch only the
 * classification + session-table part.  `session` is the Session AS PARSED (src = sender,
 * not canonicalised), in session_key layout; has_flags = flags.is_some().
 */
typedef struct fb_parsed_pkt {
    fb_session_key session;    /*  0 */
    uint32_t packet_length;    /* 40: L4 payload bytes                                        */
    uint32_t ip_packet_length; /* 44                                                          */
    uint8_t tcp_flags;         /* 48: ignored (taken as 0) when has_flags is 0                 */
    uint8_t has_flags;         /* 49: non-zero = Some(flags), 0 = None                         */
    uint16_t reserved;         /* 50: 0                                                        */
    uint32_t pkt_index;        /* 52: copied to fb_pkt_out.pkt_index                           */
} fb_parsed_pkt;               /* 56 bytes */

/* One DNS-diverted packet: payload = frames[payload_offset .. +payload_length). */
typedef struct fb_dns_out {
    uint32_t pkt_index;
    uint32_t payload_offset; /* absolute byte offset in the frame buffer; TCP: after the 2-byte
                                length prefix (src/packets.rs:646-647)                       */
    uint32_t payload_length;
    uint8_t protocol; /* 6 / 17 */
    uint8_t family;   /* 2 / 10 */
    uint16_t reserved;
} fb_dns_out; /* 16 bytes */

/* PACKET_STATS (src/packets.rs:28-83, 211-227, 336, 346) + batch bookkeeping. */
typedef struct fb_batch_stats {
    uint64_t total_processed; /* SessionPackets reaching process_parsed_packet (pre-filter)  */
    uint64_t tcp_processed;
    uint64_t udp_processed;
    uint64_t ipv4_processed;
    uint64_t ipv6_processed;
    uint64_t new_sessions;     /* flow-table inserts  (fb_flow_update only)                   */
    uint64_t updated_sessions; /* flow-table hits     (fb_flow_update only)                   */
    uint64_t n_session;        /* records written to out[] (class SESSION)                    */
    uint64_t n_dns;            /* records written to dns[] (class DNS)                        */
    uint64_t n_drop;           /* parse_packet_pcap -> None                                   */
    uint64_t n_filtered;       /* rejected by the session filter                              */
    uint64_t bad_offsets;      /* frames with invalid offsets (counted in n_drop too)         */
    uint64_t error;            /* nonzero = failure bits: 2 the two-pass dense path's offset scan
                                  waited too long (its records are not trusted and the update
                                  that follows skips them; FB_ERR_INTERNAL, not expected),
                                  4 flow-table partition full (FB_ERR_TABLE_FULL), 8 more records
                                  than the update scratch of the last parse launch holds,
                                  16 a table-update LDS spin expired (FB_ERR_INTERNAL),
                                  32 a dense tile offset put records past the batch (those
                                  records dropped, never written outside the buffers;
                                  FB_ERR_INTERNAL, not expected)                          */
    uint64_t reserved[3];
} fb_batch_stats; /* 128 bytes */

/* IPv6 LAN network (init_local_cache, src/ip.rs:164-191): ip & mask(prefix) == net. */
typedef struct fb_lan_v6 {
    uint32_t net[4]; /* network address, session_key word format (already masked)          */
    uint32_t prefix; /* 0..128                                                               */
    uint32_t reserved[3];
} fb_lan_v6; /* 32 bytes */

/* One own address (FlodbaddInterface v4/v6 addresses, src/capture.rs:964-970). */
typedef struct fb_ip {
    uint32_t addr[4]; /* session_key word format */
    uint32_t family;  /* 2 / 10 */
    uint32_t reserved[3];
} fb_ip; /* 32 bytes */

typedef struct fb_config {
    uint32_t abi_version;          /* must be FB_ABI_VERSION                                  */
    uint32_t filter;               /* fb_filter; FlodbaddCapture::new() uses GLOBAL_ONLY      */
    const uint8_t* service_bitmap; /* FB_SERVICE_BITMAP_BYTES; NULL -> built-in table
                                      (src/port_vulns_db.rs, bit p <=> name(p) != "")        */
    const fb_lan_v6* lan_v6;       /* may be NULL when n_lan_v6 == 0                          */
    uint32_t n_lan_v6;             /* <= FB_MAX_LAN_V6                                        */
    uint32_t n_own_ips;            /* <= FB_MAX_OWN_IPS                                       */
    const fb_ip* own_ips;          /* may be NULL when n_own_ips == 0                         */
    uint64_t flow_capacity;        /* INITIAL flow-table slots: rounded up to a power of two
                                      >= 512, at most FB_MAX_FLOW_CAPACITY; 0 = no table.
                                      Stored as partitions of 512 slots chosen by the key hash.
                                      The table grows (x2, rehashed on the device, before an
                                      update call) when the occupancy the last completed updates
                                      reported, projected over the updates still in flight,
                                      would fill a partition: the reference's map is unbounded
                                      (src/packets.rs:330).  A partition that still fills inside
                                      one batch reports error bit 4 (FB_ERR_TABLE_FULL)      */
    uint32_t max_batch_packets;    /* host-mode staging capacity (packets per call)           */
    uint32_t flags;                /* FB_CFG_*                                                */
    uint64_t max_batch_bytes;      /* host-mode staging capacity (frame bytes per call)       */
} fb_config;

/* determine_conn_state (src/packets.rs:539-559) outcome, fixed at the flow's first FIN/RST
 * packet (src/packets.rs:192-197, 422-426). */
enum fb_conn_state {
    FB_CONN_NONE = 0, /* conn_state None: no FIN/RST seen yet */
    FB_CONN_SF = 1,
    FB_CONN_S0 = 2,
    FB_CONN_REJ = 3,
    FB_CONN_S1 = 4,
    FB_CONN_OTHER = 5 /* "-" */
};

/* fb_flow_rec.hist_mask: bit k set <=> the history string contains FB_HIST_CHARS[k]
 * (map_tcp_flags alphabet, src/packets.rs:561-601). */
#define FB_HIST_CHARS "SsHhFfRr><Aa-"

/* A packet position in the stream of flow updates of one context: (update call << 32) | pkt_index,
 * where the update call counts fb_flow_update*_dev / fb_process*_dev calls since fb_create /
 * fb_flow_clear (from 0).  Stands for the wall-clock `now` the reference samples per packet
 * (src/packets.rs:209) -- a host maps it to capture timestamps.  FB_SEEN_NONE = None. */
#define FB_SEEN_NONE 0xFFFFFFFFFFFFFFFFull
#define FB_CALL_NONE 0xFFFFFFFFu /* fb_flow_mrec.char_call: the character has not occurred */

/* Flow-table export record: canonical key + SessionStats integer counters
 * (src/sessions.rs:76-82; update rules src/packets.rs:111-120, 383-391) + the ordered per-flow
 * state (src/packets.rs:187-198, 410-426): positions stand for start_time / last_activity /
 * end_time, hist_len = history.len(), conn_state as above.  The history string itself comes from
 * fb_flow_history_dev, batch by batch. */
typedef struct fb_flow_rec {
    fb_session_key key;      /*   0 */
    uint64_t outbound_bytes; /*  40 */
    uint64_t inbound_bytes;  /*  48 */
    uint64_t orig_pkts;      /*  56 */
    uint64_t resp_pkts;      /*  64 */
    uint64_t orig_ip_bytes;  /*  72 */
    uint64_t resp_ip_bytes;  /*  80 */
    uint64_t first_seen;     /*  88: position of the flow's first packet (start_time)         */
    uint64_t last_seen;      /*  96: position of its latest packet (last_activity)            */
    uint64_t end_seen;       /* 104: position of its first FIN/RST packet (end_time), or NONE */
    uint32_t hist_len;       /* 112: history.len() (TCP packets of the flow)                  */
    uint16_t hist_mask;      /* 116: characters present in history (FB_HIST_CHARS bits)       */
    uint8_t conn_state;      /* 118: fb_conn_state                                             */
    uint8_t end_mask;        /* 119: hist_mask & 0xFF at end_seen (the characters S s H h F f R r
                                conn_state was decided on); 0 while end_seen is NONE              */
    uint32_t slot;           /* 120: table slot (the flow id of fb_flow_history_dev)           */
    uint32_t session_flags;  /* 124: fb_session_flags as stored when the session was inserted
                                (src/packets.rs:429-435: is_local_src/dst, is_self_src/dst of the
                                canonical key under the configuration of that update call; and
                                dst_service is Some, src/packets.rs:441-466)                      */
    uint32_t segment_count;  /* 128: SessionStats.segment_count -- TCP packets with PSH: 1 for a
                                PSH first packet (src/packets.rs:414-420), +1 per later one
                                (140-160)                                                          */
    uint8_t in_segment;      /* 132: SessionStats.in_segment -- 0 right after a TCP PSH packet, 1
                                after any other (src/packets.rs:151-159, 376, 418)                 */
    uint8_t reserved[3];     /* 133 */
} fb_flow_rec;               /* 136 bytes.  Segment state under the no-timeout model: the
                                reference also ends a segment when a packet arrives >= 5 s of wall
                                clock after the flow's last one (segment_timeout, src/packets.rs:
                                137-149, 182-185); positions carry no clock.        */

/* Capture-time state of a flow on a timed context (fb_config.flags FB_CFG_TIMED; per-frame capture
 * timestamps handed to every update call with fb_set_frame_times).  The reference samples the wall
 * clock per packet (`now = Utc::now()`, src/packets.rs:230) and keeps, per session, start_time,
 * last_activity, end_time and the segment state (src/packets.rs:137-186 update, 352-380 + 414-426
 * insert): a TCP packet with PSH ends a segment, and so does any packet arriving >= 5 s
 * (segment_timeout, src/packets.rs:379) after the flow's previous one while a segment is open, which
 * then opens a new segment at that packet.  Here `now` is the frame's capture timestamp (ns), so the
 * state is a deterministic function of the input; chrono's num_milliseconds (truncation toward zero)
 * is applied to the same differences.  segment_count / in_segment of fb_flow_rec carry the timed state
 * on a timed context.  The reference accumulates total_segment_interarrival as an f64 running sum of
 * (ms / 1000.0) terms; this keeps the exact integer sum of the ms terms (the f64 running sum differs
 * from total_ms / 1000.0 by its own rounding, at most ~n ulp) and the divisor of the last accepted
 * term, so segment_interarrival = total_ms / 1000.0 / div (0.0 when div is 0). */
typedef struct fb_flow_time {
    uint64_t start_time_ns;            /*  0: SessionStats.start_time (the insert packet's time)      */
    uint64_t last_activity_ns;         /*  8: the flow's latest packet's time (arrival order)         */
    uint64_t end_time_ns;              /* 16: first FIN/RST packet's time; FB_SEEN_NONE = None          */
    uint64_t current_segment_start_ns; /* 24 */
    uint64_t last_segment_end_ns;      /* 32: FB_SEEN_NONE = None                                       */
    int64_t total_segment_interarrival_ms; /* 40: sum of the accepted segment interarrivals (ms)   */
    uint32_t segment_interarrival_div; /* 48: segment_count - 1 when the last term was accepted      */
    uint32_t segment_count;            /* 52: SessionStats.segment_count (timed)                       */
    uint8_t in_segment;                /* 56 */
    uint8_t reserved[3];               /* 57 */
    uint32_t slot;                     /* 60: table slot (joins fb_flow_rec.slot)                      */
} fb_flow_time;                        /* 64 bytes */
#define FB_SEGMENT_TIMEOUT_MS 5000 /* segment_timeout: 5.0 s, src/packets.rs:379 */

/* fb_flow_rec.session_flags (SessionInfo.is_local_src / is_local_dst / is_self_src / is_self_dst,
 * src/sessions.rs:40-61, set once at insert, src/packets.rs:429-435; bits 0-3 have the same values
 * as fb_enrich_bits) and FB_SESSION_DST_SERVICE: SessionInfo.dst_service is Some, i.e. the
 * service-port table names the canonical key's dst port at insert (src/packets.rs:441-466). */
enum fb_session_flags {
    FB_SESSION_LOCAL_SRC = 1u,
    FB_SESSION_LOCAL_DST = 2u,
    FB_SESSION_SELF_SRC = 4u,
    FB_SESSION_SELF_DST = 8u,
    FB_SESSION_DST_SERVICE = 16u
};

typedef struct fb_ctx fb_ctx;

/* ---- lifecycle ------------------------------------------------------------------------ */
uint32_t fb_abi_version(void);
const char* fb_last_error(void); /* thread-local text of the last failure */
fb_ctx* fb_create(int device, const fb_config* cfg); /* NULL on failure (see fb_last_error) */
int fb_destroy(fb_ctx* ctx);

/* ---- runtime configuration (each takes effect for the next call on the context) -------- */
int fb_set_filter(fb_ctx* ctx, uint32_t filter);                 /* set_filter, capture.rs:185 */
int fb_set_service_bitmap(fb_ctx* ctx, const uint8_t* bitmap);   /* CloudModel update, port_vulns.rs:350-380 */
int fb_set_lan_v6(fb_ctx* ctx, const fb_lan_v6* nets, uint32_t n); /* init_local_cache, ip.rs:164 */
int fb_set_own_ips(fb_ctx* ctx, const fb_ip* ips, uint32_t n);
/* Profiling hook (the reference's PACKET_STATS timing role, src/packets.rs:28-83): when `event`
 * (from fb_event_create, caller-owned; NULL clears) is set, fb_process_dev / fb_process_seg_dev
 * record it on their stream between the parse and the session-table update. */
int fb_set_stage_event(fb_ctx* ctx, void* event);
/* Timed contexts (FB_CFG_TIMED): the per-frame capture timestamps of the NEXT update call
 * (fb_flow_update*_dev, fb_process*_dev incl. the async and parsed-packet forms, fb_process_parsed):
 * d_ts[i] = frame i's capture time in ns since the Unix epoch (pcap header time, as the reference's
 * Utc::now() would read it), indexed by the records' pkt_index -- a DEVICE pointer that must stay
 * valid until that call's work completes on its stream (for fb_process_seg_async_dev: until
 * fb_flow_join or a later call's wait on it).  An update call that gets past the checks of its own
 * arguments consumes the pointer, whether it then succeeds or fails (a later refusal by its parse, an
 * allocation, a launch): the call after it needs fb_set_frame_times again.  A call refused for its own
 * arguments leaves the pointer armed, and an update call on a timed context with nothing armed fails
 * with FB_ERR_INVAL before doing anything.  Untimed contexts: fb_set_frame_times itself is refused. */
int fb_set_frame_times(fb_ctx* ctx, const uint64_t* d_ts);
/* Test / diagnostic knobs of one context (never needed in production; each takes effect for the
 * next call): FB_DEBUG_DENSE_STEAL_POLLS -- the polls a dense look-back waits for a predecessor's
 * word before computing that tile's sums itself (default 4096; 0 forces the fallback path);
 * FB_DEBUG_DENSE_OFFSET_SKEW -- fault injection, added (mod 2^32) to the session half of every
 * dense tile offset, as a corrupted look-back word would be (< 2^32; logged on stderr when set);
 * FB_DEBUG_VIEW_DIRECT -- non-zero: fb_flow_export_view_dev stores one record per lane instead of staging
 * a step's records in LDS (same result; the shape the staged copy-out is measured against);
 * FB_DEBUG_ZEEK_DIRECT -- non-zero: fb_format_zeek_dev stores every step's lines straight to global memory,
 * the path a step too large for the LDS staging takes (same bytes);
 * FB_DEBUG_LEARN_HASH_MASK -- ANDed into the fingerprint hash of fb_flow_learn_endpoints_dev before the tag
 * and the home slot are taken from it, so the tests can force equal tags and shared probe chains without
 * inverting the hash (as fb_dns_track_config.hash_mask); 0 restores all bits.  (Bit 63 is the tag's "used"
 * bit, set in every tag: a mask of bit 63 alone leaves no hash bit -- one tag, one home, one probe chain.);
 * FB_DEBUG_DNS_LAUNCH -- the number the DNS tracker gives its next kernel launch (the stamps of its table
 * slots are launch numbers, and a tracker past launch 0xF0000000 restamps what it holds before its next
 * call: a week of capture, or this knob).  FB_ERR_INVAL without fb_dns_track_enable, for 0 or a value of
 * 2^32 and more, and for a value below the current number -- going backwards would leave published slots
 * reading "not yet".;
 * FB_DEBUG_WL_NAME_HASH_MASK -- ANDed into the hash of a domain pattern and of every part of a name that is
 * looked up among the patterns (fb_set_whitelist_dom); 0 restores all bits.  Setting it rebuilds the installed
 * pattern tables and forgets the match state of every name; the rows never depend on it. */
enum fb_debug_knob {
    FB_DEBUG_DENSE_STEAL_POLLS = 1,
    FB_DEBUG_DENSE_OFFSET_SKEW = 2,
    FB_DEBUG_VIEW_DIRECT = 3,
    FB_DEBUG_ZEEK_DIRECT = 4,
    FB_DEBUG_LEARN_HASH_MASK = 6, /* (5 stays unassigned: the refusal of an unknown knob is tested with it) */
    FB_DEBUG_DNS_LAUNCH = 7,
    FB_DEBUG_WL_NAME_HASH_MASK = 8
};
int fb_debug_set(fb_ctx* ctx, uint32_t knob, uint64_t value);
/* Whether the fused parse + upsert calls (fb_process_seg_dev, fb_process_seg_async_dev) store the
 * SESSION records in d_out (default 1).  With 0 the session table is their only per-packet output,
 * as in the reference's capture loop, which drops each ParsedPacket once process_parsed_packet has
 * updated the DashMap (src/capture.rs:1036-1061): d_out then receives only the DNS side records at
 * the segment tails, d_seg / d_class / d_stats are unchanged, and the history, export and
 * enrichment calls work as before (the update reads the parse's own update entries either way). */
int fb_set_session_records(fb_ctx* ctx, int emit);

/*
 * Device-resident parse + classify (parse_packet_pcap + the per-packet part of
 * process_parsed_packet).  All pointers are DEVICE pointers; the call is asynchronous on
 * `stream`.  Outputs, all optional except d_stats:
 *   d_out   : >= n fb_pkt_out, class-SESSION records, packet order (stable compaction)
 *   d_dns   : >= n fb_dns_out, class-DNS records, packet order
 *   d_class : n bytes, fb_class of every frame
 *   d_stats : one fb_batch_stats (overwritten, not accumulated)
 * d_frames (here, in fb_process_dev, in the frame-taking *_seg_* calls and in fb_seg_batch) may
 * have any byte alignment: the kernels address the frames by offsets relative to it and check
 * every load against frames_bytes, and no byte at or past frames_bytes takes part in a result,
 * whatever lies there in memory.
 * One pass (k_parse_dense): 512-frame tiles whose batch-wide offsets come from a decoupled
 * look-back; a look-back that finds a predecessor tile unpublished for long computes that tile's
 * counts itself instead of waiting on it, so the call never depends on every workgroup being
 * resident and is safe on a GPU shared with other work.
 */
int fb_parse_classify_dev(fb_ctx* ctx, const uint8_t* d_frames, uint64_t frames_bytes,
                          const uint32_t* d_offsets, uint32_t n, fb_pkt_out* d_out,
                          fb_dns_out* d_dns, uint8_t* d_class, fb_batch_stats* d_stats,
                          void* stream);

/*
 * Host-memory variant: host buffers in, host buffers out (staged through the context's
 * pinned buffers with hipMemcpyAsync H2D/D2H).  Synchronous: returns after the results are
 * in host memory.  `out`/`dns` need room for n records; *n_out / *n_dns receive the counts.
 * Any of out, dns, cls, stats may be NULL.
 */
int fb_parse_classify(fb_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes,
                      const uint32_t* offsets, uint32_t n, fb_pkt_out* out, uint32_t* n_out,
                      fb_dns_out* dns, uint32_t* n_dns, uint8_t* cls, fb_batch_stats* stats,
                      void* stream);

/*
 * Flow-table upsert of SESSION records (the DashMap entry()/update_session_stats part of
 * process_parsed_packet, src/packets.rs:329-535, integer counters only).  d_recs/d_n are
 * device pointers; the record count is read on the device from d_stats->n_session of the
 * fb_parse_classify_dev call that produced them, so no host round trip is needed.
 * new_sessions / updated_sessions are ADDED into d_stats.
 */
int fb_flow_update_dev(fb_ctx* ctx, const fb_pkt_out* d_recs, fb_batch_stats* d_stats,
                       void* stream);
/* The same for dense records that did not come from this context's last parse (records routed from
 * other ranks, fb_route_records_dev; a host's own record buffer): max_n = a host bound of the count,
 * the count itself is d_stats->n_session on the device (min with max_n).  max_n = 0 is an update
 * call without records. */
int fb_flow_update_records_dev(fb_ctx* ctx, const fb_pkt_out* d_recs, uint32_t max_n, fb_batch_stats* d_stats,
                               void* stream);

/*
 * Batched process_parsed_packet (src/packets.rs:202-537) without the decode: canonical key,
 * originator, Local/Global filter, history char for each fb_parsed_pkt, stream-compacted into
 * d_out (class SESSION, input order).  A record with a protocol other than 6/17 or a family other
 * than 2/10 is classified DROP.  DEVICE pointers, asynchronous; follow with fb_flow_update_dev
 * for the session-table upsert.  d_class (n bytes) may be NULL; d_stats is required.
 */
int fb_process_parsed_dev(fb_ctx* ctx, const fb_parsed_pkt* d_in, uint32_t n, fb_pkt_out* d_out,
                          uint8_t* d_class, fb_batch_stats* d_stats, void* stream);
/* Host-memory variant of fb_process_parsed_dev followed by the session-table upsert when the
 * context has a flow table (new_sessions / updated_sessions filled).  Synchronous. */
int fb_process_parsed(fb_ctx* ctx, const fb_parsed_pkt* in, uint32_t n, fb_pkt_out* out,
                      uint32_t* n_out, uint8_t* cls, fb_batch_stats* stats, void* stream);

/* Device-resident parse + classify + flow upsert: fb_parse_classify_dev followed by
 * fb_flow_update_dev on the same stream (d_out is required: the update reads the records). */
int fb_process_dev(fb_ctx* ctx, const uint8_t* d_frames, uint64_t frames_bytes,
                   const uint32_t* d_offsets, uint32_t n, fb_pkt_out* d_out, fb_dns_out* d_dns,
                   uint8_t* d_class, fb_batch_stats* d_stats, void* stream);

/*
 * Segmented output (one wavefront-compacted segment per FB_SEG_FRAMES frames; no cross-segment
 * compaction, so the kernel streams with no inter-workgroup dependency).  Segment s holds the
 * frames [64s, 64s+64) and owns d_out records [64s, 64s+64) (3584 bytes):
 *   - its SESSION records, packet order, in records [64s, 64s + n_session(s))
 *   - its DNS side records (fb_dns_out, 16 B), packet order, the j-th at byte offset
 *     (s+1)*3584 - 16*(j+1) of d_out (packed at the segment's tail)
 *   - d_seg[s] = n_session(s) | n_dns(s) << 16; the other bytes are left unwritten.
 * d_out needs room for ceil(n/64)*64 records, d_seg for ceil(n/64) words.  Same classification,
 * record layout and stats as fb_parse_classify_dev (which compacts across the whole batch).
 * DEVICE pointers, asynchronous.  d_class may be NULL; d_stats is required.
 */
#define FB_SEG_FRAMES 64u
int fb_parse_classify_seg_dev(fb_ctx* ctx, const uint8_t* d_frames, uint64_t frames_bytes,
                              const uint32_t* d_offsets, uint32_t n, fb_pkt_out* d_out,
                              uint32_t* d_seg, uint8_t* d_class, fb_batch_stats* d_stats,
                              void* stream);
/*
 * Several segmented batches in ONE launch: the same results as fb_parse_classify_seg_dev called
 * once per batch (each batch its own frames, offsets, d_out, d_seg, d_class, d_stats), but the
 * kernel streams from one batch into the next without a launch boundary, so the per-launch
 * start-up (configuration load, the first offsets -> headers round trips) and the tail are paid
 * once.  `batches` is a HOST array of `count` (1..FB_MAX_SEG_BATCHES) descriptors holding DEVICE
 * pointers; each batch follows the fb_parse_classify_seg_dev rules.  Asynchronous.
 */
#define FB_MAX_SEG_BATCHES 32u
typedef struct fb_seg_batch {
    const uint8_t* d_frames;
    uint64_t frames_bytes;     /* < 4 GiB */
    const uint32_t* d_offsets; /* n + 1 entries */
    uint32_t n;
    uint32_t reserved;         /* 0 */
    fb_pkt_out* d_out;         /* ceil(n/64)*64 records */
    uint32_t* d_seg;           /* ceil(n/64) words */
    uint8_t* d_class;          /* n bytes, or NULL */
    fb_batch_stats* d_stats;   /* required */
} fb_seg_batch;                /* 64 bytes */
int fb_parse_classify_seg_batches_dev(fb_ctx* ctx, const fb_seg_batch* batches, uint32_t count, void* stream);

/* ---- resident queue-fed parse: one batch per call without a launch per batch ----------------
 * A capture loop that hands over one batch at a time (src/capture.rs:1036-1061 runs the pair per
 * packet; a GPU capture engine fills one device buffer at a time) pays a kernel launch per call
 * above: its prologue and the tail of the last segments.  fb_seg_queue_create launches ONE
 * resident parse kernel on an internal stream; fb_seg_queue_submit hands it a batch through a
 * ring in pinned host memory (no launch, no stream operation) and returns a ticket; the batch's
 * outputs (segmented layout and stats, exactly as fb_parse_classify_seg_dev writes them) are
 * complete once fb_seg_queue_query(ticket) returns FB_OK.  Not stream-ordered: the batch's frames
 * and offsets must be in device memory when it is submitted, and stay untouched (like its output
 * buffers) until its ticket completes.  The context's configuration is captured at create.  While
 * a queue lives its kernel holds two workgroups on every CU (every one must be resident: the grid is
 * sized by the occupancy query); what it leaves free -- the registers of a fifth wave per SIMD, a third
 * of the LDS -- runs copies and small kernels beside it, and a kernel that needs more of a CU waits
 * until fb_seg_queue_destroy.  One queue per device at a time (a second create fails with
 * FB_ERR_INVAL while the first lives).  A queue left idle for idle_ms (0 = 5,000 ms) stops itself,
 * and one whose blocks were not all running idle_ms after create (CUs held by other work) is
 * reported the same way: its calls then fail with FB_ERR_INTERNAL (destroy it, create a new one).
 * HARD RULES while a queue lives:
 *   - never hipFree / fb_dev_free device memory on its device: the free waits for the resident
 *     kernel (measured: a 1-MB hipFree waited 4.8 s, until the idle limit stopped the kernel, while
 *     hipMalloc, H2D and D2H copies did not wait) -- free only after fb_seg_queue_destroy;
 *   - one producer thread: submit / query / wait / destroy of one queue are not synchronised with
 *     each other (two concurrent submits would write the same ring slot and hand out one ticket);
 *   - at most FB_QUEUE_MAX_SUBMISSIONS batches over the queue's life (the kernel numbers batches in
 *     32 bits): the submit after that fails with FB_ERR_INVAL -- destroy the queue and create a new
 *     one (at ~24 us per 1M-frame batch that is ~28 h of continuous capture). */
#define FB_QUEUE_MAX_DEPTH 32u
#define FB_QUEUE_MAX_SUBMISSIONS (0xFFFFFFFFull - FB_QUEUE_MAX_DEPTH)
typedef struct fb_seg_queue fb_seg_queue;
fb_seg_queue* fb_seg_queue_create(fb_ctx* ctx, uint32_t depth /* 1..FB_QUEUE_MAX_DEPTH, 0 = 8 */, uint32_t idle_ms);
/* FB_QUEUE_SHARED: the kernel takes one workgroup on each of an eighth of the CUs (instead of two on
 * every CU), leaving the rest of the device to the session-table update kernels (K2's two 80-KB
 * workgroups need a CU's whole LDS), so a host can apply each completed batch to the context's
 * table (fb_flow_update_seg_dev on the batch's d_out / d_seg, on a stream of its own) while the
 * queue keeps parsing -- one batch per call WITH the upsert.  The update must then allocate nothing
 * (hipFree would wait for the queue): create the context with FB_CFG_FIXED_TABLE and
 * max_batch_packets >= the largest batch, and run no history / enrichment / export that grows
 * scratch while the queue lives. */
#define FB_QUEUE_SHARED 1u
fb_seg_queue* fb_seg_queue_create_ex(fb_ctx* ctx, uint32_t depth, uint32_t idle_ms, uint32_t flags);
/* Blocks only while `depth` batches are in flight (until the oldest of them completes). */
int fb_seg_queue_submit(fb_seg_queue* q, const fb_seg_batch* batch, uint64_t* ticket);
/* Lower this queue's submission limit below FB_QUEUE_MAX_SUBMISSIONS (tests of the limit; a host
 * that wants to recycle its queue earlier).  FB_ERR_INVAL if `limit` is above the maximum or below
 * the batches already submitted. */
int fb_seg_queue_set_limit(fb_seg_queue* q, uint64_t limit);
int fb_seg_queue_query(fb_seg_queue* q, uint64_t ticket); /* FB_OK done, 1 pending, < 0 error */
int fb_seg_queue_wait(fb_seg_queue* q, uint64_t ticket);  /* polls until done (no blocking wait) */
int fb_seg_queue_destroy(fb_seg_queue* q);                /* after the submitted batches complete */

/* Dense records from a segmented batch of n frames (d_seg_out / d_seg of the calls above): the
 * SESSION records into d_out and the DNS side records into d_dns, batch-wide packet order, as
 * fb_parse_classify_dev lays them out (either may be NULL).  The counts are those of the
 * segments (= n_session / n_dns of the batch's stats).  DEVICE pointers, asynchronous; one
 * compaction at a time per context (it uses context scratch). */
int fb_seg_compact_dev(fb_ctx* ctx, const fb_pkt_out* d_seg_out, const uint32_t* d_seg, uint32_t n,
                       fb_pkt_out* d_out, fb_dns_out* d_dns, void* stream);

/* fb_process_parsed_dev with segmented output (same segment layout; no DNS records). */
int fb_process_parsed_seg_dev(fb_ctx* ctx, const fb_parsed_pkt* d_in, uint32_t n,
                              fb_pkt_out* d_out, uint32_t* d_seg, uint8_t* d_class,
                              fb_batch_stats* d_stats, void* stream);
/* Flow-table upsert of the SESSION records of a segmented batch of n frames (d_out / d_seg of
 * fb_parse_classify_seg_dev or fb_process_parsed_seg_dev); new/updated ADDED into d_stats. */
int fb_flow_update_seg_dev(fb_ctx* ctx, const fb_pkt_out* d_out, const uint32_t* d_seg, uint32_t n,
                           fb_batch_stats* d_stats, void* stream);
/* fb_parse_classify_seg_dev followed by fb_flow_update_seg_dev on the same stream, with the same
 * results.  Prefer it when the records are only needed for the table: its parse also writes each
 * session record's table partition to context scratch, and its update's bucketing pass reads
 * those instead of re-reading and hashing the records (DESIGN.md §4 has the C4 timings). */
int fb_process_seg_dev(fb_ctx* ctx, const uint8_t* d_frames, uint64_t frames_bytes,
                       const uint32_t* d_offsets, uint32_t n, fb_pkt_out* d_out, uint32_t* d_seg,
                       uint8_t* d_class, fb_batch_stats* d_stats, void* stream);
/* Pipelined fb_process_seg_dev for a stream of batches (continuous capture): the parse of this
 * batch is ordered on `stream`, its table update runs on the context's own update stream after
 * it, and `stream` waits only for the update of the batch two calls back -- so each parse overlaps
 * the previous batch's update.  Same results as fb_process_seg_dev over the same batches.  The
 * parse's outputs (records, segment counts, stats' parse fields) are ordered on `stream` as usual;
 * the update's (new/updated sessions in d_stats, the table) only after fb_flow_join(ctx, stream).
 * d_out / d_seg / d_stats are read by the update until the call two batches later has been issued
 * (rotate two buffer sets: reusing the previous batch's buffers is allowed but waits for its
 * update, i.e. does not overlap).  Every other entry point that reads or writes the table (update,
 * export, count, clear, history, enrichment, the fused calls) joins the update stream itself. */
int fb_process_seg_async_dev(fb_ctx* ctx, const uint8_t* d_frames, uint64_t frames_bytes,
                             const uint32_t* d_offsets, uint32_t n, fb_pkt_out* d_out, uint32_t* d_seg,
                             uint8_t* d_class, fb_batch_stats* d_stats, void* stream);
/* Order `stream` after every table update fb_process_seg_async_dev has issued. */
int fb_flow_join(fb_ctx* ctx, void* stream);

/*
 * History characters of the LAST flow update on this context, grouped per flow: a stable sort of
 * that batch's TCP records (those with FB_META_HAS_FLAGS) by (flow slot, record order), i.e. for
 * every flow the characters it appended to its history string in this batch, in packet order
 * (src/packets.rs:187-198, 410-426).  d_hist[p] = fb_pkt_out.hist_char, d_hist_slot[p] = the
 * flow's fb_flow_rec.slot, for p < *d_n_hist (device u32).  Appending each run to the flow's
 * string, batch after batch, reproduces the reference's history.  Both arrays need room for the
 * last update's record slots: the n frames / packets of its batch (dense), ceil(n/64)*64
 * (segmented); slots past *d_n_hist are scratch.  The update's d_recs (and d_seg, d_stats) must
 * still be valid.  DEVICE pointers, asynchronous on `stream`.  A host that does not want the strings
 * itself enables the device store instead: fb_hist_store_append_dev appends the same runs on the device.
 */
int fb_flow_history_dev(fb_ctx* ctx, uint8_t* d_hist, uint32_t* d_hist_slot, uint32_t* d_n_hist,
                        void* stream);

/* ---- new-session enrichment (src/packets.rs:429-485; ASN src/asn.rs:32-63 + src/asn_db.rs:144-166;
 *      blacklists src/blacklists.rs:205-260, 456-560) -------------------------------------------- */
/* One ASN range (Db's RecordInternal, src/asn_db.rs:47-54) with IPs in session_key word layout.
 * One table per family, sorted by (start, end) as Db::from_tsv leaves it (src/asn_db.rs:137);
 * `record` is the caller's index of (as_number, country, owner). */
typedef struct fb_asn_range {
    uint32_t start[4];
    uint32_t end[4];
    uint32_t as_number;
    uint32_t record;
    uint32_t reserved[2];
} fb_asn_range; /* 48 bytes */
/* One IpNet of blacklist `list` (< FB_MAX_BLACKLISTS): addr/prefix as parsed (the host bits of
 * addr are ignored, as IpNet::contains does); a plain IP is a /32 or /128 (src/blacklists.rs:128-135). */
typedef struct fb_cidr {
    uint32_t addr[4];
    uint32_t family; /* 2 / 10 */
    uint32_t prefix;
    uint32_t list;
    uint32_t reserved;
} fb_cidr; /* 32 bytes */
#define FB_MAX_BLACKLISTS 64u
int fb_set_asn_tables(fb_ctx* ctx, const fb_asn_range* v4, uint32_t n4, const fb_asn_range* v6, uint32_t n6);
int fb_set_blacklists(fb_ctx* ctx, const fb_cidr* nets, uint32_t n);
/* Batched get_asn + is_ip_blacklisted for arbitrary addresses: d_asn[i] = fb_asn_range.record of
 * Db::lookup (its exact binary search), -1 = None; d_lists[i] bit l = some range of blacklist l
 * contains the address.  Either output may be NULL.  DEVICE pointers, asynchronous. */
int fb_ip_lookup_dev(fb_ctx* ctx, const fb_ip* d_ips, uint32_t n, int32_t* d_asn, uint64_t* d_lists,
                     void* stream);
/* The per-new-session lookups of process_parsed_packet for the flows in the table. */
typedef struct fb_flow_enrich {
    uint32_t slot;           /* fb_flow_rec.slot                                                  */
    uint32_t flags;          /* FB_ENRICH_* (src/packets.rs:429-435)                               */
    int32_t src_asn;         /* record of get_asn(src_ip) when !is_local_src, else -1 (packets.rs:468-485) */
    int32_t dst_asn;
    uint64_t src_blacklists; /* lists containing src_ip when !is_local_src (blacklists.rs:545-556) */
    uint64_t dst_blacklists;
} fb_flow_enrich;            /* 32 bytes */
enum fb_enrich_bits {
    FB_ENRICH_LOCAL_SRC = 1u, /* is_lan_ip(key.src_ip) */
    FB_ENRICH_LOCAL_DST = 2u,
    FB_ENRICH_SELF_SRC = 4u,  /* own_ips.contains(key.src_ip) */
    FB_ENRICH_SELF_DST = 8u
};
/* Enrich every flow of the table (new_only = 0) or only those the last update call created
 * (new_only = 1: the reference does these lookups when it inserts a session).  Records in no
 * particular order; *d_n (device u64) receives the count.  DEVICE pointers, asynchronous. */
int fb_flow_enrich_dev(fb_ctx* ctx, uint32_t new_only, fb_flow_enrich* d_out, uint64_t cap, uint64_t* d_n,
                       void* stream);

/* ---- DNS divert parse (src/dns.rs:35-99: DnsPacket::parse of dns-parser 0.8.0, then the query /
 *      response bookkeeping) ------------------------------------------------------------------ */
#define FB_DNS_MAX_NAME 256u  /* bytes of the dotted first-question name kept per message */
#define FB_DNS_MAX_ADDRS 8u   /* A / AAAA answers kept per message */
enum fb_dns_status {          /* DnsPacket::parse outcome (dns_parser::Error variants) */
    FB_DNS_OK = 0,
    FB_DNS_HEADER_TOO_SHORT = 1,
    FB_DNS_UNEXPECTED_EOF = 2,
    FB_DNS_BAD_POINTER = 3,
    FB_DNS_UNKNOWN_LABEL_FORMAT = 4,
    FB_DNS_LABEL_NOT_ASCII = 5,
    FB_DNS_INVALID_QUERY_TYPE = 6,
    FB_DNS_INVALID_QUERY_CLASS = 7,
    FB_DNS_INVALID_TYPE = 8,
    FB_DNS_INVALID_CLASS = 9,
    FB_DNS_WRONG_RDATA_LENGTH = 10,
    FB_DNS_ADDITIONAL_OPT = 11
};
enum fb_dns_flags {
    FB_DNS_QUERY = 1u,            /* header.query (QR bit clear)                              */
    FB_DNS_HAS_QUESTION = 2u,     /* questions.get(0) is Some                                 */
    FB_DNS_REVERSE = 4u,          /* the first qname ends with .in-addr.arpa / .ip6.arpa      */
    FB_DNS_NAME_TRUNCATED = 8u,   /* the name is longer than FB_DNS_MAX_NAME - 1 bytes         */
    FB_DNS_ADDRS_TRUNCATED = 16u  /* more than FB_DNS_MAX_ADDRS A / AAAA answers              */
};
typedef struct fb_dns_msg {
    uint32_t pkt_index;  /* the frame (fb_dns_out.pkt_index)                          */
    uint16_t id;         /* header.id (the transaction id the bookkeeping keys on)   */
    uint8_t status;      /* fb_dns_status                                            */
    uint8_t flags;       /* fb_dns_flags                                             */
    uint16_t questions;  /* header counts                                            */
    uint16_t answers;
    uint16_t name_len;   /* bytes of names[i] (dotted, no terminator needed)         */
    uint8_t n_addrs;     /* A / AAAA answers in addrs[i * FB_DNS_MAX_ADDRS ..]        */
    uint8_t reserved;
} fb_dns_msg;            /* 16 bytes */
/* Parse the DNS payloads of a batch's DNS side records (fb_parse_classify_dev's d_dns) the way
 * DnsPacket::parse does, keeping what process_dns_packet uses: id, query bit, the first
 * question's name, the A / AAAA answers in order.  n = d_dns entries; with d_stats non-NULL only
 * the first d_stats->n_dns (read on the device) are parsed.  d_names: n * FB_DNS_MAX_NAME bytes,
 * 4-byte aligned (the name is written a dword at a time; bytes past name_len are unspecified),
 * d_addrs: n * FB_DNS_MAX_ADDRS fb_ip.  DEVICE pointers, asynchronous.  The ordered bookkeeping
 * (pending queries by id, resolutions) runs on the device too, over these arrays where they lie:
 * fb_dns_track_dev below. */
int fb_dns_parse_dev(fb_ctx* ctx, const uint8_t* d_frames, uint64_t frames_bytes, const fb_dns_out* d_dns,
                     uint32_t n, const fb_batch_stats* d_stats, fb_dns_msg* d_msgs, char* d_names,
                     fb_ip* d_addrs, void* stream);

/* ---- DNS tracker: DnsPacketProcessor's state on the device (src/dns.rs:16-121) -------------------
 * pending_dns_queries (transaction id -> name) and dns_resolutions (address -> name) kept in device
 * memory and brought forward, in packet order, from what fb_dns_parse_dev wrote.  Names are interned:
 * every distinct first-question name (the exact bytes, case-sensitive) gets a name id, 1-based, that
 * never changes or disappears until fb_dns_track_clear; 0 means "none" everywhere. */
#define FB_DNS_EXPIRY_NS 30000000000ull /* pending queries this old are dropped (src/dns.rs:115-117) */
#define FB_DNS_MAX_NAMES ((1u << 24) - 1u) /* name ids are 24 bits */
typedef struct fb_dns_track_config {
    uint64_t name_capacity; /*  0: distinct names before the first growth (0 = 65,536)                  */
    uint64_t addr_capacity; /*  8: resolved addresses before the first growth (0 = 262,144)             */
    uint64_t hash_mask;     /* 16: testing knob: the bits of the 64-bit hashes that are used (0 = all);
                                   a narrow mask forces tag collisions and many insert rounds          */
    uint32_t flags;         /* 24: 0                                                                    */
    uint32_t reserved;      /* 28: 0                                                                    */
} fb_dns_track_config; /* 32 bytes */
typedef struct fb_dns_track_stats {
    uint64_t messages;    /*  0: messages read (min(n, d_stats->n_dns))                                 */
    uint64_t queries;     /*  8: queries accepted (status ok, a question, no reverse lookup)            */
    uint64_t responses;   /* 16: responses with status ok                                               */
    uint64_t matched;     /* 24: responses that took a pending name                                     */
    uint64_t resolutions; /* 32: address -> name writes (the kept answers of the matched responses)     */
    uint64_t names_new;   /* 40: names first seen in this call                                          */
    uint64_t addrs_new;   /* 48: addresses first seen in this call                                      */
    uint64_t rounds;      /* 56: insert rounds (kernel launches) of the longer of the two insert loops  */
} fb_dns_track_stats; /* 64 bytes */
typedef struct fb_dns_track_info {
    uint64_t names;         /*  0: names stored                                                         */
    uint64_t addrs;         /*  8: addresses stored                                                     */
    uint64_t name_capacity; /* 16: names / addresses the tables take before they grow                   */
    uint64_t addr_capacity; /* 24                                                                       */
    uint64_t pending;       /* 32: transaction ids with a pending query                                 */
    uint64_t messages;      /* 40: messages handed to fb_dns_track_dev so far (the next call's first order) */
    uint64_t writes;        /* 48: changes whenever a resolution is written, or the state is cleared    */
    uint64_t reserved;      /* 56                                                                       */
} fb_dns_track_info; /* 64 bytes */
typedef struct fb_dns_resolution {
    fb_ip ip;          /*  0                                                                            */
    uint32_t name_id;  /* 32                                                                            */
    uint32_t reserved; /* 36                                                                            */
    uint64_t order;    /* 40: the running message number of the response that wrote it                  */
} fb_dns_resolution; /* 48 bytes */
/* Make the tracker's state (cfg NULL: the defaults).  Works on a context without a flow table, as
 * fb_dns_parse_dev does; a context that never calls it allocates nothing and runs no tracker code.
 * FB_ERR_INVAL for non-zero flags / reserved, capacities above FB_DNS_MAX_NAMES / 2^28, or when
 * tracking is already enabled. */
int fb_dns_track_enable(fb_ctx* ctx, const fb_dns_track_config* cfg);
/* Empty the state (names, pending, resolutions, the message count); the domain plane of
 * fb_flow_domains is zeroed, since its ids die with the store.  FB_ERR_INVAL without tracking. */
int fb_dns_track_clear(fb_ctx* ctx);
/* Apply n parsed messages, in order, exactly as process_dns_packet does (src/dns.rs:35-99):
 *   status != FB_DNS_OK               skipped
 *   query, a question, not reverse    pending[id] = name
 *   any other query                   nothing
 *   response                          name = pending.remove(id); if there was one, every kept A / AAAA
 *                                     answer address -> name (the later packet wins)
 * d_msgs / d_names / d_addrs: DEVICE arrays as fb_dns_parse_dev writes them (d_names 4-byte aligned;
 * the bytes past name_len are ignored).  d_stats (may be NULL): only the first d_stats->n_dns messages
 * are read.  d_ts (may be NULL): frame times indexed by fb_dns_msg.pkt_index (fb_set_frame_times'
 * array); a query accepted without it never expires.  d_taken (may be NULL): n words, the name id each
 * response took, 0 for none and for non-responses.  `out` (HOST, may be NULL): the call's counters.
 * SYNCHRONOUS: the insert rounds read a device counter between launches, and the tables grow before a
 * call that could fill them.  FB_ERR_TABLE_FULL (state unchanged) when they cannot grow, FB_ERR_INVAL
 * (state unchanged) without tracking, for a misaligned d_names, or when the message count would pass 2^40. */
int fb_dns_track_dev(fb_ctx* ctx, const fb_dns_msg* d_msgs, const char* d_names, const fb_ip* d_addrs, uint32_t n,
                     const fb_batch_stats* d_stats, const uint64_t* d_ts, uint32_t* d_taken,
                     fb_dns_track_stats* out, void* stream);
/* Drop the pending queries whose capture time t has now_ns - t >= FB_DNS_EXPIRY_NS (the reference keeps
 * the younger ones, src/dns.rs:115-117); queries stored without a time stay.  *dropped (HOST, may be
 * NULL).  Synchronous. */
int fb_dns_expire(fb_ctx* ctx, uint64_t now_ns, uint64_t* dropped);
int fb_dns_track_info_get(fb_ctx* ctx, fb_dns_track_info* out); /* synchronous (counts pending) */
/* Every resolution, in no particular order; *d_n (device u64) receives their number, the first
 * min(cap, *d_n) are stored.  DEVICE pointers, asynchronous. */
int fb_dns_export_resolutions_dev(fb_ctx* ctx, fb_dns_resolution* d_out, uint64_t cap, uint64_t* d_n, void* stream);
/* pending, indexed by transaction id: d_name_id[65536] (0: none) and d_time[65536] (may be NULL;
 * UINT64_MAX: stored without a time).  DEVICE pointers, asynchronous. */
int fb_dns_export_pending_dev(fb_ctx* ctx, uint32_t* d_name_id, uint64_t* d_time, void* stream);
/* The strings of n ids: d_out[n * FB_DNS_MAX_NAME] (zero-filled past the length), d_len[n]; an
 * unknown id gives length 0.  DEVICE pointers, asynchronous. */
int fb_dns_names_dev(fb_ctx* ctx, const uint32_t* d_ids, uint64_t n, char* d_out, uint16_t* d_len, void* stream);
/* dns_resolutions.get(ip) for n addresses: the name id, 0 for none -- the domain pass's own device
 * function.  DEVICE pointers, asynchronous. */
int fb_dns_lookup_dev(fb_ctx* ctx, const fb_ip* d_ips, uint64_t n, uint32_t* d_name_id, void* stream);

/* ---- domain pass: populate_domain_names (src/capture.rs:1307-1411) over the tracked resolutions --
 * For every CURRENT flow (FB_VIEW_CURRENT's predicate: status byte 0, or FB_STATUS_CURRENT set; without
 * a status plane every flow) each side whose address has a resolution, whose name is neither "Unknown"
 * nor "Resolving" and whose id differs from the stored one is written; nothing is ever unset.  A flow
 * with either side written counts as `changed` and gets the pass time (fb_set_pass_time).  The ids live
 * in a per-slot plane made by the first pass; they follow their flows through a growth and a purge, and
 * fb_flow_clear / fb_dns_track_clear zero them. */
typedef struct fb_flow_domain {
    uint32_t src_name_id; /* 0 */
    uint32_t dst_name_id; /* 4 */
} fb_flow_domain; /* 8 bytes */
typedef struct fb_dom_stats {
    uint64_t flows;       /*  0: flows in the table                                                     */
    uint64_t current;     /*  8: of them current (the ones looked up)                                   */
    uint64_t src_set;     /* 16: source ids written                                                     */
    uint64_t dst_set;     /* 24: destination ids written                                                */
    uint64_t changed;     /* 32: flows with either side written                                         */
    uint64_t with_domain; /* 40: flows with either id non-zero after the pass                           */
    uint64_t reserved[2]; /* 48                                                                         */
} fb_dom_stats; /* 64 bytes */
/* Synchronous: waits for the updates in flight, like fb_flow_blacklist; timed and untimed contexts.
 * `flags` must be 0; `out` may be NULL.  FB_ERR_INVAL without a flow table or without tracking. */
int fb_flow_domains(fb_ctx* ctx, uint32_t flags, fb_dom_stats* out, void* stream);
/* The ids of every table slot (min(cap, capacity) records, slot order; zeros before the first pass)
 * into DEVICE memory.  Asynchronous. */
int fb_flow_domains_dev(fb_ctx* ctx, fb_flow_domain* d_out, uint64_t cap, void* stream);

/* ---- L7 pass: process attribution against a socket snapshot (src/l7.rs:208-500, 1020-1279) ----------
 * The host hands over what the reference's resolver task reads from the OS -- one ordered socket list
 * with the owning process of each socket as an id of the caller's -- and one call of fb_flow_l7 is one
 * cycle of that task over the sessions populate_l7 (src/capture.rs:1414-1495) would have queued: every
 * CURRENT flow (fb_flow_domains' predicate) that has no process yet and is not marked failed is looked up.
 *   exact  try_exact_match_from_index: a socket of the flow's protocol whose (local, remote) is (src, dst)
 *          -- form A -- or (dst, src) -- form B --; UDP compares the local side only.  With src_port !=
 *          dst_port the lowest-index form-A socket, else the lowest-index form-B socket; with equal ports
 *          the lowest index of either.  Addresses compare as IpAddr: the family counts.
 *   fuzzy  try_fuzzy_match, only after an exact miss: the lowest-index socket of the flow's protocol whose
 *          local_port is src_port or dst_port and whose local address is 0.0.0.0, ::, src_ip or dst_ip
 *          (any pairing of port and address).
 * A socket none of whose pids is a known process makes the reference's scan continue
 * (extract_l7_from_socket, src/l7.rs:1137-1199): the host leaves such sockets out.  A looked-up flow that
 * matches nothing has `tries` raised by one (it stays at 255); once tries > max_retries it is
 * FB_L7_FAILED and is not looked up again (src/l7.rs:456-470).  A flow that gets a process counts as
 * `changed` and gets the pass time (fb_set_pass_time; src/capture.rs:1470-1474); the retry bookkeeping
 * does not stamp.  A resolved flow is never looked up again (src/l7.rs:919-922, src/capture.rs:1452).
 * The elements live in a per-slot plane made by the first pass; they follow their flows through a growth
 * and a purge, and fb_flow_clear / fb_l7_clear zero them. */
#define FB_L7_MAX_SOCKETS (1u << 22)
#define FB_L7_DEFAULT_MAX_RETRIES 5u /* MAX_L7_RETRIES, src/l7.rs:83-89 */
typedef struct fb_l7_socket {
    uint32_t local_ip[4];  /*  0: session_key word order (IPv4: word 0, the others 0)                  */
    uint32_t remote_ip[4]; /* 16                                                                       */
    uint16_t local_port;   /* 32                                                                       */
    uint16_t remote_port;  /* 34                                                                       */
    uint8_t protocol;      /* 36: 6 / 17                                                               */
    uint8_t local_family;  /* 37: 2 / 10                                                               */
    uint8_t remote_family; /* 38: TCP 2 / 10; UDP 0 (2 / 10 accepted: the remote side is ignored)      */
    uint8_t reserved0;     /* 39: 0                                                                    */
    uint32_t reserved1;    /* 40: 0                                                                    */
    uint32_t process_id;   /* 44: >= 1, the caller's id of the first pid found in its process table    */
} fb_l7_socket; /* 48 bytes; the array is in the snapshot's list order, which is part of the input */
enum fb_l7_source { FB_L7_NONE = 0, FB_L7_EXACT = 1, FB_L7_FUZZY = 2, FB_L7_FAILED = 3 };
typedef struct fb_l7_rec {
    uint32_t process_id; /* 0: 0 = no process                                                          */
    uint8_t source;      /* 4: fb_l7_source                                                            */
    uint8_t tries;       /* 5: lookups that matched nothing (0 once resolved)                          */
    uint16_t reserved;   /* 6: 0                                                                       */
} fb_l7_rec; /* 8 bytes */
typedef struct fb_l7_params {
    uint32_t max_retries; /* 0: 0..255; 255 never fails a flow                                         */
    uint32_t flags;       /* 4: 0                                                                      */
    uint32_t reserved[2]; /* 8: 0                                                                      */
} fb_l7_params; /* 16 bytes; NULL = {FB_L7_DEFAULT_MAX_RETRIES, 0} */
typedef struct fb_l7_stats {
    uint64_t flows;     /*  0: flows in the table                                                      */
    uint64_t current;   /*  8: of them current                                                         */
    uint64_t looked_up; /* 16: of them without a process and not failed: the ones looked up            */
    uint64_t exact;     /* 24: resolved by the exact phase in this call                                */
    uint64_t fuzzy;     /* 32: resolved by the fuzzy phase in this call                                */
    uint64_t failed;    /* 40: became FB_L7_FAILED in this call                                        */
    uint64_t resolved;  /* 48: flows with a process after the call                                     */
    uint64_t changed;   /* 56: exact + fuzzy: the flows stamped                                        */
} fb_l7_stats; /* 64 bytes */
/* The checks fb_set_l7_sockets makes, on the host alone: FB_ERR_INVAL for a bad protocol or family, a
 * process_id of 0, a non-zero reserved field, an IPv4 address with a non-zero word 1-3, or
 * n > FB_L7_MAX_SOCKETS. */
int fb_l7_validate(const fb_l7_socket* socks, uint64_t n);
/* Install a snapshot: the list is copied and indexed before the call returns (n == 0: a valid, empty
 * snapshot).  FB_ERR_INVAL (fb_l7_validate) leaves the installed snapshot as it was.  Nothing is ever
 * truncated.  Synchronous. */
int fb_set_l7_sockets(fb_ctx* ctx, const fb_l7_socket* socks, uint64_t n);
/* One pass.  Synchronous: waits for the updates in flight, like fb_flow_domains; timed and untimed
 * contexts.  `params` may be NULL (the defaults), `out` may be NULL.  FB_ERR_INVAL without a flow table,
 * without an installed snapshot, or for max_retries > 255 / non-zero flags or reserved words. */
int fb_flow_l7(fb_ctx* ctx, const fb_l7_params* params, fb_l7_stats* out, void* stream);
/* The element of every table slot (min(cap, capacity) records, slot order; zeros before the first pass)
 * into DEVICE memory.  Asynchronous. */
int fb_flow_l7_dev(fb_ctx* ctx, fb_l7_rec* d_out, uint64_t cap, void* stream);
/* Drop the snapshot and zero the plane: every flow is unresolved again.  Synchronous. */
int fb_l7_clear(fb_ctx* ctx);
/* The match of n caller-supplied keys (session_key layout, as fb_flow_rec carries them) against the
 * installed snapshot with the pass's own device function: d_out[i] = {process_id, FB_L7_EXACT / _FUZZY or
 * 0, 0, 0}.  FB_ERR_INVAL without a snapshot.  DEVICE pointers, asynchronous. */
int fb_l7_lookup_dev(fb_ctx* ctx, const fb_session_key* d_keys, uint64_t n, fb_l7_rec* d_out, void* stream);
/* The names of the L7 plane's process ids, for the process-aware whitelist check and learning (DESIGN.md
 * 3.19).  For a process id p < n: match_id[p] is the caller's id (>= 1) of the ASCII-lower-cased process name
 * -- the reference matches with eq_ignore_ascii_case (src/whitelists.rs:716-724) --, name_id[p] the caller's
 * id (>= 1) of the name verbatim -- new_from_sessions' fingerprint compares the string itself, so "Curl" and
 * "curl" are two endpoints but one match class.  Entry 0 stands for "no process" and is stored as 0.
 * A flow's process is x = its fb_l7_rec.process_id when the plane exists, x != 0 and x < n; else it has none
 * (no L7 pass yet, unresolved, FB_L7_FAILED, an id beyond the table).  The arrays are copied (HOST pointers);
 * a second call replaces the table, n == 0 removes it.  FB_ERR_INVAL for a zero id at p >= 1 or a NULL array
 * with n != 0; an invalid call leaves the installed table as it was.  fb_l7_clear and fb_flow_clear zero the
 * plane and leave the table.  Without a table every pass runs as it did before this call existed.
 * Synchronous. */
int fb_set_l7_process_names(fb_ctx* ctx, const uint32_t* match_id, const uint32_t* name_id, uint64_t n);

int fb_flow_count(fb_ctx* ctx, uint64_t* n_flows, void* stream); /* synchronous */
/* Copy every flow (slot order) to host memory; *n = flows written (<= cap). Synchronous. */
int fb_flow_export(fb_ctx* ctx, fb_flow_rec* out, uint64_t cap, uint64_t* n, void* stream);
/* Same, into DEVICE memory; *d_n (device u64) receives the count. Asynchronous. */
int fb_flow_export_dev(fb_ctx* ctx, fb_flow_rec* d_out, uint64_t cap, uint64_t* d_n,
                       void* stream);
/* get_sessions (src/capture.rs:1578-1612): the flows that pass `filter` (fb_filter) evaluated at
 * query time, as the reference does per SessionInfo: LOCAL_ONLY keeps is_local_session! (is_lan_ip
 * of both key addresses under the context's CURRENT LAN configuration, src/sessions.rs:660-672),
 * GLOBAL_ONLY keeps is_global_session!, ALL keeps everything (= fb_flow_export).  Slot order.
 * Host variant synchronous; the _dev variant asynchronous, *d_n (device u64) = flows written. */
int fb_flow_export_sessions(fb_ctx* ctx, uint32_t filter, fb_flow_rec* out, uint64_t cap, uint64_t* n,
                            void* stream);
int fb_flow_export_sessions_dev(fb_ctx* ctx, uint32_t filter, fb_flow_rec* d_out, uint64_t cap, uint64_t* d_n,
                                void* stream);
int fb_flow_clear(fb_ctx* ctx, void* stream); /* clear_all_sessions, src/capture.rs:396 */
/* Flow-table geometry and growth.  `generation` counts the slot moves since fb_create -- growths and
 * purges (fb_flow_age) --: each moves flows to new slots (fb_flow_rec.slot, the history's flow ids),
 * and fb_flow_slot_remap gives the last move's old -> new slot map (old capacity entries, 0xFFFFFFFF =
 * empty, or removed by a purge) so a host that keys per-flow state by slot can follow.  flows /
 * max_partition are those the last completed update (or purge) reported (no device wait).  Synchronous. */
typedef struct fb_flow_table_info {
    uint64_t capacity;      /* slots */
    uint64_t partitions;    /* of 512 slots */
    uint64_t generation;    /* slot moves: growths and purges */
    uint64_t flows;         /* occupied slots after the last completed update */
    uint64_t max_partition; /* fullest partition then */
    uint64_t reserved[3];
} fb_flow_table_info;
int fb_flow_table_info_get(fb_ctx* ctx, fb_flow_table_info* info);
int fb_flow_slot_remap(fb_ctx* ctx, uint32_t* old_to_new, uint64_t cap, uint64_t* n);
/* The table's deterministic 64-bit key hash (the reference's DashMap uses SipHash with a random
 * per-process key, src/sessions.rs:23 + dashmap RandomState, so it has no reproducible hash). */
uint64_t fb_flow_hash(const fb_session_key* key);

/* Every flow's fb_flow_time (timed contexts), with its table slot (join with fb_flow_rec.slot of an
 * export: the orders differ).  Device form: asynchronous, *d_n = records; host form: synchronous. */
int fb_flow_export_times_dev(fb_ctx* ctx, fb_flow_time* d_out, uint64_t cap, uint64_t* d_n, void* stream);
int fb_flow_export_times(fb_ctx* ctx, fb_flow_time* out, uint64_t cap, uint64_t* n, void* stream);

/* ---- session aging (update_sessions_status, src/capture.rs:1497-1551; timed contexts) -----------
 * The reference ages its session map on every get_sessions / get_current_sessions: it recomputes each
 * session's SessionStatus {active, added, activated, deactivated} against the wall clock, rebuilds
 * current_sessions (activity within CONNECTION_CURRENT_TIMEOUT) and removes the sessions whose last
 * activity is older than CONNECTION_RETENTION_TIMEOUT (src/sessions.rs:10-15: 60 s / 180 s / 86400 s).
 * fb_flow_age does that over the whole table for a caller-supplied `now_ns` (the clock of the capture
 * timestamps), with the reference's comparisons (capture.rs:1514-1536) done without wrap-around:
 *   active  = last_activity + activity_ns >= now      added   = start_time + activity_ns >= now
 *   current = now < last_activity + current_ns        expired = now > last_activity + retention_ns
 *   activated = !previous.active && active            deactivated = previous.active && !active
 * The result is one status byte per table slot (FB_STATUS_* bits; fb_flow_status_dev, joined on
 * fb_flow_rec.slot).  A zero byte is a flow no aging call has seen since its insert: it has the
 * reference's insert status (active, added, activated; src/packets.rs:497-502), which is also the
 * `previous` of its first aging, and is a member of current_sessions (src/packets.rs:532).
 * With FB_AGE_PURGE the expired flows are removed and the partitions that held them re-packed, which
 * moves flows to other slots: when stats.purged > 0 the generation (fb_flow_table_info) rises by one,
 * fb_flow_slot_remap gives this call's old -> new slot map (capacity entries; 0xFFFFFFFF = empty or
 * removed), the history of the last update is no longer available (fb_flow_history_dev), and the
 * occupancy fb_flow_table_info_get reports is the purged table's.  When nothing was removed neither the
 * generation nor the remap changes.  A removed flow that sends again is inserted afresh.
 * Synchronous: waits for the updates in flight, like a table growth.  FB_ERR_INVAL on a context
 * without a flow table or without FB_CFG_TIMED (no clock).  `params` NULL = the reference's spans;
 * `out` may be NULL. */
typedef struct fb_age_params {
    uint64_t activity_ns;  /* CONNECTION_ACTIVITY_TIMEOUT  (60 s)    */
    uint64_t current_ns;   /* CONNECTION_CURRENT_TIMEOUT   (180 s)   */
    uint64_t retention_ns; /* CONNECTION_RETENTION_TIMEOUT (86400 s) */
    uint64_t reserved;     /* 0 */
} fb_age_params;
typedef struct fb_age_stats {
    uint64_t flows;         /* flows in the table when the call started                       */
    uint64_t active;        /* of those: status.active, ...                                   */
    uint64_t added;
    uint64_t activated;
    uint64_t deactivated;
    uint64_t current;       /* members of current_sessions                                    */
    uint64_t purged;        /* flows removed (0 without FB_AGE_PURGE)                         */
    uint64_t remaining;     /* flows - purged                                                 */
    uint64_t max_partition; /* fullest partition after the call (slots of 512)                */
    uint64_t reserved[7];
} fb_age_stats; /* 128 bytes */
#define FB_AGE_PURGE 1u
/* fb_flow_status_dev bytes */
#define FB_STATUS_ACTIVE 1u
#define FB_STATUS_ADDED 2u
#define FB_STATUS_ACTIVATED 4u
#define FB_STATUS_DEACTIVATED 8u
#define FB_STATUS_CURRENT 16u
#define FB_STATUS_AGED 128u
int fb_flow_age(fb_ctx* ctx, uint64_t now_ns, const fb_age_params* params, uint32_t flags, fb_age_stats* out,
                void* stream);
/* The status byte of every table slot (min(cap, capacity) bytes, slot order; all zero before the first
 * fb_flow_age) into DEVICE memory.  Asynchronous. */
int fb_flow_status_dev(fb_ctx* ctx, uint8_t* d_out, uint64_t cap, void* stream);

/* ---- whitelist conformance (recompute_whitelist_for_sessions, src/whitelists.rs:810-1023, over
 *      is_session_in_whitelist / endpoint_matches_with_reason, src/whitelists.rs:341-732) ----------
 * The reference checks every session against the flattened endpoint list of the active whitelist and
 * keeps SessionInfo.is_whitelisted, the whitelist_exceptions list and the whitelist_conformance flag.
 * fb_flow_whitelist does that check for every flow of the table in one pass, for a session whose
 * dst_domain and l7 are None (the device knows neither; the host expands the domains it has resolved
 * into address endpoints before fb_set_whitelist and resolves the flows marked FB_WL_HOST_CHECK):
 *   - protocol, port and process must match (src/whitelists.rs:465-491): an endpoint with a process
 *     never matches here -- unless it carries a process_match_id and a process-name table is installed
 *     (fb_set_l7_process_names) when the pass runs: then process_matches is "the flow's match id equals
 *     the endpoint's" (a flow without a process never matches), the rest of the endpoint is evaluated as the
 *     same endpoint without a process is, and its key is no host-check key on account of the process;
 *   - a domain endpoint does not match by domain; with `ip` specified, an address match returns true at
 *     once and a mismatch fails the endpoint, whatever its AS fields say (src/whitelists.rs:503-531);
 *   - with neither domain nor ip, every specified AS field must equal the session's dst_asn
 *     (src/whitelists.rs:534-595), which is Db::lookup of the destination unless it is a LAN address
 *     (src/packets.rs:468-485; LAN under the context's CURRENT configuration), None without ASN tables;
 *     an endpoint with nothing specified matches every session.
 * One compiled WhitelistEndpoint (src/whitelists.rs:24-34): */
#define FB_WL_NEVER 0xFFu /* family: an `ip` string that does not parse (ip_matches is false for it);
                             protocol: a string that is neither TCP nor UDP ignoring ASCII case */
#define FB_WL_HAS_PORT 1u
#define FB_WL_HAS_ASN 2u
#define FB_WL_HAS_OWNER 4u
#define FB_WL_HAS_COUNTRY 8u
#define FB_WL_HAS_DOMAIN 16u  /* `domain` is Some */
#define FB_WL_HAS_PROCESS 32u /* `process` is Some */
typedef struct fb_wl_endpoint {
    uint32_t addr[4];    /*  0: `ip`, session_key word order; the host bits of a net are ignored       */
    uint8_t family;      /* 16: 0 = no ip, 2, 10, FB_WL_NEVER                                          */
    uint8_t prefix;      /* 17: <= 32 / <= 128; a plain IP is a /32 or /128                            */
    uint8_t protocol;    /* 18: 0 = any, 6, 17, FB_WL_NEVER                                            */
    uint8_t flags;       /* 19: FB_WL_HAS_*                                                            */
    uint16_t port;       /* 20: with FB_WL_HAS_PORT                                                    */
    uint16_t reserved;   /* 22: 0                                                                      */
    uint32_t as_number;  /* 24: with FB_WL_HAS_ASN                                                     */
    uint32_t owner_id;   /* 28: with FB_WL_HAS_OWNER: the caller's id of the ASCII-lower-cased string  */
    uint32_t country_id; /* 32: with FB_WL_HAS_COUNTRY (ids < 0xFFFFFFFF)                               */
    union {              /* 36: one word under two names                                               */
        uint32_t reserved2;        /* its name before the device knew processes: 0                     */
        uint32_t process_match_id; /* with FB_WL_HAS_PROCESS: the caller's id (>= 1) of the ASCII-lower-cased
                                      process name, as fb_set_l7_process_names' match_id names it; 0: the
                                      device has no id for the name                                    */
    };
} fb_wl_endpoint;        /* 40 bytes */
#define FB_WL_MAX_EXACT (1u << 24) /* endpoints that match by one address (/32, /128), per call       */
#define FB_WL_MAX_OTHER (1u << 16) /* every other endpoint (nets, AS-only, domain-only, process); an
                                      exact-address endpoint with a process_match_id counts as exact  */
/* Install the flattened endpoint list of the active whitelist (copied and indexed before the call
 * returns).  rec_owner_id[r] / rec_country_id[r]: the caller's id of the lower-cased owner / country
 * string of fb_asn_range.record r (the reference compares them with eq_ignore_ascii_case); NULL with
 * n_records 0, and a record >= n_records has strings no endpoint equals.  n == 0 is an active whitelist
 * without endpoints: every session is NonConforming (src/whitelists.rs:413-421).  A list beyond
 * FB_WL_MAX_EXACT / FB_WL_MAX_OTHER, or an endpoint with a bad family / prefix / protocol, fails with
 * FB_ERR_INVAL and leaves the installed list as it was: nothing is ever truncated. */
int fb_set_whitelist(fb_ctx* ctx, const fb_wl_endpoint* eps, uint64_t n, const uint32_t* rec_owner_id,
                     const uint32_t* rec_country_id, uint32_t n_records);
/* reset_whitelist (src/capture.rs:131-149): no list is active and every flow's state is Unknown. */
int fb_clear_whitelist(fb_ctx* ctx);
/* The state byte of a table slot: 0 = Unknown (no pass has seen the flow since its insert), else
 * FB_WL_CONFORMING or FB_WL_NONCONFORMING; a NonConforming flow also has FB_WL_HOST_CHECK when some
 * endpoint with a domain or a process matches its protocol and port -- the necessary condition for such
 * an endpoint to match once the host knows the flow's domain or process: a superset of the flows the
 * host has to look at, never a verdict. */
#define FB_WL_CONFORMING 1u
#define FB_WL_NONCONFORMING 2u
#define FB_WL_HOST_CHECK 4u
#define FB_WL_MASK_UNKNOWN 128u /* fb_flow_export_whitelist_dev's state_mask: the flows with a zero byte */
typedef struct fb_wl_stats {
    uint64_t flows;         /* flows in the table                                                      */
    uint64_t conforming;
    uint64_t nonconforming;
    uint64_t host_check;    /* of the nonconforming: FB_WL_HOST_CHECK set                              */
    uint64_t changed;       /* flows whose state byte differs from before the call (the reference bumps
                               last_modified for those, src/whitelists.rs:975-982)                     */
    union {                 /* 40: three words, the first under two names                             */
        uint64_t reserved[3];
        uint64_t dom_overflow; /* of the host_check: marked because their name matched more patterns than
                                  FB_WL_NAME_MATCHES (fb_set_whitelist_dom); 0 for a list without patterns */
    };
} fb_wl_stats; /* 64 bytes */
/* Evaluate every flow against the installed list (the reference's incremental selection is an
 * optimisation of a pure function of the session, so a full pass gives the same states).  Synchronous:
 * waits for the updates in flight, like fb_flow_age; timed and untimed contexts.  `flags` must be 0;
 * `out` may be NULL.  FB_ERR_INVAL without a flow table or without an installed list. */
int fb_flow_whitelist(fb_ctx* ctx, uint32_t flags, fb_wl_stats* out, void* stream);
/* The state byte of every table slot (min(cap, capacity) bytes, slot order; zero before the first pass)
 * into DEVICE memory.  Asynchronous.  The bytes follow their flows through a growth and a purge
 * (fb_flow_slot_remap's map), and fb_flow_clear zeroes them. */
int fb_flow_whitelist_dev(fb_ctx* ctx, uint8_t* d_out, uint64_t cap, void* stream);
/* The fb_flow_rec of the flows whose state byte has a bit of `state_mask` (FB_WL_* bits;
 * FB_WL_MASK_UNKNOWN selects the zero bytes), slot order -- the whitelist exceptions are
 * FB_WL_NONCONFORMING; the caller sorts them by Session.  *d_n (device u64) = the matching flows (only
 * the first `cap` are written).  DEVICE pointers, asynchronous. */
int fb_flow_export_whitelist_dev(fb_ctx* ctx, uint32_t state_mask, fb_flow_rec* d_out, uint64_t cap, uint64_t* d_n,
                                 void* stream);

/* ---- domain endpoints on the device (domain_matches, src/whitelists.rs:602-679) ---------------------
 * fb_set_whitelist with the domain patterns of the list beside the endpoints: ep_pattern[i] is the 1-based
 * id of endpoint i's pattern (only with FB_WL_HAS_DOMAIN), 0 when the device has none -- that endpoint is what
 * it is under fb_set_whitelist: it never matches by domain and its key is a host-check key.  Pattern p is
 * pattern_bytes[pattern_off[p - 1], pattern_off[p]) (pattern_off[0] = 0), lower-cased by the caller; the call
 * classifies it (a name n of the DNS tracker, ASCII A-Z lower-cased, matches
 *   no '*': n == pattern;  "*.s": some n[i] == '.' with n[i + 1:] == s;  else "q.*": n == q or some n[i] == '.'
 *   with n[:i] == q;  else one '*', "a*b": n starts with a, ends with b and is longer than both;  else never).
 * An endpoint with a pattern id matches a flow whose protocol, port and process match (the process as under
 * fb_set_whitelist) and whose dst_name_id (the domain plane, as of the last fb_flow_domains) names a matching
 * name; then its `ip`, if any, decides as before.  FB_ERR_INVAL, the installed list untouched, for what
 * fb_set_whitelist refuses and for: an id above n_patterns, an id on an endpoint without FB_WL_HAS_DOMAIN, more
 * than FB_WL_MAX_GENERAL patterns of the a*b kind, pattern bytes of 2^32 and more, more than 2^24 - 1 patterns,
 * offsets that do not ascend from 0.  fb_set_whitelist is this call with no patterns.
 * Every name keeps the ids of the patterns it matches: FB_WL_NAME_MATCHES per name, ascending, zero-padded; a
 * name that matches more keeps the least and an overflow flag, and a NonConforming flow of such a name gets
 * FB_WL_HOST_CHECK when one of its four keys has a domain endpoint with an id (fb_wl_stats.dom_overflow counts
 * them).  Names are matched once, by the first fb_flow_whitelist / fb_wl_name_matches_dev after they appear;
 * fb_set_whitelist*, fb_clear_whitelist, fb_dns_track_clear and FB_DEBUG_WL_NAME_HASH_MASK start over. */
#define FB_WL_MAX_GENERAL 1024u
#define FB_WL_NAME_MATCHES 8u
int fb_set_whitelist_dom(fb_ctx* ctx, const fb_wl_endpoint* eps, uint64_t n, const uint32_t* ep_pattern,
                         const uint8_t* pattern_bytes, const uint64_t* pattern_off, uint64_t n_patterns,
                         const uint32_t* rec_owner_id, const uint32_t* rec_country_id, uint32_t n_records);
/* Brings the match state up to date, then d_rows[i * FB_WL_NAME_MATCHES ..] / d_flags[i] (bit 0: overflow) of
 * name id d_ids[i]; id 0, an id beyond the stored names, no installed patterns or no DNS tracking: zeros.
 * DEVICE pointers.  FB_ERR_INVAL without an installed list. */
int fb_wl_name_matches_dev(fb_ctx* ctx, const uint32_t* d_ids, uint64_t n, uint32_t* d_rows, uint8_t* d_flags,
                           void* stream);
typedef struct fb_wl_dom_info {
    uint64_t patterns[5];      /*  0: installed patterns per kind: exact, suffix, prefix, general, never       */
    uint64_t names_done;       /* 40: names whose row is up to date (ids 1 .. names_done)                      */
    uint64_t names_matched;    /* 48: of them with a non-empty row                                             */
    uint64_t names_overflowed; /* 56: of them with the overflow flag                                           */
} fb_wl_dom_info; /* 64 bytes */
int fb_wl_dom_info_get(fb_ctx* ctx, fb_wl_dom_info* out);

/* ---- blacklist pass over the session table (src/blacklists.rs:456-731, src/capture.rs:1850-1871) ----
 * recompute_blacklist_for_sessions gives every session the names of the lists one of whose ranges
 * contains its source or destination address -- an address whose is_local flag was set when the
 * session was inserted is left out (fb_flow_rec.session_flags, NOT the context's current LAN
 * configuration, unlike fb_flow_enrich_dev) -- as "blacklist:<name>" tags in `criticality`.  Here the
 * names are one 64-bit word per table slot, bit l = list l of fb_set_blacklists; zero = not blacklisted,
 * also the state of a flow no pass has seen (the reference's empty criticality at insert).  The words
 * follow their flows through a growth and a purge, and fb_flow_clear zeroes them. */
#define FB_BL_MARK_WHITELIST 1u /* the fallback of src/capture.rs:1858-1871: a blacklisted flow whose
                                   whitelist state byte is 0 (Unknown) gets FB_WL_NONCONFORMING |
                                   FB_WL_BLACKLISTED; no other byte of that plane is touched */
#define FB_WL_BLACKLISTED 8u    /* whitelist state byte: the reason is "Session is blacklisted" (the
                                   next fb_flow_whitelist replaces the byte, as the reference's pass
                                   replaces state and reason) */
typedef struct fb_bl_stats {
    uint64_t flows;             /* flows in the table                                                  */
    uint64_t blacklisted;       /* mask != 0 after the call                                            */
    uint64_t changed;           /* mask differs from before the call (the reference bumps last_modified
                                   for exactly these, src/blacklists.rs:655-689)                       */
    uint64_t newly_blacklisted; /* 0 before, != 0 after                                                */
    uint64_t cleared;           /* != 0 before, 0 after                                                */
    uint64_t wl_marked;         /* with FB_BL_MARK_WHITELIST: state bytes set by the fallback          */
    uint64_t reserved[2];
} fb_bl_stats; /* 64 bytes */
/* One pass over every flow against the lists installed by fb_set_blacklists (none installed, or n = 0:
 * valid, every mask becomes 0 -- the reference with an empty list set).  Synchronous: waits for the
 * updates in flight, like fb_flow_age / fb_flow_whitelist; timed and untimed contexts.  `flags`:
 * FB_BL_MARK_WHITELIST or 0 (without it the whitelist plane is neither read nor allocated); `out` may be
 * NULL.  FB_ERR_INVAL for other flag bits or without a flow table. */
int fb_flow_blacklist(fb_ctx* ctx, uint32_t flags, fb_bl_stats* out, void* stream);
/* The mask word of every table slot (min(cap, capacity) words, slot order; zeros before the first
 * pass) into DEVICE memory.  Asynchronous. */
int fb_flow_blacklist_dev(fb_ctx* ctx, uint64_t* d_out, uint64_t cap, void* stream);
/* The fb_flow_rec of the flows with a non-zero mask (get_blacklisted_sessions: the caller sorts them by
 * Session; slot order inside the 256 slots a workgroup compacts at a time, those runs in the order the
 * workgroups claimed their place), and beside each its mask in d_masks[cap] (may be NULL).  *d_n (device
 * u64) = the matching flows (only the first `cap` are written).  DEVICE pointers, asynchronous. */
int fb_flow_export_blacklisted_dev(fb_ctx* ctx, fb_flow_rec* d_out, uint64_t* d_masks, uint64_t cap, uint64_t* d_n,
                                   void* stream);

/* ---- anomaly pass over the session table (src/analyzer.rs) -------------------------------------------
 * The reference's SessionAnalyzer scores every session with an Extended Isolation Forest over a
 * 10-feature vector (compute_features, src/analyzer.rs:716-793) and writes "anomaly:<level>[/<diagnostic>]"
 * into `criticality` (analyze_session, 562-660).  The forest crate's generator and tree layout are not
 * part of the reference's sources, so the model is DEFINED here: the host trains and
 * installs a forest in the format below, the device computes the features of every flow from the table,
 * walks every tree in f64 and keeps, per table slot, the exact sum of the leaf values, the level and the
 * diagnostic codes.  Every operation is a separately rounded IEEE double operation (no fused
 * multiply-add), so a host restatement reproduces every bit.
 *
 * Features (index: value), one double[FB_AN_FEATURES] per flow:
 *   0 process: 0.0 (no L7 here)                      1 duration: timed contexts, (double)ms / 1000.0 with
 *   ms = (int64)(t - start_time_ns) / 1000000 (truncated toward zero; may be negative), t = end_time_ns
 *   when set, else last_activity_ns; untimed contexts 0.0 (no clock)
 *   2 (double)(inbound_bytes + outbound_bytes)       3 (double)(orig_pkts + resp_pkts)
 *   4 segment interarrival: timed, div ? ((double)total_segment_interarrival_ms / 1000.0) / (double)div
 *     : 0.0; untimed 0.0                             5 outbound ? (double)inbound / (double)outbound : 0.0
 *   6 packets ? (double)(in + out) / (double)(orig + resp) : 0.0
 *   7 (double)service_code[dst_port] when the stored FB_SESSION_DST_SERVICE flag is set, else 0.0
 *   8 1.0 when the stored FB_SESSION_SELF_DST flag is set, else 0.0         9 missed bytes: 0.0
 *   (src/packets.rs:364: always 0 on the capture path) */
#define FB_AN_FEATURES 10
#define FB_IF_MAX_TREES 64
#define FB_IF_MAX_TREE_NODES 255 /* sample_size <= 128 -> at most 255 nodes */
#define FB_IF_MAX_DEPTH 12       /* the reference's recursion cap, src/analyzer.rs:523 */
#define FB_IF_LEAF 0xFFFFFFFFu
#define FB_AN_MAX_SERVICE_CODE 1000000u /* service codes are below this */
typedef struct fb_if_node {        /* 96 bytes */
    double normal[FB_AN_FEATURES]; /*  0: internal node: split normal; leaf: zeros                       */
    double value;                  /* 80: internal: split offset b; leaf: depth + c(size), host-computed */
    uint32_t left, right;          /* 88, 92: indices RELATIVE to the tree's first node, both > this
                                      node's index; left == FB_IF_LEAF marks a leaf                       */
} fb_if_node;
/* Tree t is nodes [first[t], first[t + 1]), its root first; first[0] = 0, first[n_trees] = n_nodes.
 * The walk of one tree: from the root, at an internal node s = 0.0; for j = 0..9: s = s + x[j] *
 * normal[j] (each product and each sum rounded on its own); left iff s < value (a NaN goes right); at
 * the leaf its value is added to path_sum (0.0 at the start, trees in order). */
typedef struct fb_an_params {
    double mean[FB_AN_FEATURES];   /*   0: feature_stats, src/analyzer.rs:317-353                        */
    double std[FB_AN_FEATURES];    /*  80 */
    double suspicious_cut;         /* 160: level 2 iff path_sum <= suspicious_cut (and not level 3)      */
    double abnormal_cut;           /* 168: level 3 iff path_sum <= abnormal_cut; a cut is -log2(score
                                      threshold) * c(sample_size) * n_trees, i.e. score >= threshold
                                      (src/analyzer.rs:586-592) decided on the path sum                   */
    uint32_t has_stats;            /* 176: 0 / 1: the reference's counts > 1; 0: every diagnostic code 0 */
    uint32_t sample_size;          /* 180: the forest's sample size (kept for the host's score)          */
} fb_an_params;                    /* 184 bytes */
enum fb_an_level { FB_AN_UNSEEN = 0, FB_AN_NORMAL = 1, FB_AN_SUSPICIOUS = 2, FB_AN_ABNORMAL = 3 };
/* Diagnostic codes (src/analyzer.rs:356-487), two bits per feature i in fb_an_rec.diag (bits 2i, 2i + 1),
 * only for a suspicious or abnormal flow: the reference's FEATURE_DEFS call indices 0, 6 and 8
 * categorical (its table names index 6 DestService and index 7 AvgPacketSize although the vector holds
 * them the other way round; kept).  Categorical: FB_AN_DIAG_DEVIATES iff std <= 1e-6 && |x - mean| >
 * 1e-6.  Numeric: std > 1e-6: z = (x - mean) / std, HIGH iff z >= 2.5, LOW iff z <= -2.5; else
 * DEVIATES iff |x - mean| > 1e-6. */
enum fb_an_diag { FB_AN_DIAG_NONE = 0, FB_AN_DIAG_HIGH = 1, FB_AN_DIAG_LOW = 2, FB_AN_DIAG_DEVIATES = 3 };
typedef struct fb_an_rec {
    double path_sum;     /*  0: sum of the leaf values over the trees                                    */
    uint32_t diag;       /*  8: fb_an_diag codes                                                         */
    uint8_t level;       /* 12: fb_an_level; 0 with the other fields 0: no pass has seen the flow        */
    uint8_t reserved[3]; /* 13 */
} fb_an_rec;             /* 16 bytes */
typedef struct fb_an_stats {
    uint64_t flows;           /* flows in the table                                                      */
    uint64_t normal;          /* level after the call                                                    */
    uint64_t suspicious;
    uint64_t abnormal;
    uint64_t changed;         /* the record differs from before the call                                 */
    uint64_t newly_anomalous; /* level < 2 before, >= 2 after                                            */
    uint64_t cleared;         /* level >= 2 before, < 2 after                                            */
    uint64_t reserved;
} fb_an_stats; /* 64 bytes */
/* FB_OK iff the forest is one fb_set_anomaly_model installs: 1 <= n_trees <= FB_IF_MAX_TREES, first[]
 * as above with 1 <= nodes per tree <= FB_IF_MAX_TREE_NODES, every child index above its parent's and
 * inside the tree, every leaf at most FB_IF_MAX_DEPTH below the root, every value and normal finite.
 * These rules bound the device's walk.  Host only: needs no device. */
int fb_if_validate(const fb_if_node* nodes, uint64_t n_nodes, const uint32_t* first, uint32_t n_trees);
/* The service codes alone (HOST pointer, copied): uint32[65536] indexed by port, each <
 * FB_AN_MAX_SERVICE_CODE; NULL = zeros, the state of a new context.  They are what feature 7 reads, in
 * fb_flow_features_dev too, so training data can be exported before there is a model. */
int fb_set_service_codes(fb_ctx* ctx, const uint32_t* service_code);
/* Install the model (HOST pointers, copied): the forest, its parameters and the service codes (as
 * fb_set_service_codes; NULL = zeros).  FB_ERR_INVAL -- and the installed model and codes stay as they
 * were -- for a forest fb_if_validate rejects, a non-finite mean / std, a NaN cut, has_stats > 1 or a
 * service code out of range.  The plane keeps its records. */
int fb_set_anomaly_model(fb_ctx* ctx, const fb_if_node* nodes, uint64_t n_nodes, const uint32_t* first,
                         uint32_t n_trees, const fb_an_params* params, const uint32_t* service_code);
/* No model installed (the service codes stay); every record back to zero (as fb_clear_whitelist does
 * with its states). */
int fb_clear_anomaly_model(fb_ctx* ctx);
/* One pass over every flow with the installed model.  Synchronous: waits for the updates in flight, like
 * fb_flow_blacklist; timed and untimed contexts.  `flags` must be 0; `out` may be NULL.  FB_ERR_INVAL
 * without a flow table or without a model. */
int fb_flow_anomaly(fb_ctx* ctx, uint32_t flags, fb_an_stats* out, void* stream);
/* The record of every table slot (min(cap, capacity) records, slot order; zeros before the first pass)
 * into DEVICE memory.  Asynchronous.  Records follow their flows through a growth and a purge, and
 * fb_flow_clear zeroes them. */
int fb_flow_anomaly_dev(fb_ctx* ctx, fb_an_rec* d_out, uint64_t cap, void* stream);
/* The fb_flow_rec of the flows whose level is >= min_level (1..3), and beside each its record in
 * d_recs[cap] (may be NULL); order as fb_flow_export_blacklisted_dev.  *d_n (device u64) = the matching
 * flows (only the first `cap` are written).  DEVICE pointers, asynchronous. */
int fb_flow_export_anomalous_dev(fb_ctx* ctx, uint32_t min_level, fb_flow_rec* d_out, fb_an_rec* d_recs,
                                 uint64_t cap, uint64_t* d_n, void* stream);
/* Every flow's feature vector (the training data): d_feat[cap][FB_AN_FEATURES] and beside each its table
 * slot in d_slot[cap]; *d_n = the flows.  Needs no model (feature 7 reads the installed service codes).
 * DEVICE pointers, asynchronous. */
int fb_flow_features_dev(fb_ctx* ctx, double* d_feat, uint32_t* d_slot, uint64_t cap, uint64_t* d_n,
                         void* stream);
/* The walk over n caller-supplied vectors d_feat[n][FB_AN_FEATURES] -> d_path_sum[n], with the installed
 * forest and the pass's own device function.  FB_ERR_INVAL without a model.  DEVICE pointers,
 * asynchronous. */
int fb_if_score_dev(fb_ctx* ctx, const double* d_feat, uint64_t n, double* d_path_sum, void* stream);

/* ---- incremental queries: last_modified and the view export (src/capture.rs:411-426, 1578-1760) -------
 * The reference's getters take an `incremental` flag and then return only the sessions whose
 * last_modified is newer than the getter's last full fetch.  It sets last_modified = now at a packet
 * (src/packets.rs:342, 524), at a blacklist change (src/blacklists.rs:655-689, src/capture.rs:1867-1868)
 * and at a whitelist change (src/whitelists.rs:975-982), and when the analyzer re-tags a session
 * (src/analyzer.rs:655-676); the status update leaves it alone (src/capture.rs:1497-1551).
 * Here a flow's last_modified is max(last_activity_ns, stamp): the packet part is the time plane's
 * last_activity_ns (timed contexts; nothing is stored on the packet path), the stamp is one uint64 per
 * table slot that the passes write -- the pass time of fb_set_pass_time, on the clock of the frame
 * times -- into exactly the flows they changed:
 *   fb_flow_blacklist  the flows counted as `changed`, and those FB_BL_MARK_WHITELIST marks (`wl_marked`);
 *   fb_flow_whitelist  the flows counted as `changed`;
 *   fb_flow_anomaly    the flows whose level or diagnostic codes differ from before the call (a new
 *                      path_sum alone does not show in the criticality string and does not stamp);
 *   fb_flow_domains    the flows counted as `changed` (src/capture.rs:1397-1399);
 *   fb_flow_age        never.
 * A zero stamp: no pass has modified the flow.  The stamps follow their flows through a growth and a
 * purge (a purged flow that returns starts at 0), and fb_flow_clear zeroes them.
 *
 * fb_set_pass_time: the stamp later passes write.  0 -- the state of a new context -- means "do not
 * stamp": no stamp plane is allocated and every pass runs the code it ran before there were stamps. */
int fb_set_pass_time(fb_ctx* ctx, uint64_t now_ns);
/* The raw stamp of every table slot (min(cap, capacity) words, slot order; zeros while no stamped pass
 * has run) into DEVICE memory.  Asynchronous. */
int fb_flow_modified_dev(fb_ctx* ctx, uint64_t* d_out, uint64_t cap, void* stream);

/* One record per selected flow: everything the separate exports and per-slot planes hold about it,
 * joined on the device.  A plane no pass has made yet contributes zeros; on an untimed context `time`
 * is zero except its slot. */
typedef struct fb_flow_view {
    fb_flow_rec rec;           /*   0: as fb_flow_export_sessions writes it                              */
    fb_flow_time time;         /* 136: as fb_flow_export_times writes it (slot set)                      */
    uint64_t last_modified_ns; /* 200: max(time.last_activity_ns, stamp_ns); untimed: stamp_ns           */
    uint64_t stamp_ns;         /* 208: the stamp plane's element (fb_flow_modified_dev)                  */
    uint64_t bl_mask;          /* 216: fb_flow_blacklist_dev's word                                      */
    fb_an_rec an;              /* 224: fb_flow_anomaly_dev's record                                      */
    uint8_t status;            /* 240: fb_flow_status_dev's byte                                         */
    uint8_t wl_state;          /* 241: fb_flow_whitelist_dev's byte                                      */
    uint8_t reserved[14];      /* 242: zeros                                                             */
} fb_flow_view;                /* 256 bytes; an output array starts at a 16-byte boundary                */
enum fb_view_set {
    FB_VIEW_ALL = 0,           /* every flow                                                             */
    FB_VIEW_CURRENT = 1,       /* status byte 0, or FB_STATUS_CURRENT set (get_current_sessions)         */
    FB_VIEW_BLACKLISTED = 2,   /* mask != 0                                                              */
    FB_VIEW_WL_EXCEPTIONS = 3, /* FB_WL_NONCONFORMING set                                                */
    FB_VIEW_ANOMALOUS = 4      /* level >= FB_AN_SUSPICIOUS                                              */
};
#define FB_VIEW_MODIFIED_SINCE 1u /* fb_view_query.flags: and last_modified_ns > since_ns (strict, as the
                                     reference skips last_modified <= last_fetch_ts)                     */
typedef struct fb_view_query {
    uint64_t since_ns; /*  0: read with FB_VIEW_MODIFIED_SINCE                                           */
    uint32_t set;      /*  8: fb_view_set; a set whose plane no pass has made selects nothing -- except
                              FB_VIEW_CURRENT, which then selects every flow (a zero byte is current)    */
    uint32_t filter;   /* 12: fb_filter, evaluated now against the current LAN configuration, as
                              fb_flow_export_sessions does                                               */
    uint32_t flags;    /* 16: FB_VIEW_MODIFIED_SINCE or 0                                                */
    uint32_t reserved; /* 20: 0                                                                          */
} fb_view_query;       /* 24 bytes */
/* The fb_flow_view of the flows the query selects; order as fb_flow_export_blacklisted_dev.  *d_n (device
 * u64) = the matching flows (only the first `cap` are written; cap may be 0).  One sweep: per slot the
 * predicate reads the table line, 8 B of the time record, the stamp and one plane element; the selected
 * records of a step are staged in LDS and written out by the whole workgroup in 16-B columns.  DEVICE
 * pointers (d_out 16-B aligned), asynchronous; the host variant is synchronous, *n = records written.
 * FB_ERR_INVAL for an unknown set, filter or flag bit, a non-zero `reserved`, FB_VIEW_MODIFIED_SINCE on a
 * context without FB_CFG_TIMED (no packet clock), or a context without a flow table. */
int fb_flow_export_view_dev(fb_ctx* ctx, const fb_view_query* query, fb_flow_view* d_out, uint64_t cap, uint64_t* d_n,
                            void* stream);
int fb_flow_export_view(fb_ctx* ctx, const fb_view_query* query, fb_flow_view* out, uint64_t cap, uint64_t* n,
                        void* stream);

/* ---- whitelist learning (Whitelists::new_from_sessions, src/whitelists.rs:103-177) ----
 * The distinct endpoints of the flows a query selects.  An endpoint is the fingerprint (dst_ip, family,
 * dst_port, protocol, dst_name_id): dst_name_id is the domain plane's id of the flow (fb_flow_domains),
 * 0 -- the reference's None -- before any domain pass and without DNS tracking.  Each endpoint carries a
 * representative session, the least of its flows under Session's derived Ord (inside a group: source
 * address, then source port), so it depends neither on the table's layout nor on a race.  While a
 * process-name table is installed (fb_set_l7_process_names) the fingerprint has a sixth member, the flow's
 * verbatim process name id (proc_name_id, 0: no process). */
typedef struct fb_learned_endpoint {
    uint32_t dst_ip[4];     /*  0: session_key word order                                                */
    uint32_t rep_src_ip[4]; /* 16: the representative session's source                                   */
    uint16_t dst_port;      /* 32 */
    uint16_t rep_src_port;  /* 34 */
    uint8_t protocol;       /* 36: 6 / 17                                                                */
    uint8_t family;         /* 37: 2 / 10                                                                */
    uint16_t reserved;      /* 38: 0                                                                     */
    uint32_t dst_name_id;   /* 40: the domain plane's id, 0 = no domain                                  */
    uint32_t rep_slot;      /* 44: the representative's table slot                                       */
    uint32_t sessions;      /* 48: selected flows with this fingerprint                                  */
    union {                 /* 52: three words under two sets of names                                   */
        uint32_t reserved2[3];        /* their name before the device knew processes: 0                  */
        struct {
            uint32_t proc_name_id;    /* the flow's verbatim process name id (fb_set_l7_process_names), 0 =
                                         no process; written only while a name table is installed (else 0) */
            uint32_t reserved3[2];    /* 0                                                               */
        };
    };
} fb_learned_endpoint;      /* 64 bytes; an output array starts at a 16-byte boundary                    */
typedef struct fb_learn_stats {
    uint64_t flows;     /*  0: flows in the table                                                        */
    uint64_t selected;  /*  8: of them selected by the query                                             */
    uint64_t endpoints; /* 16: distinct fingerprints among the selected (= *d_n)                         */
    uint64_t written;   /* 24: records written: min(endpoints, cap)                                      */
    uint64_t rounds;    /* 32: insert rounds the index took                                              */
    uint64_t reserved[3];
} fb_learn_stats; /* 64 bytes */
/* One record per distinct endpoint of the flows `query` selects (read exactly as fb_flow_export_view_dev
 * reads it, same FB_ERR_INVAL cases), in ascending rep_slot order; *d_n (device u64) = the distinct
 * endpoints, only the first `cap` are written (cap may be 0).  Two calls on an unchanged table write
 * identical bytes.  Reads the table and the planes only.  d_out, d_n: DEVICE pointers (d_out 16-B aligned);
 * out: HOST, may be NULL.  Synchronous (the insert rounds read a counter between launches), after the
 * updates in flight.  FB_ERR_INTERNAL if the index insert did not converge within its round bound. */
int fb_flow_learn_endpoints_dev(fb_ctx* ctx, const fb_view_query* query, fb_learned_endpoint* d_out, uint64_t cap,
                                uint64_t* d_n, fb_learn_stats* out, void* stream);

/* ---- Zeek conn.log export (format_sessions_zeek, src/sessions.rs:694-774) ----------
 * One text line per fb_flow_view record, formatted on the device: 21 tab-separated fields and '\n'
 *   ts uid id.orig_h id.orig_p id.resp_h id.resp_p proto service duration orig_bytes resp_bytes conn_state
 *   local_orig local_resp missed_bytes history orig_pkts orig_ip_bytes resp_pkts resp_ip_bytes tunnel_parents
 * (the header line is the caller's).  ts = time.start_time_ns as secs[.micros], trailing zeros dropped;
 * duration = (end_time_ns - start_time_ns) truncated to microseconds as [-]secs.6 digits, "-" without an
 * end; both in integer arithmetic, equal to the reference's f64 text for 2^14 <= secs < 2^33 and
 * |micros| < 2^52 (records outside are counted in ts_inexact).  Addresses as Rust's Display prints them;
 * uid = the 128 bits {fb_flow_hash(key), mix(hash ^ start_time_ns)} as a version-4 UUID (the reference
 * draws a random one, src/packets.rs:350); service, local_orig, local_resp, tunnel_parents "-",
 * missed_bytes 0, as the reference leaves them.
 * FB_ZEEK_FIXED_MAX: the longest line without its history -- ts 18 (11 + '.' + 6), uid 36, two addresses
 * of 39, two ports of 5, proto 3, four "-", duration 18 ('-' + 10 + '.' + 6: |end - start| < 2^63 ns),
 * six counters of 20, conn_state 3, missed_bytes 1, 20 tabs, '\n'. */
#define FB_ZEEK_FIXED_MAX 312u
/* The kernel's shape, for the tests that sit on its thresholds: records per workgroup step, the bytes of
 * a step the write-out stages in LDS (a larger step is stored directly), and the history length from
 * which the wave copies a history together. */
#define FB_ZEEK_STEP 256u
#define FB_ZEEK_STAGE_BYTES 40000u
#define FB_ZEEK_COOP_HIST 64u
typedef struct fb_zeek_stats {
    uint64_t lines;          /*  0: records given (n)                                                    */
    uint64_t bytes;          /*  8: bytes all n lines need                                               */
    uint64_t lines_written;  /* 16: leading lines that fit text_cap entirely                             */
    uint64_t ts_inexact;     /* 24: records outside the exact ts / duration range (above)                */
    uint64_t hist_mismatch;  /* 32: records whose rec.hist_len != the blob's length                      */
    uint64_t reserved[3];
} fb_zeek_stats;             /* 64 bytes */
/* The lines of d_views[0 .. n) -- what fb_flow_export_view_dev wrote; the table is not touched -- into
 * d_text: line i is d_text[d_line_off[i] .. d_line_off[i + 1]), input order.  The history characters are
 * an input: d_hist[d_hist_off[slot] .. d_hist_off[slot + 1]) for rec.slot (d_hist_off has n_slots + 1
 * entries, non-decreasing, inside d_hist).  d_hist NULL: every history field is empty and hist_mismatch
 * stays 0.  With a blob its length decides what is written; a record whose hist_len disagrees, or whose
 * slot is >= n_slots (empty history), is counted in hist_mismatch.  Lines that do not fit text_cap
 * entirely are not written and nothing at or past d_text + text_cap is stored; d_line_off (n + 1 entries)
 * and d_stats are complete either way, so a caller can size a retry.  n == 0 writes d_line_off[0] = 0 and
 * zero stats.  DEVICE pointers, asynchronous, no host round trip.  FB_ERR_INVAL for a NULL ctx, d_views,
 * d_line_off or d_stats, a blob without offsets, d_text NULL with text_cap != 0, d_views not
 * 16-byte aligned, or a context without FB_CFG_TIMED (no clock to print). */
int fb_format_zeek_dev(fb_ctx* ctx, const fb_flow_view* d_views, uint64_t n, const uint8_t* d_hist,
                       const uint64_t* d_hist_off, uint64_t n_slots, uint8_t* d_text, uint64_t text_cap,
                       uint64_t* d_line_off, fb_zeek_stats* d_stats, void* stream);
/* The same lines from history indexed by RECORD: d_hist_off has n + 1 entries and record i's characters are
 * d_hist[d_hist_off[i] .. d_hist_off[i + 1]) -- what fb_hist_store_lengths_dev / fb_hist_store_gather_dev
 * write for the view records' slots.  Everything else (both write paths, hist_mismatch = stored length !=
 * rec.hist_len, the text_cap rule, the errors) is fb_format_zeek_dev's. */
int fb_format_zeek_hist_dev(fb_ctx* ctx, const fb_flow_view* d_views, uint64_t n, const uint8_t* d_hist,
                            const uint64_t* d_hist_off, uint8_t* d_text, uint64_t text_cap, uint64_t* d_line_off,
                            fb_zeek_stats* d_stats, void* stream);

/* ---- device-resident session history (fb_histstore.hip) -------------------------------
 * SessionStats.history (src/packets.rs:187-198, 410-426) kept on the device, opt-in: after
 * fb_hist_store_enable, fb_hist_store_append_dev after every update appends that update's characters
 * (fb_flow_history_dev's runs) to per-flow chains of 64-byte blocks -- a u32 link and 60 bytes of 4-bit
 * codes (1 + the FB_HIST_CHARS index, low nibble first): FB_HIST_BLOCK_CHARS characters a block.  A flow's
 * chain follows it through table growths and purges (a purge returns the removed flows' blocks to the
 * store's free stack; fb_flow_clear empties the store).  A context that never enables the store behaves
 * exactly as before, and so does every other entry point with a store.
 * Memory: 16 B per table slot, 64 B per started block (a flow of L characters holds ceil(L / 120)); the pool
 * starts at block_capacity blocks and doubles (one allocation, one device-to-device copy, ids unchanged) when
 * the blocks in use plus the record slots of the appends in flight could pass it.  With FB_CFG_FIXED_TABLE
 * the store never allocates or frees device memory after fb_hist_store_enable (the rule a live resident
 * queue needs): an append the pool cannot be shown to hold fails with FB_ERR_TABLE_FULL instead, before any
 * of its kernels has run, and the update scratch it sizes its run scratch by must not grow either (enable
 * after the largest batch's scratch exists, or keep batches within it).
 * FB_HIST_COOP_RUN: the run length (characters one flow gained in one update) from which a wavefront
 * appends the run together instead of one lane; FB_HIST_COOP_GATHER: the stored length from which a
 * wavefront decodes a chain together in fb_hist_store_gather_dev. */
#define FB_HIST_BLOCK_CHARS 120u
#ifndef FB_HIST_COOP_RUN /* (a build may override it to measure another value; 2 .. FB_HIST_BLOCK_CHARS) */
#define FB_HIST_COOP_RUN 32u
#endif
#define FB_HIST_COOP_GATHER 64u
typedef struct fb_hist_store_config {
    uint64_t block_capacity; /*  0: blocks of the first pool (0 = 2^20)                                   */
    uint64_t max_blocks;     /*  8: the pool never grows past this (0 = 2^32 - 2)                         */
    uint32_t flags;          /* 16: must be 0                                                             */
    uint32_t reserved[3];    /* 20: must be 0                                                             */
} fb_hist_store_config;      /* 32 bytes */
typedef struct fb_hist_store_info {
    uint64_t blocks_capacity;   /*  0: blocks the pool holds                                              */
    uint64_t blocks_high_water; /*  8: ids ever taken from the bump cursor                                */
    uint64_t blocks_free;       /* 16: ids on the free stack                                              */
    uint64_t blocks_in_use;     /* 24: high water - free = the sum of ceil(len / 120) over the flows      */
    uint64_t chars;             /* 32: characters stored                                                  */
    uint64_t flows;             /* 40: slots with a non-empty history                                     */
    uint64_t appends;           /* 48: appends that ran since enable                                      */
    uint64_t missed_updates;    /* 56: update calls since enable that no append followed                  */
} fb_hist_store_info;           /* 64 bytes */
/* Enables the store (cfg NULL = defaults).  FB_ERR_INVAL without a flow table, for non-zero flags /
 * reserved, when the store is already enabled, or when the table has taken an update since create /
 * fb_flow_clear (the store cannot know the earlier characters). */
int fb_hist_store_enable(fb_ctx* ctx, const fb_hist_store_config* cfg);
/* Appends the LAST update's history characters.  Same preconditions as fb_flow_history_dev (the update's
 * d_recs, d_seg and d_stats still valid; joins the update stream); asynchronous on `stream` with no device
 * wait unless the pool may be too small (above).  A second append for the same update, or an append after an
 * empty update, appends nothing and returns FB_OK; so does one whose update's slots have since moved (a
 * purge), which stays counted in missed_updates.  FB_ERR_INVAL without a store. */
int fb_hist_store_append_dev(fb_ctx* ctx, void* stream);
/* d_off[0 .. n]: the exclusive scan of the stored lengths of n slots, d_off[n] the total.  d_slots NULL:
 * slots 0 .. n - 1; else slot i is the u32 at (const char*)d_slots + i * stride_bytes (4 for a packed
 * array; sizeof(fb_flow_view) with d_slots = &d_views[0].rec.slot for view records).  A slot at or past the
 * table's capacity has length 0.  DEVICE pointers, asynchronous. */
int fb_hist_store_lengths_dev(fb_ctx* ctx, const void* d_slots, uint64_t stride_bytes, uint64_t n, uint64_t* d_off,
                              void* stream);
/* The characters of the same slots, decoded to FB_HIST_CHARS letters: slot i's at d_chars[d_off[i] ..
 * d_off[i + 1]).  A range that ends past `cap` is not written at all and nothing at or past d_chars + cap
 * is stored.  With d_slots NULL and n = the table's capacity the pair (d_chars, d_off) is what
 * fb_format_zeek_dev takes.  DEVICE pointers, asynchronous. */
int fb_hist_store_gather_dev(fb_ctx* ctx, const void* d_slots, uint64_t stride_bytes, uint64_t n, const uint64_t* d_off,
                             uint8_t* d_chars, uint64_t cap, void* stream);
/* The store's counters.  Synchronous (waits for the updates and appends in flight). */
int fb_hist_store_info_get(fb_ctx* ctx, fb_hist_store_info* info);

/* ---- multi-GPU session table (BASELINE configs[4]) ------------------------------
 * The reference runs one capture task per interface into ONE shared DashMap (src/capture.rs:946-1016,
 * src/packets.rs:329-535); W ranks that each parse a contiguous packet-index shard into their own
 * table merge them into that one table:
 *   1. every rank exports its table with fb_flow_export_merge_dev: records grouped by owner rank
 *      (the key's fb_flow_hash high word scaled to [0, world)), d_counts[world] = group sizes;
 *   2. all-to-all of the groups (RCCL), each owner receiving every rank's group in rank order;
 *   3. the owner merges them with fb_flow_merge_dev: one fb_flow_rec per key;
 *   4. all-gather of the owners' merged records.
 * The result equals the table ONE context builds from the same packets in global order (call k of
 * every rank = its shard of global batch k; global batch k is the ranks' shards in rank order) --
 * integer sums (segment_count too), MIN first_seen / end_seen, MAX last_seen, hist_len SUM,
 * hist_mask OR, in_segment and session flags from the records holding the key's latest / earliest
 * packet -- and conn_state / end_mask re-decided at the global first FIN/RST: the ending rank's
 * end_mask OR the S s H h of the other ranks that precede it (their first occurrence in an earlier
 * call, or in the same call on a lower rank).  Exact for any number of update calls per rank.  The
 * shard layout: global batch k is split into contiguous packet-index ranges, rank r's before rank
 * r+1's.  fb_flow_export_merge_dev takes the layout of equal shards of equal-size batches -- call k
 * of every rank is its shard of global batch k, starting at the same index `shard_first` in each --
 * and makes positions (k << 32) | (shard_first + pkt_index).  fb_flow_export_merge_map_dev takes
 * any layout -- unequal per-call batches, a short tail batch, a rank that makes no call for a batch
 * whose shard is empty -- as a call map: call_map[k] = (global batch of this rank's update call k)
 * << 32 | (global index of that shard's first packet), global batches increasing with k; positions
 * become (call_map[k] >> 32) << 32 | ((call_map[k] & 0xFFFFFFFF) + pkt_index) and char_call the
 * global batch numbers. */
typedef struct fb_flow_mrec {
    fb_flow_rec rec;        /* positions global; rec.slot = the exporting rank                    */
    uint32_t char_call[4];  /* update call of the flow's first S, s, H, h (FB_CALL_NONE: none)     */
} fb_flow_mrec;             /* 152 bytes */
/* Every flow of the table, grouped by owner rank (slot order inside a group), into d_out (room for
 * cap records); d_counts: `world` device u64 group sizes.  1 <= world <= 64, rank < world.
 * DEVICE pointers, asynchronous. */
int fb_flow_export_merge_dev(fb_ctx* ctx, uint32_t world, uint32_t rank, uint64_t shard_first, fb_flow_mrec* d_out,
                             uint64_t cap, uint64_t* d_counts, void* stream);
/* The same with a host call map (n_calls >= the context's update calls since create / clear; the
 * map is copied before the call returns). */
int fb_flow_export_merge_map_dev(fb_ctx* ctx, uint32_t world, uint32_t rank, const uint64_t* call_map, uint32_t n_calls,
                                 fb_flow_mrec* d_out, uint64_t cap, uint64_t* d_counts, void* stream);
/* Merge n records received by one owner (each rank's group, in rank order; a key at most once per
 * rank) into one fb_flow_rec per key (slot 0), in the order of each key's first record; *d_n
 * (device u64) = keys.  d_out: room for n records.  DEVICE pointers, asynchronous. */
int fb_flow_merge_dev(fb_ctx* ctx, const fb_flow_mrec* d_in, uint64_t n, fb_flow_rec* d_out, uint64_t* d_n,
                      void* stream);
/* Routed global table (every kind of session state exact, the capture-time state of timed contexts
 * included): instead of merging per-rank tables, each rank parses its shard (fb_parse_classify_dev,
 * no update) and routes every SESSION record to the owner of its key BEFORE the update; the owner
 * then runs ONE update call per global batch over what it received -- every rank's group in rank
 * order, i.e. the flow's packets in global order -- so its table is exactly the single-table state of
 * its flows (history, conn_state, timeouts).  This groups a rank's n_session (*d_stats, at most max_n)
 * dense records by owner (stable), makes pkt_index global (+ shard_first: the index of the shard's
 * first frame in the global batch), and with d_ts (the shard's frame times) writes each record's
 * capture time to d_ts_out beside it; d_counts[world] = group sizes.  The host moves the groups
 * (all-to-all), scatters the received times into a global-batch-sized array by pkt_index for
 * fb_set_frame_times, and calls fb_flow_update_records_dev on the received records (with a stats
 * struct whose n_session is their count; an owner that received none still makes the call, so update
 * calls stay global batches).  DEVICE pointers, asynchronous. */
int fb_route_records_dev(fb_ctx* ctx, const fb_pkt_out* d_recs, const fb_batch_stats* d_stats, uint32_t max_n,
                         uint32_t world, uint64_t shard_first, const uint64_t* d_ts, fb_pkt_out* d_out,
                         uint64_t* d_ts_out, uint64_t* d_counts, void* stream);
/* The owner rank fb_flow_export_merge_dev assigns a key to. */
uint32_t fb_flow_owner(const fb_session_key* key, uint32_t world);

/* ---- host ingest ring (replaces the reader thread -> Vec<u8> -> mpsc(1000) -> processor path,
 *      src/capture.rs:1016, 1082-1142, 1183-1249) ---------------------------------------------
 * The producer (capture callback) appends frames to the current batch of a ring of pinned host
 * batches; a full batch is submitted as H2D (copy stream) -> fb_process_dev (parse + classify +
 * session-table upsert, or fb_parse_classify_dev with FB_RING_NO_FLOW) -> batch stats back, while
 * the producer fills the next one.  With every batch in flight the producer waits for the oldest
 * (no drop-on-full).  The session table stays in HBM (fb_flow_export); DNS side records come back
 * with their payload bytes (fb_ring_poll_dns).  One producer thread per ring, one ring per ctx. */
typedef struct fb_ring fb_ring;
typedef struct fb_ring_config {
    uint32_t slots;       /* pinned batches, 2..64 (0 = 4)                       */
    uint32_t max_packets; /* frames per batch                                    */
    uint64_t max_bytes;   /* frame bytes per batch, < 4 GiB                      */
    uint32_t flags;       /* FB_RING_*                                           */
    uint32_t copy_threads; /* threads of fb_ring_push_block's copy into the pinned batch (the
                              producer + copy_threads - 1 helpers the ring owns; 0 or 1 = the
                              producer alone; at most 64); other calls are unaffected */
} fb_ring_config;
#define FB_RING_NO_FLOW 1u /* parse + classify only, no session-table update */
typedef struct fb_ring_dns {
    uint64_t packet_seq;     /* frames pushed into the ring before this one          */
    uint64_t payload_offset; /* into the payload buffer of fb_ring_poll_dns          */
    uint32_t payload_length;
    uint8_t protocol;        /* 6 / 17 */
    uint8_t family;          /* 2 / 10 */
    uint16_t reserved;
} fb_ring_dns; /* 24 bytes */
fb_ring* fb_ring_create(fb_ctx* ctx, const fb_ring_config* cfg); /* NULL on failure */
int fb_ring_destroy(fb_ring* r);
int fb_ring_push(fb_ring* r, const uint8_t* frame, uint32_t caplen);            /* copies one frame */
int fb_ring_push_block(fb_ring* r, const uint8_t* frames, const uint32_t* offsets, uint32_t n);
uint8_t* fb_ring_reserve(fb_ring* r, uint32_t caplen); /* zero-copy: write the frame there before the
                                                           next push/reserve/submit; NULL on error */
/* Zero-copy block for bulk producers (TPACKET_V3 blocks, capture engines): room for n frames of
 * `bytes` in total in one batch.  The caller writes the frames at the returned pointer and
 * offsets[k] = *base + (start of frame k within that area), k < n, before the next ring call. */
uint8_t* fb_ring_reserve_block(fb_ring* r, uint32_t n, uint64_t bytes, uint32_t** offsets, uint32_t* base);
int fb_ring_submit(fb_ring* r);                        /* submit the partly filled batch now      */
int fb_ring_sync(fb_ring* r);                          /* submit + wait for every batch           */
/* Totals over the completed batches (fields summed, error OR-ed), batches completed, frames pushed. */
int fb_ring_stats(fb_ring* r, fb_batch_stats* total, uint64_t* batches, uint64_t* frames);
/* Dequeue DNS side records of completed batches, their payloads packed into `payload`. */
int fb_ring_poll_dns(fb_ring* r, fb_ring_dns* out, uint32_t cap, uint8_t* payload, uint64_t payload_cap,
                     uint32_t* n, uint64_t* n_bytes);

/* ---- small device-memory helpers (so hosts without a GPU runtime binding can drive the
 *      device-resident entry points, e.g. through ctypes) ------------------------------- */
int fb_dev_alloc(void** p, uint64_t bytes);
int fb_dev_free(void* p);
int fb_host_alloc_pinned(void** p, uint64_t bytes);
int fb_host_free_pinned(void* p);
int fb_memcpy_h2d(void* dst, const void* src, uint64_t bytes, void* stream); /* async */
int fb_memcpy_d2h(void* dst, const void* src, uint64_t bytes, void* stream); /* async */
int fb_memset_dev(void* dst, int value, uint64_t bytes, void* stream);       /* async */
int fb_stream_create(void** stream);
int fb_stream_destroy(void* stream);
int fb_stream_sync(void* stream);
int fb_event_create(void** ev);
int fb_event_destroy(void* ev);
int fb_event_record(void* ev, void* stream);
int fb_event_elapsed_ms(float* ms, void* ev_start, void* ev_stop); /* syncs ev_stop */
int fb_event_query(void* ev); /* FB_OK once the event completed, 1 while pending: a capture loop
                                 polls it instead of blocking (no wake-up latency)          */
/* Busy-wait until the event completed: the polled completion without a call per poll. */
int fb_event_spin(void* ev);
int fb_device_count(int* n);
int fb_set_device(int device);
int fb_ctx_device(const fb_ctx* ctx, int* device); /* the device fb_create bound the context to */

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* FLODBADD_GPU_H */
