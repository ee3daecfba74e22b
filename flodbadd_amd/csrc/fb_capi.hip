// fb_capi.hip -- C ABI (include/flodbadd_gpu.h) over the gfx950 kernels.
//
// Host-side counterpart of the reference capture task's per-packet calls
// (src/capture.rs:1036-1061 / 1219-1249): a context owns the device-resident configuration
// (service-port bitmap, filter, IPv6 LAN prefixes, own IPs), the look-back scratch, the flow
// table and (lazily) host-mode staging buffers.  Every entry point returns an fb_err code;
// nothing aborts.  No CPU fallback exists: without a gfx950 device fb_create fails.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "fb_host.h"
#include "fb_internal.h"
#include "fb_l7_index.h"
#include "service_ports_default.inc"  // kDefaultServiceBitmap[8192] (generated at build time)

using namespace fbk;

namespace fbk {

static thread_local char g_err[512] = "";

int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace fbk

// Update scratch of one table update (K1 bucketing -> K1c -> K1t -> K2).  Two sets: the pipelined
// call buckets batch k (on the caller's stream, right after its parse) into set k & 1 while the
// update stream applies batch k - 1 from the other set.
struct UpdScratch {
    DevBuf<uint32_t> entries;   // [flow_recs] bucketed record slots (or combined ids)
    DevBuf<FlowEntry> comb;     // k_flow_combine entries (2 units each), comb_cap of them
    DevBuf<uint32_t> rows;      // [flow_chunks][flow_parts]
    DevBuf<uint32_t> cols;      // [flow_parts][flow_chunks]
    DevBuf<uint32_t> rows_h;    // [flow_chunks][flow_parts] combined groups' rows before k_flow_combine
    DevBuf<uint32_t> e_orig;    // [flow_recs] combined groups' original entry words (history)
    DevBuf<uint2> e_sort;       // [flow_recs] combined groups' records in record order (history)
    DevBuf<uint32_t> hot;       // [flow_recs / 16 + 16] hot groups for k_flow_combine
    DevBuf<uint32_t> ctl;       // [4] its counters (FlowParams::ctl)
    DevBuf<uint32_t> order;     // [flow_parts + kK2Lead + 1] K2's partition order (FlowParams::order)
};
// Per-record scratch of an update, [flow_recs] each: made together by ensure_flow_scratch (the buffers of
// the odd async batches by the first pipelined call after it).
struct RecScratch {
    DevBuf<uint32_t> hword;      // K2's history word per entry
    DevBuf<uint32_t> rec_part;   // partition per record slot (fb_process_seg_dev)
    DevBuf<uint32_t> rec_part2;  // ... of the odd async batches
    DevBuf<uint4> rec_ent;       // update entry (UpdEnt, 64 B) per record slot
    DevBuf<uint4> rec_ent2;      // ... of the odd async batches
    DevBuf<uint32_t> agg_slot;   // [flow_recs / 2 + 1] table slot per combined entry
};
// Dense output (fb_parse_classify_dev & co., fb_seg_compact_dev): segment counts + their scan, and the
// single-pass kernel's per-tile look-back words (k_parse_dense), for `cap` segments.
struct ScanScratch {
    DevBuf<uint32_t> cseg;               // [cap] segment counts (dense pass 1)
    DevBuf<unsigned long long> cpre;     // [cap] batch-wide offset of every segment
    DevBuf<unsigned long long> cstatus;  // [seg_scan_tiles(cap)] scan look-back words
    DevBuf<uint32_t> cticket;            // scan ticket counter
    DevBuf<unsigned long long> dstatus;  // [cap / parse_dense_tile_segs() + 1]
    uint64_t cap = 0;                    // segments
    uint32_t scan_epoch = 0;             // epoch of the last scan (0: status needs zeroing)
    uint32_t dense_epoch = 0;            // epoch of the last dense launch (0: status needs zeroing)
};
// Host-mode staging: the frames, the per-packet arrays (`pkts_cap` packets) and the stats grow apart.
struct Staging {
    struct Pkts {
        DevBuf<uint32_t> offsets;
        DevBuf<fb_pkt_out> out;
        DevBuf<fb_dns_out> dns;
        DevBuf<uint8_t> cls;
    };
    DevBuf<uint8_t> frames;
    Pkts pk;
    DevBuf<fb_batch_stats> stats;
};
// The installed whitelist's domain patterns (fb_set_whitelist_dom, fb_wl_domain.hip) and the match state of the
// DNS tracker's names against them: rows / flags hold `cap` names (and id 0), valid for the ids 1 .. upto.
struct WlDomDev {
    WlDomIndex host;  // what the tables were made from (the mask knob rebuilds them)
    DevBuf<uint8_t> blob;
    DevBuf<uint32_t> off, len[kWlDomHashed], pid[kWlDomHashed], gpid, gstar;
    DevBuf<unsigned long long> hash[kWlDomHashed];
    DevBuf<uint32_t> rows;
    DevBuf<uint8_t> flags;
    DevBuf<unsigned long long> ctr;  // [2] names with a non-empty row, names overflowed (of the ids 1 .. upto)
    uint64_t cap = 0, upto = 0;
    bool active() const { return host.n_patterns() != 0u; }
    WlDomTables tables() const {
        WlDomTables t = host.tables();  // the counts and the mask; every pointer replaced by the device's
        t.blob = blob;
        t.off = off;
        for (uint32_t k = 0; k < kWlDomHashed; ++k) {
            t.hash[k] = hash[k];
            t.len[k] = len[k];
            t.pid[k] = pid[k];
        }
        t.gpid = gpid;
        t.gstar = gstar;
        return t;
    }
};
// The installed whitelist's index (fb_set_whitelist, fb_whitelist.hip).
struct WlDev {
    DevBuf<uint32_t> a4, k4, k6, gkey, gbeg, owner, country, dpid;
    DevBuf<unsigned long long> kp4, kp6;  // with_proc: instead of k4 / k6
    DevBuf<unsigned long long> dkp;       // the domain endpoints with a pattern id (WlIndex::dpid / dkp)
    DevBuf<uint4> a6;
    DevBuf<WlRule> rules;
    uint32_t n4 = 0, n6 = 0, ng = 0, nr = 0, records = 0, nd = 0;
    bool with_proc = false;  // WlIndex::with_proc: the process-aware instances run
    WlDomDev dom;
    WlTables tables() const {
        return {a4, k4, a6, k6, gkey, gbeg, rules, owner, country, kp4, kp6, n4, n6, ng, nr, records, dpid, dkp, nd};
    }
};
// The names of the L7 plane's process ids (fb_set_l7_process_names); n 0: no table.
struct L7Names {
    DevBuf<uint32_t> match_id, name_id;
    uint32_t n = 0;
};
// The installed anomaly model (fb_set_anomaly_model, fb_anomaly.hip).
struct AnModel {
    DevBuf<fb_if_node> nodes;
    DevBuf<uint32_t> first;
    DevBuf<uint32_t> service;  // [65536]; empty: every code 0
    uint32_t trees = 0;
    fb_an_params prm = {};
    bool active = false;
    AnForest forest() const {
        AnForest f;
        if (active) {
            f.nodes = nodes;
            f.first = first;
            f.n_trees = trees;
            f.prm = prm;
        }
        f.service_code = service;
        return f;
    }
};
// The installed socket snapshot's index (fb_set_l7_sockets, fb_l7_index.h).
struct L7Dev {
    DevBuf<L7Pair> pairs;
    DevBuf<L7Local> locals;
    uint32_t n_pairs = 0, n_locals = 0;
    bool active = false;
    L7Tables tables() const { return {pairs, locals, n_pairs, n_locals}; }
};
// Enrichment tables (fb_set_asn_tables / fb_set_blacklists, fb_enrich.hip).
struct EnrichDev {
    DevBuf<fb_asn_range> asn4, asn6;
    DevBuf<uint32_t> bl4_pos;
    DevBuf<uint4> bl6_pos;
    DevBuf<unsigned long long> bl4_mask, bl6_mask;
    uint32_t n4 = 0, n6 = 0, m4 = 0, m6 = 0;
    EnrichTables tables() const { return {asn4, asn6, bl4_pos, bl4_mask, bl6_pos, bl6_mask, n4, n6, m4, m6}; }
};

// Per-slot planes: arrays beside the table, one element per slot, that a flow's element follows through
// every slot move.  Described once here; the functions below (plane_ensure .. plane_copy_out) are the
// only code that allocates, moves, clears or frees one, so a new plane is one entry and its pass.
enum PlaneId : uint32_t { kPlaneTime, kPlaneStatus, kPlaneWl, kPlaneBl, kPlaneAn, kPlaneMod, kPlaneDom, kPlaneHist,
                          kPlaneL7, kPlanes };
struct PlaneDesc {
    size_t elem;       // bytes per slot
    const char* name;  // in error text
    bool lazy;         // made (zeroed) by the first pass that writes it, a zero element standing for "no pass
                       // has seen the flow": fb_flow_clear zeroes it.  Else: made with a timed context's table,
                       // and an insert rewrites the element
    bool age_moves;    // k_flow_age moves it in place with the slots of a purge; else it follows through the
                       // slot map the purge publishes
    hipError_t (*remap)(const void* old, const uint32_t* remap, unsigned long long old_cap, void* nw, hipStream_t s);
};
static const PlaneDesc kPlaneDesc[kPlanes] = {
    {sizeof(FlowTime), "time plane", false, true, launch_plane_remap<FlowTime>},        // fb_time.hip
    {1, "status plane", true, true, launch_plane_remap<uint8_t>},                       // fb_age.hip, kAge*
    {1, "whitelist plane", true, false, launch_plane_remap<uint8_t>},                   // fb_whitelist.hip, FB_WL_*
    {8, "blacklist plane", true, false, launch_plane_remap<unsigned long long>},        // fb_blacklist.hip
    {sizeof(fb_an_rec), "anomaly plane", true, false, launch_plane_remap<fb_an_rec>},   // fb_anomaly.hip
    // the passes' last_modified stamps (fb_set_pass_time; read by fb_view.hip): made by the first stamped pass
    {8, "stamp plane", true, false, launch_plane_remap<unsigned long long>},
    {sizeof(fb_flow_domain), "domain plane", true, false, launch_plane_remap<uint2>},   // fb_domains.hip
    // the history store's {head, tail, len, reserved} (fb_histstore.hip): made by fb_hist_store_enable
    {sizeof(uint4), "history plane", true, false, launch_plane_remap<uint4>},
    {sizeof(fb_l7_rec), "L7 plane", true, false, launch_plane_remap<uint2>},           // fb_l7.hip
};
static_assert(sizeof(fb_flow_domain) == sizeof(uint2), "one name-id pair per slot");
static_assert(sizeof(fb_l7_rec) == sizeof(uint2), "one L7 element per slot");
// the counter words of one synchronous pass over the table (pass_begin / pass_end)
constexpr uint32_t kPassStatWords = std::max({kAgeStatWords, kWlCounters, kBlCounters, kAnCounters, kDomCounters, kL7Counters});

// The flow table and the arrays sized by its capacity: made together (table_alloc), and replaced together by
// a growth.  A plane is an array beside the table, one element per slot (kPlaneDesc); empty: not made yet.
struct FlowTable {
    uint64_t cap = 0;     // slots
    uint32_t parts = 0;   // partitions of kFlowSlots slots
    uint32_t shift = 64;  // 64 - log2(parts)
    DevBuf<FlowSlot> slots;
    DevBuf<unsigned long long> partials;  // [4 * parts] per-partition new / updated / occupied / history
    DevBuf<uint32_t> hcount;              // [cap] history characters per slot of the last update
    DevBuf<uint32_t> part_base;           // [parts + 1] history output offset per partition
    DevBuf<uint32_t> hist_slow;           // [parts + 1] count + partitions for the general history kernel
    DevBuf<uint4> char_call;              // [cap] first update call of S s H h per slot (the merge's)
    DevBuf<uint8_t> plane[kPlanes];       // [cap * kPlaneDesc[p].elem]
};

// What a fused parse writes and the update of the same batch reads, per record slot: the table partition
// and the update entry (RecScratch buffers).  A value of one call, handed from the entry point to its
// parse and its update; empty: no fused hand-off.
struct FusedParts { uint32_t* part = nullptr; uint4* ent = nullptr; };
// The last table update, as the history calls need it: valid until the update's scratch is reallocated,
// its slots move (a growth, a purge, a clear) or an empty update follows.
struct LastUpdate {
    FlowParams p;
    uint32_t slots = 0, chunks = 0;
    bool valid = false;
    void invalidate() { valid = false; }
    uint32_t live_slots() const { return valid ? slots : 0u; }  // record slots whose history can still be read
};
// Record slots of a segmented batch of n frames: whole segments.
static constexpr uint32_t seg_slots(uint32_t n) { return (n + FB_SEG_FRAMES - 1) / FB_SEG_FRAMES * FB_SEG_FRAMES; }

struct fb_ctx {
    int device = 0;
    std::unique_ptr<DevConfig> h_cfg;  // host shadow
    DevBuf<DevConfig> d_cfg;
    bool cfg_dirty = true;
    DevBuf<unsigned long long> d_tick;  // [kTickWords] k_parse_seg stats words
    bool need_reset = true;       // zero the tick + error words before the next launch
    uint32_t epoch = 0;           // parse launches so far: its parity picks the launch's error word
    uint32_t seg_grid = 0;        // streaming segmented kernel: co-resident blocks
    uint32_t seg_grid_async = 0;  // ... in the pipelined call: FB_ASYNC_BPC blocks per CU (not the full
                                  // grid), so the previous batch's table update keeps part of each CU
    DevBuf<uint32_t> d_error;     // [4] error words, indexed by launch & 3 (a launch clears the next one's;
                                  // a pipelined update still writes the one two launches back)
    ScanScratch sc;               // dense output scratch (ensure_compact_scratch)
    // single-pass dense output (k_parse_dense): grid, and the look-back's polls before it computes a late
    // predecessor's sums itself (fb_debug_set FB_DEBUG_DENSE_STEAL_POLLS; tests set 0 to force that path)
    uint32_t dense_grid = 0;
    uint32_t steal_polls = 1u << 12;
    unsigned long long dn_skew = 0ull;  // FB_DEBUG_DENSE_OFFSET_SKEW: fault injection (k_parse_dense copy bounds)
    // flow table
    FlowTable tb;
    template <typename T>
    T* plane(PlaneId p) const { return reinterpret_cast<T*>(tb.plane[p].get()); }
    UpdScratch us[2];               // update scratch sets (set 1: pipelined calls only, allocated lazily)
    RecScratch rs;
    uint32_t comb_cap = 0;
    uint64_t flow_recs = 0;         // scratch capacity (multiple of kFlowChunk)
    uint32_t last_n = 0;            // packets of the last parse launch (bounds its records)
    // growth: the occupancy each update reports in host-mapped memory, updates issued
    PinnedBuf<FlowMailbox> mbox;    // host-mapped (written by k_flow_finish)
    uint64_t upd_seq = 0;           // table updates issued (the mailbox's seq counts them from 1)
    uint64_t grown_seq = 0;         // upd_seq at the last growth (older reports describe the old geometry)
    uint64_t clear_seq = 0;         // upd_seq at the last fb_flow_clear (older reports are void)
    uint64_t generation = 0;        // slot moves: growths and purges
    bool grow = true;               // FB_CFG_FIXED_TABLE clears it
    DevBuf<uint32_t> d_remap;       // the last growth's (or purge's) old -> new slot map
    DevBuf<unsigned long long> d_pass_stats;  // [kPassStatWords]
    uint64_t pass_time = 0;         // fb_set_pass_time: what the passes stamp the flows they change with (0: no stamps)
    bool view_direct = false;       // FB_DEBUG_VIEW_DIRECT: the view export's one-lane-per-record copy-out
    // Zeek export (fb_format_zeek_dev, fb_zeek.hip): rocPRIM's scan storage
    bool zeek_direct = false;       // FB_DEBUG_ZEEK_DIRECT: no LDS staging of the text
    StreamScratch zeek_tmp;
    // endpoint learning (fb_flow_learn_endpoints_dev, fb_learn.hip): the per-table-slot arrays, the endpoint index
    StreamScratch learn_slots, learn_index;
    unsigned long long learn_hash_mask = ~0ull;  // FB_DEBUG_LEARN_HASH_MASK
    unsigned long long wl_name_hash_mask = ~0ull;  // FB_DEBUG_WL_NAME_HASH_MASK
    // timed contexts (FB_CFG_TIMED, fb_time.hip): the capture-time pass's scratch
    bool timed = false;
    StreamScratch tscratch;
    // session aging (fb_flow_age, fb_age.hip): the buffer the next purge writes its slot map into (swapped
    // with d_remap when the purge removed something); reallocated when its size is not the table's
    DevBuf<uint32_t> d_age_remap;
    // whitelist conformance (fb_set_whitelist / fb_flow_whitelist, fb_whitelist.hip)
    bool wl_active = false;
    WlDev wl;
    AnModel an;     // anomaly pass (fb_set_anomaly_model / fb_flow_anomaly, fb_anomaly.hip)
    EnrichDev en;   // fb_set_asn_tables / fb_set_blacklists
    L7Dev l7;       // L7 pass (fb_set_l7_sockets / fb_flow_l7, fb_l7.hip)
    L7Names l7_names;  // fb_set_l7_process_names: what the whitelist pass and the endpoint learning read processes by
    WlProcNames proc_names() const {
        return {plane<fb_l7_rec>(kPlaneL7), l7_names.match_id, l7_names.name_id, l7_names.n};
    }
    // DNS tracker (fb_dns_track_enable, fb_dnstrack.hip); null: tracking is off (freed by fb_destroy)
    DnsTrack* dns = nullptr;
    // history store (fb_hist_store_enable, fb_histstore.hip); null: off (freed by fb_destroy).  hs_updates:
    // non-empty update calls since enable; hs_seen: the one the last append call looked at; hs_applied: the
    // updates an append ran for
    HistStore* hs = nullptr;
    uint64_t hs_updates = 0, hs_seen = 0, hs_applied = 0;
    StreamScratch mscratch;  // multi-GPU merge scratch (export owner counts / merge tables)
    DevBuf<unsigned long long> d_n;
    // ordered per-flow state: update calls since create/clear
    uint32_t flow_batch = 0;
    bool emit_records = true;               // fb_set_session_records: fused calls store SESSION records
    // fb_process_seg_async_dev: updates on the context's own stream, one batch behind the parses
    DevStream upd;
    DevEvent ev_parsed;
    // after the last fb_flow_history_dev: it reads the last update's shared scratch (history words,
    // partials, slot counts, combined-entry slots), which the next update rewrites -- that update
    // waits for it on every stream it uses, whichever stream the history ran on
    DevEvent ev_hist;
    bool hist_pending = false;
    DevEvent ev_upd[2];                         // after the update of async batch k (k & 1)
    uint64_t async_k = 0;                       // async batches issued
    uint32_t upd_word[2] = {4u, 4u};            // error word (launch & 3) of the async update in slot k & 1 (4: none)
    // Borrowed, never freed here: the caller's buffers and event.
    hipEvent_t stage_event = nullptr;  // fb_set_stage_event (caller-owned): recorded between the
                                       // parse and the update of fb_process[_seg]_dev
    const unsigned long long* next_ts = nullptr;  // fb_set_frame_times arms it, take_frame_times alone reads + clears it
    const void* async_prev[3] = {nullptr, nullptr, nullptr};  // the last async batch's records, counts, stats
    LastUpdate last;                      // all an update leaves for later calls (the history calls read it)
    DevBuf<uint8_t> d_hist_cnt;           // per-block slot counts of hot history partitions (lazy), bytes
    Staging st;                           // host-mode staging (ensure_staging)
};

int fbk::ctx_device(const fb_ctx* c) { return c->device; }

// A call (or a ring batch) reported a nonzero device error word: the scratch the launches share
// (stats tick words, error words) is zeroed before the context's next launch.
int fbk::ctx_report_error(fb_ctx* c, uint64_t e) {
    c->need_reset = true;
    if (e & 4u) return set_err(FB_ERR_TABLE_FULL, "flow table full (error word %llu)", (unsigned long long)e);
    return set_err(FB_ERR_INTERNAL, "device error word %llu (2: offset scan expired, 8: update scratch "
                   "overflow, 16: table-update spin expired, 32: dense tile offset past the batch)",
                   (unsigned long long)e);
}

// Entry points that read or write the table or the update scratch first order their stream after
// the last pipelined update (fb_process_seg_async_dev runs updates on the context's own stream);
// host code that frees or rewrites that scratch waits for it.
static int join_updates(fb_ctx* c, hipStream_t s) {
    if (c->async_k == 0) return FB_OK;
    HIP_TRY(hipStreamWaitEvent(s, c->ev_upd[(c->async_k - 1u) & 1u], 0));
    return FB_OK;
}
// A parse launch zeroes the error word of the launch after it ((launch + 1) & 3).  A pipelined
// update still in flight may own that word (it sets bits there and copies it into its stats at
// the end): the stream waits for that update first, so no failure bit of it is lost.
static int guard_next_error_word(fb_ctx* c, hipStream_t s) {
    if (c->async_k == 0) return FB_OK;
    const uint32_t z = (c->epoch + 2u) & 3u;
    for (uint32_t k = 0; k < 2; ++k)
        if (c->upd_word[k] == z) HIP_TRY(hipStreamWaitEvent(s, c->ev_upd[k], 0));
    return FB_OK;
}
static int drain_updates(fb_ctx* c) {
    if (c->async_k && c->upd) HIP_TRY(hipStreamSynchronize(c->upd));
    if (c->hist_pending) HIP_TRY(hipEventSynchronize(c->ev_hist));  // (before scratch is freed)
    return FB_OK;
}

// ---- per-slot planes (kPlaneDesc) ----------------------------------------------------------------
static hipError_t plane_zero(fb_ctx* c, PlaneId p, hipStream_t s) {
    return c->tb.plane[p] ? hipMemsetAsync(c->tb.plane[p], 0, c->tb.cap * kPlaneDesc[p].elem, s) : hipSuccess;
}
// The plane exists (made zeroed when it does not).
static int plane_ensure(fb_ctx* c, PlaneId p, hipStream_t s) {
    if (c->tb.plane[p]) return FB_OK;
    if (c->tb.plane[p].alloc(c->tb.cap * kPlaneDesc[p].elem) != hipSuccess)
        return set_err(FB_ERR_NOMEM, "%s", kPlaneDesc[p].name);
    HIP_TRY(plane_zero(c, p, s));
    return FB_OK;
}
// A slot move (remap[old slot] = new slot, ~0u: none) into a table of new_cap slots: nw, new_cap elements
// the caller allocated, is zeroed and every element put at its flow's new slot.
static hipError_t plane_move(const fb_ctx* c, PlaneId p, const uint32_t* remap, uint64_t new_cap, hipStream_t s,
                             void* nw) {
    const hipError_t e = hipMemsetAsync(nw, 0, new_cap * kPlaneDesc[p].elem, s);
    return e != hipSuccess ? e : kPlaneDesc[p].remap(c->tb.plane[p], remap, c->tb.cap, nw, s);
}
// A table of `cap` slots (a power of two, kFlowSlots at least) with the arrays sized by it, and the planes
// `like` has: whole, or t is left empty and the name of what could not be allocated returned (else null).
static const char* table_alloc(FlowTable& t, uint64_t cap, const FlowTable* like) {
    const uint64_t parts = cap / kFlowSlots;
    const char* failed = nullptr;
    const hipError_t e = alloc_group(t, [&](FlowTable& n) {
        n.cap = cap;
        n.parts = (uint32_t)parts;
        for (n.shift = 64u; (1ull << (64u - n.shift)) < parts;) --n.shift;
        failed = "flow table";
        hipError_t a = n.slots.alloc(cap);
        if (a != hipSuccess) return a;
        failed = "flow table partials";
        a = alloc_each(n.partials, 4ull * parts, n.hcount, cap, n.part_base, parts + 1ull, n.hist_slow, parts + 1ull);
        if (a != hipSuccess) return a;
        failed = "character-call array";
        a = n.char_call.alloc(cap);
        for (uint32_t p = 0; a == hipSuccess && like && p < kPlanes; ++p) {
            failed = kPlaneDesc[p].name;
            if (like->plane[p]) a = n.plane[p].alloc(cap * kPlaneDesc[p].elem);
        }
        return a;
    });
    return e == hipSuccess ? nullptr : failed;
}
// After a purge that moved slots: the planes k_flow_age does not move itself follow through the slot map
// it published (c->d_remap).  A plane whose move failed is dropped -- every flow reads as unseen /
// Unknown again -- rather than left behind its flows, and the call reports the error.
static int planes_follow_purge(fb_ctx* c, hipStream_t s) {
    int rc = FB_OK;
    for (uint32_t p = 0; p < kPlanes; ++p) {
        if (kPlaneDesc[p].age_moves || !c->tb.plane[p]) continue;
        DevBuf<uint8_t> nw;
        hipError_t e = nw.alloc(c->tb.cap * kPlaneDesc[p].elem);
        if (e == hipSuccess) e = plane_move(c, (PlaneId)p, c->d_remap, c->tb.cap, s, nw);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            nw.reset();
            if (!rc) rc = set_err(FB_ERR_HIP, "%s remap: %s", kPlaneDesc[p].name, hipGetErrorString(e));
        }
        c->tb.plane[p] = std::move(nw);
    }
    return rc;
}
// fb_flow_clear: every flow is gone, so the lazily made planes read "unseen" everywhere.
static int planes_clear(fb_ctx* c, hipStream_t s) {
    for (uint32_t p = 0; p < kPlanes; ++p)
        if (kPlaneDesc[p].lazy) HIP_TRY(plane_zero(c, (PlaneId)p, s));
    return FB_OK;
}
// The fb_flow_*_dev getters: min(cap, table capacity) elements; a plane no pass has made reads zeros.
static int plane_copy_out(fb_ctx* c, PlaneId p, void* d_out, uint64_t cap, void* stream) {
    if (!c || (cap && !d_out)) return set_err(FB_ERR_INVAL, "bad arguments");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t bytes = std::min<uint64_t>(cap, c->tb.cap) * kPlaneDesc[p].elem;
    if (bytes == 0) return FB_OK;
    if (c->tb.plane[p])
        HIP_TRY(hipMemcpyAsync(d_out, c->tb.plane[p], bytes, hipMemcpyDeviceToDevice, s));
    else
        HIP_TRY(hipMemsetAsync(d_out, 0, bytes, s));
    return FB_OK;
}

// A synchronous pass over the table (fb_flow_age / _whitelist / _blacklist) drains the updates in flight
// and starts from `words` zeroed counter words; pass_end reads them back once the pass has run.
static int pass_begin(fb_ctx* c, uint32_t words, hipStream_t s) {
    const int rc = drain_updates(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if (!c->d_pass_stats && c->d_pass_stats.alloc(kPassStatWords) != hipSuccess)
        return set_err(FB_ERR_NOMEM, "pass counters");
    HIP_TRY(hipMemsetAsync(c->d_pass_stats, 0, words * 8ull, s));
    return FB_OK;
}
static int pass_end(fb_ctx* c, unsigned long long* h, uint32_t words, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(h, c->d_pass_stats, words * 8ull, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FB_OK;
}

// The stamp plane a pass writes when a pass time is set (made on first use), else null: the pass then runs
// its unstamped kernel instance.
static int pass_stamps(fb_ctx* c, hipStream_t s, unsigned long long** mod) {
    *mod = nullptr;
    if (c->pass_time == 0) return FB_OK;
    const int rc = plane_ensure(c, kPlaneMod, s);
    if (!rc) *mod = c->plane<unsigned long long>(kPlaneMod);
    return rc;
}

// The host form of a compacting export: a device buffer of `cap` records of `rec` bytes, the _dev export
// into it (run(d_out), counting into c->d_n), the count read back, min(count, cap) records copied out.
template <typename Run>
static int export_to_host(fb_ctx* c, void* out, uint64_t cap, size_t rec, uint64_t* n, hipStream_t s, const char* what,
                          Run run) {
    DevBuf<uint8_t> d_out;
    if (d_out.alloc(cap * rec) != hipSuccess) return set_err(FB_ERR_NOMEM, "export buffer");
    unsigned long long h = 0;
    const int rc = run(d_out.get());
    hipError_t e = rc ? hipSuccess : hipMemcpyAsync(&h, c->d_n, 8, hipMemcpyDeviceToHost, s);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(s);
    const uint64_t got = std::min<uint64_t>(h, cap);
    if (!rc && e == hipSuccess && got) e = hipMemcpyAsync(out, d_out, got * rec, hipMemcpyDeviceToHost, s);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(s);
    if (rc) return rc;
    if (e != hipSuccess) return set_err(FB_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    *n = got;
    return FB_OK;
}

// fb_flow_history_dev / fb_hist_store_append_dev: the history characters of the last update (c->last,
// valid: the caller saw live_slots() != 0) into the caller's three outputs, on `s`, which the caller has
// ordered after the pipelined updates.  `then` runs after the kernel (the store appends what it wrote);
// the event the next update waits for comes after both.
template <typename Then>
static int last_history(fb_ctx* c, uint32_t* d_slot, uint8_t* d_chars, uint32_t* d_n, hipStream_t s, Then then) {
    const uint64_t cnt_bytes = flow_history_cnt_bytes(c->last.chunks);
    if (cnt_bytes > c->d_hist_cnt.size()) {
        HIP_TRY(hipStreamSynchronize(s));
        if (c->d_hist_cnt.alloc(cnt_bytes) != hipSuccess)
            return set_err(FB_ERR_NOMEM, "history block counts (%llu bytes)", (unsigned long long)cnt_bytes);
    }
    if (c->ev_hist.create() != hipSuccess) return set_err(FB_ERR_HIP, "history event");
    HIP_TRY(launch_flow_history(c->last.p, c->last.chunks, d_slot, d_chars, d_n, c->tb.hist_slow,
                                cnt_bytes ? reinterpret_cast<uint32_t*>(c->d_hist_cnt.get()) : nullptr, s));
    if (const int rc = then()) return rc;
    HIP_TRY(hipEventRecord(c->ev_hist, s));
    c->hist_pending = true;
    return FB_OK;
}

namespace fbk {
bool build_blacklist_tables(const fb_cidr* nets, uint32_t n, std::vector<uint32_t>& p4,
                            std::vector<unsigned long long>& m4, std::vector<uint4>& p6,
                            std::vector<unsigned long long>& m6);
}

// Replace a device array with a copy of host data (n elements); empty -> an empty buffer.
template <typename T>
static int upload_array(DevBuf<T>& d, const T* h, size_t n) {
    if (d.alloc(n) != hipSuccess) return set_err(FB_ERR_NOMEM, "enrichment table");
    if (n) HIP_TRY(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return FB_OK;
}

// One update scratch set sized for c->flow_recs records.
static int alloc_upd_scratch(fb_ctx* c, UpdScratch& u, hipStream_t s) {
    const uint64_t recs = c->flow_recs, rows = recs / kFlowChunk * c->tb.parts;
    const hipError_t e = alloc_group(u, [&](UpdScratch& n) {
        return alloc_each(n.entries, recs, n.comb, (uint64_t)c->comb_cap * 2ull, n.rows_h, rows, n.e_orig, recs, n.e_sort,
                          recs, n.rows, rows, n.cols, rows, n.hot, recs / 16 + 16, n.ctl, 4,
                          n.order, (uint64_t)c->tb.parts + kK2Lead + 1u);
    });
    if (e != hipSuccess) return set_err(FB_ERR_NOMEM, "flow update scratch (%llu records)", (unsigned long long)recs);
    HIP_TRY(hipMemsetAsync(u.ctl, 0, 16, s));
    return FB_OK;
}

// Session-table update scratch for batches of up to `recs` records (grown, never shrunk).  A growth
// replaces RecScratch, so a fused entry point calls this for its batch before it picks its FusedParts.
static int ensure_flow_scratch(fb_ctx* c, uint64_t recs, hipStream_t s) {
    if (!c->tb.slots) return FB_OK;
    recs = std::max<uint64_t>(recs, kFlowChunk);
    recs = (recs + kFlowChunk - 1) / kFlowChunk * kFlowChunk;
    if (recs <= c->flow_recs) return FB_OK;
    int rc = drain_updates(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    const bool had_set1 = c->us[1].entries != nullptr;
    for (UpdScratch& u : c->us) u = UpdScratch();
    c->comb_cap = 0;
    c->last.invalidate();  // its scratch is gone
    c->flow_recs = 0;
    const hipError_t e = alloc_group(c->rs, [&](RecScratch& r) {
        return alloc_each(r.hword, recs, r.rec_part, recs, r.rec_ent, recs * kUpdEntU4, r.agg_slot, recs / 2 + 1);
    });
    if (e != hipSuccess) return set_err(FB_ERR_NOMEM, "flow update scratch (%llu records)", (unsigned long long)recs);
    c->flow_recs = recs;
    // combined entries: at most one per two records of the hot groups; a quarter of the batch's
    // records is room for any skew we measured (past it a hot group just stays plain)
    c->comb_cap = (uint32_t)(recs / 4 + 256);
    rc = alloc_upd_scratch(c, c->us[0], s);
    if (!rc && had_set1) rc = alloc_upd_scratch(c, c->us[1], s);
    return rc;
}

static int upload_cfg(fb_ctx* c, hipStream_t s) {
    if (!c->cfg_dirty) return FB_OK;
    HIP_TRY(hipStreamSynchronize(s));  // nothing on this stream may still read d_cfg
    HIP_TRY(hipMemcpyAsync(c->d_cfg, c->h_cfg.get(), sizeof(DevConfig), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->cfg_dirty = false;
    return FB_OK;
}

// Zero the stats tick words and both error words before the next launch (at create, and after
// a call reported an error).  Stream-ordered: the launches run on `s`, which may be a
// non-blocking stream that does not synchronise with the null stream.
static int reset_launch_scratch(fb_ctx* c, hipStream_t s) {
    if (!c->need_reset) return FB_OK;
    const int rc = drain_updates(c);  // a pipelined update may still write an error word
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->d_tick, 0, kTickWords * 8ull, s));
    HIP_TRY(hipMemsetAsync(c->d_error, 0, 16, s));
    c->need_reset = false;
    return FB_OK;
}

static uint64_t dense_status_words(uint64_t nseg) { return nseg / parse_dense_tile_segs() + 1; }

// Scan scratch of the dense entry points, for batches of up to `n` frames (grown, never shrunk).
static int ensure_compact_scratch(fb_ctx* c, uint64_t n, hipStream_t s) {
    const uint64_t nseg = (n + FB_SEG_FRAMES - 1) / FB_SEG_FRAMES;
    if (nseg <= c->sc.cap) return FB_OK;
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t want = std::max<uint64_t>(nseg, 1024);
    const hipError_t e = alloc_group(c->sc, [&](ScanScratch& n) {
        return alloc_each(n.cseg, want, n.cpre, want, n.cstatus, seg_scan_tiles((uint32_t)want), n.cticket, 1, n.dstatus,
                          dense_status_words(want));
    });
    if (e != hipSuccess) return set_err(FB_ERR_NOMEM, "dense-output scratch (%llu segments)", (unsigned long long)want);
    HIP_TRY(hipMemsetAsync(c->sc.cticket, 0, 4, s));
    c->sc.cap = want;
    return FB_OK;
}

// The next scan's scratch: a fresh epoch (the status words are zeroed, stream-ordered, when the
// 8-bit epoch wraps).
static int scan_scratch(fb_ctx* c, hipStream_t s, SegScanScratch& sc) {
    if (c->sc.scan_epoch == 0u || c->sc.scan_epoch >= 255u) {
        HIP_TRY(hipMemsetAsync(c->sc.cstatus, 0, seg_scan_tiles((uint32_t)c->sc.cap) * 8ull, s));
        c->sc.scan_epoch = 0u;
    }
    sc.status = c->sc.cstatus;
    sc.ticket = c->sc.cticket;
    sc.epoch = ++c->sc.scan_epoch;
    sc.err = c->d_error + (c->epoch & 3u);
    return FB_OK;
}

static void set_lan(DevConfig* d, const fb_lan_v6* nets, uint32_t n) {
    d->n_lan_v6 = n;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t p = std::min<uint32_t>(nets[i].prefix, 128u);
        for (int k = 0; k < 4; ++k) {
            int bits = (int)p - 32 * k;
            uint32_t m = bits >= 32 ? 0xFFFFFFFFu : (bits <= 0 ? 0u : 0xFFFFFFFFu << (32 - bits));
            d->lan_v6[i].mask[k] = m;
            d->lan_v6[i].net[k] = nets[i].net[k] & m;
        }
    }
}

extern "C" {

uint32_t fb_abi_version(void) { return FB_ABI_VERSION; }
const char* fb_last_error(void) { return g_err; }

int fb_device_count(int* n) {
    if (!n) return set_err(FB_ERR_INVAL, "n is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *n = e == hipSuccess ? c : 0;
    return FB_OK;
}

int fb_ctx_device(const fb_ctx* ctx, int* device) {
    if (!ctx || !device) return set_err(FB_ERR_INVAL, "ctx or device is NULL");
    *device = ctx->device;
    return FB_OK;
}

fb_ctx* fb_create(int device, const fb_config* cfg) {
    if (!cfg) { set_err(FB_ERR_INVAL, "cfg is NULL"); return nullptr; }
    if (cfg->abi_version != FB_ABI_VERSION) {
        set_err(FB_ERR_INVAL, "abi_version %u != %u", cfg->abi_version, FB_ABI_VERSION);
        return nullptr;
    }
    if (cfg->filter > FB_FILTER_ALL || cfg->n_lan_v6 > FB_MAX_LAN_V6 || cfg->n_own_ips > FB_MAX_OWN_IPS ||
        (cfg->n_lan_v6 && !cfg->lan_v6) || (cfg->n_own_ips && !cfg->own_ips)) {
        set_err(FB_ERR_INVAL, "invalid fb_config field");
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        set_err(FB_ERR_NODEV, "device %d not available (%d HIP devices)", device, ndev);
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(FB_ERR_NODEV, "device %d is not gfx950 (%s)", device, prop.gcnArchName);
        return nullptr;
    }
    DeviceGuard g(device);
    fb_ctx* c = new (std::nothrow) fb_ctx();
    if (!c) { set_err(FB_ERR_NOMEM, "fb_ctx"); return nullptr; }
    c->device = device;
    {
        // The segmented kernel streams with no inter-workgroup wait; its grid is the co-resident
        // block count only so that every block stays busy until the batch is done.
        int sb = 0;
        if (occupancy_parse_seg(&sb) != hipSuccess || sb < 1) sb = 1;
        c->seg_grid = std::min<uint32_t>((uint32_t)(sb * prop.multiProcessorCount), 1023u);  // 10-bit stats tickets
#ifndef FB_ASYNC_BPC
#define FB_ASYNC_BPC 1  // round 3: with unsorted update entries 2 blocks per CU led (12.88 vs 12.55 Gpps);
                        // with the entries sorted by partition 1 block leaves K2 more of each CU
                        // (14.19-14.22 vs 13.74-13.75; 3 blocks 13.49-13.80)
#endif
        c->seg_grid_async = std::min<uint32_t>((uint32_t)(FB_ASYNC_BPC * prop.multiProcessorCount), c->seg_grid);
        int db = 0;
        if (occupancy_parse_dense(&db) != hipSuccess || db < 1) db = 1;
        c->dense_grid = std::min<uint32_t>((uint32_t)(db * prop.multiProcessorCount), 1023u);  // 10-bit stats tickets
    }
    c->h_cfg.reset(new (std::nothrow) DevConfig());
    bool ok = c->h_cfg != nullptr;
    if (ok) {
        memset(c->h_cfg.get(), 0, sizeof(DevConfig));
        memcpy(c->h_cfg->service_bitmap, cfg->service_bitmap ? cfg->service_bitmap : kDefaultServiceBitmap,
               FB_SERVICE_BITMAP_BYTES);
        c->h_cfg->filter = cfg->filter;
        set_lan(c->h_cfg.get(), cfg->lan_v6, cfg->n_lan_v6);
        c->h_cfg->n_own = cfg->n_own_ips;
        for (uint32_t i = 0; i < cfg->n_own_ips; ++i) c->h_cfg->own[i] = cfg->own_ips[i];
    }
    ok = ok && c->d_cfg.alloc(1) == hipSuccess;
    ok = ok && c->d_error.alloc(4) == hipSuccess && hipMemset(c->d_error, 0, 16) == hipSuccess;
    ok = ok && c->d_tick.alloc(kTickWords) == hipSuccess && hipMemset(c->d_tick, 0, kTickWords * 8ull) == hipSuccess;
    ok = ok && c->d_n.alloc(2) == hipSuccess;
    if (ok && cfg->flow_capacity > kFlowMaxCapacity) {
        set_err(FB_ERR_INVAL, "flow_capacity %llu > %llu slots", (unsigned long long)cfg->flow_capacity,
                (unsigned long long)kFlowMaxCapacity);
        ok = false;
    }
    if (ok && cfg->flow_capacity) {
        uint64_t cap = kFlowSlots;
        while (cap < cfg->flow_capacity) cap <<= 1;
        ok = table_alloc(c->tb, cap, nullptr) == nullptr &&
             hipMemset(c->tb.slots, 0, cap * sizeof(FlowSlot)) == hipSuccess &&
             c->mbox.alloc(1, hipHostMallocMapped) == hipSuccess;
        if (ok) memset(c->mbox.get(), 0, sizeof(FlowMailbox));
        c->grow = (cfg->flags & FB_CFG_FIXED_TABLE) == 0u;
        c->timed = (cfg->flags & FB_CFG_TIMED) != 0u;
        if (ok && c->timed)  // (zeroed on the null stream, which upload_cfg below synchronises before the return)
            ok = plane_ensure(c, kPlaneTime, nullptr) == FB_OK;
        ok = ok && ensure_flow_scratch(c, cfg->max_batch_packets, nullptr) == FB_OK;
    }
    ok = ok && upload_cfg(c, nullptr) == FB_OK;
    if (!ok) {
        if (g_err[0] == 0) set_err(FB_ERR_NOMEM, "device allocation failed");
        fb_destroy(c);
        return nullptr;
    }
    return c;
}

int fb_destroy(fb_ctx* c) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    DeviceGuard g(c->device);
    (void)hipDeviceSynchronize();
    dnstrack_free(c->dns);
    histstore_free(c->hs);
    delete c;
    return FB_OK;
}

int fb_set_filter(fb_ctx* c, uint32_t filter) {
    if (!c || filter > FB_FILTER_ALL) return set_err(FB_ERR_INVAL, "bad ctx or filter");
    if (c->h_cfg->filter != filter) { c->h_cfg->filter = filter; c->cfg_dirty = true; }
    return FB_OK;
}

int fb_set_service_bitmap(fb_ctx* c, const uint8_t* bm) {
    if (!c || !bm) return set_err(FB_ERR_INVAL, "bad ctx or bitmap");
    memcpy(c->h_cfg->service_bitmap, bm, FB_SERVICE_BITMAP_BYTES);
    c->cfg_dirty = true;
    return FB_OK;
}

int fb_set_lan_v6(fb_ctx* c, const fb_lan_v6* nets, uint32_t n) {
    if (!c || n > FB_MAX_LAN_V6 || (n && !nets)) return set_err(FB_ERR_INVAL, "bad lan_v6 table");
    set_lan(c->h_cfg.get(), nets, n);
    c->cfg_dirty = true;
    return FB_OK;
}

int fb_set_stage_event(fb_ctx* c, void* event) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    c->stage_event = (hipEvent_t)event;  // the caller's event (fb_event_create); not owned
    return FB_OK;
}

int fb_set_frame_times(fb_ctx* c, const uint64_t* d_ts) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->timed) return set_err(FB_ERR_INVAL, "the context was created without FB_CFG_TIMED");
    c->next_ts = reinterpret_cast<const unsigned long long*>(d_ts);
    return FB_OK;
}

// Every update call of a timed context takes the frame times armed before it: once, after its own argument
// checks and before any device work, so it consumes them whether it then succeeds or fails.  Untimed: null.
static int take_frame_times(fb_ctx* c, const unsigned long long** ts) {
    if (c->timed && !c->next_ts)
        return set_err(FB_ERR_INVAL, "a timed context needs fb_set_frame_times before each update call");
    *ts = c->next_ts;
    c->next_ts = nullptr;
    return FB_OK;
}

static int wl_dom_set_mask(fb_ctx* c, unsigned long long mask);  // (with the whitelist calls)
int fb_debug_set(fb_ctx* c, uint32_t knob, uint64_t value) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    switch (knob) {
        case FB_DEBUG_DENSE_STEAL_POLLS:
            c->steal_polls = (uint32_t)std::min<uint64_t>(value, 0xFFFFFFFFull);
            return FB_OK;
        case FB_DEBUG_DENSE_OFFSET_SKEW:
            if (value > 0xFFFFFFFFull) return set_err(FB_ERR_INVAL, "skew %llu >= 2^32", (unsigned long long)value);
            c->dn_skew = value;
            if (value) fprintf(stderr, "flodbadd_gpu: FB_DEBUG_DENSE_OFFSET_SKEW %llu active on this context (fault injection)\n",
                               (unsigned long long)value);
            return FB_OK;
        case FB_DEBUG_VIEW_DIRECT:
            c->view_direct = value != 0;
            return FB_OK;
        case FB_DEBUG_ZEEK_DIRECT:
            c->zeek_direct = value != 0;
            return FB_OK;
        case FB_DEBUG_LEARN_HASH_MASK:
            c->learn_hash_mask = value ? value : ~0ull;
            return FB_OK;
        case FB_DEBUG_WL_NAME_HASH_MASK:
            return wl_dom_set_mask(c, value ? value : ~0ull);
        case FB_DEBUG_DNS_LAUNCH:
            if (!c->dns) return set_err(FB_ERR_INVAL, "DNS tracking is not enabled (fb_dns_track_enable)");
            return dnstrack_set_launch(c->dns, value);
        default:
            return set_err(FB_ERR_INVAL, "unknown debug knob %u", knob);
    }
}

int fb_set_session_records(fb_ctx* c, int emit) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    c->emit_records = emit != 0;
    return FB_OK;
}

int fb_set_own_ips(fb_ctx* c, const fb_ip* ips, uint32_t n) {
    if (!c || n > FB_MAX_OWN_IPS || (n && !ips)) return set_err(FB_ERR_INVAL, "bad own-ip table");
    c->h_cfg->n_own = n;
    for (uint32_t i = 0; i < n; ++i) c->h_cfg->own[i] = ips[i];
    c->cfg_dirty = true;
    return FB_OK;
}

// Launch of the segmented streaming kernel over `sb` (frames, or the parsed packets `parsed`), on at most
// `grid_max` blocks.  `fp` non-empty: one frame batch whose session table update follows (the fused entry
// points, which order `s` after the updates still reading `fp`) -- the kernel also writes each SESSION record
// slot's table partition there, so the update's histogram pass reads 4 B per record instead of the record.
#ifdef FB_SEG_TRACE
static unsigned long long* g_strace = nullptr;
// diagnostic builds only: the last k_parse_seg launch's per-block trace (4 x 2048 words), after a sync
extern "C" __attribute__((visibility("default"))) int fb_seg_trace_last(unsigned long long* out) {
    if (!g_strace || hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpy(out, g_strace, 8u * 4u * 2048u, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
static int launch_seg(fb_ctx* c, const SegBatches& sb, uint32_t n_max, const fb_parsed_pkt* parsed, hipStream_t s,
                      FusedParts fp, uint32_t grid_max, SegPass pass = SegPass::kSegments,
                      fb_pkt_out* dense_out = nullptr, fb_dns_out* dense_dns = nullptr) {
    int rc = reset_launch_scratch(c, s);
    if (!rc) rc = upload_cfg(c, s);
    if (!rc) rc = ensure_flow_scratch(c, n_max, s);
    if (rc) return rc;
    c->last_n = n_max;
    ParseParams p;
    memset(&p, 0, sizeof(p));
    p.pre = c->sc.cpre;
    p.dense_out = dense_out;
    p.dense_dns = dense_dns;
    p.parsed = parsed;
    p.n = parsed ? sb.b[0].n : 0u;
    p.rec_part = fp.part;
    p.rec_ent = fp.ent;
    p.no_records = p.rec_part && !c->emit_records ? 1u : 0u;
    p.part_shift = c->tb.shift;
    p.cfg = c->d_cfg;
    p.tick = c->d_tick;
    if (pass != SegPass::kDenseOut) {
        rc = guard_next_error_word(c, s);
        if (rc) return rc;
    }
    // dense pass 2 belongs to pass 1's launch: same error word, no new parity
    const uint32_t launch = pass == SegPass::kDenseOut ? c->epoch : ++c->epoch;
    p.error = c->d_error + (launch & 3u);
    p.error_next = c->d_error + ((launch + 1u) & 3u);
    const uint32_t waves = parse_seg_block_threads() / 64u;
    const uint32_t grid = std::max<uint32_t>(1u, std::min<uint32_t>(grid_max, (sb.total_segs + waves - 1) / waves));
#ifdef FB_SEG_TRACE
    if (!g_strace && hipMalloc(&g_strace, 8u * 4u * 2048u) != hipSuccess) return set_err(FB_ERR_NOMEM, "trace");
    HIP_TRY(hipMemsetAsync(g_strace, 0, 8u * 4u * 2048u, s));
    p.dtrace = g_strace;
#endif
    HIP_TRY(launch_parse_seg(p, sb, grid, s, pass));
    return FB_OK;
}

static SegBatches one_batch(const uint8_t* frames, uint64_t frames_bytes, const uint32_t* offsets, uint32_t n,
                            fb_pkt_out* out, uint32_t* seg, uint8_t* cls, fb_batch_stats* stats) {
    SegBatches sb;
    memset(&sb, 0, sizeof(sb));
    sb.count = 1;
    SegBatch& B = sb.b[0];
    B.frames = frames;
    B.offsets = offsets;
    B.out = out;
    B.seg = seg;
    B.cls = cls;
    B.stats = stats;
    B.n = n;
    B.frames_bytes = (uint32_t)frames_bytes;
    sb.total_segs = (n + FB_SEG_FRAMES - 1) / FB_SEG_FRAMES;
    return sb;
}

int fb_parse_classify_seg_batches_dev(fb_ctx* c, const fb_seg_batch* batches, uint32_t count, void* stream) {
    if (!c || !batches || count == 0 || count > FB_MAX_SEG_BATCHES)
        return set_err(FB_ERR_INVAL, "ctx, batches and 1 <= count <= FB_MAX_SEG_BATCHES are required");
    SegBatches sb;
    memset(&sb, 0, sizeof(sb));
    uint64_t segs = 0;
    uint32_t n_max = 0;
    for (uint32_t k = 0; k < count; ++k) {
        const fb_seg_batch& x = batches[k];
        if (!x.d_stats) return set_err(FB_ERR_INVAL, "batch %u: d_stats is required", k);
        if (x.n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "batch %u: n > FB_MAX_BATCH_PACKETS", k);
        if (x.frames_bytes > 0xFFFFFFFFull) return set_err(FB_ERR_INVAL, "batch %u: frames_bytes must be < 4 GiB", k);
        if (!x.d_offsets || (x.n && (!x.d_out || !x.d_seg)))
            return set_err(FB_ERR_INVAL, "batch %u: d_offsets, d_out and d_seg are required", k);
        if (x.n && x.frames_bytes && !x.d_frames) return set_err(FB_ERR_INVAL, "batch %u: d_frames is NULL", k);
        SegBatch& B = sb.b[k];
        B.frames = x.d_frames;
        B.offsets = x.d_offsets;
        B.out = x.d_out;
        B.seg = x.d_seg;
        B.cls = x.d_class;
        B.stats = x.d_stats;
        B.n = x.n;
        B.frames_bytes = (uint32_t)x.frames_bytes;
        B.seg_start = (uint32_t)segs;
        segs += (x.n + FB_SEG_FRAMES - 1) / FB_SEG_FRAMES;
        n_max = std::max(n_max, x.n);
    }
    if (segs > 0xFFFFFFFFull / FB_SEG_FRAMES) return set_err(FB_ERR_INVAL, "too many frames in one launch");
    sb.count = count;
    sb.total_segs = (uint32_t)segs;
    DeviceGuard g(c->device);
    return launch_seg(c, sb, n_max, nullptr, (hipStream_t)stream, {}, c->seg_grid);
}

#ifdef FB_DN_TRACE
static unsigned long long* g_dtrace = nullptr;
// diagnostic builds only: the last dense launch's trace (4 x (8192 + 1024) words), after a device sync
extern "C" __attribute__((visibility("default"))) int fb_dense_trace_last(unsigned long long* out) {
    if (!g_dtrace || hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpy(out, g_dtrace, 8u * 4u * (8192u + 1024u), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
// ---- resident queue-fed parse (k_parse_seg_queue, fb_parse.hip) ------------------------------------
#ifdef FB_QUEUE_TRACE
static unsigned long long g_qtrace[kQTraceAll];
#endif
struct fb_seg_queue {
    int device = 0;
    uint32_t depth = 0;  // batches in flight at most
    uint32_t slots = 0;  // ring slots: depth rounded up to a power of two (the kernel masks)
    PinnedBuf<QueueHost> h;      // coherent, mapped host memory (the kernel's ring and completion words)
    DevBuf<QueueDev> d_ring;     // the device side of the ring
    DevBuf<DevConfig> d_cfg;     // the context's configuration when the queue was created
    DevBuf<unsigned long long> d_tick;
    DevBuf<uint32_t> d_blk;
    DevBuf<uint32_t> d_head;
    DevBuf<uint32_t> d_err;
    DevBuf<unsigned long long> d_trace;  // -DFB_QUEUE_TRACE builds
    DevStream stream;            // (declared after the buffers: destroyed before they are freed)
    uint64_t submitted = 0;
    uint64_t limit = FB_QUEUE_MAX_SUBMISSIONS;  // the kernel's batch numbers are 32-bit (k_parse_seg_queue)
    bool launched = false;
    hipError_t gone = hipSuccess;  // what the stream reported when the kernel was found gone
    uint32_t grid = 0;             // the kernel's blocks (all must be resident at once)
    uint64_t idle_ns = 0;          // idle_ms in ns
    std::chrono::steady_clock::time_point created;
    bool not_resident = false;     // its blocks were not all running idle_ms after create
    bool counted = false;          // holds its device's live-queue count
};
// One live queue per device: a second one's blocks could never all be resident beside the first's
// (two blocks per CU each), so its kernel would not start and nothing on the device could report it.
static std::mutex g_queue_mu;
static uint32_t g_queue_live[64];

static void queue_free(fb_seg_queue* q) {
    if (q->counted) {
        std::lock_guard<std::mutex> lk(g_queue_mu);
        --g_queue_live[q->device];
    }
    delete q;
}

static uint64_t hload(const unsigned long long* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }

// FB_OK once the kernel is gone or going (a block expired, or -- every `every` calls, a runtime call --
// the kernel has ended), 1 while it runs
static int queue_kernel_gone(fb_seg_queue* q, uint64_t spin, uint64_t every) {
    if (hload(&q->h->status) & kQueueExpired) return FB_OK;
    if (spin % every != every - 1u) return 1;
    const hipError_t e = hipStreamQuery(q->stream);
    if (e == hipErrorNotReady) {
        // every block counts itself into pad[3] when it starts; a kernel some of whose blocks never
        // ran (the CUs held by other work) cannot complete a batch, and its resident blocks are not
        // the ones waiting -- only the host can notice
        if (hload(&q->h->pad[3]) != q->grid &&
            (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() -
                                                                          q->created).count() > q->idle_ns) {
            q->not_resident = true;
            return FB_OK;
        }
        return 1;
    }
    q->gone = e;
    return FB_OK;
}

static int queue_gone_error(fb_seg_queue* q) {
    const QueueHost* h = q->h;
    if (q->not_resident)
        return set_err(FB_ERR_INTERNAL,
                       "the queue kernel's blocks are not all running (%llu of %u started within idle_ms): the "
                       "device's CUs are held by other work; destroy the queue",
                       (unsigned long long)hload(&h->pad[3]), q->grid);
    return set_err(FB_ERR_INTERNAL,
                   "the queue kernel has stopped (status %llu, stream: %s; a block left after %llu ticks idle "
                   "waiting for batch %llu (block %llu), tail %llu): destroy the queue",
                   (unsigned long long)hload(&h->status), hipGetErrorString(q->gone), (unsigned long long)hload(&h->pad[0]),
                   (unsigned long long)(hload(&h->pad[1]) & 0xFFFFFFFFu), (unsigned long long)(hload(&h->pad[1]) >> 32),
                   (unsigned long long)hload(&h->pad[2]));
}

fb_seg_queue* fb_seg_queue_create(fb_ctx* c, uint32_t depth, uint32_t idle_ms) {
    return fb_seg_queue_create_ex(c, depth, idle_ms, 0u);
}

fb_seg_queue* fb_seg_queue_create_ex(fb_ctx* c, uint32_t depth, uint32_t idle_ms, uint32_t flags) {
    if (flags & ~FB_QUEUE_SHARED) {
        set_err(FB_ERR_INVAL, "unknown queue flags 0x%x", flags);
        return nullptr;
    }
    if (!c) {
        set_err(FB_ERR_INVAL, "ctx is NULL");
        return nullptr;
    }
    if (depth == 0u) depth = 8u;
    if (depth > kQueueMax) {
        set_err(FB_ERR_INVAL, "depth %u > FB_QUEUE_MAX_DEPTH", depth);
        return nullptr;
    }
    DeviceGuard g(c->device);
    {
        std::lock_guard<std::mutex> lk(g_queue_mu);
        if (c->device < 0 || c->device >= 64) {
            set_err(FB_ERR_INVAL, "device %d", c->device);
            return nullptr;
        }
        if (g_queue_live[c->device]) {
            set_err(FB_ERR_INVAL, "device %d already runs a queue (one per device: destroy it first)", c->device);
            return nullptr;
        }
        ++g_queue_live[c->device];  // (released by queue_free, or below)
    }
    fb_seg_queue* q = new (std::nothrow) fb_seg_queue();
    if (!q) {
        std::lock_guard<std::mutex> lk(g_queue_mu);
        --g_queue_live[c->device];
        set_err(FB_ERR_NOMEM, "queue");
        return nullptr;
    }
    q->counted = true;
    q->device = c->device;
    q->depth = depth;
    q->slots = 1u;
    while (q->slots < depth) q->slots <<= 1;
    bool ok = q->h.alloc(1, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess;
    if (ok) memset(q->h.get(), 0, sizeof(QueueHost));
    ok = ok && q->d_cfg.alloc(1) == hipSuccess &&
         hipMemcpy(q->d_cfg, c->h_cfg.get(), sizeof(DevConfig), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && q->d_tick.alloc(kQueueMax * 8u) == hipSuccess && hipMemset(q->d_tick, 0, kQueueMax * 64u) == hipSuccess;
    ok = ok && q->d_blk.alloc(kQueueMax) == hipSuccess && hipMemset(q->d_blk, 0, kQueueMax * 4u) == hipSuccess;
    ok = ok && q->d_head.alloc(kQueueMax * kQueueHeadWords) == hipSuccess &&
         hipMemset(q->d_head, 0, kQueueMax * kQueueHeadWords * 4u) == hipSuccess;
    ok = ok && q->d_err.alloc(1) == hipSuccess && hipMemset(q->d_err, 0, 4) == hipSuccess;
    ok = ok && q->d_ring.alloc(1) == hipSuccess && hipMemset(q->d_ring, 0, sizeof(QueueDev)) == hipSuccess;
    ok = ok && q->stream.create() == hipSuccess;
#ifdef FB_QUEUE_TRACE
    if (ok) {
        std::vector<unsigned long long> t0((size_t)kQTraceAll, 0ull);
        std::fill(t0.begin() + kQtFirst * kQTraceN, t0.begin() + (kQtArr0 + 1) * kQTraceN, ~0ull);
        ok = q->d_trace.alloc(t0.size()) == hipSuccess &&
             hipMemcpy(q->d_trace, t0.data(), t0.size() * 8u, hipMemcpyHostToDevice) == hipSuccess;
    }
#endif
    if (!ok) {
        queue_free(q);
        set_err(FB_ERR_NOMEM, "queue resources");
        return nullptr;
    }
    QueueParams p;
    p.cfg = q->d_cfg;
    p.h = q->h.dev();
    p.d = q->d_ring;
    p.tick = q->d_tick;
    p.blk_done = q->d_blk;
    p.head = q->d_head;
    p.error = q->d_err;
    p.depth = q->slots;
    p.idle_ticks = (unsigned long long)(idle_ms ? idle_ms : 5000u) * 100000ull;  // s_memrealtime: 100 MHz
    p.trace = q->d_trace;
    // two blocks per CU, not k_parse_seg's three: the resident kernel must leave room on every CU for
    // the work the host issues while it runs -- blit kernels of pageable copies (a capture loop reads
    // its results back), other streams' kernels; at three blocks (80 VGPRs x 6 waves per SIMD) a D2H
    // copy into pageable memory waited until the queue's kernel had left (round-5 probe)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus < 1) cus = 1;
    // every block must be resident at once: a batch completes when every block has passed it
    int occ = 0;
    if (occupancy_parse_seg_queue(&occ) != hipSuccess || occ < 1) occ = 1;
    // FB_QUEUE_SHARED: one block per CU, so the session-table update kernels (K1 96 KB + K2 80 KB of
    // LDS, 80 / 128 VGPRs) fit beside it (two blocks leave ~66 KB of LDS)
    const int bpc = (flags & FB_QUEUE_SHARED) ? 1 : FB_QUEUE_BPC;
    uint32_t grid = std::min<uint32_t>(c->seg_grid, (uint32_t)(std::min(bpc, occ) * cus));
    // ... and on only a share of the CUs (the dispatcher spreads a small grid one block per CU): K2's
    // two 80-KB workgroups per CU need a CU's whole LDS, so every CU holding a queue block runs one.
    // C4-mix 1M-frame batches + the update beside them: CUs / 1, 2, 4, 8, 16, 32 -> 1.8, 2.6, 3.3,
    // 3.75, 2.3, 1.2 Gpps (past 8 the parse on too few CUs is the step; profiles/r06_shared_queue_div_sweep.txt)
    if (flags & FB_QUEUE_SHARED) grid = std::max<uint32_t>(1u, grid / FB_QUEUE_SHARED_DIV);
    q->grid = grid;
    q->idle_ns = (uint64_t)(idle_ms ? idle_ms : 5000u) * 1000000ull;
    q->created = std::chrono::steady_clock::now();
    if (launch_parse_seg_queue(p, grid, q->stream) != hipSuccess) {
        queue_free(q);
        set_err(FB_ERR_HIP, "queue kernel launch");
        return nullptr;
    }
    q->launched = true;
    return q;
}

int fb_seg_queue_submit(fb_seg_queue* q, const fb_seg_batch* x, uint64_t* ticket) {
    if (!q || !x) return set_err(FB_ERR_INVAL, "queue and batch are required");
    if (!x->d_stats) return set_err(FB_ERR_INVAL, "d_stats is required");
    if (x->n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "n > FB_MAX_BATCH_PACKETS");
    if (x->frames_bytes > 0xFFFFFFFFull) return set_err(FB_ERR_INVAL, "frames_bytes must be < 4 GiB");
    if (!x->d_offsets || (x->n && (!x->d_out || !x->d_seg))) return set_err(FB_ERR_INVAL, "d_offsets, d_out and d_seg are required");
    if (x->n && x->frames_bytes && !x->d_frames) return set_err(FB_ERR_INVAL, "d_frames is NULL");
    const uint64_t k = q->submitted, S = q->slots;
    // the kernel carries batch numbers, ring claims and completion words in 32 bits: past 2^32 a
    // claim's expected value and a slot's completion word would repeat an old batch's, so a queue
    // takes at most `limit` batches and is then recycled by the host
    if (k >= q->limit)
        return set_err(FB_ERR_INVAL, "the queue took its %llu batches (32-bit batch numbers): destroy it and create a "
                       "new one", (unsigned long long)q->limit);
    // at most `depth` batches in flight, and a slot is reused only once its previous batch (k - S) is
    // complete -- its completion word is stored after the kernel has reset the slot's state
    const uint64_t back[2] = {q->depth, S};
    for (const uint64_t b : back) {
        if (k < b) continue;  // (no such batch yet)
        const uint64_t prev = k - b;
        for (uint64_t spin = 0; hload(&q->h->cdone[prev & (S - 1u)]) != prev + 1u; ++spin) {
            if (queue_kernel_gone(q, spin, 4096u) == FB_OK && hload(&q->h->cdone[prev & (S - 1u)]) != prev + 1u)
                return queue_gone_error(q);
            __builtin_ia32_pause();
        }
    }
    QueueHost* h = q->h;
    memcpy((void*)&h->desc[k & (S - 1u)], x, sizeof(fb_seg_batch));
    __atomic_store_n(&h->tail, (unsigned long long)(k + 1u), __ATOMIC_RELEASE);  // after the descriptor
    q->submitted = k + 1u;
    if (ticket) *ticket = k;
    return FB_OK;
}

int fb_seg_queue_set_limit(fb_seg_queue* q, uint64_t limit) {
    if (!q) return set_err(FB_ERR_INVAL, "queue is NULL");
    if (limit > FB_QUEUE_MAX_SUBMISSIONS || limit < q->submitted)
        return set_err(FB_ERR_INVAL, "limit %llu outside [%llu, FB_QUEUE_MAX_SUBMISSIONS]", (unsigned long long)limit,
                       (unsigned long long)q->submitted);
    q->limit = limit;
    return FB_OK;
}

static int queue_poll(fb_seg_queue* q, uint64_t t, uint64_t spin, uint64_t every) {
    if (!q) return set_err(FB_ERR_INVAL, "queue is NULL");
    if (t >= q->submitted) return set_err(FB_ERR_INVAL, "ticket %llu was not issued", (unsigned long long)t);
    if (t + q->depth < q->submitted) return FB_OK;  // a later submission waited for it
    const uint64_t slot = t & (q->slots - 1u);
    if (hload(&q->h->cdone[slot]) == t + 1u) return FB_OK;
    if (queue_kernel_gone(q, spin, every) == FB_OK && hload(&q->h->cdone[slot]) != t + 1u)
        return queue_gone_error(q);
    return 1;
}

int fb_seg_queue_query(fb_seg_queue* q, uint64_t t) { return queue_poll(q, t, 0u, 1u); }

int fb_seg_queue_wait(fb_seg_queue* q, uint64_t t) {
    for (uint64_t spin = 0;; ++spin) {
        const int rc = queue_poll(q, t, spin, 4096u);
        if (rc != 1) return rc;
        __builtin_ia32_pause();
    }
}

int fb_seg_queue_destroy(fb_seg_queue* q) {
    if (!q) return set_err(FB_ERR_INVAL, "queue is NULL");
    DeviceGuard g(q->device);
    __atomic_store_n(&q->h->stop, 1ull, __ATOMIC_RELEASE);  // the kernel leaves once the submitted batches are done
    int rc = FB_OK;
    if (q->launched && hipStreamSynchronize(q->stream) != hipSuccess) rc = set_err(FB_ERR_HIP, "queue kernel");
#ifdef FB_QUEUE_TRACE
    if (q->d_trace) hipMemcpy(g_qtrace, q->d_trace, sizeof(g_qtrace), hipMemcpyDeviceToHost);
#endif
    queue_free(q);
    return rc;
}
#ifdef FB_QUEUE_TRACE
// diagnostic builds only: the last destroyed queue's trace (kQTraceAll words: QTrace order, then per block)
extern "C" __attribute__((visibility("default"))) int fb_seg_queue_trace_last(unsigned long long* out) {
    memcpy(out, g_qtrace, sizeof(g_qtrace));
    return (int)kQTraceAll;
}
#endif

static int parse_seg(fb_ctx* c, const uint8_t* d_frames, uint64_t frames_bytes, const uint32_t* d_offsets, uint32_t n,
                     fb_pkt_out* d_out, uint32_t* d_seg, uint8_t* d_class, fb_batch_stats* d_stats, void* stream,
                     FusedParts fp, uint32_t grid_max) {
    if (!c || !d_stats) return set_err(FB_ERR_INVAL, "ctx and d_stats are required");
    if (n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "n %u > FB_MAX_BATCH_PACKETS", n);
    if (frames_bytes > 0xFFFFFFFFull) return set_err(FB_ERR_INVAL, "frames_bytes must be < 4 GiB");
    if (n && (!d_offsets || !d_out || !d_seg)) return set_err(FB_ERR_INVAL, "d_offsets, d_out and d_seg are required");
    if (n && frames_bytes && !d_frames) return set_err(FB_ERR_INVAL, "d_frames is NULL");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(fb_batch_stats), s));
        return FB_OK;
    }
    return launch_seg(c, one_batch(d_frames, frames_bytes, d_offsets, n, d_out, d_seg, d_class, d_stats), n, nullptr,
                      s, fp, grid_max);
}

int fb_parse_classify_seg_dev(fb_ctx* c, const uint8_t* d_frames, uint64_t frames_bytes, const uint32_t* d_offsets,
                              uint32_t n, fb_pkt_out* d_out, uint32_t* d_seg, uint8_t* d_class,
                              fb_batch_stats* d_stats, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx and d_stats are required");
    return parse_seg(c, d_frames, frames_bytes, d_offsets, n, d_out, d_seg, d_class, d_stats, stream, {}, c->seg_grid);
}

int fb_process_parsed_seg_dev(fb_ctx* c, const fb_parsed_pkt* d_in, uint32_t n, fb_pkt_out* d_out, uint32_t* d_seg,
                              uint8_t* d_class, fb_batch_stats* d_stats, void* stream) {
    if (!c || !d_stats) return set_err(FB_ERR_INVAL, "ctx and d_stats are required");
    if (n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "n %u > FB_MAX_BATCH_PACKETS", n);
    if (n && (!d_in || !d_out || !d_seg)) return set_err(FB_ERR_INVAL, "d_in, d_out and d_seg are required");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(fb_batch_stats), s));
        return FB_OK;
    }
    return launch_seg(c, one_batch(nullptr, 0, nullptr, n, d_out, d_seg, d_class, d_stats), n, d_in, s, {}, c->seg_grid);
}

int fb_seg_compact_dev(fb_ctx* c, const fb_pkt_out* d_seg_out, const uint32_t* d_seg, uint32_t n, fb_pkt_out* d_out,
                       fb_dns_out* d_dns, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "n %u > FB_MAX_BATCH_PACKETS", n);
    if (n && (!d_seg_out || !d_seg)) return set_err(FB_ERR_INVAL, "d_seg_out and d_seg are required");
    if (n == 0 || (!d_out && !d_dns)) return FB_OK;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_compact_scratch(c, n, s);
    if (rc) return rc;
    SegScanScratch sc;
    rc = scan_scratch(c, s, sc);
    if (rc) return rc;
    HIP_TRY(launch_seg_compact(d_seg_out, d_seg, (n + FB_SEG_FRAMES - 1) / FB_SEG_FRAMES, c->sc.cpre, sc, d_out, d_dns,
                               s));
    return FB_OK;
}

// Dense output in two passes of the segmented kernel (fb_compact.hip): pass 1 counts every 64-frame
// segment (classes and batch stats too), the scan turns the counts into batch-wide offsets, pass 2
// parses again and stores each record at its offset -- at C2 the frames are still in the Infinity
// Cache for pass 2.  No kernel of the path waits on another workgroup.
// Frame batches take the single-pass kernel (k_parse_dense: tiles ordered by ticket, decoupled
// look-back, records kept in registers until the tile's offset is known); parsed-packet batches
// (and FB_DENSE_TWO_PASS builds, for A/B timing) the two passes below.
static int parse_dense_single(fb_ctx* c, const uint8_t* d_frames, uint64_t frames_bytes, const uint32_t* d_offsets,
                              uint32_t n, fb_pkt_out* d_out, fb_dns_out* d_dns, uint8_t* d_class,
                              fb_batch_stats* d_stats, hipStream_t s) {
    int rc = reset_launch_scratch(c, s);
    if (!rc) rc = upload_cfg(c, s);
    if (!rc) rc = ensure_flow_scratch(c, n, s);
    if (!rc) rc = ensure_compact_scratch(c, n, s);
    if (rc) return rc;
    const uint32_t nseg = (n + FB_SEG_FRAMES - 1) / FB_SEG_FRAMES;
    if (c->sc.dense_epoch == 0u || c->sc.dense_epoch >= 255u) {
        HIP_TRY(hipMemsetAsync(c->sc.dstatus, 0, dense_status_words(c->sc.cap) * 8ull, s));
        c->sc.dense_epoch = 0u;
    }
    c->last_n = n;
    ParseParams p;
    memset(&p, 0, sizeof(p));
    p.cfg = c->d_cfg;
    p.tick = c->d_tick;
    rc = guard_next_error_word(c, s);
    if (rc) return rc;
    const uint32_t launch = ++c->epoch;
    p.error = c->d_error + (launch & 3u);
    p.error_next = c->d_error + ((launch + 1u) & 3u);
    p.dense_out = d_out;
    p.dense_dns = d_dns;
    p.dstatus = c->sc.dstatus;
    p.steal_polls = c->steal_polls;
    p.dn_skew = c->dn_skew;
#ifdef FB_DN_TRACE
    if (!g_dtrace) {
        if (hipMalloc(&g_dtrace, 8u * 4u * (8192u + 1024u)) != hipSuccess) return set_err(FB_ERR_NOMEM, "trace");
    }
    HIP_TRY(hipMemsetAsync(g_dtrace, 0, 8u * 4u * (8192u + 1024u), s));
    p.dtrace = g_dtrace;
#endif
    p.dep = ++c->sc.dense_epoch;
    p.ntiles = (nseg + parse_dense_tile_segs() - 1) / parse_dense_tile_segs();
    const uint32_t grid = std::max<uint32_t>(1u, std::min<uint32_t>(c->dense_grid, p.ntiles));
    SegBatch b;
    memset(&b, 0, sizeof(b));
    b.frames = d_frames;
    b.offsets = d_offsets;
    b.cls = d_class;
    b.stats = d_stats;
    b.n = n;
    b.frames_bytes = (uint32_t)frames_bytes;
    HIP_TRY(launch_parse_dense(p, b, grid, s));
    return FB_OK;
}

static int parse_dense(fb_ctx* c, const uint8_t* d_frames, uint64_t frames_bytes, const uint32_t* d_offsets,
                       const fb_parsed_pkt* d_in, uint32_t n, fb_pkt_out* d_out, fb_dns_out* d_dns, uint8_t* d_class,
                       fb_batch_stats* d_stats, hipStream_t s) {
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(fb_batch_stats), s));
        return FB_OK;
    }
#ifndef FB_DENSE_TWO_PASS
    if (!d_in) return parse_dense_single(c, d_frames, frames_bytes, d_offsets, n, d_out, d_dns, d_class, d_stats, s);
#endif
    int rc = ensure_compact_scratch(c, n, s);
    if (rc) return rc;
    rc = launch_seg(c, one_batch(d_frames, frames_bytes, d_offsets, n, nullptr, c->sc.cseg, d_class, d_stats), n, d_in,
                    s, {}, c->seg_grid, SegPass::kCount);
    if (rc || (!d_out && !d_dns)) return rc;
    const uint32_t nseg = (n + FB_SEG_FRAMES - 1) / FB_SEG_FRAMES;
    SegScanScratch sc;
    rc = scan_scratch(c, s, sc);
    if (rc) return rc;
    HIP_TRY(launch_seg_scan(c->sc.cseg, nseg, c->sc.cpre, sc, s));
    return launch_seg(c, one_batch(d_frames, frames_bytes, d_offsets, n, nullptr, nullptr, nullptr, nullptr), n, d_in, s,
                      {}, c->seg_grid, SegPass::kDenseOut, d_out, d_dns);
}

int fb_parse_classify_dev(fb_ctx* c, const uint8_t* d_frames, uint64_t frames_bytes,
                          const uint32_t* d_offsets, uint32_t n, fb_pkt_out* d_out, fb_dns_out* d_dns,
                          uint8_t* d_class, fb_batch_stats* d_stats, void* stream) {
    if (!c || !d_stats) return set_err(FB_ERR_INVAL, "ctx and d_stats are required");
    if (n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "n %u > FB_MAX_BATCH_PACKETS", n);
    if (frames_bytes > 0xFFFFFFFFull) return set_err(FB_ERR_INVAL, "frames_bytes must be < 4 GiB");
    if (n && !d_offsets) return set_err(FB_ERR_INVAL, "d_offsets is NULL");
    if (n && frames_bytes && !d_frames) return set_err(FB_ERR_INVAL, "d_frames is NULL");
    DeviceGuard g(c->device);
    return parse_dense(c, d_frames, frames_bytes, d_offsets, nullptr, n, d_out, d_dns, d_class, d_stats,
                       (hipStream_t)stream);
}

int fb_process_parsed_dev(fb_ctx* c, const fb_parsed_pkt* d_in, uint32_t n, fb_pkt_out* d_out,
                          uint8_t* d_class, fb_batch_stats* d_stats, void* stream) {
    if (!c || !d_stats) return set_err(FB_ERR_INVAL, "ctx and d_stats are required");
    if (n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "n %u > FB_MAX_BATCH_PACKETS", n);
    if (n && !d_in) return set_err(FB_ERR_INVAL, "d_in is NULL");
    DeviceGuard g(c->device);
    return parse_dense(c, nullptr, 0, nullptr, d_in, n, d_out, nullptr, d_class, d_stats, (hipStream_t)stream);
}

static int ensure_staging(fb_ctx* c, uint64_t n, uint64_t bytes) {
    Staging& st = c->st;
    if (bytes > st.frames.size() && st.frames.alloc(std::max<uint64_t>(bytes, 1 << 20)) != hipSuccess)
        return set_err(FB_ERR_NOMEM, "staging frames");
    if (n > st.pk.cls.size()) {
        const uint64_t want = std::max<uint64_t>(n, 4096);
        const hipError_t e = alloc_group(st.pk, [&](Staging::Pkts& p) {
            return alloc_each(p.offsets, want + 1, p.out, want, p.dns, want, p.cls, want);
        });
        if (e != hipSuccess) return set_err(FB_ERR_NOMEM, "staging packets");
    }
    if (!st.stats && st.stats.alloc(1) != hipSuccess) return set_err(FB_ERR_NOMEM, "staging stats");
    return FB_OK;
}

static int check_error_word(fb_ctx* c, hipStream_t s) {
    uint32_t e = 0;
    HIP_TRY(hipMemcpyAsync(&e, c->d_error + (c->epoch & 3u), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (e) return ctx_report_error(c, e);
    return FB_OK;
}

int fb_parse_classify(fb_ctx* c, const uint8_t* frames, uint64_t frames_bytes, const uint32_t* offsets,
                      uint32_t n, fb_pkt_out* out, uint32_t* n_out, fb_dns_out* dns, uint32_t* n_dns,
                      uint8_t* cls, fb_batch_stats* stats, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "n too large");
    if (frames_bytes > 0xFFFFFFFFull) return set_err(FB_ERR_INVAL, "frames_bytes must be < 4 GiB");
    if ((n && !offsets) || (frames_bytes && !frames)) return set_err(FB_ERR_INVAL, "NULL input");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_staging(c, n, frames_bytes);
    if (rc) return rc;
    if (frames_bytes) HIP_TRY(hipMemcpyAsync(c->st.frames, frames, frames_bytes, hipMemcpyHostToDevice, s));
    if (n) HIP_TRY(hipMemcpyAsync(c->st.pk.offsets, offsets, (uint64_t)(n + 1) * 4, hipMemcpyHostToDevice, s));
    rc = fb_parse_classify_dev(c, c->st.frames, frames_bytes, c->st.pk.offsets, n, out ? c->st.pk.out.get() : nullptr,
                               dns ? c->st.pk.dns.get() : nullptr, cls ? c->st.pk.cls.get() : nullptr, c->st.stats, s);
    if (rc) return rc;
    fb_batch_stats st;
    HIP_TRY(hipMemcpyAsync(&st, c->st.stats, sizeof(st), hipMemcpyDeviceToHost, s));
    rc = check_error_word(c, s);  // synchronises the stream
    if (rc) return rc;
    if (out && st.n_session)
        HIP_TRY(hipMemcpyAsync(out, c->st.pk.out, st.n_session * sizeof(fb_pkt_out), hipMemcpyDeviceToHost, s));
    if (dns && st.n_dns)
        HIP_TRY(hipMemcpyAsync(dns, c->st.pk.dns, st.n_dns * sizeof(fb_dns_out), hipMemcpyDeviceToHost, s));
    if (cls && n) HIP_TRY(hipMemcpyAsync(cls, c->st.pk.cls, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n_out) *n_out = (uint32_t)st.n_session;
    if (n_dns) *n_dns = (uint32_t)st.n_dns;
    if (stats) *stats = st;
    return FB_OK;
}

// An update call without records still counts as one (the high word of flow positions).
static int empty_update(fb_ctx* c) {
    ++c->flow_batch;
    c->last.invalidate();
    return FB_OK;
}

// ---- table growth -------------------------------------------------------------------------------
// Doubles the table on the device: every slot re-inserted into 2x partitions (k_flow_grow), the old
// -> new slot map kept for fb_flow_slot_remap.  Drains the updates in flight first: growth is rare.
// The grown table is a second FlowTable, and the slot map a buffer of its own, until the growth is
// complete; only then are they swapped with the context's, which leave with this scope -- a failed growth
// leaves the context as it was.
static int grow_table(fb_ctx* c, hipStream_t s, uint32_t k) {
    int rc = drain_updates(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    FlowTable nw;
    DevBuf<uint32_t> remap;
    if (const char* what = table_alloc(nw, c->tb.cap << k, &c->tb)) return set_err(FB_ERR_NOMEM, "grown %s", what);
    if (remap.alloc(c->tb.cap) != hipSuccess) return set_err(FB_ERR_NOMEM, "slot remap");
    HIP_TRY(hipMemsetAsync(nw.slots, 0, nw.cap * sizeof(FlowSlot), s));
    HIP_TRY(launch_flow_grow(c->tb.slots, c->tb.parts, k, nw.shift, nw.slots, remap, c->tb.char_call, nw.char_call, s));
    for (uint32_t p = 0; p < kPlanes; ++p)  // every plane made so far follows its flows' new slots
        if (c->tb.plane[p]) HIP_TRY(plane_move(c, (PlaneId)p, remap, nw.cap, s, nw.plane[p]));
    HIP_TRY(hipStreamSynchronize(s));
    std::swap(c->tb, nw);
    c->d_remap.swap(remap);
    c->grown_seq = c->upd_seq;
    ++c->generation;
    // scratch sized by the partition count (K1 rows / K2 columns), history sort bits: rebuilt
    const uint64_t recs = c->flow_recs;
    const bool had_set1 = c->us[1].entries != nullptr;
    for (UpdScratch& u : c->us) u = UpdScratch();
    c->flow_recs = 0;
    rc = ensure_flow_scratch(c, recs, s);
    if (!rc && had_set1) rc = alloc_upd_scratch(c, c->us[1], s);
    c->last.invalidate();  // the last update's slots moved: its history is no longer available
    return rc;
}

// Before an update call: grow while the occupancy the last completed update reported, plus the new
// flows of the updates still in flight (each estimated at the last reported update's count) and of
// this one (twice that: arrival rates rise), spread over the partitions, plus slack for the spread
// between partitions, would pass 7/8 of a partition, or the flows 3/4 of the table.  The report sits
// in host-mapped memory; the decision needs the report of the update two calls back (the second call
// after a create / clear: the first update's), so a host that enqueues asynchronous batches faster
// than the device runs them waits here for that report (the device keeps the previous batch's work)
// instead of projecting from an older one -- or from none, which let the table fill.  A burst
// beyond the estimate inside one batch can still fill a partition: the update then reports error
// bit 4 (FB_ERR_TABLE_FULL).
static constexpr uint64_t kGrowPart = kFlowSlots * 7u / 8u;
static constexpr double kMailboxWaitS = 120.0;
static int maybe_grow(fb_ctx* c, hipStream_t s) {
    if (!c->tb.slots || !c->grow) return FB_OK;
    const volatile FlowMailbox* m = c->mbox;
    const uint64_t issued = c->upd_seq - c->clear_seq;              // updates since create / clear
    const uint64_t need = c->clear_seq + (issued >= 2u ? issued - 1u : issued);
    uint64_t seq = __atomic_load_n(&m->seq, __ATOMIC_ACQUIRE);
    if (seq < need) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spin = 0; (seq = __atomic_load_n(&m->seq, __ATOMIC_ACQUIRE)) < need; ++spin) {
            if (spin > 64u) std::this_thread::yield();
            if ((spin & 1023u) == 0u &&
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > kMailboxWaitS)
                return set_err(FB_ERR_HIP, "no table-occupancy report from update %llu after %.0f s",
                               (unsigned long long)need, kMailboxWaitS);
        }
    }
    if (seq == 0 || seq <= c->clear_seq) return FB_OK;
    const uint64_t flows = m->flows, newf = m->new_flows;
    const uint64_t ahead = c->upd_seq - seq + 2u;  // in flight, plus this call counted twice
    // the smallest k (table x 2^k) that holds the projection: one growth (one slot remap) per call
    uint32_t k = 0;
    for (;; ++k) {
        const uint64_t parts = (uint64_t)c->tb.parts << k;
        if ((c->tb.cap << k) > kFlowMaxCapacity || k > 5u) {
            if (k > 0) --k;
            break;
        }
        // a report from before a growth describes other partitions: only its flow count is used there
        const uint64_t maxp = (k == 0 && seq > c->grown_seq) ? m->max_part : flows / parts + 3u * kFlowSlots / 16u;
        const uint64_t add = (ahead * newf + parts - 1u) / parts;
        if (maxp + add + kFlowSlots / 32u <= kGrowPart && flows + ahead * newf <= (c->tb.cap << k) * 3u / 4u) break;
    }
    return k ? grow_table(c, s, k) : FB_OK;
}

// One table update.  `split` (the pipelined call): the bucketing kernels (K1, K1c) run on `s_bucket`
// -- the caller's stream (possibly the null stream), right after the parse that wrote the batch's
// partitions, into update scratch set `set` -- and the rest (K1t, K2, the stats fold) on `s` after
// an event; otherwise everything runs on `s` with set 0.  `ts`: the frame times the entry point took.
// `fp`: what this batch's fused parse wrote -- the entry point grew the table and sized the scratch
// (for seg_slots(n), which rounds to the same chunks as the parse's n) before it, so neither changes here.
static int flow_update(fb_ctx* c, const fb_pkt_out* d_recs, const uint32_t* d_seg, uint32_t n_slots,
                       fb_batch_stats* d_stats, hipStream_t s, const unsigned long long* ts, FusedParts fp = {},
                       bool split = false, hipStream_t s_bucket = nullptr, uint32_t set = 0) {
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    DeviceGuard g(c->device);
    if (!split) s_bucket = s;
    static_assert(kFlowChunk % FB_SEG_FRAMES == 0, "a chunk is whole segments");
    if (fp.part && n_slots > c->flow_recs) return set_err(FB_ERR_INTERNAL, "fused update without scratch for its batch");
    int rc = split ? FB_OK : join_updates(c, s);
    if (!rc && !split && !fp.part) rc = maybe_grow(c, s);
    if (!rc) rc = ensure_flow_scratch(c, n_slots, s_bucket);
    if (!rc && set == 1u && !c->us[1].entries) rc = alloc_upd_scratch(c, c->us[1], s_bucket);
    if (rc) return rc;
    if (c->hist_pending) {  // the last history's reads of the shared update scratch come first
        HIP_TRY(hipStreamWaitEvent(s_bucket, c->ev_hist, 0));
        if (s != s_bucket) HIP_TRY(hipStreamWaitEvent(s, c->ev_hist, 0));
        c->hist_pending = false;
    }
    const UpdScratch& u = c->us[set];
    // record slots of the batch: at most last_n records (dense) / n_slots slots (segmented)
    const uint32_t chunks = (uint32_t)std::max<uint64_t>(1, ((uint64_t)n_slots + kFlowChunk - 1) / kFlowChunk);
    FlowParams p;
    p.recs = d_recs;
    p.seg = d_seg;
    p.n_slots = n_slots;
    p.stats = d_stats;
    p.table = c->tb.slots;
    p.entries = u.entries;
    p.comb = u.comb;
    p.comb_cap = c->comb_cap;
    p.rows = u.rows;
    p.cols = u.cols;
    p.partials = c->tb.partials;
    p.error = c->d_error + (c->epoch & 3u);
    p.max_recs = (uint32_t)std::min<uint64_t>((uint64_t)chunks * kFlowChunk, c->flow_recs);
    p.parts = c->tb.parts;
    p.part_shift = c->tb.shift;
    p.chunk_stride = (uint32_t)(c->flow_recs / kFlowChunk);
    p.batch = c->flow_batch;
    p.rows_h = u.rows_h;
    p.e_orig = u.e_orig;
    p.e_sort = u.e_sort;
    p.hcount = c->tb.hcount;
    p.part_base = c->tb.part_base;
    p.hword = c->rs.hword;
    p.hot = u.hot;
    p.ctl = u.ctl;
#ifndef FB_K2_ORDER
#define FB_K2_ORDER 1
#endif
    p.order = FB_K2_ORDER ? u.order.get() : nullptr;
    p.agg_slot = c->rs.agg_slot;
    p.hot_cap = (uint32_t)(c->flow_recs / 16 + 16);
    p.rec_part = fp.part;
    p.ent = fp.ent;
    p.char_call = c->tb.char_call;
    const uint32_t slots = std::min(p.max_recs, n_slots);
    if (c->timed) {  // the capture-time pass's scratch (K2 writes its sort input into it)
        uint32_t bits = 0;
        while ((1ull << bits) < c->tb.cap) ++bits;
        const uint64_t need = time_scratch_bytes(slots, bits);
        rc = c->tscratch.acquire(need, s, "capture-time scratch");
        if (rc) return rc;
        p.tkv = time_key_array(c->tscratch.get());
        HIP_TRY(launch_time_prepare(c->tscratch.get(), slots, s));
        p.hot = nullptr;  // no combined entries: every record is a plain entry K2 places
    }
    HIP_TRY(launch_flow_bucket(p, chunks, s_bucket));
    if (split) {
        // (K1t stays on the update stream: beside the next batch's parse it takes ~95 us instead of
        // 10, but on the parse stream it delays that parse instead -- C4 12.85 vs 12.57 Gpps)
        HIP_TRY(hipEventRecord(c->ev_parsed, s_bucket));
        HIP_TRY(hipStreamWaitEvent(s, c->ev_parsed, 0));
    }
    HIP_TRY(launch_flow_apply(p, chunks, s));
    HIP_TRY(launch_flow_finish(d_stats, c->tb.partials, c->tb.parts, c->d_error + (c->epoch & 3u), c->mbox.dev(),
                               ++c->upd_seq, s));
    if (c->timed) {  // the capture-time pass over the placed records (fb_time.hip)
        HIP_TRY(launch_time_update(p, slots, c->tb.cap, c->plane<FlowTime>(kPlaneTime), ts, c->tscratch.get(), s));
        rc = c->tscratch.release(s);
        if (rc) return rc;
    }
    ++c->flow_batch;
    if (c->hs) ++c->hs_updates;
    c->last.p = p;
    c->last.slots = slots;
    c->last.chunks = chunks;
    c->last.valid = true;
    return FB_OK;
}

int fb_flow_update_dev(fb_ctx* c, const fb_pkt_out* d_recs, fb_batch_stats* d_stats, void* stream) {
    if (!c || !d_recs || !d_stats) return set_err(FB_ERR_INVAL, "ctx, d_recs and d_stats are required");
    const unsigned long long* ts = nullptr;
    if (int rc = take_frame_times(c, &ts)) return rc;
    return flow_update(c, d_recs, nullptr, c->last_n, d_stats, (hipStream_t)stream, ts);
}

int fb_flow_update_records_dev(fb_ctx* c, const fb_pkt_out* d_recs, uint32_t max_n, fb_batch_stats* d_stats,
                               void* stream) {
    if (!c || !d_stats || (max_n && !d_recs)) return set_err(FB_ERR_INVAL, "ctx, d_recs and d_stats are required");
    if (max_n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "max_n %u > FB_MAX_BATCH_PACKETS", max_n);
    const unsigned long long* ts = nullptr;
    if (int rc = take_frame_times(c, &ts)) return rc;
    if (max_n == 0) return empty_update(c);
    return flow_update(c, d_recs, nullptr, max_n, d_stats, (hipStream_t)stream, ts);
}

int fb_flow_update_seg_dev(fb_ctx* c, const fb_pkt_out* d_out, const uint32_t* d_seg, uint32_t n,
                           fb_batch_stats* d_stats, void* stream) {
    if (!c || !d_out || !d_seg || !d_stats) return set_err(FB_ERR_INVAL, "ctx, d_out, d_seg and d_stats are required");
    if (n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "n %u > FB_MAX_BATCH_PACKETS", n);
    const unsigned long long* ts = nullptr;
    if (int rc = take_frame_times(c, &ts)) return rc;
    if (n == 0) return empty_update(c);
    return flow_update(c, d_out, d_seg, seg_slots(n), d_stats, (hipStream_t)stream, ts);
}

int fb_process_seg_dev(fb_ctx* c, const uint8_t* d_frames, uint64_t frames_bytes, const uint32_t* d_offsets,
                       uint32_t n, fb_pkt_out* d_out, uint32_t* d_seg, uint8_t* d_class, fb_batch_stats* d_stats,
                       void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if (n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "n %u > FB_MAX_BATCH_PACKETS", n);
    const unsigned long long* ts = nullptr;
    int rc = take_frame_times(c, &ts);
    if (rc) return rc;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    rc = maybe_grow(c, s);  // before the parse writes partitions of this geometry
    if (!rc) rc = ensure_flow_scratch(c, seg_slots(n), s);  // ... and before the buffers it writes are picked
    // the parse rewrites them, and a pipelined update may still read them (an empty batch has no parse)
    if (!rc && n) rc = join_updates(c, s);
    const FusedParts fp{c->rs.rec_part.get(), c->rs.rec_ent.get()};
    if (!rc) rc = parse_seg(c, d_frames, frames_bytes, d_offsets, n, d_out, d_seg, d_class, d_stats, stream, fp, c->seg_grid);
    if (rc == FB_OK && c->stage_event) rc = hipEventRecord(c->stage_event, s) == hipSuccess
                                                ? FB_OK : set_err(FB_ERR_HIP, "stage event record failed");
    if (rc == FB_OK) rc = n == 0 ? empty_update(c) : flow_update(c, d_out, d_seg, seg_slots(n), d_stats, s, ts, fp);
    return rc;
}

// Pipelined fb_process_seg_dev: the parse of batch k runs on `stream`, its table update on the
// context's update stream after it, and `stream` waits only for the update of batch k-2 (which
// read the partition buffer and the records this call's slot reuses) -- so the parse of one batch
// overlaps the update of the one before.  Async batch k writes partition buffer k & 1.
int fb_process_seg_async_dev(fb_ctx* c, const uint8_t* d_frames, uint64_t frames_bytes, const uint32_t* d_offsets,
                             uint32_t n, fb_pkt_out* d_out, uint32_t* d_seg, uint8_t* d_class,
                             fb_batch_stats* d_stats, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if (n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "n %u > FB_MAX_BATCH_PACKETS", n);
    const unsigned long long* ts = nullptr;
    if (int rc = take_frame_times(c, &ts)) return rc;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (!c->upd && (c->upd.create() != hipSuccess || c->ev_parsed.create() != hipSuccess ||
                    c->ev_upd[0].create() != hipSuccess || c->ev_upd[1].create() != hipSuccess))
        return set_err(FB_ERR_HIP, "update stream / events");
    const uint32_t slot = (uint32_t)(c->async_k & 1u);
    int rc = maybe_grow(c, s);  // before this batch's parse writes partitions (drains the pipeline if it grows)
    if (!rc) rc = ensure_flow_scratch(c, seg_slots(n), s);
    if (rc) return rc;
    if (!c->rs.rec_part2 && c->rs.rec_part2.alloc(c->flow_recs) != hipSuccess)
        return set_err(FB_ERR_NOMEM, "second partition buffer");
    if (!c->rs.rec_ent2 && c->rs.rec_ent2.alloc(c->flow_recs * kUpdEntU4) != hipSuccess)
        return set_err(FB_ERR_NOMEM, "second update-entry buffer");
    // the same slot's previous batch (k-2): its update must be done before this parse rewrites the
    // slot's partition buffer; before any async batch, the last synchronous update is on `s` already
    if (c->async_k >= 2) HIP_TRY(hipStreamWaitEvent(s, c->ev_upd[slot], 0));
    // a batch that reuses the previous batch's records, counts or stats buffer waits for its
    // update too (no overlap: rotate two buffer sets to get it)
    if (c->async_k >= 1 && (d_out == c->async_prev[0] || d_seg == c->async_prev[1] || d_stats == c->async_prev[2]))
        HIP_TRY(hipStreamWaitEvent(s, c->ev_upd[slot ^ 1u], 0));
    const FusedParts fp = slot ? FusedParts{c->rs.rec_part2.get(), c->rs.rec_ent2.get()}
                               : FusedParts{c->rs.rec_part.get(), c->rs.rec_ent.get()};
    rc = parse_seg(c, d_frames, frames_bytes, d_offsets, n, d_out, d_seg, d_class, d_stats, stream, fp, c->seg_grid_async);
    if (rc == FB_OK && c->stage_event) rc = hipEventRecord(c->stage_event, s) == hipSuccess
                                                ? FB_OK : set_err(FB_ERR_HIP, "stage event record failed");
    if (rc) return rc;
    // the bucketing kernels follow the parse on `stream` (into scratch set k & 1, which update k-2
    // -- waited for above -- was the last to read); the update stream takes over after them
    rc = n == 0 ? empty_update(c) : flow_update(c, d_out, d_seg, seg_slots(n), d_stats, c->upd, ts, fp, true, s, slot);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev_upd[slot], c->upd));
    c->upd_word[slot] = c->epoch & 3u;  // the word flow_update handed this update
    c->async_prev[0] = d_out;
    c->async_prev[1] = d_seg;
    c->async_prev[2] = d_stats;
    ++c->async_k;
    return FB_OK;
}

int fb_flow_join(fb_ctx* c, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    DeviceGuard g(c->device);
    return join_updates(c, (hipStream_t)stream);
}

int fb_process_dev(fb_ctx* c, const uint8_t* d_frames, uint64_t frames_bytes, const uint32_t* d_offsets,
                   uint32_t n, fb_pkt_out* d_out, fb_dns_out* d_dns, uint8_t* d_class,
                   fb_batch_stats* d_stats, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if (!d_out) return set_err(FB_ERR_INVAL, "d_out is required");
    const unsigned long long* ts = nullptr;
    if (int rc = take_frame_times(c, &ts)) return rc;
    int rc = fb_parse_classify_dev(c, d_frames, frames_bytes, d_offsets, n, d_out, d_dns, d_class, d_stats, stream);
    if (rc) return rc;
    if (c->stage_event) HIP_TRY(hipEventRecord(c->stage_event, (hipStream_t)stream));
    if (n == 0) return empty_update(c);
    return flow_update(c, d_out, nullptr, c->last_n, d_stats, (hipStream_t)stream, ts);
}

int fb_process_parsed(fb_ctx* c, const fb_parsed_pkt* in, uint32_t n, fb_pkt_out* out, uint32_t* n_out,
                      uint8_t* cls, fb_batch_stats* stats, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "n too large");
    if (n && !in) return set_err(FB_ERR_INVAL, "NULL input");
    const unsigned long long* ts = nullptr;
    int rc = c->tb.slots ? take_frame_times(c, &ts) : FB_OK;
    if (rc) return rc;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_staging(c, n, (uint64_t)n * sizeof(fb_parsed_pkt));
    if (rc) return rc;
    const fb_parsed_pkt* d_in = reinterpret_cast<const fb_parsed_pkt*>(c->st.frames.get());
    if (n) HIP_TRY(hipMemcpyAsync(c->st.frames, in, (uint64_t)n * sizeof(fb_parsed_pkt), hipMemcpyHostToDevice, s));
    rc = fb_process_parsed_dev(c, d_in, n, c->st.pk.out, cls ? c->st.pk.cls.get() : nullptr, c->st.stats, s);
    if (rc) return rc;
    if (n && c->tb.slots) {
        rc = flow_update(c, c->st.pk.out, nullptr, c->last_n, c->st.stats, s, ts);
        if (rc) return rc;
    } else if (c->tb.slots) {
        empty_update(c);
    }
    fb_batch_stats st;
    HIP_TRY(hipMemcpyAsync(&st, c->st.stats, sizeof(st), hipMemcpyDeviceToHost, s));
    rc = check_error_word(c, s);  // synchronises the stream
    if (rc) return rc;
    if (out && st.n_session)
        HIP_TRY(hipMemcpyAsync(out, c->st.pk.out, st.n_session * sizeof(fb_pkt_out), hipMemcpyDeviceToHost, s));
    if (cls && n) HIP_TRY(hipMemcpyAsync(cls, c->st.pk.cls, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n_out) *n_out = (uint32_t)st.n_session;
    if (stats) *stats = st;
    return FB_OK;
}

int fb_flow_history_dev(fb_ctx* c, uint8_t* d_hist, uint32_t* d_hist_slot, uint32_t* d_n_hist, void* stream) {
    if (!c || !d_n_hist) return set_err(FB_ERR_INVAL, "ctx and d_n_hist are required");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    int jr = join_updates(c, s);
    if (jr) return jr;
    if (c->last.live_slots() == 0) {
        HIP_TRY(hipMemsetAsync(d_n_hist, 0, 4, s));
        return FB_OK;
    }
    if (!d_hist || !d_hist_slot) return set_err(FB_ERR_INVAL, "d_hist and d_hist_slot are required");
    return last_history(c, d_hist_slot, d_hist, d_n_hist, s, [] { return FB_OK; });
}

// ---- enrichment ----------------------------------------------------------------------------
static bool asn_less(const fb_asn_range& a, const fb_asn_range& b, bool v6) {
    const int nw = v6 ? 4 : 1;
    for (int k = 0; k < nw; ++k)
        if (a.start[k] != b.start[k]) return a.start[k] < b.start[k];
    for (int k = 0; k < nw; ++k)
        if (a.end[k] != b.end[k]) return a.end[k] < b.end[k];
    return false;
}

static bool asn_valid(const fb_asn_range& a, bool v6) {  // start <= end (src/asn_db.rs:111-128)
    const int nw = v6 ? 4 : 1;
    for (int k = 0; k < nw; ++k)
        if (a.start[k] != a.end[k]) return a.start[k] < a.end[k];
    return true;
}

int fb_set_asn_tables(fb_ctx* c, const fb_asn_range* v4, uint32_t n4, const fb_asn_range* v6, uint32_t n6) {
    if (!c || (n4 && !v4) || (n6 && !v6)) return set_err(FB_ERR_INVAL, "bad arguments");
    DeviceGuard g(c->device);
    HIP_TRY(hipDeviceSynchronize());  // no launch may still read the old tables
    // Db::from_tsv: drop start > end, then the stable sort by (start, end) (src/asn_db.rs:111-137)
    std::vector<fb_asn_range> a4, a6;
    for (uint32_t i = 0; i < n4; ++i)
        if (asn_valid(v4[i], false)) a4.push_back(v4[i]);
    for (uint32_t i = 0; i < n6; ++i)
        if (asn_valid(v6[i], true)) a6.push_back(v6[i]);
    std::stable_sort(a4.begin(), a4.end(), [](const fb_asn_range& x, const fb_asn_range& y) { return asn_less(x, y, false); });
    std::stable_sort(a6.begin(), a6.end(), [](const fb_asn_range& x, const fb_asn_range& y) { return asn_less(x, y, true); });
    int rc = upload_array(c->en.asn4, a4.data(), a4.size());
    if (!rc) rc = upload_array(c->en.asn6, a6.data(), a6.size());
    c->en.n4 = rc ? 0 : (uint32_t)a4.size();
    c->en.n6 = rc ? 0 : (uint32_t)a6.size();
    return rc;
}

int fb_set_blacklists(fb_ctx* c, const fb_cidr* nets, uint32_t n) {
    if (!c || (n && !nets)) return set_err(FB_ERR_INVAL, "bad arguments");
    std::vector<uint32_t> p4;
    std::vector<unsigned long long> m4, m6;
    std::vector<uint4> p6;
    if (!build_blacklist_tables(nets, n, p4, m4, p6, m6))
        return set_err(FB_ERR_INVAL, "blacklist entry with a bad family, prefix or list (< %u)", FB_MAX_BLACKLISTS);
    DeviceGuard g(c->device);
    HIP_TRY(hipDeviceSynchronize());
    int rc = upload_array(c->en.bl4_pos, p4.data(), p4.size());
    if (!rc) rc = upload_array(c->en.bl4_mask, m4.data(), m4.size());
    if (!rc) rc = upload_array(c->en.bl6_pos, p6.data(), p6.size());
    if (!rc) rc = upload_array(c->en.bl6_mask, m6.data(), m6.size());
    c->en.m4 = rc ? 0 : (uint32_t)p4.size();
    c->en.m6 = rc ? 0 : (uint32_t)p6.size();
    return rc;
}

int fb_ip_lookup_dev(fb_ctx* c, const fb_ip* d_ips, uint32_t n, int32_t* d_asn, uint64_t* d_lists, void* stream) {
    if (!c || (n && !d_ips)) return set_err(FB_ERR_INVAL, "bad arguments");
    DeviceGuard g(c->device);
    HIP_TRY(launch_ip_lookup(c->en.tables(), d_ips, n, d_asn, (unsigned long long*)d_lists, (hipStream_t)stream));
    return FB_OK;
}

int fb_flow_enrich_dev(fb_ctx* c, uint32_t new_only, fb_flow_enrich* d_out, uint64_t cap, uint64_t* d_n,
                       void* stream) {
    if (!c || !d_n || (cap && !d_out)) return set_err(FB_ERR_INVAL, "bad arguments");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_n, 0, 8, s));
    if (!c->tb.slots || (new_only && c->flow_batch == 0)) return FB_OK;
    int rc = join_updates(c, s);
    if (!rc) rc = upload_cfg(c, s);
    if (rc) return rc;
    HIP_TRY(launch_flow_enrich(c->en.tables(), c->d_cfg, c->tb.slots, c->tb.cap, new_only ? 1u : 0u,
                               c->flow_batch - 1u, d_out, cap, (unsigned long long*)d_n, s));
    return FB_OK;
}

int fb_dns_parse_dev(fb_ctx* c, const uint8_t* d_frames, uint64_t frames_bytes, const fb_dns_out* d_dns, uint32_t n,
                     const fb_batch_stats* d_stats, fb_dns_msg* d_msgs, char* d_names, fb_ip* d_addrs, void* stream) {
    if (!c || (n && (!d_dns || !d_msgs || !d_names || !d_addrs || !d_frames)))
        return set_err(FB_ERR_INVAL, "bad arguments");
    if (reinterpret_cast<uintptr_t>(d_names) & 3u) return set_err(FB_ERR_INVAL, "d_names must be 4-byte aligned");
    DeviceGuard g(c->device);
    HIP_TRY(launch_dns_parse(d_frames, frames_bytes, d_dns, n, d_stats, d_msgs, d_names, d_addrs, (hipStream_t)stream));
    return FB_OK;
}

int fb_flow_count(fb_ctx* c, uint64_t* n_flows, void* stream) {
    if (!c || !n_flows) return set_err(FB_ERR_INVAL, "bad arguments");
    *n_flows = 0;
    if (!c->tb.slots) return FB_OK;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long h = 0;
    const int rc = join_updates(c, s);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->d_n, 0, 8, s));
    HIP_TRY(launch_flow_count(c->tb.slots, c->tb.cap, c->d_n, s));
    HIP_TRY(hipMemcpyAsync(&h, c->d_n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n_flows = h;
    return FB_OK;
}

int fb_flow_export_sessions_dev(fb_ctx* c, uint32_t filter, fb_flow_rec* d_out, uint64_t cap, uint64_t* d_n,
                                void* stream) {
    if (!c || !d_n || (cap && !d_out) || filter > FB_FILTER_ALL) return set_err(FB_ERR_INVAL, "bad arguments");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_n, 0, 8, s));
    if (!c->tb.slots) return FB_OK;
    int rc = join_updates(c, s);
    if (!rc && filter != FB_FILTER_ALL) rc = upload_cfg(c, s);  // the LAN configuration as of now
    if (rc) return rc;
    HIP_TRY(launch_flow_export(c->tb.slots, c->tb.cap, d_out, cap, (unsigned long long*)d_n, s, filter, c->d_cfg,
                               c->plane<FlowTime>(kPlaneTime)));
    return FB_OK;
}

int fb_flow_export_times_dev(fb_ctx* c, fb_flow_time* d_out, uint64_t cap, uint64_t* d_n, void* stream) {
    if (!c || !d_n || (cap && !d_out)) return set_err(FB_ERR_INVAL, "bad arguments");
    if (!c->timed) return set_err(FB_ERR_INVAL, "the context was created without FB_CFG_TIMED");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_n, 0, 8, s));
    int rc = join_updates(c, s);
    if (rc) return rc;
    HIP_TRY(launch_time_export(c->tb.slots, c->plane<FlowTime>(kPlaneTime), c->tb.cap, d_out, cap,
                               (unsigned long long*)d_n, s));
    return FB_OK;
}

int fb_flow_export_times(fb_ctx* c, fb_flow_time* out, uint64_t cap, uint64_t* n, void* stream) {
    if (!c || !n || (cap && !out)) return set_err(FB_ERR_INVAL, "bad arguments");
    *n = 0;
    if (!c->timed) return set_err(FB_ERR_INVAL, "the context was created without FB_CFG_TIMED");
    if (cap == 0) return FB_OK;
    DeviceGuard g(c->device);
    return export_to_host(c, out, cap, sizeof(fb_flow_time), n, (hipStream_t)stream, "time export", [&](void* d_out) {
        return fb_flow_export_times_dev(c, (fb_flow_time*)d_out, cap, reinterpret_cast<uint64_t*>(c->d_n.get()), stream);
    });
}

int fb_flow_export_dev(fb_ctx* c, fb_flow_rec* d_out, uint64_t cap, uint64_t* d_n, void* stream) {
    return fb_flow_export_sessions_dev(c, FB_FILTER_ALL, d_out, cap, d_n, stream);
}

// ---- session aging (fb_age.hip) ---------------------------------------------------------------------
// Synchronous, like a growth: drains the updates in flight, runs k_flow_age over every partition and
// reads the call's counters back.  A purge that removed flows moved others inside their partitions:
// its slot map replaces the last growth's, the generation rises, the last update's history is gone,
// and -- everything being drained -- the host writes the purged table's occupancy into the mailbox, so
// fb_flow_table_info_get and maybe_grow's projection see the table as it is now.
int fb_flow_age(fb_ctx* c, uint64_t now_ns, const fb_age_params* params, uint32_t flags, fb_age_stats* out,
                void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if (!c->timed) return set_err(FB_ERR_INVAL, "the context was created without FB_CFG_TIMED (aging needs the clock)");
    if (flags & ~FB_AGE_PURGE) return set_err(FB_ERR_INVAL, "unknown flags %u", flags);
    static const fb_age_params kReference = {60ull * 1000000000ull, 180ull * 1000000000ull, 86400ull * 1000000000ull, 0};
    const fb_age_params& ap = params ? *params : kReference;  // src/sessions.rs:10-15
    const bool purge = (flags & FB_AGE_PURGE) != 0u;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    int rc = pass_begin(c, kAgeStatWords, s);
    if (!rc) rc = plane_ensure(c, kPlaneStatus, s);
    if (rc) return rc;
    if (purge && c->d_age_remap.size() != c->tb.cap && c->d_age_remap.alloc(c->tb.cap) != hipSuccess)
        return set_err(FB_ERR_NOMEM, "slot remap");
    AgeArgs a;
    a.table = c->tb.slots;
    a.plane = c->plane<FlowTime>(kPlaneTime);
    a.char_call = c->tb.char_call;
    a.status = c->plane<uint8_t>(kPlaneStatus);
    a.remap = purge ? c->d_age_remap.get() : nullptr;
    a.stats = c->d_pass_stats;
    a.now = now_ns;
    a.activity = ap.activity_ns;
    a.current = ap.current_ns;
    a.retention = ap.retention_ns;
    a.purge = purge ? 1u : 0u;
    HIP_TRY(launch_flow_age(a, c->tb.parts, s));
    unsigned long long h[kAgeStatWords] = {};
    rc = pass_end(c, h, kAgeStatWords, s);
    if (rc) return rc;
    if (h[6]) {  // flows were removed: survivors of their partitions may have moved
        c->d_remap.swap(c->d_age_remap);  // (the old map is reallocated if its size is not the table's)
        ++c->generation;
        c->last.invalidate();  // the last update's slots moved: its history is no longer available
        c->mbox->flows = h[7];
        c->mbox->max_part = h[8];
        if (c->hs && c->tb.plane[kPlaneHist])  // the removed flows' blocks, read off the plane before it moves
            rc = histstore_free_sweep(c->hs, c->plane<uint4>(kPlaneHist), c->d_remap, c->tb.cap, s);
        if (rc) return rc;
        rc = planes_follow_purge(c, s);
        if (rc) return rc;
    }
    if (out) {
        memset(out, 0, sizeof(*out));
        out->flows = h[0];
        out->active = h[1];
        out->added = h[2];
        out->activated = h[3];
        out->deactivated = h[4];
        out->current = h[5];
        out->purged = h[6];
        out->remaining = h[7];
        out->max_partition = h[8];
    }
    return FB_OK;
}

int fb_flow_status_dev(fb_ctx* c, uint8_t* d_out, uint64_t cap, void* stream) {
    return plane_copy_out(c, kPlaneStatus, d_out, cap, stream);
}

// ---- whitelist conformance (fb_whitelist.hip) -----------------------------------------------------
// The list is validated and indexed on the host first (build_whitelist_index), so a refused list
// leaves the installed one untouched; then the old arrays are replaced (no launch may still read them).
// The pattern tables of d.host on the device (the match state is the caller's to reset).
static int wl_dom_upload(WlDomDev& d) {
    const WlDomIndex& h = d.host;
    int rc = upload_array(d.blob, h.blob.data(), h.blob.size());
    if (!rc) rc = upload_array(d.off, h.off.data(), h.off.size());
    for (uint32_t k = 0; !rc && k < kWlDomHashed; ++k) {
        rc = upload_array(d.hash[k], h.hash[k].data(), h.hash[k].size());
        if (!rc) rc = upload_array(d.len[k], h.len[k].data(), h.len[k].size());
        if (!rc) rc = upload_array(d.pid[k], h.pid[k].data(), h.pid[k].size());
    }
    if (!rc) rc = upload_array(d.gpid, h.gpid.data(), h.gpid.size());
    if (!rc) rc = upload_array(d.gstar, h.gstar.data(), h.gstar.size());
    return rc;
}
// No name's row is valid any more.
static int wl_dom_forget(WlDomDev& d) {
    d.upto = 0;
    if (d.ctr) HIP_TRY(hipMemset(d.ctr, 0, 16));
    return FB_OK;
}
// FB_DEBUG_WL_NAME_HASH_MASK: the installed pattern tables again under the new mask, every name to be matched again.
static int wl_dom_set_mask(fb_ctx* c, unsigned long long mask) {
    c->wl_name_hash_mask = mask;
    WlDomDev& d = c->wl.dom;
    if (!d.active()) return FB_OK;
    DeviceGuard g(c->device);
    HIP_TRY(hipDeviceSynchronize());
    const std::vector<uint8_t> blob(d.host.blob);
    const std::vector<uint64_t> off(d.host.off.begin(), d.host.off.end());
    if (!build_wl_dom_index(blob.data(), off.data(), off.size() - 1u, mask, d.host))
        return set_err(FB_ERR_INTERNAL, "domain pattern tables");
    const int rc = wl_dom_upload(d);
    return rc ? rc : wl_dom_forget(d);
}
// The names (upto, n_names] of the DNS tracker matched against the installed patterns; the rows grow with the
// tracker's store.  Waits for what it launched: the rows are read by whatever stream comes next.
static int wl_dom_sync(fb_ctx* c, hipStream_t s) {
    WlDomDev& d = c->wl.dom;
    if (!d.active() || !c->dns) return FB_OK;
    const DnsTables t = dnstrack_tables(c->dns);
    const uint64_t n = t.n_names;
    if (n <= d.upto) return FB_OK;
    if (!d.ctr) {
        if (d.ctr.alloc(2) != hipSuccess) return set_err(FB_ERR_NOMEM, "name match counters");
        HIP_TRY(hipMemsetAsync(d.ctr, 0, 16, s));
    }
    if (n > d.cap) {
        uint64_t cap = std::max<uint64_t>(2ull * d.cap, 1024ull);
        while (cap < n) cap *= 2ull;
        DevBuf<uint32_t> rows;
        DevBuf<uint8_t> flags;
        if (alloc_each(rows, (cap + 1ull) * FB_WL_NAME_MATCHES, flags, cap + 1ull) != hipSuccess)
            return set_err(FB_ERR_NOMEM, "name match rows (%llu names)", (unsigned long long)cap);
        if (d.upto) {
            HIP_TRY(hipMemcpyAsync(rows, d.rows, (d.upto + 1ull) * FB_WL_NAME_MATCHES * 4ull, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(flags, d.flags, d.upto + 1ull, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        d.rows = std::move(rows);
        d.flags = std::move(flags);
        d.cap = cap;
    }
    HIP_TRY(launch_wl_name_match(d.tables(), t.names, t.name_len, (uint32_t)d.upto + 1u, (uint32_t)n, d.rows, d.flags, d.ctr, s));
    HIP_TRY(hipStreamSynchronize(s));
    d.upto = n;
    return FB_OK;
}

int fb_set_whitelist_dom(fb_ctx* c, const fb_wl_endpoint* eps, uint64_t n, const uint32_t* ep_pattern,
                         const uint8_t* pattern_bytes, const uint64_t* pattern_off, uint64_t n_patterns,
                         const uint32_t* rec_owner_id, const uint32_t* rec_country_id, uint32_t n_records) {
    if (!c || (n && !eps) || (n_records && (!rec_owner_id || !rec_country_id)) || (n_patterns && !pattern_off))
        return set_err(FB_ERR_INVAL, "bad arguments");
    if (n > (uint64_t)FB_WL_MAX_EXACT + FB_WL_MAX_OTHER)
        return set_err(FB_ERR_INVAL, "%llu endpoints: more than FB_WL_MAX_EXACT + FB_WL_MAX_OTHER", (unsigned long long)n);
    if (n_patterns > (1u << 24) - 1u)
        return set_err(FB_ERR_INVAL, "%llu patterns: more than 2^24 - 1", (unsigned long long)n_patterns);
    if (n_patterns && pattern_off[n_patterns] && !pattern_bytes) return set_err(FB_ERR_INVAL, "pattern_bytes is NULL");
    WlDomDev dom;
    if (!build_wl_dom_index(pattern_bytes, pattern_off, n_patterns, c->wl_name_hash_mask, dom.host))
        return set_err(FB_ERR_INVAL, "domain patterns: offsets that do not ascend from 0, 2^32 bytes or more, or more than "
                       "%u patterns of the a*b kind", FB_WL_MAX_GENERAL);
    WlIndex ix;
    if (!build_whitelist_index(eps, n, ix, ep_pattern, n_patterns))
        return set_err(FB_ERR_INVAL, "whitelist endpoint with a bad family, prefix, protocol or flags, more than "
                       "%u exact-address / %u other endpoints, or a pattern id above n_patterns or without FB_WL_HAS_DOMAIN",
                       FB_WL_MAX_EXACT, FB_WL_MAX_OTHER);
    DeviceGuard g(c->device);
    HIP_TRY(hipDeviceSynchronize());
    c->wl_active = false;
    c->wl = WlDev();  // (no launch may still read it) -- and it stays empty when an upload fails
    WlDev w;
    int rc = upload_array(w.a4, ix.a4.data(), ix.a4.size());
    if (!rc) rc = upload_array(w.k4, ix.k4.data(), ix.k4.size());
    if (!rc) rc = upload_array(w.a6, ix.a6.data(), ix.a6.size());
    if (!rc) rc = upload_array(w.k6, ix.k6.data(), ix.k6.size());
    if (!rc) rc = upload_array(w.kp4, ix.kp4.data(), ix.kp4.size());
    if (!rc) rc = upload_array(w.kp6, ix.kp6.data(), ix.kp6.size());
    if (!rc) rc = upload_array(w.gkey, ix.gkey.data(), ix.gkey.size());
    if (!rc) rc = upload_array(w.gbeg, ix.gbeg.data(), ix.gkey.empty() ? 0 : ix.gbeg.size());
    if (!rc) rc = upload_array(w.rules, ix.rules.data(), ix.rules.size());
    if (!rc) rc = upload_array(w.owner, rec_owner_id, n_records);
    if (!rc) rc = upload_array(w.country, rec_country_id, n_records);
    if (!rc) rc = upload_array(w.dpid, ix.dpid.data(), ix.dpid.size());
    if (!rc) rc = upload_array(w.dkp, ix.dkp.data(), ix.dkp.size());
    if (!rc && dom.active()) rc = wl_dom_upload(dom);
    if (rc) return rc;
    w.n4 = (uint32_t)ix.a4.size();
    w.n6 = (uint32_t)ix.a6.size();
    w.ng = (uint32_t)ix.gkey.size();
    w.nr = (uint32_t)ix.rules.size();
    w.records = n_records;
    w.with_proc = ix.with_proc;
    w.nd = (uint32_t)ix.dpid.size();
    w.dom = std::move(dom);  // (no name matched yet)
    c->wl = std::move(w);
    c->wl_active = true;
    return FB_OK;
}

int fb_set_whitelist(fb_ctx* c, const fb_wl_endpoint* eps, uint64_t n, const uint32_t* rec_owner_id,
                     const uint32_t* rec_country_id, uint32_t n_records) {
    return fb_set_whitelist_dom(c, eps, n, nullptr, nullptr, nullptr, 0u, rec_owner_id, rec_country_id, n_records);
}

int fb_wl_name_matches_dev(fb_ctx* c, const uint32_t* d_ids, uint64_t n, uint32_t* d_rows, uint8_t* d_flags, void* stream) {
    if (!c || (n && (!d_ids || !d_rows || !d_flags))) return set_err(FB_ERR_INVAL, "bad arguments");
    if (!c->wl_active) return set_err(FB_ERR_INVAL, "no whitelist is installed (fb_set_whitelist)");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int rc = wl_dom_sync(c, s);
    if (rc) return rc;
    const WlDomDev& d = c->wl.dom;
    HIP_TRY(launch_wl_name_rows(d_ids, n, d.rows, d.flags, (uint32_t)d.upto, d_rows, d_flags, s));
    return FB_OK;
}

int fb_wl_dom_info_get(fb_ctx* c, fb_wl_dom_info* out) {
    if (!c || !out) return set_err(FB_ERR_INVAL, "bad arguments");
    memset(out, 0, sizeof(*out));
    if (!c->wl_active) return FB_OK;
    const WlDomDev& d = c->wl.dom;
    for (uint32_t k = 0; k < kWlDomKinds; ++k) out->patterns[k] = d.host.count[k];
    out->names_done = d.upto;
    if (d.ctr && d.upto) {
        DeviceGuard g(c->device);
        unsigned long long h[2] = {};
        HIP_TRY(hipMemcpy(h, d.ctr, 16, hipMemcpyDeviceToHost));
        out->names_matched = h[0];
        out->names_overflowed = h[1];
    }
    return FB_OK;
}

int fb_clear_whitelist(fb_ctx* c) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    DeviceGuard g(c->device);
    HIP_TRY(hipDeviceSynchronize());
    c->wl_active = false;
    const int rc = wl_dom_forget(c->wl.dom);
    if (rc) return rc;
    HIP_TRY(plane_zero(c, kPlaneWl, nullptr));  // every state back to Unknown
    HIP_TRY(hipStreamSynchronize(nullptr));
    return FB_OK;
}

// Synchronous, like fb_flow_age: drains the updates in flight, one pass, the counters read back.
int fb_flow_whitelist(fb_ctx* c, uint32_t flags, fb_wl_stats* out, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if (!c->wl_active) return set_err(FB_ERR_INVAL, "no whitelist is installed (fb_set_whitelist)");
    if (flags) return set_err(FB_ERR_INVAL, "unknown flags %u", flags);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    int rc = pass_begin(c, kWlCounters, s);
    if (!rc) rc = upload_cfg(c, s);  // the LAN configuration as of now
    if (!rc) rc = plane_ensure(c, kPlaneWl, s);
    unsigned long long* mod = nullptr;
    if (!rc) rc = pass_stamps(c, s, &mod);
    const bool with_dom = c->wl.nd != 0u;  // the names that appeared since the last call are matched first
    if (!rc && with_dom) rc = wl_dom_sync(c, s);
    if (rc) return rc;
    const WlDomDev& d = c->wl.dom;
    const WlDomFlows df = {c->dns ? c->plane<fb_flow_domain>(kPlaneDom) : nullptr, d.rows, d.flags, (uint32_t)d.upto};
    // (whether a process endpoint with an id matches or asks for the host is decided here, by the name table
    // installed now: fb_set_whitelist and fb_set_l7_process_names may come in either order)
    HIP_TRY(launch_flow_whitelist(c->wl.tables(), c->en.tables(), c->d_cfg, c->tb.slots, c->tb.cap, c->plane<uint8_t>(kPlaneWl),
                                  c->d_pass_stats, s, mod, c->pass_time, c->wl.with_proc, c->proc_names(),
                                  with_dom ? &df : nullptr));
    unsigned long long h[kWlCounters] = {};
    rc = pass_end(c, h, kWlCounters, s);
    if (rc) return rc;
    if (out) {
        memset(out, 0, sizeof(*out));
        out->flows = h[0];
        out->conforming = h[1];
        out->nonconforming = h[2];
        out->host_check = h[3];
        out->changed = h[4];
        out->dom_overflow = h[5];
    }
    return FB_OK;
}

int fb_flow_whitelist_dev(fb_ctx* c, uint8_t* d_out, uint64_t cap, void* stream) {
    return plane_copy_out(c, kPlaneWl, d_out, cap, stream);
}

int fb_flow_export_whitelist_dev(fb_ctx* c, uint32_t state_mask, fb_flow_rec* d_out, uint64_t cap, uint64_t* d_n,
                                 void* stream) {
    if (!c || !d_n || (cap && !d_out)) return set_err(FB_ERR_INVAL, "bad arguments");
    if (state_mask & ~(FB_WL_CONFORMING | FB_WL_NONCONFORMING | FB_WL_HOST_CHECK | FB_WL_MASK_UNKNOWN))
        return set_err(FB_ERR_INVAL, "unknown state_mask bits %u", state_mask);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_n, 0, 8, s));
    if (!c->tb.slots) return FB_OK;
    const int rc = join_updates(c, s);
    if (rc) return rc;
    HIP_TRY(launch_flow_export_whitelist(c->tb.slots, c->plane<uint8_t>(kPlaneWl), c->tb.cap, state_mask, d_out, cap,
                                         (unsigned long long*)d_n, c->plane<FlowTime>(kPlaneTime), s));
    return FB_OK;
}

// ---- blacklist pass (fb_blacklist.hip) ---------------------------------------------------------------
// Synchronous, like fb_flow_age / fb_flow_whitelist: drains the updates in flight, one pass, the
// counters read back.  The lists are whatever fb_set_blacklists installed last (none: every mask 0).
int fb_flow_blacklist(fb_ctx* c, uint32_t flags, fb_bl_stats* out, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if (flags & ~FB_BL_MARK_WHITELIST) return set_err(FB_ERR_INVAL, "unknown flags %u", flags);
    const bool mark = (flags & FB_BL_MARK_WHITELIST) != 0u;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    int rc = pass_begin(c, kBlCounters, s);
    if (!rc) rc = plane_ensure(c, kPlaneBl, s);
    // the fallback writes the whitelist plane, which no whitelist pass may have made yet
    if (!rc && mark) rc = plane_ensure(c, kPlaneWl, s);
    unsigned long long* mod = nullptr;
    if (!rc) rc = pass_stamps(c, s, &mod);
    if (rc) return rc;
    HIP_TRY(launch_flow_blacklist(c->en.tables(), c->tb.slots, c->tb.cap, c->plane<unsigned long long>(kPlaneBl),
                                  mark ? c->plane<uint8_t>(kPlaneWl) : nullptr, c->d_pass_stats, s, mod, c->pass_time));
    unsigned long long h[kBlCounters] = {};
    rc = pass_end(c, h, kBlCounters, s);
    if (rc) return rc;
    if (out) {
        memset(out, 0, sizeof(*out));
        out->flows = h[0];
        out->blacklisted = h[1];
        out->changed = h[2];
        out->newly_blacklisted = h[3];
        out->cleared = h[4];
        out->wl_marked = h[5];
    }
    return FB_OK;
}

int fb_flow_blacklist_dev(fb_ctx* c, uint64_t* d_out, uint64_t cap, void* stream) {
    return plane_copy_out(c, kPlaneBl, d_out, cap, stream);
}

int fb_flow_export_blacklisted_dev(fb_ctx* c, fb_flow_rec* d_out, uint64_t* d_masks, uint64_t cap, uint64_t* d_n,
                                   void* stream) {
    if (!c || !d_n || (cap && !d_out)) return set_err(FB_ERR_INVAL, "bad arguments");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_n, 0, 8, s));
    if (!c->tb.slots || !c->tb.plane[kPlaneBl]) return FB_OK;  // no pass yet: no flow has a mask
    const int rc = join_updates(c, s);
    if (rc) return rc;
    HIP_TRY(launch_flow_export_blacklisted(c->tb.slots, c->plane<unsigned long long>(kPlaneBl), c->tb.cap, d_out,
                                           (unsigned long long*)d_masks, cap, (unsigned long long*)d_n,
                                           c->plane<FlowTime>(kPlaneTime), s));
    return FB_OK;
}

// ---- DNS tracker (fb_dnstrack.hip) and the domain pass (fb_domains.hip) -------------------------------
static int dns_ready(const fb_ctx* c) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->dns) return set_err(FB_ERR_INVAL, "DNS tracking is not enabled (fb_dns_track_enable)");
    return FB_OK;
}

int fb_dns_track_enable(fb_ctx* c, const fb_dns_track_config* cfg) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (c->dns) return set_err(FB_ERR_INVAL, "DNS tracking is already enabled");
    DeviceGuard g(c->device);
    return dnstrack_create(&c->dns, cfg);
}

int fb_dns_track_clear(fb_ctx* c) {
    int rc = dns_ready(c);
    if (rc) return rc;
    DeviceGuard g(c->device);
    rc = drain_updates(c);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    rc = dnstrack_clear(c->dns, nullptr);
    if (!rc) rc = wl_dom_forget(c->wl.dom);  // the ids died with the store: so did their match rows
    if (rc) return rc;
    HIP_TRY(plane_zero(c, kPlaneDom, nullptr));  // the ids died with the store
    HIP_TRY(hipStreamSynchronize(nullptr));
    return FB_OK;
}

int fb_dns_track_dev(fb_ctx* c, const fb_dns_msg* d_msgs, const char* d_names, const fb_ip* d_addrs, uint32_t n,
                     const fb_batch_stats* d_stats, const uint64_t* d_ts, uint32_t* d_taken, fb_dns_track_stats* out,
                     void* stream) {
    const int rc = dns_ready(c);
    if (rc) return rc;
    if (n && (!d_msgs || !d_names || !d_addrs)) return set_err(FB_ERR_INVAL, "bad arguments");
    if (reinterpret_cast<uintptr_t>(d_names) & 3u) return set_err(FB_ERR_INVAL, "d_names must be 4-byte aligned");
    DeviceGuard g(c->device);
    return dnstrack_track(c->dns, d_msgs, d_names, d_addrs, n, d_stats, (const unsigned long long*)d_ts, d_taken, out,
                          (hipStream_t)stream);
}

int fb_dns_expire(fb_ctx* c, uint64_t now_ns, uint64_t* dropped) {
    const int rc = dns_ready(c);
    if (rc) return rc;
    DeviceGuard g(c->device);
    return dnstrack_expire(c->dns, now_ns, dropped, nullptr);
}

int fb_dns_track_info_get(fb_ctx* c, fb_dns_track_info* out) {
    const int rc = dns_ready(c);
    if (rc) return rc;
    if (!out) return set_err(FB_ERR_INVAL, "out is NULL");
    DeviceGuard g(c->device);
    return dnstrack_info(c->dns, out, nullptr);
}

int fb_dns_export_resolutions_dev(fb_ctx* c, fb_dns_resolution* d_out, uint64_t cap, uint64_t* d_n, void* stream) {
    const int rc = dns_ready(c);
    if (rc) return rc;
    if (!d_n || (cap && !d_out)) return set_err(FB_ERR_INVAL, "bad arguments");
    DeviceGuard g(c->device);
    return dnstrack_export_resolutions(c->dns, d_out, cap, d_n, (hipStream_t)stream);
}

int fb_dns_export_pending_dev(fb_ctx* c, uint32_t* d_name_id, uint64_t* d_time, void* stream) {
    const int rc = dns_ready(c);
    if (rc) return rc;
    if (!d_name_id) return set_err(FB_ERR_INVAL, "d_name_id is NULL");
    DeviceGuard g(c->device);
    return dnstrack_export_pending(c->dns, d_name_id, d_time, (hipStream_t)stream);
}

int fb_dns_names_dev(fb_ctx* c, const uint32_t* d_ids, uint64_t n, char* d_out, uint16_t* d_len, void* stream) {
    const int rc = dns_ready(c);
    if (rc) return rc;
    if (n && (!d_ids || !d_out || !d_len)) return set_err(FB_ERR_INVAL, "bad arguments");
    if (reinterpret_cast<uintptr_t>(d_out) & 3u) return set_err(FB_ERR_INVAL, "d_out must be 4-byte aligned");
    DeviceGuard g(c->device);
    return dnstrack_names(c->dns, d_ids, n, d_out, d_len, (hipStream_t)stream);
}

int fb_dns_lookup_dev(fb_ctx* c, const fb_ip* d_ips, uint64_t n, uint32_t* d_name_id, void* stream) {
    const int rc = dns_ready(c);
    if (rc) return rc;
    if (n && (!d_ips || !d_name_id)) return set_err(FB_ERR_INVAL, "bad arguments");
    DeviceGuard g(c->device);
    return dnstrack_lookup(c->dns, d_ips, n, d_name_id, (hipStream_t)stream);
}

// Synchronous, like fb_flow_blacklist: drains the updates in flight, one pass, the counters read back.
int fb_flow_domains(fb_ctx* c, uint32_t flags, fb_dom_stats* out, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if (!c->dns) return set_err(FB_ERR_INVAL, "DNS tracking is not enabled (fb_dns_track_enable)");
    if (flags) return set_err(FB_ERR_INVAL, "unknown flags %u", flags);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    int rc = pass_begin(c, kDomCounters, s);
    if (!rc) rc = plane_ensure(c, kPlaneDom, s);
    unsigned long long* mod = nullptr;
    if (!rc) rc = pass_stamps(c, s, &mod);
    if (rc) return rc;
    HIP_TRY(launch_flow_domains(dnstrack_tables(c->dns), c->tb.slots, c->tb.cap, c->plane<uint8_t>(kPlaneStatus),
                                c->plane<uint2>(kPlaneDom), c->d_pass_stats, s, mod, c->pass_time));
    unsigned long long h[kDomCounters] = {};
    rc = pass_end(c, h, kDomCounters, s);
    if (rc) return rc;
    if (out) {
        memset(out, 0, sizeof(*out));
        out->flows = h[0];
        out->current = h[1];
        out->src_set = h[2];
        out->dst_set = h[3];
        out->changed = h[4];
        out->with_domain = h[5];
    }
    return FB_OK;
}

int fb_flow_domains_dev(fb_ctx* c, fb_flow_domain* d_out, uint64_t cap, void* stream) {
    return plane_copy_out(c, kPlaneDom, d_out, cap, stream);
}

// ---- L7 pass (fb_l7.hip) -----------------------------------------------------------------------------
int fb_l7_validate(const fb_l7_socket* socks, uint64_t n) {
    if (n && !socks) return set_err(FB_ERR_INVAL, "socks is NULL");
    if (n > FB_L7_MAX_SOCKETS) return set_err(FB_ERR_INVAL, "%llu sockets: more than FB_L7_MAX_SOCKETS", (unsigned long long)n);
    for (uint64_t i = 0; i < n; ++i)
        if (!l7_socket_valid(socks[i]))
            return set_err(FB_ERR_INVAL, "socket %llu: protocol 6 / 17, families 2 / 10 (remote: 0 for UDP), process_id >= 1, "
                           "reserved fields 0, IPv4 addresses in word 0 alone", (unsigned long long)i);
    return FB_OK;
}

int fb_set_l7_sockets(fb_ctx* c, const fb_l7_socket* socks, uint64_t n) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    int rc = fb_l7_validate(socks, n);
    if (rc) return rc;
    std::vector<L7Pair> pairs;
    std::vector<L7Local> locals;
    if (!build_l7_index(socks, n, pairs, locals)) return set_err(FB_ERR_INVAL, "socket snapshot");
    DeviceGuard g(c->device);
    L7Dev d;  // uploaded whole before it replaces the installed one
    rc = upload_array(d.pairs, pairs.data(), pairs.size());
    if (!rc) rc = upload_array(d.locals, locals.data(), locals.size());
    if (rc) return rc;
    d.n_pairs = (uint32_t)pairs.size();
    d.n_locals = (uint32_t)locals.size();
    d.active = true;
    HIP_TRY(hipDeviceSynchronize());  // (no launch may still read the old one)
    c->l7 = std::move(d);
    return FB_OK;
}

// The arrays are checked and uploaded whole before they replace the installed table.
int fb_set_l7_process_names(fb_ctx* c, const uint32_t* match_id, const uint32_t* name_id, uint64_t n) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (n && (!match_id || !name_id)) return set_err(FB_ERR_INVAL, "match_id / name_id is NULL");
    if (n > 0xFFFFFFFFull) return set_err(FB_ERR_INVAL, "%llu process ids: more than 32 bits hold", (unsigned long long)n);
    for (uint64_t p = 1; p < n; ++p)
        if (match_id[p] == 0u || name_id[p] == 0u)
            return set_err(FB_ERR_INVAL, "process %llu: match_id and name_id are ids >= 1", (unsigned long long)p);
    DeviceGuard g(c->device);
    L7Names d;
    if (n) {
        std::vector<uint32_t> m(match_id, match_id + n), v(name_id, name_id + n);
        m[0] = v[0] = 0u;  // "no process"
        int rc = upload_array(d.match_id, m.data(), m.size());
        if (!rc) rc = upload_array(d.name_id, v.data(), v.size());
        if (rc) return rc;
        d.n = (uint32_t)n;
    }
    const int rc = drain_updates(c);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (no launch may still read the old one)
    c->l7_names = std::move(d);
    return FB_OK;
}

int fb_l7_clear(fb_ctx* c) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    DeviceGuard g(c->device);
    const int rc = drain_updates(c);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    c->l7 = L7Dev();
    HIP_TRY(plane_zero(c, kPlaneL7, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return FB_OK;
}

// Synchronous, like fb_flow_domains: drains the updates in flight, one pass, the counters read back.
int fb_flow_l7(fb_ctx* c, const fb_l7_params* params, fb_l7_stats* out, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if (!c->l7.active) return set_err(FB_ERR_INVAL, "no socket snapshot is installed (fb_set_l7_sockets)");
    fb_l7_params prm = {FB_L7_DEFAULT_MAX_RETRIES, 0u, {0u, 0u}};
    if (params) prm = *params;
    if (prm.max_retries > 255u || prm.flags || prm.reserved[0] || prm.reserved[1])
        return set_err(FB_ERR_INVAL, "fb_l7_params: max_retries 0..255, flags and reserved words 0");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    int rc = pass_begin(c, kL7Counters, s);
    if (!rc) rc = plane_ensure(c, kPlaneL7, s);
    unsigned long long* mod = nullptr;
    if (!rc) rc = pass_stamps(c, s, &mod);
    if (rc) return rc;
    HIP_TRY(launch_flow_l7(c->l7.tables(), c->tb.slots, c->tb.cap, c->plane<uint8_t>(kPlaneStatus),
                           c->plane<uint2>(kPlaneL7), prm.max_retries, c->d_pass_stats, s, mod, c->pass_time));
    unsigned long long h[kL7Counters] = {};
    rc = pass_end(c, h, kL7Counters, s);
    if (rc) return rc;
    if (out) {
        out->flows = h[0];
        out->current = h[1];
        out->looked_up = h[2];
        out->exact = h[3];
        out->fuzzy = h[4];
        out->failed = h[5];
        out->resolved = h[6];
        out->changed = h[7];
    }
    return FB_OK;
}

int fb_flow_l7_dev(fb_ctx* c, fb_l7_rec* d_out, uint64_t cap, void* stream) {
    return plane_copy_out(c, kPlaneL7, d_out, cap, stream);
}

int fb_l7_lookup_dev(fb_ctx* c, const fb_session_key* d_keys, uint64_t n, fb_l7_rec* d_out, void* stream) {
    if (!c || (n && (!d_keys || !d_out))) return set_err(FB_ERR_INVAL, "bad arguments");
    if (!c->l7.active) return set_err(FB_ERR_INVAL, "no socket snapshot is installed (fb_set_l7_sockets)");
    DeviceGuard g(c->device);
    HIP_TRY(launch_l7_lookup(c->l7.tables(), d_keys, n, d_out, (hipStream_t)stream));
    return FB_OK;
}

// ---- anomaly pass (fb_anomaly.hip) -------------------------------------------------------------------
int fb_if_validate(const fb_if_node* nodes, uint64_t n_nodes, const uint32_t* first, uint32_t n_trees) {
    if (!forest_valid(nodes, n_nodes, first, n_trees))
        return set_err(FB_ERR_INVAL, "forest: 1..%u trees of 1..%u nodes, children above their parent and inside the tree, "
                       "leaves at most %u below the root, finite values and normals", FB_IF_MAX_TREES, FB_IF_MAX_TREE_NODES,
                       FB_IF_MAX_DEPTH);
    return FB_OK;
}

static bool service_codes_valid(const uint32_t* service_code) {
    for (uint32_t p = 0; service_code && p < 65536u; ++p)
        if (service_code[p] >= FB_AN_MAX_SERVICE_CODE) return false;
    return true;
}

int fb_set_service_codes(fb_ctx* c, const uint32_t* service_code) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!service_codes_valid(service_code)) return set_err(FB_ERR_INVAL, "a service code is %u or above", FB_AN_MAX_SERVICE_CODE);
    DeviceGuard g(c->device);
    HIP_TRY(hipDeviceSynchronize());  // no sweep in flight reads the old codes
    return upload_array(c->an.service, service_code, service_code ? (size_t)65536 : (size_t)0);
}

// Everything is checked, and the new arrays are on the device, before the installed model is touched.
int fb_set_anomaly_model(fb_ctx* c, const fb_if_node* nodes, uint64_t n_nodes, const uint32_t* first, uint32_t n_trees,
                         const fb_an_params* prm, const uint32_t* service_code) {
    if (!c || !nodes || !first || !prm) return set_err(FB_ERR_INVAL, "bad arguments");
    const int v = fb_if_validate(nodes, n_nodes, first, n_trees);
    if (v) return v;
    for (int j = 0; j < FB_AN_FEATURES; ++j)
        if (!std::isfinite(prm->mean[j]) || !std::isfinite(prm->std[j]))
            return set_err(FB_ERR_INVAL, "feature %d: mean / std not finite", j);
    if (std::isnan(prm->suspicious_cut) || std::isnan(prm->abnormal_cut) || prm->has_stats > 1u)
        return set_err(FB_ERR_INVAL, "a cut is NaN, or has_stats is not 0 / 1");
    if (!service_codes_valid(service_code)) return set_err(FB_ERR_INVAL, "a service code is %u or above", FB_AN_MAX_SERVICE_CODE);
    DeviceGuard g(c->device);
    AnModel m;
    int rc = upload_array(m.nodes, nodes, (size_t)n_nodes);
    if (!rc) rc = upload_array(m.first, first, (size_t)n_trees + 1u);
    if (!rc) rc = upload_array(m.service, service_code, service_code ? (size_t)65536 : (size_t)0);
    if (rc) return rc;
    const hipError_t e = hipDeviceSynchronize();  // no pass in flight reads the old arrays
    if (e != hipSuccess) return set_err(FB_ERR_HIP, "hipDeviceSynchronize: %s", hipGetErrorString(e));
    m.trees = n_trees;
    m.prm = *prm;
    m.active = true;
    c->an = std::move(m);
    return FB_OK;
}

int fb_clear_anomaly_model(fb_ctx* c) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    DeviceGuard g(c->device);
    HIP_TRY(hipDeviceSynchronize());
    c->an.active = false;
    HIP_TRY(plane_zero(c, kPlaneAn, nullptr));  // every record back to "unseen"
    HIP_TRY(hipStreamSynchronize(nullptr));
    return FB_OK;
}

// Synchronous, like fb_flow_blacklist: drains the updates in flight, one pass, the counters read back.
int fb_flow_anomaly(fb_ctx* c, uint32_t flags, fb_an_stats* out, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if (!c->an.active) return set_err(FB_ERR_INVAL, "no anomaly model is installed (fb_set_anomaly_model)");
    if (flags) return set_err(FB_ERR_INVAL, "unknown flags %u", flags);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    int rc = pass_begin(c, kAnCounters, s);
    if (!rc) rc = plane_ensure(c, kPlaneAn, s);
    unsigned long long* mod = nullptr;
    if (!rc) rc = pass_stamps(c, s, &mod);
    if (rc) return rc;
    HIP_TRY(launch_flow_anomaly(c->an.forest(), c->tb.slots, c->plane<FlowTime>(kPlaneTime), c->tb.cap,
                                c->plane<fb_an_rec>(kPlaneAn), c->d_pass_stats, s, mod, c->pass_time));
    unsigned long long h[kAnCounters] = {};
    rc = pass_end(c, h, kAnCounters, s);
    if (rc) return rc;
    if (out) {
        memset(out, 0, sizeof(*out));
        out->flows = h[0];
        out->normal = h[1];
        out->suspicious = h[2];
        out->abnormal = h[3];
        out->changed = h[4];
        out->newly_anomalous = h[5];
        out->cleared = h[6];
    }
    return FB_OK;
}

int fb_flow_anomaly_dev(fb_ctx* c, fb_an_rec* d_out, uint64_t cap, void* stream) {
    return plane_copy_out(c, kPlaneAn, d_out, cap, stream);
}

int fb_flow_export_anomalous_dev(fb_ctx* c, uint32_t min_level, fb_flow_rec* d_out, fb_an_rec* d_recs, uint64_t cap,
                                 uint64_t* d_n, void* stream) {
    if (!c || !d_n || (cap && !d_out)) return set_err(FB_ERR_INVAL, "bad arguments");
    if (min_level < FB_AN_NORMAL || min_level > FB_AN_ABNORMAL) return set_err(FB_ERR_INVAL, "min_level %u", min_level);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_n, 0, 8, s));
    if (!c->tb.slots || !c->tb.plane[kPlaneAn]) return FB_OK;  // no pass yet: no flow has a level
    const int rc = join_updates(c, s);
    if (rc) return rc;
    HIP_TRY(launch_flow_export_anomalous(c->tb.slots, c->plane<fb_an_rec>(kPlaneAn), c->tb.cap, min_level, d_out, d_recs,
                                         cap, (unsigned long long*)d_n, c->plane<FlowTime>(kPlaneTime), s));
    return FB_OK;
}

int fb_flow_features_dev(fb_ctx* c, double* d_feat, uint32_t* d_slot, uint64_t cap, uint64_t* d_n, void* stream) {
    if (!c || !d_n || (cap && (!d_feat || !d_slot))) return set_err(FB_ERR_INVAL, "bad arguments");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_n, 0, 8, s));
    if (!c->tb.slots) return FB_OK;
    const int rc = join_updates(c, s);
    if (rc) return rc;
    HIP_TRY(launch_flow_features(c->tb.slots, c->plane<FlowTime>(kPlaneTime), c->an.forest().service_code, c->tb.cap, d_feat,
                                 d_slot, cap, (unsigned long long*)d_n, s));
    return FB_OK;
}

int fb_if_score_dev(fb_ctx* c, const double* d_feat, uint64_t n, double* d_path_sum, void* stream) {
    if (!c || (n && (!d_feat || !d_path_sum))) return set_err(FB_ERR_INVAL, "bad arguments");
    if (!c->an.active) return set_err(FB_ERR_INVAL, "no anomaly model is installed (fb_set_anomaly_model)");
    if (n == 0) return FB_OK;
    DeviceGuard g(c->device);
    HIP_TRY(launch_if_score(c->an.forest(), d_feat, n, d_path_sum, (hipStream_t)stream));
    return FB_OK;
}

// ---- incremental queries: the pass clock, the stamp plane, the view export (fb_view.hip) ----------------
int fb_set_pass_time(fb_ctx* c, uint64_t now_ns) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    c->pass_time = now_ns;
    return FB_OK;
}

int fb_flow_modified_dev(fb_ctx* c, uint64_t* d_out, uint64_t cap, void* stream) {
    return plane_copy_out(c, kPlaneMod, d_out, cap, stream);
}

static int view_query_check(const fb_ctx* c, const fb_view_query* q) {
    if (!q) return set_err(FB_ERR_INVAL, "query is NULL");
    if (q->set > FB_VIEW_ANOMALOUS) return set_err(FB_ERR_INVAL, "unknown set %u", q->set);
    if (q->filter > FB_FILTER_ALL) return set_err(FB_ERR_INVAL, "unknown filter %u", q->filter);
    if (q->flags & ~FB_VIEW_MODIFIED_SINCE) return set_err(FB_ERR_INVAL, "unknown flags %u", q->flags);
    if (q->reserved) return set_err(FB_ERR_INVAL, "reserved field is %u", q->reserved);
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if ((q->flags & FB_VIEW_MODIFIED_SINCE) && !c->timed)
        return set_err(FB_ERR_INVAL, "FB_VIEW_MODIFIED_SINCE needs FB_CFG_TIMED (last_modified has no packet clock)");
    return FB_OK;
}

// The table, every plane and the (checked) query as the kernels read them.
static ViewArgs view_args(const fb_ctx* c, const fb_view_query* q) {
    ViewArgs a;
    a.table = c->tb.slots;
    a.time = c->plane<FlowTime>(kPlaneTime);
    a.status = c->plane<uint8_t>(kPlaneStatus);
    a.wl = c->plane<uint8_t>(kPlaneWl);
    a.bl = c->plane<unsigned long long>(kPlaneBl);
    a.an = c->plane<fb_an_rec>(kPlaneAn);
    a.mod = c->plane<unsigned long long>(kPlaneMod);
    a.cfg = c->d_cfg;
    a.cap = c->tb.cap;
    a.since = q->since_ns;
    a.set = q->set;
    a.filter = q->filter;
    a.flags = q->flags;
    return a;
}

int fb_flow_export_view_dev(fb_ctx* c, const fb_view_query* q, fb_flow_view* d_out, uint64_t cap, uint64_t* d_n,
                            void* stream) {
    if (!c || !d_n || (cap && !d_out) || (reinterpret_cast<uintptr_t>(d_out) & 15u))
        return set_err(FB_ERR_INVAL, "ctx and d_n are required, d_out (16-B aligned) unless cap is 0");
    int rc = view_query_check(c, q);
    if (rc) return rc;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_n, 0, 8, s));
    rc = join_updates(c, s);
    if (!rc && q->filter != FB_FILTER_ALL) rc = upload_cfg(c, s);  // the LAN configuration as of now
    if (rc) return rc;
    const ViewArgs a = view_args(c, q);
    HIP_TRY(launch_flow_view(a, d_out, cap, (unsigned long long*)d_n, !c->view_direct, s));
    return FB_OK;
}

int fb_flow_export_view(fb_ctx* c, const fb_view_query* q, fb_flow_view* out, uint64_t cap, uint64_t* n, void* stream) {
    if (!c || !n || (cap && !out)) return set_err(FB_ERR_INVAL, "bad arguments");
    *n = 0;
    int rc = view_query_check(c, q);
    if (rc) return rc;
    if (cap == 0) return FB_OK;
    DeviceGuard g(c->device);
    uint64_t total = 0;
    rc = fb_flow_count(c, &total, stream);
    if (rc) return rc;
    const uint64_t m = std::min(total, cap);
    if (m == 0) return FB_OK;
    return export_to_host(c, out, m, sizeof(fb_flow_view), n, (hipStream_t)stream, "view export", [&](void* d_out) {
        return fb_flow_export_view_dev(c, q, (fb_flow_view*)d_out, m, reinterpret_cast<uint64_t*>(c->d_n.get()), stream);
    });
}

// ---- endpoint learning (fb_learn.hip) ----------------------------------------------------------------
// Synchronous, like the passes: drains the updates in flight; it writes no plane and no stamp.
int fb_flow_learn_endpoints_dev(fb_ctx* c, const fb_view_query* q, fb_learned_endpoint* d_out, uint64_t cap,
                                uint64_t* d_n, fb_learn_stats* out, void* stream) {
    if (!c || !d_n || (cap && !d_out) || (reinterpret_cast<uintptr_t>(d_out) & 15u))
        return set_err(FB_ERR_INVAL, "ctx and d_n are required, d_out (16-B aligned) unless cap is 0");
    int rc = view_query_check(c, q);
    if (rc) return rc;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    rc = drain_updates(c);
    if (!rc && q->filter != FB_FILTER_ALL) rc = upload_cfg(c, s);  // the LAN configuration as of now
    if (rc) return rc;
    return learn_endpoints(view_args(c, q), c->plane<uint2>(kPlaneDom), c->proc_names(), c->learn_hash_mask, c->learn_slots,
                           c->learn_index, d_out, cap, (unsigned long long*)d_n, out, s);
}

// ---- Zeek conn.log export (fb_zeek.hip) -----------------------------------------------------------
static int format_zeek(fb_ctx* c, const fb_flow_view* d_views, uint64_t n, const uint8_t* d_hist,
                       const uint64_t* d_hist_off, uint64_t n_slots, bool by_record, uint8_t* d_text, uint64_t text_cap,
                       uint64_t* d_line_off, fb_zeek_stats* d_stats, void* stream) {
    if (!c || !d_views || !d_line_off || !d_stats)
        return set_err(FB_ERR_INVAL, "ctx, d_views, d_line_off and d_stats are required");
    if (d_hist && !d_hist_off) return set_err(FB_ERR_INVAL, "a history blob needs its offsets");
    if (text_cap && !d_text) return set_err(FB_ERR_INVAL, "d_text is NULL with text_cap %llu", (unsigned long long)text_cap);
    if (reinterpret_cast<uintptr_t>(d_views) & 15u) return set_err(FB_ERR_INVAL, "d_views must be 16-byte aligned");
    if (!c->timed) return set_err(FB_ERR_INVAL, "the Zeek export needs FB_CFG_TIMED (there is no clock to print)");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(fb_zeek_stats), s));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_line_off, 0, 8, s));
        return FB_OK;
    }
    // the scan's storage: shared by every call on the context, so each use waits for the one before it, and
    // a reallocation waits for that use on the host before the old buffer is freed
    size_t want = 0;
    HIP_TRY(zeek_scan_tmp_bytes(n, &want));
    const int rc = c->zeek_tmp.acquire(want, s, "Zeek export scan scratch");
    if (rc) return rc;
    ZeekArgs a;
    a.views = d_views;
    a.n = n;
    a.hist = d_hist;
    a.hist_off = reinterpret_cast<const unsigned long long*>(d_hist_off);
    a.n_slots = n_slots;
    a.by_record = by_record;
    a.text = d_text;
    a.cap = text_cap;
    a.off = reinterpret_cast<unsigned long long*>(d_line_off);
    a.stats = d_stats;
    HIP_TRY(launch_zeek(a, !c->zeek_direct, c->zeek_tmp.get(), c->zeek_tmp.capacity(), s));
    return c->zeek_tmp.release(s);
}

int fb_format_zeek_dev(fb_ctx* c, const fb_flow_view* d_views, uint64_t n, const uint8_t* d_hist,
                       const uint64_t* d_hist_off, uint64_t n_slots, uint8_t* d_text, uint64_t text_cap,
                       uint64_t* d_line_off, fb_zeek_stats* d_stats, void* stream) {
    return format_zeek(c, d_views, n, d_hist, d_hist_off, n_slots, false, d_text, text_cap, d_line_off, d_stats, stream);
}

int fb_format_zeek_hist_dev(fb_ctx* c, const fb_flow_view* d_views, uint64_t n, const uint8_t* d_hist,
                            const uint64_t* d_hist_off, uint8_t* d_text, uint64_t text_cap, uint64_t* d_line_off,
                            fb_zeek_stats* d_stats, void* stream) {
    return format_zeek(c, d_views, n, d_hist, d_hist_off, n, true, d_text, text_cap, d_line_off, d_stats, stream);
}

// ---- device-resident history (fb_histstore.hip) ---------------------------------------------------------
static int hs_ready(fb_ctx* c) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->hs) return set_err(FB_ERR_INVAL, "the history store is not enabled (fb_hist_store_enable)");
    return FB_OK;
}

int fb_hist_store_enable(fb_ctx* c, const fb_hist_store_config* cfg) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if (c->hs) return set_err(FB_ERR_INVAL, "the history store is already enabled");
    if (c->flow_batch != 0)
        return set_err(FB_ERR_INVAL, "the table has taken %u update calls since create / clear: their characters "
                       "are not known to the store", c->flow_batch);
    static const fb_hist_store_config kDefault = {};
    if (!cfg) cfg = &kDefault;
    if (cfg->flags || cfg->reserved[0] || cfg->reserved[1] || cfg->reserved[2])
        return set_err(FB_ERR_INVAL, "flags and reserved must be 0");
    DeviceGuard g(c->device);
    int rc = drain_updates(c);
    if (!rc) rc = plane_ensure(c, kPlaneHist, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    rc = histstore_create(&c->hs, cfg, c->grow, c->flow_recs);
    c->hs_updates = c->hs_seen = c->hs_applied = 0;
    return rc;
}

int fb_hist_store_append_dev(fb_ctx* c, void* stream) {
    int rc = hs_ready(c);
    if (rc) return rc;
    if (c->hs_seen == c->hs_updates) return FB_OK;  // this update has had its append (or there was none)
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    rc = join_updates(c, s);
    if (rc) return rc;
    const uint32_t n = c->last.live_slots();
    if (n == 0) return FB_OK;  // the update's slots have moved since (a purge): it stays a missed update
    // everything that can fail, wait or allocate comes before the first kernel (last_history's: before its own)
    rc = histstore_admit(c->hs, n, s);
    if (rc) return rc;
    if (flow_history_cnt_bytes(c->last.chunks) > c->d_hist_cnt.size() || c->flow_recs > histstore_scratch_slots(c->hs)) {
        rc = drain_updates(c);  // before either is reallocated (last_history grows the block counts)
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        rc = histstore_scratch(c->hs, c->flow_recs);
        if (rc) return rc;
    }
    rc = plane_ensure(c, kPlaneHist, s);  // (dropped by a purge whose move failed: every history starts again)
    if (rc) return rc;
    rc = last_history(c, histstore_run_slots(c->hs), histstore_run_chars(c->hs), histstore_run_count(c->hs), s, [&] {
        return histstore_append(c->hs, c->plane<uint4>(kPlaneHist), c->tb.cap, n, n, s);
    });
    if (rc) return rc;
    c->hs_seen = c->hs_updates;
    ++c->hs_applied;
    return FB_OK;
}

int fb_hist_store_lengths_dev(fb_ctx* c, const void* d_slots, uint64_t stride_bytes, uint64_t n, uint64_t* d_off,
                              void* stream) {
    int rc = hs_ready(c);
    if (rc) return rc;
    if (!d_off || (d_slots && (stride_bytes < 4 || (stride_bytes & 3u) || (reinterpret_cast<uintptr_t>(d_slots) & 3u))))
        return set_err(FB_ERR_INVAL, "d_off is required; d_slots and stride_bytes must be multiples of 4");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    rc = join_updates(c, s);
    if (rc) return rc;
    return histstore_lengths(c->hs, c->plane<uint4>(kPlaneHist), c->tb.cap, d_slots, stride_bytes, n, d_off, s);
}

int fb_hist_store_gather_dev(fb_ctx* c, const void* d_slots, uint64_t stride_bytes, uint64_t n, const uint64_t* d_off,
                             uint8_t* d_chars, uint64_t cap, void* stream) {
    int rc = hs_ready(c);
    if (rc) return rc;
    if (!d_off || (cap && !d_chars) ||
        (d_slots && (stride_bytes < 4 || (stride_bytes & 3u) || (reinterpret_cast<uintptr_t>(d_slots) & 3u))))
        return set_err(FB_ERR_INVAL, "d_off and d_chars are required; d_slots and stride_bytes must be multiples of 4");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    rc = join_updates(c, s);
    if (rc) return rc;
    return histstore_gather(c->hs, c->plane<uint4>(kPlaneHist), c->tb.cap, d_slots, stride_bytes, n, d_off, d_chars, cap, s);
}

int fb_hist_store_info_get(fb_ctx* c, fb_hist_store_info* info) {
    int rc = hs_ready(c);
    if (rc) return rc;
    if (!info) return set_err(FB_ERR_INVAL, "info is NULL");
    memset(info, 0, sizeof(*info));
    DeviceGuard g(c->device);
    rc = drain_updates(c);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());  // (appends run on the caller's streams)
    rc = histstore_info(c->hs, c->plane<uint4>(kPlaneHist), c->tb.cap, info, nullptr);
    info->appends = c->hs_applied;
    info->missed_updates = c->hs_updates - c->hs_applied;
    return rc;
}

// ---- multi-GPU merge (fb_merge.hip) ---------------------------------------------------------------
// The export, the routing and the merge share c->mscratch and may be called on different streams.
static constexpr const char* kMergeScratch = "merge scratch";

static int export_merge(fb_ctx* c, uint32_t world, uint32_t rank, uint64_t shard_first, const uint64_t* call_map,
                        uint32_t n_calls, fb_flow_mrec* d_out, uint64_t cap, uint64_t* d_counts, void* stream) {
    if (!c || !d_counts || (cap && !d_out)) return set_err(FB_ERR_INVAL, "ctx, d_counts and d_out are required");
    if (world == 0 || world > 64 || rank >= world) return set_err(FB_ERR_INVAL, "1 <= world <= 64, rank < world");
    if (!c->tb.slots) return set_err(FB_ERR_INVAL, "context was created without a flow table");
    if (call_map) {  // every position the table holds names a call below flow_batch
        if (n_calls < c->flow_batch)
            return set_err(FB_ERR_INVAL, "call map has %u entries, the table holds %u update calls", n_calls,
                           c->flow_batch);
        for (uint32_t k = 0; k < c->flow_batch; ++k) {
            const uint64_t gb = call_map[k] >> 32, first = call_map[k] & 0xFFFFFFFFull;
            if (gb >= 0xFFFFFFFFull || (k && gb <= (call_map[k - 1] >> 32)))
                return set_err(FB_ERR_INVAL, "call map: global batches must increase with the calls (call %u)", k);
            if (first + FB_MAX_BATCH_PACKETS > 0xFFFFFFFFull)
                return set_err(FB_ERR_INVAL, "call map: call %u's shard starts past 2^32 - FB_MAX_BATCH_PACKETS", k);
        }
    }
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t cnt_bytes = merge_export_scratch_bytes(c->tb.cap, world);
    int rc = join_updates(c, s);
    if (!rc) rc = c->mscratch.acquire(cnt_bytes + (call_map ? 8ull * std::max<uint32_t>(c->flow_batch, 1u) : 0ull), s, kMergeScratch);
    if (rc) return rc;
    unsigned long long* d_map = nullptr;
    if (call_map && c->flow_batch) {
        d_map = reinterpret_cast<unsigned long long*>(static_cast<char*>(c->mscratch.get()) + cnt_bytes);
        HIP_TRY(hipMemcpyAsync(d_map, call_map, 8ull * c->flow_batch, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(launch_merge_export(c->tb.slots, c->tb.char_call, c->tb.cap, world, rank, shard_first,
                                call_map ? d_map : nullptr, d_out, cap, (unsigned long long*)d_counts,
                                c->mscratch.get(), s));
    return c->mscratch.release(s);
}

int fb_flow_export_merge_dev(fb_ctx* c, uint32_t world, uint32_t rank, uint64_t shard_first, fb_flow_mrec* d_out,
                             uint64_t cap, uint64_t* d_counts, void* stream) {
    if (shard_first + FB_MAX_BATCH_PACKETS > 0xFFFFFFFFull)
        return set_err(FB_ERR_INVAL, "shard_first past 2^32 - FB_MAX_BATCH_PACKETS");
    return export_merge(c, world, rank, shard_first, nullptr, 0u, d_out, cap, d_counts, stream);
}

int fb_flow_export_merge_map_dev(fb_ctx* c, uint32_t world, uint32_t rank, const uint64_t* call_map, uint32_t n_calls,
                                 fb_flow_mrec* d_out, uint64_t cap, uint64_t* d_counts, void* stream) {
    if (!call_map && n_calls) return set_err(FB_ERR_INVAL, "call_map is NULL");
    if (!call_map) {  // (a table that took no update call holds no flow)
        static const uint64_t none = 0ull;
        call_map = &none;
    }
    return export_merge(c, world, rank, 0ull, call_map, n_calls, d_out, cap, d_counts, stream);
}

int fb_route_records_dev(fb_ctx* c, const fb_pkt_out* d_recs, const fb_batch_stats* d_stats, uint32_t max_n,
                         uint32_t world, uint64_t shard_first, const uint64_t* d_ts, fb_pkt_out* d_out,
                         uint64_t* d_ts_out, uint64_t* d_counts, void* stream) {
    if (!c || !d_stats || !d_counts || (max_n && (!d_recs || !d_out)))
        return set_err(FB_ERR_INVAL, "ctx, d_stats, d_counts, d_recs and d_out are required");
    if (world == 0 || world > 64) return set_err(FB_ERR_INVAL, "1 <= world <= 64");
    if (max_n > FB_MAX_BATCH_PACKETS) return set_err(FB_ERR_INVAL, "max_n > FB_MAX_BATCH_PACKETS");
    if (shard_first + FB_MAX_BATCH_PACKETS > 0xFFFFFFFFull) return set_err(FB_ERR_INVAL, "shard_first too large");
    if ((d_ts == nullptr) != (d_ts_out == nullptr)) return set_err(FB_ERR_INVAL, "d_ts and d_ts_out go together");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int rc = c->mscratch.acquire(route_scratch_bytes(max_n, world), s, kMergeScratch);
    if (rc) return rc;
    HIP_TRY(launch_route(d_recs, d_stats, max_n, world, shard_first, reinterpret_cast<const unsigned long long*>(d_ts),
                         d_out, reinterpret_cast<unsigned long long*>(d_ts_out), (unsigned long long*)d_counts,
                         c->mscratch.get(), s));
    return c->mscratch.release(s);
}

int fb_flow_merge_dev(fb_ctx* c, const fb_flow_mrec* d_in, uint64_t n, fb_flow_rec* d_out, uint64_t* d_n,
                      void* stream) {
    if (!c || !d_n || (n && (!d_in || !d_out))) return set_err(FB_ERR_INVAL, "ctx, d_in, d_out and d_n are required");
    if (n >= 0xFFFFFFFFull) return set_err(FB_ERR_INVAL, "n %llu >= 2^32", (unsigned long long)n);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int rc = c->mscratch.acquire(n ? merge_scratch_bytes(n) : 0, s, kMergeScratch);
    if (rc) return rc;
    HIP_TRY(launch_merge(d_in, n, d_out, (unsigned long long*)d_n, c->mscratch.get(), s));
    return c->mscratch.release(s);
}

int fb_flow_export_sessions(fb_ctx* c, uint32_t filter, fb_flow_rec* out, uint64_t cap, uint64_t* n, void* stream) {
    if (!c || !n || (cap && !out) || filter > FB_FILTER_ALL) return set_err(FB_ERR_INVAL, "bad arguments");
    *n = 0;
    if (!c->tb.slots || cap == 0) return FB_OK;
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    uint64_t total = 0;
    const int rc = fb_flow_count(c, &total, stream);
    if (rc) return rc;
    const uint64_t m = std::min(total, cap);
    if (m == 0) return FB_OK;
    return export_to_host(c, out, m, sizeof(fb_flow_rec), n, s, "flow export", [&](void* d_out) {
        return fb_flow_export_sessions_dev(c, filter, (fb_flow_rec*)d_out, m, reinterpret_cast<uint64_t*>(c->d_n.get()), stream);
    });
}

int fb_flow_export(fb_ctx* c, fb_flow_rec* out, uint64_t cap, uint64_t* n, void* stream) {
    return fb_flow_export_sessions(c, FB_FILTER_ALL, out, cap, n, stream);
}

int fb_flow_table_info_get(fb_ctx* c, fb_flow_table_info* info) {
    if (!c || !info) return set_err(FB_ERR_INVAL, "bad arguments");
    memset(info, 0, sizeof(*info));
    if (!c->tb.slots) return FB_OK;
    info->capacity = c->tb.cap;
    info->partitions = c->tb.parts;
    info->generation = c->generation;
    const volatile FlowMailbox* m = c->mbox;
    const uint64_t seq = __atomic_load_n(&m->seq, __ATOMIC_ACQUIRE);
    if (seq && seq > c->clear_seq) {
        info->flows = m->flows;
        info->max_partition = m->max_part;
    }
    return FB_OK;
}

int fb_flow_slot_remap(fb_ctx* c, uint32_t* old_to_new, uint64_t cap, uint64_t* n) {
    if (!c || !n || (cap && !old_to_new)) return set_err(FB_ERR_INVAL, "bad arguments");
    *n = 0;
    if (!c->d_remap) return FB_OK;
    DeviceGuard g(c->device);
    const uint64_t m = std::min<uint64_t>(cap, c->d_remap.size());
    if (m) HIP_TRY(hipMemcpy(old_to_new, c->d_remap, m * 4ull, hipMemcpyDeviceToHost));
    *n = m;
    return FB_OK;
}

int fb_flow_clear(fb_ctx* c, void* stream) {
    if (!c) return set_err(FB_ERR_INVAL, "ctx is NULL");
    if (!c->tb.slots) return FB_OK;
    DeviceGuard g(c->device);
    int rc = join_updates(c, (hipStream_t)stream);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->tb.slots, 0, c->tb.cap * sizeof(FlowSlot), (hipStream_t)stream));
    rc = planes_clear(c, (hipStream_t)stream);
    if (!rc && c->hs) rc = histstore_clear(c->hs, (hipStream_t)stream);  // (the plane went with planes_clear)
    if (rc) return rc;
    c->flow_batch = 0;
    c->clear_seq = c->upd_seq;
    c->last.invalidate();
    return FB_OK;
}

// ---- device-memory helpers -------------------------------------------------------------
int fb_dev_alloc(void** p, uint64_t bytes) {
    if (!p) return set_err(FB_ERR_INVAL, "p is NULL");
    *p = nullptr;
    if (hipMalloc(p, bytes ? bytes : 1) != hipSuccess) return set_err(FB_ERR_NOMEM, "hipMalloc(%llu)", (unsigned long long)bytes);
    return FB_OK;
}
int fb_dev_free(void* p) { HIP_TRY(hipFree(p)); return FB_OK; }
int fb_host_alloc_pinned(void** p, uint64_t bytes) {
    if (!p) return set_err(FB_ERR_INVAL, "p is NULL");
    *p = nullptr;
    if (hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess)
        return set_err(FB_ERR_NOMEM, "hipHostMalloc(%llu)", (unsigned long long)bytes);
    return FB_OK;
}
int fb_host_free_pinned(void* p) { HIP_TRY(hipHostFree(p)); return FB_OK; }
int fb_memcpy_h2d(void* d, const void* s, uint64_t b, void* st) {
    HIP_TRY(hipMemcpyAsync(d, s, b, hipMemcpyHostToDevice, (hipStream_t)st));
    return FB_OK;
}
int fb_memcpy_d2h(void* d, const void* s, uint64_t b, void* st) {
    HIP_TRY(hipMemcpyAsync(d, s, b, hipMemcpyDeviceToHost, (hipStream_t)st));
    return FB_OK;
}
int fb_memset_dev(void* d, int v, uint64_t b, void* st) {
    HIP_TRY(hipMemsetAsync(d, v, b, (hipStream_t)st));
    return FB_OK;
}
int fb_stream_create(void** st) {
    if (!st) return set_err(FB_ERR_INVAL, "NULL");
    HIP_TRY(hipStreamCreateWithFlags((hipStream_t*)st, hipStreamNonBlocking));
    return FB_OK;
}
int fb_stream_destroy(void* st) { HIP_TRY(hipStreamDestroy((hipStream_t)st)); return FB_OK; }
int fb_stream_sync(void* st) { HIP_TRY(hipStreamSynchronize((hipStream_t)st)); return FB_OK; }
int fb_event_create(void** ev) {
    if (!ev) return set_err(FB_ERR_INVAL, "NULL");
    HIP_TRY(hipEventCreate((hipEvent_t*)ev));
    return FB_OK;
}
int fb_event_destroy(void* ev) { HIP_TRY(hipEventDestroy((hipEvent_t)ev)); return FB_OK; }
int fb_event_record(void* ev, void* st) { HIP_TRY(hipEventRecord((hipEvent_t)ev, (hipStream_t)st)); return FB_OK; }
int fb_event_elapsed_ms(float* ms, void* a, void* b) {
    if (!ms) return set_err(FB_ERR_INVAL, "NULL");
    HIP_TRY(hipEventSynchronize((hipEvent_t)b));
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
    return FB_OK;
}
int fb_event_query(void* ev) {
    const hipError_t e = hipEventQuery((hipEvent_t)ev);
    if (e == hipErrorNotReady) return 1;
    HIP_TRY(e);
    return FB_OK;
}
// Busy-wait (no blocking sync, no wake-up latency) until the event completed.
int fb_event_spin(void* ev) {
    for (;;) {
        const hipError_t e = hipEventQuery((hipEvent_t)ev);
        if (e == hipSuccess) return FB_OK;
        if (e != hipErrorNotReady) HIP_TRY(e);
    }
}
int fb_set_device(int d) { HIP_TRY(hipSetDevice(d)); return FB_OK; }

}  // extern "C"
