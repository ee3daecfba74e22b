// fb_blacklist.hip -- the blacklist pass over every flow of the table (fb_flow_blacklist): the
// reference's recompute_blacklist_for_sessions (src/blacklists.rs:456-731) and the "Session is
// blacklisted" fallback that follows it in update_sessions_internal (src/capture.rs:1858-1871).
//
// The reference collects, per session, the names of the lists one of whose ranges contains the source
// or the destination address -- an address whose is_local flag was set AT INSERT is left out
// (snapshot.is_local_src / _dst, src/blacklists.rs:547-551, 596-606) --, sorts and de-duplicates them
// and writes them into `criticality` as "blacklist:<name>" tags.  The set of names is the union of the
// two addresses' list masks (bl_lookup over fb_set_blacklists' elementary intervals), so one 64-bit
// word per flow is the whole answer; the host turns it into the strings.
//
// The words live in a per-slot plane of their own: FlowSlot and the update kernels are
// untouched, and a zero word (no pass has seen the flow) is the reference's insert state, an empty
// criticality.
#include "fb_internal.h"

namespace fbk {

// k_flow_whitelist's geometry: one lane per table slot, 256-thread workgroups striding over the table.
// Per occupied slot one 128-B line of the table (tag, key and hist_state are all in it) and the old
// mask word; the two interval searches advance in one loop, so each step has both probes in flight
// (flow_lookups of fb_enrich.hip without its ASN half).  The word is stored only when it changed.
// kMark (FB_BL_MARK_WHITELIST): a flow with a non-zero mask whose whitelist state byte is 0 (Unknown)
// gets FB_WL_NONCONFORMING | FB_WL_BLACKLISTED; no other byte of that plane is read or written.
// kStamp (a pass time is set, fb_set_pass_time): the flows whose word changed, and those the fallback
// marked, get `now` in the stamp plane -- the reference's last_modified bumps (src/blacklists.rs:655-689,
// src/capture.rs:1867-1868).  The unstamped instances hold no such store.
// Counters: PassCounters (fb_internal.h).
template <bool kMark, bool kStamp>
__global__ __launch_bounds__(256) void k_flow_blacklist(const EnrichTables t, const FlowSlot* T, unsigned long long cap,
                                                        unsigned long long* mask, uint8_t* wl,
                                                        unsigned long long* stats, unsigned long long* mod,
                                                        unsigned long long now) {
    PassCounters<kBlCounters> cnt;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < cap; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        const bool occ = i < cap && T[i].tag >= 2u;
        unsigned long long nw = 0ull, old = 0ull;
        bool marked = false;
        if (occ) {
            const uint32_t* k = T[i].key;
            const uint32_t src[4] = {k[0], k[1], k[2], k[3]}, dst[4] = {k[4], k[5], k[6], k[7]};
            const bool v6 = ((k[9] >> 8) & 0xFFu) == 10u;
            const uint32_t st = T[i].hist_state;  // the flags stored at insert, not the current LAN set
            old = mask[i];
            const uint32_t n = v6 ? t.m6 : t.m4;
            uint32_t lo0 = 0u, hi0 = (st & kStateLocalSrc) ? 0u : n, lo1 = 0u, hi1 = (st & kStateLocalDst) ? 0u : n;
            for (;;) {
                const bool on0 = lo0 < hi0, on1 = lo1 < hi1;
                if (!(on0 || on1)) break;
                const uint32_t m0 = (lo0 + hi0) >> 1, m1 = (lo1 + hi1) >> 1;
                uint4 p0 = make_uint4(0u, 0u, 0u, 0u), p1 = p0;
                if (on0) p0 = bl_probe(t, v6, m0);
                if (on1) p1 = bl_probe(t, v6, m1);
                if (on0) bl_step(src, v6, p0, m0, lo0, hi0);
                if (on1) bl_step(dst, v6, p1, m1, lo1, hi1);
            }
            // (a skipped search ends with lo = 0: no interval, mask 0)
            nw = bl_mask_at(t, v6, lo0) | bl_mask_at(t, v6, lo1);
            if (nw != old) mask[i] = nw;
            if (kMark && nw != 0ull && wl[i] == 0u) {
                wl[i] = (uint8_t)(FB_WL_NONCONFORMING | FB_WL_BLACKLISTED);
                marked = true;
            }
            if (kStamp && (nw != old || marked)) mod[i] = now;
        }
        cnt.add(0, occ);
        cnt.add(1, nw != 0ull);
        cnt.add(2, nw != old);
        cnt.add(3, old == 0ull && nw != 0ull);
        cnt.add(4, old != 0ull && nw == 0ull);
        cnt.add(5, marked);
    }
    cnt.flush(stats);
}

// The flows whose mask word is not zero; out_masks (may be null): the word beside each record.
__global__ __launch_bounds__(256) void k_flow_export_blacklisted(const FlowSlot* T, const unsigned long long* mask,
                                                                 unsigned long long cap, fb_flow_rec* out,
                                                                 unsigned long long* out_masks,
                                                                 unsigned long long out_cap, unsigned long long* d_n,
                                                                 const FlowTime* plane) {
    sweep_compact(
        cap, out_cap, d_n, [=](unsigned long long i) { return T[i].tag >= 2u ? mask[i] : 0ull; },
        [=](unsigned long long i, unsigned long long pos, unsigned long long w) {
            out[pos] = flow_rec_at(T, plane, i);
            if (out_masks) out_masks[pos] = w;
        });
}

#ifndef FB_BL_GRID
#define FB_BL_GRID 1024ull  // eight steps per thread at 2^21 slots: the steady C4 call takes 125 us, against 130 at
                            // 2048 and 161 at 8192 (k_flow_enrich's grid) -- every workgroup ends with six
                            // atomics on the same six words ("Blacklist pass")
#endif
hipError_t launch_flow_blacklist(const EnrichTables& t, const FlowSlot* table, unsigned long long cap,
                                 unsigned long long* mask, uint8_t* wl, unsigned long long* stats, hipStream_t s,
                                 unsigned long long* mod, unsigned long long now) {
    if (!table || !mask || !stats || cap == 0ull) return hipErrorInvalidValue;
    if ((t.m4 && (!t.bl4_pos || !t.bl4_mask)) || (t.m6 && (!t.bl6_pos || !t.bl6_mask))) return hipErrorInvalidValue;
    const dim3 g(sweep_grid(cap, FB_BL_GRID));
    const auto k = wl ? (mod ? k_flow_blacklist<true, true> : k_flow_blacklist<true, false>)
                      : (mod ? k_flow_blacklist<false, true> : k_flow_blacklist<false, false>);
    hipLaunchKernelGGL(k, g, dim3(256), 0, s, t, table, cap, mask, wl, stats, mod, now);
    return hipGetLastError();
}

hipError_t launch_flow_export_blacklisted(const FlowSlot* table, const unsigned long long* mask, unsigned long long cap,
                                          fb_flow_rec* out, unsigned long long* out_masks, unsigned long long out_cap,
                                          unsigned long long* d_n, const FlowTime* plane, hipStream_t s) {
    if (!table || !mask || !d_n || (out_cap && !out)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_flow_export_blacklisted, dim3(sweep_grid(cap, 1024ull)), dim3(256), 0, s, table, mask, cap,
                       out, out_masks, out_cap, d_n, plane);
    return hipGetLastError();
}

}  // namespace fbk
