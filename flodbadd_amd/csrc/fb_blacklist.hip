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
// The words live in a plane of their own, one per table slot, like the status plane of fb_age.hip and
// the state plane of fb_whitelist.hip: FlowSlot and the update kernels are untouched, and a zero word
// (no pass has seen the flow) is the reference's insert state, an empty criticality.
#include "fb_internal.h"

namespace fbk {

// k_flow_whitelist's geometry: one lane per table slot, 256-thread workgroups striding over the table.
// Per occupied slot one 128-B line of the table (tag, key and hist_state are all in it) and the old
// mask word; the two interval searches advance in one loop, so each step has both probes in flight
// (flow_lookups of fb_enrich.hip without its ASN half).  The word is stored only when it changed.
// kMark (FB_BL_MARK_WHITELIST): a flow with a non-zero mask whose whitelist state byte is 0 (Unknown)
// gets FB_WL_NONCONFORMING | FB_WL_BLACKLISTED; no other byte of that plane is read or written.
// Counters as in k_flow_whitelist: a ballot per counter per step, one atomic per counter per workgroup.
template <bool kMark>
__global__ __launch_bounds__(256) void k_flow_blacklist(const EnrichTables t, const FlowSlot* T, unsigned long long cap,
                                                        unsigned long long* mask, uint8_t* wl,
                                                        unsigned long long* stats) {
    __shared__ uint32_t s_cnt[4][kBlCounters];
    uint32_t cnt[kBlCounters] = {0u, 0u, 0u, 0u, 0u, 0u};  // wave-uniform
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
        }
        cnt[0] += (uint32_t)__popcll(__ballot(occ));
        cnt[1] += (uint32_t)__popcll(__ballot(nw != 0ull));
        cnt[2] += (uint32_t)__popcll(__ballot(nw != old));
        cnt[3] += (uint32_t)__popcll(__ballot(old == 0ull && nw != 0ull));
        cnt[4] += (uint32_t)__popcll(__ballot(old != 0ull && nw == 0ull));
        cnt[5] += (uint32_t)__popcll(__ballot(marked));
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u)
        for (uint32_t k = 0; k < kBlCounters; ++k) s_cnt[wave][k] = cnt[k];
    __syncthreads();
    if (threadIdx.x < kBlCounters) {  // one atomic per counter per workgroup
        const unsigned long long s = (unsigned long long)s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] +
                                     s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (s) atomicAdd(stats + threadIdx.x, s);
    }
}

// k_flow_export (fb_flow.hip) with "the mask word is not zero" as the predicate: a ballot, one atomic
// per block, slot order inside a block's step.  out_masks (may be null): the word beside each record.
__global__ __launch_bounds__(256) void k_flow_export_blacklisted(const FlowSlot* T, const unsigned long long* mask,
                                                                 unsigned long long cap, fb_flow_rec* out,
                                                                 unsigned long long* out_masks,
                                                                 unsigned long long out_cap, unsigned long long* d_n,
                                                                 const FlowTime* plane) {
    __shared__ unsigned long long sh[4];
    __shared__ unsigned long long s_base;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < cap; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        unsigned long long w = 0ull;
        if (i < cap && T[i].tag >= 2u) w = mask[i];
        const bool take = w != 0ull;
        const unsigned long long m = __ballot(take);
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        if (lane == 0u) sh[wave] = __popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long tot = sh[0] + sh[1] + sh[2] + sh[3];
            s_base = tot ? atomicAdd(d_n, tot) : 0ull;
        }
        __syncthreads();
        unsigned long long pos = s_base + __popcll(m & ((1ull << lane) - 1ull));
        for (uint32_t v = 0; v < wave; ++v) pos += sh[v];
        if (take && pos < out_cap) {
            fb_flow_rec r = flow_rec_of(T[i], (uint32_t)i);
            if (plane) {  // a timed context: the segment state with the 5-s timeout (fb_time.hip)
                r.segment_count = plane[i].segment_count;
                r.in_segment = plane[i].in_segment;
            }
            out[pos] = r;
            if (out_masks) out_masks[pos] = w;
        }
        __syncthreads();
    }
}

#ifndef FB_BL_GRID
#define FB_BL_GRID 1024ull  // eight steps per thread at 2^21 slots: the steady C4 call takes 125 us, against 130 at
                            // 2048 and 161 at 8192 (k_flow_enrich's grid) -- every workgroup ends with six
                            // atomics on the same six words ("Blacklist pass")
#endif
hipError_t launch_flow_blacklist(const EnrichTables& t, const FlowSlot* table, unsigned long long cap,
                                 unsigned long long* mask, uint8_t* wl, unsigned long long* stats, hipStream_t s) {
    if (!table || !mask || !stats || cap == 0ull) return hipErrorInvalidValue;
    if ((t.m4 && (!t.bl4_pos || !t.bl4_mask)) || (t.m6 && (!t.bl6_pos || !t.bl6_mask))) return hipErrorInvalidValue;
    unsigned long long g = (cap + 255ull) / 256ull;
    if (g > FB_BL_GRID) g = FB_BL_GRID;
    if (wl)
        hipLaunchKernelGGL(k_flow_blacklist<true>, dim3((uint32_t)g), dim3(256), 0, s, t, table, cap, mask, wl, stats);
    else
        hipLaunchKernelGGL(k_flow_blacklist<false>, dim3((uint32_t)g), dim3(256), 0, s, t, table, cap, mask, wl, stats);
    return hipGetLastError();
}

hipError_t launch_flow_export_blacklisted(const FlowSlot* table, const unsigned long long* mask, unsigned long long cap,
                                          fb_flow_rec* out, unsigned long long* out_masks, unsigned long long out_cap,
                                          unsigned long long* d_n, const FlowTime* plane, hipStream_t s) {
    if (!table || !mask || !d_n || (out_cap && !out)) return hipErrorInvalidValue;
    unsigned long long g = (cap + 255ull) / 256ull;
    if (g > 1024ull) g = 1024ull;
    if (g == 0ull) g = 1ull;
    hipLaunchKernelGGL(k_flow_export_blacklisted, dim3((uint32_t)g), dim3(256), 0, s, table, mask, cap, out, out_masks,
                       out_cap, d_n, plane);
    return hipGetLastError();
}

}  // namespace fbk
