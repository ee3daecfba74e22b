// fb_whitelist.hip -- whitelist conformance of every flow of the table (fb_flow_whitelist): the
// reference's recompute_whitelist_for_sessions (src/whitelists.rs:810-1023), i.e. is_session_in_whitelist
// / endpoint_matches_with_reason (src/whitelists.rs:341-732) per session, for a session whose dst_domain
// and l7 are None.  The reference scans the whole endpoint list per session; a whitelist learned from the
// table (Whitelists::new_from_sessions, src/whitelists.rs:103-177: one exact-address endpoint per distinct
// (dst_ip, dst_port, protocol)) against that table is flows x endpoints tests.  Here the list is indexed
// by the host (build_whitelist_index; it, the structures and the evaluation of one flow are fb_wl_match.h's,
// one definition for these kernels and for host programs), and a flow
// costs one table read, four searches of the small group table and one search of the sorted addresses.
//
// The verdict is a boolean over the endpoints -- "some endpoint matches" --, so neither the reference's
// first-match order nor duplicates matter, and the index is free to reorder and deduplicate.
//
// The state lives in a per-slot plane of its own, one byte per table slot (FB_WL_*):
// FlowSlot and the update kernels are untouched.
#include "fb_internal.h"

namespace fbk {

namespace {

// dst_asn of a flow for wl_eval (src/packets.rs:468-485): Db::lookup of the destination unless it is a LAN
// address under the context's current configuration; the record's interned owner / country.
struct WlAsnDev {
    const WlTables& W;
    const EnrichTables& E;
    const DevConfig* cfg;
    __device__ __forceinline__ bool operator()(const uint32_t dst[4], bool v6, uint32_t& as_number, uint32_t& owner,
                                               uint32_t& country) const {
        const bool lan = v6 ? lan_v6(cfg, cfg, dst) : lan_v4(dst[0]);
        const fb_asn_range* A = v6 ? E.asn6 : E.asn4;
        const int32_t i = lan ? -1 : asn_find(A, v6 ? E.n6 : E.n4, dst, v6);
        if (i < 0) return false;
        as_number = A[i].as_number;
        const uint32_t rec = A[i].record;
        if (rec < W.n_records) {
            owner = W.rec_owner[rec];
            country = W.rec_country[rec];
        }
        return true;
    }
};

}  // namespace

// k_flow_enrich's geometry: one lane per table slot, 256-thread workgroups striding over the table.
// kStaged: the group table and the rules fit kWlLdsGroups / kWlLdsRules and every workgroup copies them
// into LDS once (coalesced), so the per-lane group searches and rule scans -- divergent addresses --
// stay on the CU.  Otherwise they are read from global memory (L2).
// kStamp (a pass time is set, fb_set_pass_time): the flows whose byte changed get `now` in the stamp plane
// (src/whitelists.rs:975-982); the unstamped instances hold no such store.
// kProc (the list has process ids, WlIndex::with_proc): the flow's process_match_id -- the L7 plane's element,
// then the name table: one dependent load pair, issued before the group searches so it is in flight with them
// -- gates the process endpoints (fb_wl_match.h).  The other instances read neither.
// kDom (the list has domain pattern ids, WlTables::nd): the flow's dst_name_id -- the domain plane's element --
// names the match row of its destination name (fb_wl_domain.hip), which decides the domain endpoints with an id
// (fb_wl_match.h); a sixth counter takes the flows left to the host because their row overflowed.  The other
// instances read neither the plane nor the rows.
// Counters: PassCounters (fb_internal.h).
template <bool kStaged, bool kStamp, bool kProc, bool kDom>
__global__ __launch_bounds__(256) void k_flow_whitelist(const WlTables W, const EnrichTables E, const DevConfig* cfg,
                                                        const FlowSlot* T, unsigned long long cap, uint8_t* state,
                                                        unsigned long long* stats, unsigned long long* mod,
                                                        unsigned long long now, const WlProcNames P, const WlDomFlows D) {
    __shared__ uint32_t s_gkey[kStaged ? kWlLdsGroups : 1u];
    __shared__ uint32_t s_gbeg[kStaged ? kWlLdsGroups + 1u : 1u];
    __shared__ uint4 s_rules[kStaged ? kWlLdsRules * 3u : 1u];
    if (kStaged) {
        for (uint32_t j = threadIdx.x; j < W.ng; j += 256u) s_gkey[j] = W.gkey[j];
        for (uint32_t j = threadIdx.x; j < W.ng + 1u; j += 256u) s_gbeg[j] = W.gbeg[j];
        const uint4* src = reinterpret_cast<const uint4*>(W.rules);
        for (uint32_t j = threadIdx.x; j < W.nr * 3u; j += 256u) s_rules[j] = src[j];
        __syncthreads();
    }
    PassCounters<kDom ? kWlCounters : kWlCounters - 1u> cnt;
    const WlAsnDev asn = {W, E, cfg};
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < cap; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        const bool occ = i < cap && T[i].tag >= 2u;
        uint32_t nb = 0u, old = 0u;
        bool over = false;
        if (occ) {
            old = state[i];
            const uint32_t pm = kProc ? wl_flow_match_id(P, i) : 0u;
            const uint32_t* row = nullptr;
            uint32_t rflags = 0u;
            if (kDom && D.plane) {  // (an id is never past the matched names: the call matched them first)
                const uint32_t nid = D.plane[i].dst_name_id;
                if (nid != 0u && nid <= D.n_names) {
                    row = D.rows + (unsigned long long)nid * FB_WL_NAME_MATCHES;
                    rflags = D.flags[nid];
                }
            }
            if (kStaged)
                nb = wl_eval<kProc, kDom>(W, asn, s_gkey, s_gbeg, reinterpret_cast<const WlRule*>(s_rules), T[i].key, pm,
                                          P.n != 0u, row, rflags, &over);
            else
                nb = wl_eval<kProc, kDom>(W, asn, W.gkey, W.gbeg, W.rules, T[i].key, pm, P.n != 0u, row, rflags, &over);
            if (nb != old) state[i] = (uint8_t)nb;
            if (kStamp && nb != old) mod[i] = now;
        }
        cnt.add(0, occ);
        cnt.add(1, (nb & FB_WL_CONFORMING) != 0u);
        cnt.add(2, (nb & FB_WL_NONCONFORMING) != 0u);
        cnt.add(3, (nb & FB_WL_HOST_CHECK) != 0u);
        cnt.add(4, occ && nb != old);
        if (kDom) cnt.add(5, over);
    }
    cnt.flush(stats);
}

// The flows whose state byte state_mask selects (FB_WL_MASK_UNKNOWN: a zero byte, or no plane yet).
__global__ __launch_bounds__(256) void k_flow_export_whitelist(const FlowSlot* T, const uint8_t* state,
                                                               unsigned long long cap, uint32_t state_mask,
                                                               fb_flow_rec* out, unsigned long long out_cap,
                                                               unsigned long long* d_n, const FlowTime* plane) {
    sweep_compact(
        cap, out_cap, d_n,
        [=](unsigned long long i) {
            if (T[i].tag < 2u) return false;
            const uint32_t b = state ? state[i] : 0u;
            return b ? (b & state_mask & 0x7Fu) != 0u : (state_mask & FB_WL_MASK_UNKNOWN) != 0u;
        },
        [=](unsigned long long i, unsigned long long pos, bool) { out[pos] = flow_rec_at(T, plane, i); });
}

#ifndef FB_WL_GRID
#define FB_WL_GRID 2048ull  // the staging copy (<= 28 KiB per workgroup) is paid once per workgroup
#endif
hipError_t launch_flow_whitelist(const WlTables& w, const EnrichTables& t, const DevConfig* cfg, const FlowSlot* table,
                                 unsigned long long cap, uint8_t* state, unsigned long long* stats, hipStream_t s,
                                 unsigned long long* mod, unsigned long long now, bool with_proc,
                                 const WlProcNames& names, const WlDomFlows* dom) {
    if (!table || !state || !stats || !cfg || cap == 0ull) return hipErrorInvalidValue;
    if ((w.ng && (!w.gkey || !w.gbeg)) || (w.nr && !w.rules) || (w.n_records && (!w.rec_owner || !w.rec_country)))
        return hipErrorInvalidValue;
    if (with_proc ? ((w.n4 && (!w.a4 || !w.kp4)) || (w.n6 && (!w.a6 || !w.kp6)) ||
                     (names.n && (!names.match_id || !names.name_id)))
                  : ((w.n4 && (!w.a4 || !w.k4)) || (w.n6 && (!w.a6 || !w.k6))))
        return hipErrorInvalidValue;
    if (dom && (!w.nd || !w.dpid || !w.dkp || (dom->n_names && (!dom->rows || !dom->flags)))) return hipErrorInvalidValue;
    const dim3 g(sweep_grid(cap, FB_WL_GRID));
    const bool staged = w.ng <= kWlLdsGroups && w.nr <= kWlLdsRules && w.ng;
    // (a list without process ids runs the kProc false instances with an empty name table, one without pattern
    // ids the kDom false ones with an empty WlDomFlows: the instances of before)
    const WlProcNames pn = with_proc ? names : WlProcNames();
    const WlDomFlows df = dom ? *dom : WlDomFlows();
    const uint32_t inst = (staged ? 8u : 0u) | (mod ? 4u : 0u) | (with_proc ? 2u : 0u) | (dom ? 1u : 0u);
    decltype(&k_flow_whitelist<false, false, false, false>) k = nullptr;
    switch (inst) {
#define FB_WL_INSTANCE(n, a, b, c, d) case n: k = k_flow_whitelist<a, b, c, d>; break;
        FB_WL_INSTANCE(0, false, false, false, false)
        FB_WL_INSTANCE(1, false, false, false, true)
        FB_WL_INSTANCE(2, false, false, true, false)
        FB_WL_INSTANCE(3, false, false, true, true)
        FB_WL_INSTANCE(4, false, true, false, false)
        FB_WL_INSTANCE(5, false, true, false, true)
        FB_WL_INSTANCE(6, false, true, true, false)
        FB_WL_INSTANCE(7, false, true, true, true)
        FB_WL_INSTANCE(8, true, false, false, false)
        FB_WL_INSTANCE(9, true, false, false, true)
        FB_WL_INSTANCE(10, true, false, true, false)
        FB_WL_INSTANCE(11, true, false, true, true)
        FB_WL_INSTANCE(12, true, true, false, false)
        FB_WL_INSTANCE(13, true, true, false, true)
        FB_WL_INSTANCE(14, true, true, true, false)
        FB_WL_INSTANCE(15, true, true, true, true)
#undef FB_WL_INSTANCE
    }
    hipLaunchKernelGGL(k, g, dim3(256), 0, s, w, t, cfg, table, cap, state, stats, mod, now, pn, df);
    return hipGetLastError();
}

hipError_t launch_flow_export_whitelist(const FlowSlot* table, const uint8_t* state, unsigned long long cap,
                                        uint32_t state_mask, fb_flow_rec* out, unsigned long long out_cap,
                                        unsigned long long* d_n, const FlowTime* plane, hipStream_t s) {
    hipLaunchKernelGGL(k_flow_export_whitelist, dim3(sweep_grid(cap, 1024ull)), dim3(256), 0, s, table, state, cap,
                       state_mask, out, out_cap, d_n, plane);
    return hipGetLastError();
}

}  // namespace fbk
