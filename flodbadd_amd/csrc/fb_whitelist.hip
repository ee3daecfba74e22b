// fb_whitelist.hip -- whitelist conformance of every flow of the table (fb_flow_whitelist): the
// reference's recompute_whitelist_for_sessions (src/whitelists.rs:810-1023), i.e. is_session_in_whitelist
// / endpoint_matches_with_reason (src/whitelists.rs:341-732) per session, for a session whose dst_domain
// and l7 are None.  The reference scans the whole endpoint list per session; a whitelist learned from the
// table (Whitelists::new_from_sessions, src/whitelists.rs:103-177: one exact-address endpoint per distinct
// (dst_ip, dst_port, protocol)) against that table is flows x endpoints tests.  Here the list is indexed
// by the host (build_whitelist_index below; the structures are described in fb_internal.h), and a flow
// costs one table read, four searches of the small group table and one search of the sorted addresses.
//
// The verdict is a boolean over the endpoints -- "some endpoint matches" --, so neither the reference's
// first-match order nor duplicates matter, and the index is free to reorder and deduplicate.
//
// The state lives in a per-slot plane of its own, one byte per table slot (FB_WL_*):
// FlowSlot and the update kernels are untouched.
#include <algorithm>

#include "fb_internal.h"

namespace fbk {

namespace {

// The index of `key` in the ascending keys[lo, hi) (bit 31 of an entry is not part of it), or ~0u.
__device__ __forceinline__ uint32_t find_key(const uint32_t* keys, uint32_t lo, uint32_t hi, uint32_t key) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1, v = keys[mid] & ~kWlGroupHostCheck;
        if (v == key) return mid;
        if (v < key) lo = mid + 1u;
        else hi = mid;
    }
    return ~0u;
}

// Some exact-address endpoint has the destination and one of the flow's four keys: the run of the
// address in the sorted array (its lower and upper bound, advanced together so each step has both
// probes in flight; they coincide until the searches part), then the keys inside the run.
template <bool kV6>
__device__ __forceinline__ bool exact_match(const WlTables& W, const uint32_t ip[4], const uint32_t keys[4]) {
    const uint32_t n = kV6 ? W.n6 : W.n4;
    uint32_t lo = 0u, hi = n, lo2 = 0u, hi2 = n;  // first address >= ip; first address > ip
    while (lo < hi || lo2 < hi2) {
        const bool on1 = lo < hi, on2 = lo2 < hi2;
        const uint32_t m1 = (lo + hi) >> 1, m2 = (lo2 + hi2) >> 1;
        uint32_t a1[4] = {0u, 0u, 0u, 0u}, a2[4] = {0u, 0u, 0u, 0u};
        if (kV6) {
            if (on1) {
                const uint4 v = W.a6[m1];
                a1[0] = v.x, a1[1] = v.y, a1[2] = v.z, a1[3] = v.w;
            }
            if (on2) {
                const uint4 v = W.a6[m2];
                a2[0] = v.x, a2[1] = v.y, a2[2] = v.z, a2[3] = v.w;
            }
        } else {
            if (on1) a1[0] = W.a4[m1];
            if (on2) a2[0] = W.a4[m2];
        }
        if (on1) {
            if (ip_lt(a1, ip, kV6)) lo = m1 + 1u;
            else hi = m1;
        }
        if (on2) {
            if (ip_lt(ip, a2, kV6)) hi2 = m2;
            else lo2 = m2 + 1u;
        }
    }
    if (lo >= lo2) return false;
    const uint32_t* kk = kV6 ? W.k6 : W.k4;
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) hit |= find_key(kk, lo, lo2, keys[k]) != ~0u;
    return hit;
}

// The state byte of one flow.  gkey / gbeg / rules: the group table and the rules where this workgroup
// reads them (its LDS copy, or global memory).
__device__ __forceinline__ uint32_t wl_eval(const WlTables& W, const EnrichTables& E, const DevConfig* cfg,
                                            const uint32_t* gkey, const uint32_t* gbeg, const WlRule* rules,
                                            const uint32_t* key) {
    const uint32_t dst[4] = {key[4], key[5], key[6], key[7]};
    const uint32_t port = key[8] >> 16, proto = key[9] & 0xFFu, fam = (key[9] >> 8) & 0xFFu;
    const bool v6 = fam == 10u;
    // protocol_matches / port_matches (src/whitelists.rs:711-732): None or equal
    const uint32_t keys[4] = {wl_key(0u, false, 0u), wl_key(0u, true, port), wl_key(proto, false, 0u),
                              wl_key(proto, true, port)};
    bool ok = false, hc = false;
    // dst_asn (src/packets.rs:468-485), looked up when the first rule with an AS field is reached
    bool asn_done = false, asn_some = false;
    uint32_t as_number = 0u, owner = ~0u, country = ~0u;
    for (int k = 0; k < 4 && !ok; ++k) {
        const uint32_t g = W.ng ? find_key(gkey, 0u, W.ng, keys[k]) : ~0u;
        if (g == ~0u) continue;
        hc |= (gkey[g] & kWlGroupHostCheck) != 0u;
        const uint32_t end = gbeg[g + 1u];
        for (uint32_t r = gbeg[g]; r < end && !ok; ++r) {
            // the whole rule first, so its three 16-B reads are in flight together (read behind the branch
            // on its kind they were two dependent round trips per rule)
            const uint4* q = reinterpret_cast<const uint4*>(rules + r);
            const uint4 a = q[0], m = q[1];
            const uint32_t kind = q[2].x, rfam = kind & 0xFFu;
            if (rfam) {  // `ip` is a net: ip & mask == network (IpNet::contains) returns true, the AS fields
                         // are not looked at (an IPv4 key's words 1-3 are 0, and so are the rule's)
                ok = rfam == fam && (((dst[0] ^ a.x) & m.x) | ((dst[1] ^ a.y) & m.y) | ((dst[2] ^ a.z) & m.z) |
                                     ((dst[3] ^ a.w) & m.w)) == 0u;
                continue;
            }
            const uint32_t want = kind >> 16;  // FB_WL_HAS_ASN / OWNER / COUNTRY
            if (want == 0u) {                  // nothing specified: matches every session
                ok = true;
                continue;
            }
            if (!asn_done) {
                asn_done = true;
                const bool lan = v6 ? lan_v6(cfg, cfg, dst) : lan_v4(dst[0]);
                const fb_asn_range* A = v6 ? E.asn6 : E.asn4;
                const int32_t i = lan ? -1 : asn_find(A, v6 ? E.n6 : E.n4, dst, v6);
                if (i >= 0) {
                    asn_some = true;
                    as_number = A[i].as_number;
                    const uint32_t rec = A[i].record;
                    if (rec < W.n_records) {
                        owner = W.rec_owner[rec];
                        country = W.rec_country[rec];
                    }
                }
            }
            // src/whitelists.rs:539-595: every specified field equals the session's (None never does)
            // (an AS rule keeps as_number, owner_id, country_id in its address words)
            ok = asn_some && (!(want & FB_WL_HAS_ASN) || a.x == as_number) &&
                 (!(want & FB_WL_HAS_OWNER) || (owner != ~0u && a.y == owner)) &&
                 (!(want & FB_WL_HAS_COUNTRY) || (country != ~0u && a.z == country));
        }
    }
    if (!ok) ok = v6 ? exact_match<true>(W, dst, keys) : exact_match<false>(W, dst, keys);
    return ok ? FB_WL_CONFORMING : (FB_WL_NONCONFORMING | (hc ? FB_WL_HOST_CHECK : 0u));
}

}  // namespace

// k_flow_enrich's geometry: one lane per table slot, 256-thread workgroups striding over the table.
// kStaged: the group table and the rules fit kWlLdsGroups / kWlLdsRules and every workgroup copies them
// into LDS once (coalesced), so the per-lane group searches and rule scans -- divergent addresses --
// stay on the CU.  Otherwise they are read from global memory (L2).
// kStamp (a pass time is set, fb_set_pass_time): the flows whose byte changed get `now` in the stamp plane
// (src/whitelists.rs:975-982); the unstamped instances hold no such store.
// Counters: PassCounters (fb_internal.h).
template <bool kStaged, bool kStamp>
__global__ __launch_bounds__(256) void k_flow_whitelist(const WlTables W, const EnrichTables E, const DevConfig* cfg,
                                                        const FlowSlot* T, unsigned long long cap, uint8_t* state,
                                                        unsigned long long* stats, unsigned long long* mod,
                                                        unsigned long long now) {
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
    PassCounters<kWlCounters> cnt;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < cap; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        const bool occ = i < cap && T[i].tag >= 2u;
        uint32_t nb = 0u, old = 0u;
        if (occ) {
            old = state[i];
            if (kStaged)
                nb = wl_eval(W, E, cfg, s_gkey, s_gbeg, reinterpret_cast<const WlRule*>(s_rules), T[i].key);
            else
                nb = wl_eval(W, E, cfg, W.gkey, W.gbeg, W.rules, T[i].key);
            if (nb != old) state[i] = (uint8_t)nb;
            if (kStamp && nb != old) mod[i] = now;
        }
        cnt.add(0, occ);
        cnt.add(1, (nb & FB_WL_CONFORMING) != 0u);
        cnt.add(2, (nb & FB_WL_NONCONFORMING) != 0u);
        cnt.add(3, (nb & FB_WL_HOST_CHECK) != 0u);
        cnt.add(4, occ && nb != old);
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
                                 unsigned long long* mod, unsigned long long now) {
    if (!table || !state || !stats || !cfg || cap == 0ull) return hipErrorInvalidValue;
    if ((w.ng && (!w.gkey || !w.gbeg)) || (w.nr && !w.rules) || (w.n4 && (!w.a4 || !w.k4)) ||
        (w.n6 && (!w.a6 || !w.k6)) || (w.n_records && (!w.rec_owner || !w.rec_country)))
        return hipErrorInvalidValue;
    const dim3 g(sweep_grid(cap, FB_WL_GRID));
    const bool staged = w.ng <= kWlLdsGroups && w.nr <= kWlLdsRules && w.ng;
    const auto k = staged ? (mod ? k_flow_whitelist<true, true> : k_flow_whitelist<true, false>)
                          : (mod ? k_flow_whitelist<false, true> : k_flow_whitelist<false, false>);
    hipLaunchKernelGGL(k, g, dim3(256), 0, s, w, t, cfg, table, cap, state, stats, mod, now);
    return hipGetLastError();
}

hipError_t launch_flow_export_whitelist(const FlowSlot* table, const uint8_t* state, unsigned long long cap,
                                        uint32_t state_mask, fb_flow_rec* out, unsigned long long out_cap,
                                        unsigned long long* d_n, const FlowTime* plane, hipStream_t s) {
    hipLaunchKernelGGL(k_flow_export_whitelist, dim3(sweep_grid(cap, 1024ull)), dim3(256), 0, s, table, state, cap,
                       state_mask, out, out_cap, d_n, plane);
    return hipGetLastError();
}

// ---- host: the index ---------------------------------------------------------------------------------
// What the device can decide about an endpoint (dst_domain = None, l7 = None):
//   protocol "never"           nothing matches it, not even the host-check condition: dropped;
//   process, or domain-only    never matches; its key is a host-check key;
//   domain + ip                matches by the address alone (a matching ip returns true, a mismatch fails
//                              the endpoint; src/whitelists.rs:503-531); its key is a host-check key too;
//   ip (unparsable)            never matches;
//   ip (address or net)        matches by the address; the AS fields are never reached;
//   neither domain nor ip      every specified AS field must match (none: matches everything).
bool build_whitelist_index(const fb_wl_endpoint* eps, uint64_t n, WlIndex& ix) {
    typedef unsigned __int128 u128;
    struct E6 {
        u128 a;
        uint32_t key;
    };
    struct Keyed {
        uint32_t key;
        WlRule r;
    };
    std::vector<unsigned long long> e4;  // address << 32 | key
    std::vector<E6> e6;
    std::vector<Keyed> rules;
    std::vector<uint32_t> hck;
    for (uint64_t i = 0; i < n; ++i) {
        const fb_wl_endpoint& e = eps[i];
        const bool v4 = e.family == 2u, v6 = e.family == 10u;
        if (!(e.family == 0u || v4 || v6 || e.family == FB_WL_NEVER)) return false;
        if ((v4 && e.prefix > 32u) || (v6 && e.prefix > 128u)) return false;
        if (!(e.protocol == 0u || e.protocol == 6u || e.protocol == 17u || e.protocol == FB_WL_NEVER)) return false;
        if (e.flags & ~0x3Fu) return false;
        if (e.protocol == FB_WL_NEVER) continue;
        const uint32_t key = wl_key(e.protocol, (e.flags & FB_WL_HAS_PORT) != 0u, e.port);
        if (e.flags & (FB_WL_HAS_DOMAIN | FB_WL_HAS_PROCESS)) hck.push_back(key);
        if ((e.flags & FB_WL_HAS_PROCESS) || e.family == FB_WL_NEVER) continue;
        if (e.family == 0u) {
            if (e.flags & FB_WL_HAS_DOMAIN) continue;
            Keyed k = {};
            k.key = key;
            k.r.kind = (uint32_t)(e.flags & (FB_WL_HAS_ASN | FB_WL_HAS_OWNER | FB_WL_HAS_COUNTRY)) << 16;
            k.r.a[0] = e.as_number;
            k.r.a[1] = e.owner_id;
            k.r.a[2] = e.country_id;
            rules.push_back(k);
            continue;
        }
        const uint32_t bits = v6 ? 128u : 32u;
        const u128 a = v6 ? ((u128)e.addr[0] << 96 | (u128)e.addr[1] << 64 | (u128)e.addr[2] << 32 | (u128)e.addr[3])
                          : (u128)e.addr[0];
        if (e.prefix == bits) {
            if (v6) e6.push_back(E6{a, key});
            else e4.push_back((unsigned long long)a << 32 | key);
            continue;
        }
        const u128 all = v6 ? ~(u128)0 : (u128)0xFFFFFFFFu;
        const u128 hostmask = e.prefix == 0u ? all : (((u128)1 << (bits - e.prefix)) - 1u);
        const u128 net = a & ~hostmask & all;  // IpNet::network()
        Keyed k = {};
        k.key = key;
        const u128 mask = ~hostmask & all;
        k.r.kind = e.family;
        if (v6) {
            for (int w = 0; w < 4; ++w) {
                k.r.a[w] = (uint32_t)(net >> (96 - 32 * w));
                k.r.m[w] = (uint32_t)(mask >> (96 - 32 * w));
            }
        } else {
            k.r.a[0] = (uint32_t)net;
            k.r.m[0] = (uint32_t)mask;
        }
        rules.push_back(k);
    }
    if (e4.size() + e6.size() > FB_WL_MAX_EXACT || rules.size() + hck.size() > FB_WL_MAX_OTHER) return false;
    std::sort(e4.begin(), e4.end());
    e4.erase(std::unique(e4.begin(), e4.end()), e4.end());
    std::sort(e6.begin(), e6.end(), [](const E6& x, const E6& y) { return x.a != y.a ? x.a < y.a : x.key < y.key; });
    e6.erase(std::unique(e6.begin(), e6.end(), [](const E6& x, const E6& y) { return x.a == y.a && x.key == y.key; }),
             e6.end());
    std::stable_sort(rules.begin(), rules.end(), [](const Keyed& x, const Keyed& y) { return x.key < y.key; });
    std::sort(hck.begin(), hck.end());
    hck.erase(std::unique(hck.begin(), hck.end()), hck.end());
    ix = WlIndex();
    for (unsigned long long v : e4) {
        ix.a4.push_back((uint32_t)(v >> 32));
        ix.k4.push_back((uint32_t)v);
    }
    for (const E6& v : e6) {
        ix.a6.push_back(make_uint4((uint32_t)(v.a >> 96), (uint32_t)(v.a >> 64), (uint32_t)(v.a >> 32), (uint32_t)v.a));
        ix.k6.push_back(v.key);
    }
    size_t r = 0, h = 0;  // merge the two ascending key sequences into the group table
    while (r < rules.size() || h < hck.size()) {
        const uint32_t key = (r < rules.size() && (h >= hck.size() || rules[r].key <= hck[h])) ? rules[r].key : hck[h];
        uint32_t word = key;
        if (h < hck.size() && hck[h] == key) {
            word |= kWlGroupHostCheck;
            ++h;
        }
        ix.gkey.push_back(word);
        ix.gbeg.push_back((uint32_t)ix.rules.size());
        for (; r < rules.size() && rules[r].key == key; ++r) ix.rules.push_back(rules[r].r);
    }
    ix.gbeg.push_back((uint32_t)ix.rules.size());
    return true;
}

}  // namespace fbk
