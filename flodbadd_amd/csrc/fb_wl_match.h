// fb_wl_match.h -- the whitelist index (fb_set_whitelist) and the evaluation of one flow
// against it: the single definition of both, for fb_whitelist.hip's kernels and for host programs alike
// (tests/wl_match_host.cpp builds it with the sanitizers).  Plain C++: nothing of HIP is needed when a host
// compiler includes it (FB_WL_HD is `inline` there -- as fb_l7_index.h does it).
//
// fb_set_whitelist compiles the endpoint list into three structures (build_whitelist_index):
//   exact   the endpoints that match by one address: per family the addresses ascending and, beside
//           each, its (protocol | any, port | any) key, ascending inside an address's run (deduplicated).
//           A list with process ids keeps key << 32 | process_match_id beside each address instead (kp4 / kp6),
//           so a run is ordered by (key, process) and one search finds a (key, process) pair;
//   rules   every other endpoint the device can match -- nets, AS-only, match-all -- sorted by the same key,
//           each with its process (0: any);
//   groups  the distinct keys of the rules and of the host-check endpoints, ascending: gkey[g]
//           (kWlGroupHostCheck: a domain endpoint, or a process endpoint without an id, has this key;
//           kWlGroupProcCheck: a process endpoint with an id has it), the group's rules
//           rules[gbeg[g] .. gbeg[g + 1]).
// A flow (protocol P, destination port Q) can only match the endpoints of its four keys wl_key(0 | P,
// none | Q): the kernel looks each up (one address search, four group searches).
//
// A list with domain pattern ids (fb_set_whitelist_dom) adds
//   domains the endpoints with a pattern id, as (pattern id, key << 32 | process_match_id), ascending and
//           deduplicated: dpid / dkp.  A flow whose destination name matched pattern p matches such an endpoint
//           when the run of p holds one of its four keys with no process or the flow's -- one search of eight
//           words per matched id (kDom; the other instances read neither the domain plane nor the rows).
//
// kProc selects the process-aware evaluation: the instances of a list without process ids (kProc false) read
// neither the L7 plane nor a rule's process word nor kp4 / kp6 -- they are the pass as it was before the
// device knew processes.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/flodbadd_gpu.h"
#include "fb_wl_domain.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FB_WL_HD __host__ __device__ __forceinline__
#else
#define FB_WL_HD inline
#endif

namespace fbk {

#if defined(__HIPCC__)
typedef uint4 WlU4;
#else
struct alignas(16) WlU4 {
    uint32_t x, y, z, w;
};
#endif

FB_WL_HD uint32_t wl_key(uint32_t proto, bool has_port, uint32_t port) {
    return proto << 17 | (has_port ? 1u << 16 | port : 0u);
}
// (a key has at most 22 bits: the two top bits of a group word are flags)
constexpr uint32_t kWlGroupHostCheck = 0x80000000u;  // the host must look whatever the device knows
constexpr uint32_t kWlGroupProcCheck = 0x40000000u;  // ... only while no process-name table is installed
constexpr uint32_t kWlGroupDomId = 0x20000000u;      // a domain endpoint with a pattern id has this key
constexpr uint32_t kWlGroupFlags = kWlGroupHostCheck | kWlGroupProcCheck | kWlGroupDomId;
struct WlRule {                   // 48 B: three 16-B LDS reads, and a net test of xor / and / or per word
    uint32_t a[4];                // family 2 / 10: the network (host bits cleared); family 0: as_number,
                                  // owner_id, country_id, 0
    uint32_t m[4];                // the prefix mask (IPv4: word 0, the other words 0 like the key's)
    uint32_t kind;                // family | FB_WL_HAS_ASN/OWNER/COUNTRY << 16 (family 0 only)
    uint32_t proc;                // the endpoint's process_match_id: 0 = any, else the flow's must equal it
    uint32_t pad[2];
};
static_assert(sizeof(WlRule) == 48, "whitelist rule is 48 B");
static_assert(sizeof(fb_wl_endpoint) == 40 && sizeof(fb_l7_rec) == 8, "whitelist / L7 ABI");
struct WlTables {
    const uint32_t* a4;   // [n4] exact IPv4 addresses
    const uint32_t* k4;   // [n4] their keys (a list without process ids)
    const WlU4* a6;       // [n6] exact IPv6 addresses (session_key word order)
    const uint32_t* k6;
    const uint32_t* gkey; // [ng]
    const uint32_t* gbeg; // [ng + 1]
    const WlRule* rules;  // [nr]
    const uint32_t* rec_owner;    // [n_records]
    const uint32_t* rec_country;
    const unsigned long long* kp4;  // [n4] key << 32 | process_match_id (a list with process ids: k4 / k6 empty)
    const unsigned long long* kp6;  // [n6]
    uint32_t n4, n6, ng, nr, n_records;
    const uint32_t* dpid;            // [nd] the domain endpoints' pattern ids, ascending
    const unsigned long long* dkp;   // [nd] key << 32 | process_match_id, ascending inside a pattern's run
    uint32_t nd;
};
// The process of a flow (fb_set_l7_process_names): x = plane[slot].process_id names one when the plane exists,
// x != 0 and x < n; its match class is match_id[x], its verbatim name name_id[x].  n == 0: no table.
struct WlProcNames {
    const fb_l7_rec* plane;
    const uint32_t* match_id;
    const uint32_t* name_id;
    uint32_t n;
};
FB_WL_HD uint32_t wl_flow_process(const WlProcNames& P, unsigned long long slot) {
    if (!P.plane || P.n == 0u) return 0u;
    const uint32_t x = P.plane[slot].process_id;
    return x < P.n ? x : 0u;
}
FB_WL_HD uint32_t wl_flow_match_id(const WlProcNames& P, unsigned long long slot) {
    const uint32_t x = wl_flow_process(P, slot);
    return x ? P.match_id[x] : 0u;
}
FB_WL_HD uint32_t wl_flow_name_id(const WlProcNames& P, unsigned long long slot) {
    const uint32_t x = wl_flow_process(P, slot);
    return x ? P.name_id[x] : 0u;
}

FB_WL_HD bool wl_ip_lt(const uint32_t a[4], const uint32_t b[4], bool v6) {
    if (!v6) return a[0] < b[0];
    for (int k = 0; k < 4; ++k)
        if (a[k] != b[k]) return a[k] < b[k];
    return false;
}

// The index of `key` in the ascending keys[lo, hi) (the flag bits of an entry are not part of it), or ~0u.
FB_WL_HD uint32_t wl_find_key(const uint32_t* keys, uint32_t lo, uint32_t hi, uint32_t key) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1, v = keys[mid] & ~kWlGroupFlags;
        if (v == key) return mid;
        if (v < key) lo = mid + 1u;
        else hi = mid;
    }
    return ~0u;
}

// Is one of the S words t[s] (bit s of `act` set) in the ascending a[lo0, hi0)?  The S bisections advance
// together, so each step has its probes in flight at once.
template <uint32_t S>
FB_WL_HD bool wl_find_any(const unsigned long long* a, uint32_t lo0, uint32_t hi0, const unsigned long long (&t)[S],
                          uint32_t act) {
    uint32_t lo[S], hi[S];
    for (uint32_t s = 0; s < S; ++s) {
        lo[s] = lo0;
        hi[s] = (act >> s & 1u) ? hi0 : lo0;
    }
    for (;;) {
        bool any = false;
        for (uint32_t s = 0; s < S; ++s) any |= lo[s] < hi[s];
        if (!any) return false;
        unsigned long long v[S];
        for (uint32_t s = 0; s < S; ++s) v[s] = lo[s] < hi[s] ? a[(lo[s] + hi[s]) >> 1] : 0ull;
        for (uint32_t s = 0; s < S; ++s) {
            if (!(lo[s] < hi[s])) continue;
            const uint32_t mid = (lo[s] + hi[s]) >> 1;
            if (v[s] == t[s]) return true;
            if (v[s] < t[s]) lo[s] = mid + 1u;
            else hi[s] = mid;
        }
    }
}

// Some exact-address endpoint has the destination and one of the flow's four keys -- and, kProc, no process
// or the flow's (pm, 0: the flow has none): the run of the address in the sorted array (its lower and upper
// bound, advanced together so each step has both probes in flight; they coincide until the searches part),
// then the keys -- kProc: the (key, process) pairs -- inside the run.
template <bool kV6, bool kProc>
FB_WL_HD bool wl_exact_match(const WlTables& W, const uint32_t ip[4], const uint32_t keys[4], uint32_t pm) {
    const uint32_t n = kV6 ? W.n6 : W.n4;
    uint32_t lo = 0u, hi = n, lo2 = 0u, hi2 = n;  // first address >= ip; first address > ip
    while (lo < hi || lo2 < hi2) {
        const bool on1 = lo < hi, on2 = lo2 < hi2;
        const uint32_t m1 = (lo + hi) >> 1, m2 = (lo2 + hi2) >> 1;
        uint32_t a1[4] = {0u, 0u, 0u, 0u}, a2[4] = {0u, 0u, 0u, 0u};
        if (kV6) {
            if (on1) {
                const WlU4 v = W.a6[m1];
                a1[0] = v.x, a1[1] = v.y, a1[2] = v.z, a1[3] = v.w;
            }
            if (on2) {
                const WlU4 v = W.a6[m2];
                a2[0] = v.x, a2[1] = v.y, a2[2] = v.z, a2[3] = v.w;
            }
        } else {
            if (on1) a1[0] = W.a4[m1];
            if (on2) a2[0] = W.a4[m2];
        }
        if (on1) {
            if (wl_ip_lt(a1, ip, kV6)) lo = m1 + 1u;
            else hi = m1;
        }
        if (on2) {
            if (wl_ip_lt(ip, a2, kV6)) hi2 = m2;
            else lo2 = m2 + 1u;
        }
    }
    if (lo >= lo2) return false;
    if (kProc) {  // each key with process 0 (any) and with the flow's own: one search of eight words
        unsigned long long t[8];
        for (int k = 0; k < 4; ++k) {
            t[k] = (unsigned long long)keys[k] << 32;
            t[4 + k] = t[k] | pm;
        }
        return wl_find_any<8>(kV6 ? W.kp6 : W.kp4, lo, lo2, t, pm ? 0xFFu : 0x0Fu);
    }
    const uint32_t* kk = kV6 ? W.k6 : W.k4;
    bool hit = false;
    for (int k = 0; k < 4; ++k) hit |= wl_find_key(kk, lo, lo2, keys[k]) != ~0u;
    return hit;
}

// Some domain endpoint has a pattern the flow's name matched (row: FB_WL_NAME_MATCHES ids ascending, zero-padded)
// and one of the flow's four keys, with no process or the flow's (pm; 0: the flow has none): the run of each
// matched id in dpid (lower and upper bound), then the (key, process) pairs inside it, as wl_exact_match.
FB_WL_HD bool wl_domain_match(const WlTables& W, const uint32_t* row, const uint32_t keys[4], uint32_t pm) {
    unsigned long long t[8];
    for (int k = 0; k < 4; ++k) {
        t[k] = (unsigned long long)keys[k] << 32;
        t[4 + k] = t[k] | pm;
    }
    for (uint32_t j = 0; j < FB_WL_NAME_MATCHES; ++j) {
        const uint32_t p = row[j];
        if (p == 0u) break;
        uint32_t lo = 0u, hi = W.nd, lo2 = 0u, hi2 = W.nd;  // first id >= p; first id > p
        while (lo < hi || lo2 < hi2) {
            const bool on1 = lo < hi, on2 = lo2 < hi2;
            const uint32_t m1 = (lo + hi) >> 1, m2 = (lo2 + hi2) >> 1;
            const uint32_t v1 = on1 ? W.dpid[m1] : 0u, v2 = on2 ? W.dpid[m2] : 0u;
            if (on1) {
                if (v1 < p) lo = m1 + 1u;
                else hi = m1;
            }
            if (on2) {
                if (p < v2) hi2 = m2;
                else lo2 = m2 + 1u;
            }
        }
        if (lo < lo2 && wl_find_any<8>(W.dkp, lo, lo2, t, pm ? 0xFFu : 0x0Fu)) return true;
    }
    return false;
}

// dst_asn of a flow (src/packets.rs:468-485) as the evaluation asks for it, at most once per flow:
//   bool asn(dst, v6, as_number, owner, country)   false: None; owner / country ~0u: a string no endpoint has
//
// The state byte of one flow.  gkey / gbeg / rules: the group table and the rules where the caller reads them
// (a workgroup's LDS copy, or global memory).  kProc: pm is the flow's process_match_id (0: None) and
// have_names whether a process-name table is installed -- without one a process endpoint with an id is what
// one without an id always is: it never matches and its key is a host-check key.
// kDom: row / row_flags are the match row and the flags byte of the flow's destination name (null: the flow has
// no domain) -- a domain endpoint with a pattern id matches by it; dom_overflow: set when the flow is marked for
// the host because the row is incomplete.
template <bool kProc, bool kDom = false, class Asn>
FB_WL_HD uint32_t wl_eval(const WlTables& W, const Asn& asn, const uint32_t* gkey, const uint32_t* gbeg,
                          const WlRule* rules, const uint32_t* key, uint32_t pm, bool have_names,
                          const uint32_t* row = nullptr, uint32_t row_flags = 0u, bool* dom_overflow = nullptr) {
    const uint32_t dst[4] = {key[4], key[5], key[6], key[7]};
    const uint32_t port = key[8] >> 16, proto = key[9] & 0xFFu, fam = (key[9] >> 8) & 0xFFu;
    const bool v6 = fam == 10u;
    // protocol_matches / port_matches (src/whitelists.rs:711-732): None or equal
    const uint32_t keys[4] = {wl_key(0u, false, 0u), wl_key(0u, true, port), wl_key(proto, false, 0u),
                              wl_key(proto, true, port)};
    bool ok = false, hc = false, domid = false;
    // dst_asn, looked up when the first rule with an AS field is reached
    bool asn_done = false, asn_some = false;
    uint32_t as_number = 0u, owner = ~0u, country = ~0u;
    for (int k = 0; k < 4 && !ok; ++k) {
        const uint32_t g = W.ng ? wl_find_key(gkey, 0u, W.ng, keys[k]) : ~0u;
        if (g == ~0u) continue;
        hc |= (gkey[g] & kWlGroupHostCheck) != 0u;
        if (kProc) hc |= !have_names && (gkey[g] & kWlGroupProcCheck) != 0u;
        if (kDom) domid |= (gkey[g] & kWlGroupDomId) != 0u;
        const uint32_t end = gbeg[g + 1u];
        for (uint32_t r = gbeg[g]; r < end && !ok; ++r) {
            // the whole rule first, so its three 16-B reads are in flight together (read behind the branch
            // on its kind they were two dependent round trips per rule)
            const WlU4* q = reinterpret_cast<const WlU4*>(rules + r);
            const WlU4 a = q[0], m = q[1], c = q[2];
            const uint32_t kind = c.x, rfam = kind & 0xFFu;
            // process_matches (src/whitelists.rs:716-724): None, or equal ignoring ASCII case (one match id)
            if (kProc && c.y != 0u && c.y != pm) continue;
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
                asn_some = asn(dst, v6, as_number, owner, country);
            }
            // src/whitelists.rs:539-595: every specified field equals the session's (None never does)
            // (an AS rule keeps as_number, owner_id, country_id in its address words)
            ok = asn_some && (!(want & FB_WL_HAS_ASN) || a.x == as_number) &&
                 (!(want & FB_WL_HAS_OWNER) || (owner != ~0u && a.y == owner)) &&
                 (!(want & FB_WL_HAS_COUNTRY) || (country != ~0u && a.z == country));
        }
    }
    if (kDom && !ok && row && domid) ok = wl_domain_match(W, row, keys, pm);
    if (!ok) ok = v6 ? wl_exact_match<true, kProc>(W, dst, keys, pm) : wl_exact_match<false, kProc>(W, dst, keys, pm);
    if (kDom && !ok && row && domid && (row_flags & 1u)) {  // the row is not all the name matches: the host's
        if (dom_overflow) *dom_overflow = true;
        hc = true;
    }
    return ok ? FB_WL_CONFORMING : (FB_WL_NONCONFORMING | (hc ? FB_WL_HOST_CHECK : 0u));
}

// ---- host only: the index ----------------------------------------------------------------------------
struct WlIndex {
    std::vector<uint32_t> a4, k4, k6, gkey, gbeg;
    std::vector<unsigned long long> kp4, kp6;  // with_proc: instead of k4 / k6
    std::vector<WlU4> a6;
    std::vector<WlRule> rules;
    bool with_proc = false;  // some endpoint has a process with an id: the kProc instances run
    std::vector<uint32_t> dpid;           // the domain endpoints with a pattern id: ordered by (pattern id, key,
    std::vector<unsigned long long> dkp;  // process), deduplicated.  Non-empty: the kDom instances run
};
// What the device can decide about an endpoint (dst_domain = None; the process by its id):
//   protocol "never"           nothing matches it, not even the host-check condition: dropped;
//   process without an id      (process_match_id 0) never matches; its key is a host-check key;
//   process with an id         the endpoint below that it is without its process, matching only flows of that
//                              process; its key is a host-check key while no name table is installed;
//   domain-only                never matches; its key is a host-check key;
//   domain + ip                matches by the address alone (a matching ip returns true, a mismatch fails
//                              the endpoint; src/whitelists.rs:503-531); its key is a host-check key too;
//   domain with a pattern id   (ep_pattern[i] != 0) also matches the flows whose name matched the pattern --
//                              protocol, port and process permitting --, and its key is no host-check key on
//                              the domain's account (kWlGroupDomId instead);
//   ip (unparsable)            never matches;
//   ip (address or net)        matches by the address; the AS fields are never reached;
//   neither domain nor ip      every specified AS field must match (none: matches everything).
// false: an endpoint with a bad family / prefix / protocol, more than FB_WL_MAX_EXACT / _OTHER, a pattern id
// above n_patterns or on an endpoint without a domain.
inline bool build_whitelist_index(const fb_wl_endpoint* eps, uint64_t n, WlIndex& ix, const uint32_t* ep_pattern = nullptr,
                                  uint64_t n_patterns = 0u) {
    typedef unsigned __int128 u128;
    struct E6 {
        u128 a;
        uint32_t key;
    };
    struct EP {  // an exact-address endpoint with a process id
        u128 a;
        unsigned long long kp;
    };
    struct Keyed {
        uint32_t key;
        WlRule r;
    };
    std::vector<unsigned long long> e4;  // address << 32 | key
    std::vector<E6> e6;
    std::vector<EP> p4, p6;
    std::vector<Keyed> rules;
    std::vector<uint32_t> hck, pck, dck;
    std::vector<std::pair<uint32_t, unsigned long long>> dom;
    for (uint64_t i = 0; i < n; ++i) {
        const fb_wl_endpoint& e = eps[i];
        const uint32_t dp = ep_pattern ? ep_pattern[i] : 0u;
        if (dp > n_patterns || (dp && !(e.flags & FB_WL_HAS_DOMAIN))) return false;
        const bool v4 = e.family == 2u, v6 = e.family == 10u;
        if (!(e.family == 0u || v4 || v6 || e.family == FB_WL_NEVER)) return false;
        if ((v4 && e.prefix > 32u) || (v6 && e.prefix > 128u)) return false;
        if (!(e.protocol == 0u || e.protocol == 6u || e.protocol == 17u || e.protocol == FB_WL_NEVER)) return false;
        if (e.flags & ~0x3Fu) return false;
        if (e.protocol == FB_WL_NEVER) continue;
        const uint32_t key = wl_key(e.protocol, (e.flags & FB_WL_HAS_PORT) != 0u, e.port);
        const bool has_proc = (e.flags & FB_WL_HAS_PROCESS) != 0u;
        const uint32_t pm = has_proc ? e.process_match_id : 0u;
        if (((e.flags & FB_WL_HAS_DOMAIN) && dp == 0u) || (has_proc && pm == 0u)) hck.push_back(key);
        if (pm != 0u && (pck.empty() || pck.back() != key)) pck.push_back(key);  // (a key, not an endpoint: not counted)
        if (dp && (dck.empty() || dck.back() != key)) dck.push_back(key);
        if (has_proc && pm == 0u) continue;
        if (dp) dom.push_back({dp, (unsigned long long)key << 32 | pm});
        if (e.family == FB_WL_NEVER) continue;
        if (e.family == 0u) {
            if (e.flags & FB_WL_HAS_DOMAIN) continue;
            Keyed k = {};
            k.key = key;
            k.r.kind = (uint32_t)(e.flags & (FB_WL_HAS_ASN | FB_WL_HAS_OWNER | FB_WL_HAS_COUNTRY)) << 16;
            k.r.proc = pm;
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
            if (pm != 0u) (v6 ? p6 : p4).push_back(EP{a, (unsigned long long)key << 32 | pm});
            else if (v6) e6.push_back(E6{a, key});
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
        k.r.proc = pm;
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
    if (e4.size() + e6.size() + p4.size() + p6.size() > FB_WL_MAX_EXACT ||
        rules.size() + hck.size() > FB_WL_MAX_OTHER)
        return false;
    std::sort(e4.begin(), e4.end());
    e4.erase(std::unique(e4.begin(), e4.end()), e4.end());
    std::sort(e6.begin(), e6.end(), [](const E6& x, const E6& y) { return x.a != y.a ? x.a < y.a : x.key < y.key; });
    e6.erase(std::unique(e6.begin(), e6.end(), [](const E6& x, const E6& y) { return x.a == y.a && x.key == y.key; }),
             e6.end());
    std::stable_sort(rules.begin(), rules.end(), [](const Keyed& x, const Keyed& y) { return x.key < y.key; });
    std::sort(hck.begin(), hck.end());
    hck.erase(std::unique(hck.begin(), hck.end()), hck.end());
    std::sort(pck.begin(), pck.end());
    pck.erase(std::unique(pck.begin(), pck.end()), pck.end());
    std::sort(dck.begin(), dck.end());
    dck.erase(std::unique(dck.begin(), dck.end()), dck.end());
    std::sort(dom.begin(), dom.end());
    dom.erase(std::unique(dom.begin(), dom.end()), dom.end());
    ix = WlIndex();
    for (const auto& d : dom) {
        ix.dpid.push_back(d.first);
        ix.dkp.push_back(d.second);
    }
    ix.with_proc = !pck.empty();
    if (ix.with_proc) {  // per family one array ordered by (address, key, process), deduplicated
        for (unsigned long long v : e4) p4.push_back(EP{(u128)(v >> 32), (v & 0xFFFFFFFFull) << 32});
        for (const E6& v : e6) p6.push_back(EP{v.a, (unsigned long long)v.key << 32});
        for (std::vector<EP>* p : {&p4, &p6}) {
            std::sort(p->begin(), p->end(), [](const EP& x, const EP& y) { return x.a != y.a ? x.a < y.a : x.kp < y.kp; });
            p->erase(std::unique(p->begin(), p->end(), [](const EP& x, const EP& y) { return x.a == y.a && x.kp == y.kp; }),
                     p->end());
        }
        for (const EP& v : p4) {
            ix.a4.push_back((uint32_t)v.a);
            ix.kp4.push_back(v.kp);
        }
        for (const EP& v : p6) {
            ix.a6.push_back(WlU4{(uint32_t)(v.a >> 96), (uint32_t)(v.a >> 64), (uint32_t)(v.a >> 32), (uint32_t)v.a});
            ix.kp6.push_back(v.kp);
        }
    } else {
        for (unsigned long long v : e4) {
            ix.a4.push_back((uint32_t)(v >> 32));
            ix.k4.push_back((uint32_t)v);
        }
        for (const E6& v : e6) {
            ix.a6.push_back(WlU4{(uint32_t)(v.a >> 96), (uint32_t)(v.a >> 64), (uint32_t)(v.a >> 32), (uint32_t)v.a});
            ix.k6.push_back(v.key);
        }
    }
    // the group table: the distinct keys of the rules and of the two host-check lists, ascending
    std::vector<uint32_t> keys(hck);
    keys.insert(keys.end(), pck.begin(), pck.end());
    keys.insert(keys.end(), dck.begin(), dck.end());
    for (const Keyed& k : rules) keys.push_back(k.key);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    size_t r = 0;
    for (const uint32_t key : keys) {
        uint32_t word = key;
        if (std::binary_search(hck.begin(), hck.end(), key)) word |= kWlGroupHostCheck;
        if (std::binary_search(pck.begin(), pck.end(), key)) word |= kWlGroupProcCheck;
        if (std::binary_search(dck.begin(), dck.end(), key)) word |= kWlGroupDomId;
        ix.gkey.push_back(word);
        ix.gbeg.push_back((uint32_t)ix.rules.size());
        for (; r < rules.size() && rules[r].key == key; ++r) ix.rules.push_back(rules[r].r);
    }
    ix.gbeg.push_back((uint32_t)ix.rules.size());
    return true;
}

}  // namespace fbk
