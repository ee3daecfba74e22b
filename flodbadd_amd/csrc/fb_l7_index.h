// fb_l7_index.h -- the socket snapshot's index (fb_set_l7_sockets) and the match of one
// session against it: the single definition of both, for fb_l7.hip's kernels and for host programs alike
// (tests/l7_index_host.cpp builds it with the sanitizers).  Plain C++: nothing of HIP is needed when a host
// compiler includes it (FB_L7_HD is `inline` there, `__host__ __device__ inline` under hipcc -- as
// fb_dns_hash.h does it).
//
// The reference matches a session by scanning the ordered socket list (resolve_l7_data, src/l7.rs:1020-1135;
// try_exact_match_from_index, src/l7.rs:1220-1279); what it returns is always the LOWEST LIST INDEX among
// the sockets that equal one of a few keys, so every distinct key keeps that index and its process id:
//   local table  key = {protocol << 24 | local_family << 16 | local_port, local_ip[4]}      (5 words)
//   pair table   key = local key, then {remote_port, remote_ip[4]}                          (10 words)
//                TCP sockets whose two families agree (a session has one family)
// both ascending by the key's words, word 0 first.  l7_match is then ten point lookups at the most.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/flodbadd_gpu.h"

#if defined(__HIPCC__)
#define FB_L7_HD __host__ __device__ inline
#else
#define FB_L7_HD inline
#endif

namespace fbk {

constexpr uint32_t kL7LocalWords = 5, kL7PairWords = 10;
template <uint32_t W>
struct alignas(16) L7Entry {
    uint32_t k[W];
    uint32_t idx;  // the lowest list index of a socket with this key
    uint32_t pid;  // that socket's process_id
};
using L7Local = L7Entry<kL7LocalWords>;
using L7Pair = L7Entry<kL7PairWords>;
static_assert(sizeof(L7Local) == 32 && sizeof(L7Pair) == 48, "whole 16-B units");
static_assert(sizeof(fb_l7_socket) == 48 && sizeof(fb_l7_rec) == 8, "L7 ABI");

struct L7Tables {
    const L7Pair* pairs;
    const L7Local* locals;
    uint32_t n_pairs, n_locals;
};

FB_L7_HD void l7_local_key(uint32_t proto, uint32_t fam, const uint32_t ip[4], uint32_t port, uint32_t* k) {
    k[0] = proto << 24 | fam << 16 | port;
    k[1] = ip[0], k[2] = ip[1], k[3] = ip[2], k[4] = ip[3];
}
FB_L7_HD void l7_pair_key(uint32_t fam, const uint32_t lip[4], uint32_t lport, const uint32_t rip[4], uint32_t rport,
                          uint32_t* k) {
    l7_local_key(6u, fam, lip, lport, k);
    k[5] = rport;
    k[6] = rip[0], k[7] = rip[1], k[8] = rip[2], k[9] = rip[3];
}
template <uint32_t W>
FB_L7_HD int l7_cmp(const uint32_t* a, const uint32_t* b) {
    for (uint32_t j = 0; j < W; ++j)
        if (a[j] != b[j]) return a[j] < b[j] ? -1 : 1;
    return 0;
}

// S bisections of one table advanced together, so that each step has its S probes in flight at once (a lane
// that ran them one after the other would wait out S x log2(n) dependent loads).  idx[s] = ~0u: key s is
// not in the table (or bit s of `act` is clear: not searched).
template <uint32_t S, uint32_t W>
FB_L7_HD void l7_find_many(const L7Entry<W>* tab, uint32_t n, const uint32_t (&key)[S][W], uint32_t act,
                           uint32_t (&idx)[S], uint32_t (&pid)[S]) {
    uint32_t lo[S], hi[S];
    for (uint32_t s = 0; s < S; ++s) {
        lo[s] = 0u;
        hi[s] = (act >> s & 1u) ? n : 0u;
        idx[s] = ~0u;
        pid[s] = 0u;
    }
    for (;;) {
        bool any = false;
        for (uint32_t s = 0; s < S; ++s) any |= lo[s] < hi[s];
        if (!any) break;
        L7Entry<W> e[S];
        for (uint32_t s = 0; s < S; ++s)
            if (lo[s] < hi[s]) e[s] = tab[(lo[s] + hi[s]) >> 1];
        for (uint32_t s = 0; s < S; ++s) {
            if (!(lo[s] < hi[s])) continue;
            const uint32_t mid = (lo[s] + hi[s]) >> 1;
            const int c = l7_cmp<W>(e[s].k, key[s]);
            if (c == 0) {
                idx[s] = e[s].idx;
                pid[s] = e[s].pid;
                hi[s] = lo[s];
            } else if (c < 0) {
                lo[s] = mid + 1u;
            } else {
                hi[s] = mid;
            }
        }
    }
}

struct L7Match {
    uint32_t pid;     // 0: no socket matches
    uint32_t source;  // FB_L7_EXACT / FB_L7_FUZZY, 0 with pid 0
};

// One session (its 10 key words, fb_session_key) against the snapshot: try_exact_match_from_index, then
// try_fuzzy_match when that found nothing.
FB_L7_HD L7Match l7_match(const L7Tables& t, const uint32_t* key) {
    const uint32_t src[4] = {key[0], key[1], key[2], key[3]}, dst[4] = {key[4], key[5], key[6], key[7]};
    const uint32_t sport = key[8] & 0xFFFFu, dport = key[8] >> 16, proto = key[9] & 0xFFu, fam = (key[9] >> 8) & 0xFFu;
    L7Match m = {0u, 0u};
    // exact: form A = the socket's local side is the source, form B = it is the destination.  The reference
    // scans the src_port bucket, then the dst_port bucket, each in list order (src/l7.rs:1227-1276): a form-A
    // socket is in the first, so with different ports the lowest A wins over any B; with equal ports both
    // forms are in the one bucket and the lowest index of either wins.
    uint32_t ia, ib, pa, pb;
    if (proto == 6u) {
        uint32_t k[2][kL7PairWords], ix[2], px[2];
        l7_pair_key(fam, src, sport, dst, dport, k[0]);
        l7_pair_key(fam, dst, dport, src, sport, k[1]);
        l7_find_many<2, kL7PairWords>(t.pairs, t.n_pairs, k, 3u, ix, px);
        ia = ix[0], ib = ix[1], pa = px[0], pb = px[1];
    } else {
        uint32_t k[2][kL7LocalWords], ix[2], px[2];
        l7_local_key(proto, fam, src, sport, k[0]);
        l7_local_key(proto, fam, dst, dport, k[1]);
        l7_find_many<2, kL7LocalWords>(t.locals, t.n_locals, k, 3u, ix, px);
        ia = ix[0], ib = ix[1], pa = px[0], pb = px[1];
    }
    if (ia != ~0u || ib != ~0u) {
        const bool a = sport != dport ? ia != ~0u : ia <= ib;  // (~0u is the largest index)
        m.pid = a ? pa : pb;
        m.source = FB_L7_EXACT;
        return m;
    }
    // fuzzy (src/l7.rs:1091-1135): the lowest index over {0.0.0.0, ::, src_ip, dst_ip} x {src_port, dst_port}
    // with the session's protocol; the two wildcards carry their own family, the addresses the session's
    const uint32_t zero[4] = {0u, 0u, 0u, 0u};
    uint32_t k[8][kL7LocalWords], ix[8], px[8];
    for (uint32_t p = 0; p < 2u; ++p) {
        const uint32_t port = p ? dport : sport;
        l7_local_key(proto, 2u, zero, port, k[4u * p]);
        l7_local_key(proto, 10u, zero, port, k[4u * p + 1u]);
        l7_local_key(proto, fam, src, port, k[4u * p + 2u]);
        l7_local_key(proto, fam, dst, port, k[4u * p + 3u]);
    }
    l7_find_many<8, kL7LocalWords>(t.locals, t.n_locals, k, sport != dport ? 0xFFu : 0x0Fu, ix, px);
    uint32_t best = ~0u;
    for (uint32_t s = 0; s < 8u; ++s)
        if (ix[s] < best) best = ix[s], m.pid = px[s];
    if (best != ~0u) m.source = FB_L7_FUZZY;
    return m;
}

// The retry rule of one resolver cycle (src/l7.rs:429-470) on a flow's plane element {process_id, source |
// tries << 8} that the pass looked up: a match sets the process and clears the count; a miss raises the
// count (it stays at 255) and fails the flow once it is above max_retries.
FB_L7_HD void l7_apply(const L7Match& m, uint32_t max_retries, uint32_t& pid, uint32_t& word) {
    if (m.pid != 0u) {
        pid = m.pid;
        word = m.source;
        return;
    }
    uint32_t tries = (word >> 8) & 0xFFu;
    if (tries < 255u) ++tries;
    word = (tries > max_retries ? (uint32_t)FB_L7_FAILED : 0u) | tries << 8;
}

// ---- host only -------------------------------------------------------------------------------------------
// fb_l7_validate's rules; they make every stored key canonical (an IPv4 address has words 1-3 zero, as a
// session key's has).
inline bool l7_socket_valid(const fb_l7_socket& s) {
    if (s.protocol != 6u && s.protocol != 17u) return false;
    if (s.local_family != 2u && s.local_family != 10u) return false;
    if (s.protocol == 6u ? (s.remote_family != 2u && s.remote_family != 10u)
                         : (s.remote_family != 0u && s.remote_family != 2u && s.remote_family != 10u))
        return false;
    if (s.reserved0 != 0u || s.reserved1 != 0u || s.process_id == 0u) return false;
    if (s.local_family == 2u && (s.local_ip[1] | s.local_ip[2] | s.local_ip[3]) != 0u) return false;
    if (s.remote_family != 10u && (s.remote_ip[1] | s.remote_ip[2] | s.remote_ip[3]) != 0u) return false;
    return true;
}

template <uint32_t W>
inline void l7_sort_unique(std::vector<L7Entry<W>>& v) {
    std::sort(v.begin(), v.end(), [](const L7Entry<W>& a, const L7Entry<W>& b) {
        const int c = l7_cmp<W>(a.k, b.k);
        return c != 0 ? c < 0 : a.idx < b.idx;
    });
    v.erase(std::unique(v.begin(), v.end(),
                        [](const L7Entry<W>& a, const L7Entry<W>& b) { return l7_cmp<W>(a.k, b.k) == 0; }),
            v.end());
}

// false: an invalid socket or more than FB_L7_MAX_SOCKETS (nothing is ever truncated)
inline bool build_l7_index(const fb_l7_socket* socks, uint64_t n, std::vector<L7Pair>& pairs,
                           std::vector<L7Local>& locals) {
    if (n > FB_L7_MAX_SOCKETS) return false;
    for (uint64_t i = 0; i < n; ++i)
        if (!l7_socket_valid(socks[i])) return false;
    pairs.clear();
    locals.clear();
    locals.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        const fb_l7_socket& s = socks[i];
        L7Local l = {};
        l7_local_key(s.protocol, s.local_family, s.local_ip, s.local_port, l.k);
        l.idx = (uint32_t)i;
        l.pid = s.process_id;
        locals.push_back(l);
        if (s.protocol == 6u && s.remote_family == s.local_family) {
            L7Pair p = {};
            l7_pair_key(s.local_family, s.local_ip, s.local_port, s.remote_ip, s.remote_port, p.k);
            p.idx = (uint32_t)i;
            p.pid = s.process_id;
            pairs.push_back(p);
        }
    }
    l7_sort_unique(pairs);
    l7_sort_unique(locals);
    return true;
}

}  // namespace fbk
