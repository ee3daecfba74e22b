// fb_wl_domain.h -- domain patterns of the whitelist (fb_set_whitelist_dom): the classification
// of a pattern, the pattern index and the match of one name against it -- domain_matches (src/whitelists.rs:
// 602-679) -- in plain C++: one definition for fb_wl_domain.hip's kernel, for fb_set_whitelist_dom and for host
// programs (tests/wl_domain_host.cpp builds it with the sanitizers), as fb_wl_match.h is.
//
// The session side is the stored name with ASCII A-Z lower-cased (bytes >= 0x80 stay); the pattern arrives
// lower-cased.  A pattern is classified in the reference's order:
//   exact    no '*'                                      n == pattern
//   suffix   starts with "*.": s = pattern[2:]           some i: n[i] == '.' and n[i + 1:] == s
//   prefix   else ends with ".*": q = pattern[:-2]       n == q, or some i: n[i] == '.' and n[:i] == q
//   general  else exactly one '*': a*b                   n starts with a, ends with b, len(n) > len(a) + len(b)
//   never    anything else                               nothing
// So the only parts of a name an exact / suffix / prefix pattern can equal are the whole name, what follows a
// dot and what precedes a dot: the "candidates".  Each kind keeps its patterns sorted by (hash of the compared
// part & mask, its length, pattern id); a candidate bisects to the run of its (hash, length) and compares bytes
// with every pattern of the run -- a hash hit is never a verdict, so the mask (FB_DEBUG_WL_NAME_HASH_MASK)
// changes the runs' lengths and nothing else.  General patterns are few (FB_WL_MAX_GENERAL) and are scanned.
//
// The hash is the fold of one element per byte under an associative operator (wl_dom_join), so the hashes of
// every prefix and suffix of a name come from two scans.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/flodbadd_gpu.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FB_WLD_HD __host__ __device__ __forceinline__
#else
#define FB_WLD_HD inline
#endif

namespace fbk {

constexpr uint32_t kWlDomExact = 0u, kWlDomSuffix = 1u, kWlDomPrefix = 2u, kWlDomGeneral = 3u, kWlDomNever = 4u,
                   kWlDomKinds = 5u, kWlDomHashed = 3u;  // the first three kinds have a hashed table
constexpr uint32_t kWlDomNone = 0xFFFFFFFFu;             // an unused word of a row while it is being filled
constexpr unsigned long long kWlDomBase = 0x9E3779B97F4A7C15ull;

// (hash, base^length) of a byte string; the identity is {0, 1}
struct WlDomHash {
    unsigned long long h, p;
};
FB_WLD_HD WlDomHash wl_dom_join(const WlDomHash& l, const WlDomHash& r) { return {l.h * r.p + r.h, l.p * r.p}; }
FB_WLD_HD WlDomHash wl_dom_byte(uint32_t b) { return {(unsigned long long)b + 1ull, kWlDomBase}; }
FB_WLD_HD uint32_t wl_dom_lower(uint32_t b) { return b - 'A' < 26u ? b + 32u : b; }
FB_WLD_HD unsigned long long wl_dom_hash(const uint8_t* p, uint32_t n) {
    WlDomHash x = {0ull, 1ull};
    for (uint32_t k = 0; k < n; ++k) x = wl_dom_join(x, wl_dom_byte(p[k]));
    return x.h;
}

struct WlDomTables {
    const uint8_t* blob;              // the patterns' bytes
    const uint32_t* off;              // [n_patterns + 1]: pattern id p is blob[off[p - 1], off[p])
    const unsigned long long* hash[kWlDomHashed];  // per kind, ascending by (hash, len, pid)
    const uint32_t* len[kWlDomHashed];             // length of the compared part
    const uint32_t* pid[kWlDomHashed];
    uint32_t n[kWlDomHashed];
    const uint32_t* gpid;             // [ng] the general patterns, ids ascending
    const uint32_t* gstar;            // [ng] where each has its '*'
    uint32_t ng, n_patterns;
    unsigned long long mask;
};

// The first entry of kind t not below (h, l).
FB_WLD_HD uint32_t wl_dom_lower_bound(const WlDomTables& T, uint32_t t, unsigned long long h, uint32_t l) {
    const unsigned long long* H = T.hash[t];
    const uint32_t* Ln = T.len[t];
    uint32_t lo = 0u, hi = T.n[t];
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const unsigned long long v = H[mid];
        if (v < h || (v == h && Ln[mid] < l)) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}
// Every pattern of kind t whose compared part equals name[start, start + l) (hash h, unmasked): hit(pattern id).
// The caller has start + l <= the name's length.
template <class Hit>
FB_WLD_HD void wl_dom_lookup(const WlDomTables& T, uint32_t t, unsigned long long h, const uint8_t* name, uint32_t start,
                             uint32_t l, Hit&& hit) {
    h &= T.mask;
    const uint32_t n = T.n[t], skip = t == kWlDomSuffix ? 2u : 0u;
    for (uint32_t i = wl_dom_lower_bound(T, t, h, l); i < n && T.hash[t][i] == h && T.len[t][i] == l; ++i) {
        const uint32_t pid = T.pid[t][i];
        const uint8_t* p = T.blob + T.off[pid - 1u] + skip;
        uint32_t k = 0u;
        while (k < l && p[k] == name[start + k]) ++k;
        if (k == l) hit(pid);
    }
}
// General pattern g (a*b) against the name of length L.
FB_WLD_HD bool wl_dom_general(const WlDomTables& T, uint32_t g, const uint8_t* name, uint32_t L) {
    const uint32_t pid = T.gpid[g], o = T.off[pid - 1u], la = T.gstar[g], lb = T.off[pid] - o - la - 1u;
    if ((unsigned long long)la + lb >= L) return false;
    const uint8_t* p = T.blob + o;
    for (uint32_t k = 0; k < la; ++k)
        if (p[k] != name[k]) return false;
    for (uint32_t k = 0; k < lb; ++k)
        if (p[la + 1u + k] != name[L - lb + k]) return false;
    return true;
}

// ---- the per-flow side (wl_eval<.., kDom>, fb_wl_match.h) ---------------------------------------------
// The match state of the stored names: rows[id * FB_WL_NAME_MATCHES] the matched pattern ids ascending,
// zero-padded; flags[id] bit 0: more matched than the row holds.  Valid for ids 1 .. n_names; plane: the domain
// plane (null: no domain pass has run -- no flow has a domain).
struct WlDomFlows {
    const fb_flow_domain* plane;
    const uint32_t* rows;
    const uint8_t* flags;
    uint32_t n_names;
};

// ---- host only: the pattern index and the match of one name -------------------------------------------
struct WlDomIndex {
    std::vector<uint8_t> blob;
    std::vector<uint32_t> off;
    std::vector<unsigned long long> hash[kWlDomHashed];
    std::vector<uint32_t> len[kWlDomHashed], pid[kWlDomHashed], gpid, gstar;
    uint32_t count[kWlDomKinds] = {};
    unsigned long long mask = ~0ull;
    uint32_t n_patterns() const { return off.empty() ? 0u : (uint32_t)off.size() - 1u; }
    WlDomTables tables() const {
        WlDomTables t = {};
        t.blob = blob.data();
        t.off = off.data();
        for (uint32_t k = 0; k < kWlDomHashed; ++k) {
            t.hash[k] = hash[k].data();
            t.len[k] = len[k].data();
            t.pid[k] = pid[k].data();
            t.n[k] = (uint32_t)pid[k].size();
        }
        t.gpid = gpid.data();
        t.gstar = gstar.data();
        t.ng = (uint32_t)gpid.size();
        t.n_patterns = n_patterns();
        t.mask = mask;
        return t;
    }
};
// The kind of a pattern; general: *star is where its '*' stands.
inline uint32_t wl_dom_classify(const uint8_t* p, uint32_t n, uint32_t* star) {
    uint32_t stars = 0u;
    for (uint32_t k = 0; k < n; ++k)
        if (p[k] == '*') {
            if (stars++ == 0u) *star = k;
        }
    if (stars == 0u) return kWlDomExact;
    if (n >= 2u && p[0] == '*' && p[1] == '.') return kWlDomSuffix;
    if (n >= 2u && p[n - 2u] == '.' && p[n - 1u] == '*') return kWlDomPrefix;
    return stars == 1u ? kWlDomGeneral : kWlDomNever;
}
// false: offsets that do not ascend from 0, a blob of 2^32 bytes or more, more than 2^24 - 1 patterns or more
// than FB_WL_MAX_GENERAL general ones.
inline bool build_wl_dom_index(const uint8_t* bytes, const uint64_t* off, uint64_t n_patterns, unsigned long long mask,
                               WlDomIndex& ix) {
    if (n_patterns > (1u << 24) - 1u) return false;
    ix = WlDomIndex();
    ix.mask = mask;
    if (n_patterns == 0u) return true;
    if (off[0] != 0u) return false;
    for (uint64_t p = 0; p < n_patterns; ++p)
        if (off[p + 1u] < off[p]) return false;
    if (off[n_patterns] >= (1ull << 32)) return false;
    ix.blob.assign(bytes, bytes + off[n_patterns]);
    ix.off.assign(off, off + n_patterns + 1u);
    struct Ent {
        unsigned long long h;
        uint32_t len, pid;
    };
    std::vector<Ent> ents[kWlDomHashed];
    for (uint32_t p = 1u; p <= n_patterns; ++p) {
        const uint8_t* s = ix.blob.data() + ix.off[p - 1u];
        const uint32_t n = ix.off[p] - ix.off[p - 1u];
        uint32_t star = 0u;
        const uint32_t kind = wl_dom_classify(s, n, &star);
        ++ix.count[kind];
        if (kind == kWlDomGeneral) {
            ix.gpid.push_back(p);
            ix.gstar.push_back(star);
        } else if (kind < kWlDomHashed) {
            const uint32_t skip = kind == kWlDomSuffix ? 2u : 0u, l = kind == kWlDomExact ? n : n - 2u;
            ents[kind].push_back(Ent{wl_dom_hash(s + skip, l) & mask, l, p});
        }
    }
    if (ix.gpid.size() > FB_WL_MAX_GENERAL) return false;
    for (uint32_t k = 0; k < kWlDomHashed; ++k) {
        std::sort(ents[k].begin(), ents[k].end(), [](const Ent& x, const Ent& y) {
            return x.h != y.h ? x.h < y.h : x.len != y.len ? x.len < y.len : x.pid < y.pid;
        });
        for (const Ent& e : ents[k]) {
            ix.hash[k].push_back(e.h);
            ix.len[k].push_back(e.len);
            ix.pid[k].push_back(e.pid);
        }
    }
    return true;
}
// One more matched id into a row filled with kWlDomNone: the least FB_WL_NAME_MATCHES stay, ascending.
inline void wl_dom_row_insert(uint32_t* row, uint32_t pid, bool& overflow) {
    for (uint32_t s = 0; s < FB_WL_NAME_MATCHES; ++s)
        if (pid < row[s]) std::swap(pid, row[s]);
    overflow |= pid != kWlDomNone;
}
// The row and the flags byte of the name raw[0, L), L <= FB_DNS_MAX_NAME, as the kernel leaves them.
inline void wl_dom_match_name(const WlDomTables& T, const uint8_t* raw, uint32_t L, uint32_t* row, uint8_t* flags) {
    uint8_t name[FB_DNS_MAX_NAME + 1u];
    WlDomHash pre[FB_DNS_MAX_NAME + 2u], suf[FB_DNS_MAX_NAME + 2u];  // of name[:k] and of name[k:]
    for (uint32_t k = 0; k < L; ++k) name[k] = (uint8_t)wl_dom_lower(raw[k]);
    pre[0] = {0ull, 1ull};
    for (uint32_t k = 0; k < L; ++k) pre[k + 1u] = wl_dom_join(pre[k], wl_dom_byte(name[k]));
    suf[L] = {0ull, 1ull};
    for (uint32_t k = L; k-- > 0u;) suf[k] = wl_dom_join(wl_dom_byte(name[k]), suf[k + 1u]);
    bool overflow = false;
    for (uint32_t s = 0; s < FB_WL_NAME_MATCHES; ++s) row[s] = kWlDomNone;
    auto hit = [&](uint32_t pid) { wl_dom_row_insert(row, pid, overflow); };
    wl_dom_lookup(T, kWlDomExact, pre[L].h, name, 0u, L, hit);
    wl_dom_lookup(T, kWlDomPrefix, pre[L].h, name, 0u, L, hit);
    for (uint32_t i = 0; i < L; ++i) {
        if (name[i] != '.') continue;
        wl_dom_lookup(T, kWlDomSuffix, suf[i + 1u].h, name, i + 1u, L - i - 1u, hit);
        wl_dom_lookup(T, kWlDomPrefix, pre[i].h, name, 0u, i, hit);
    }
    for (uint32_t g = 0; g < T.ng; ++g)
        if (wl_dom_general(T, g, name, L)) hit(T.gpid[g]);
    for (uint32_t s = 0; s < FB_WL_NAME_MATCHES; ++s)
        if (row[s] == kWlDomNone) row[s] = 0u;
    *flags = overflow ? 1u : 0u;
}

}  // namespace fbk
