// fb_dns_hash.h -- the two tag functions of the DNS tracker (fb_dnstrack.hip): the single
// definition of a name's and an address's 64-bit tag, for the kernels (the tracker's inserts and rebuilds,
// dns_lookup in fb_internal.h) and for host programs alike.  Plain C++: nothing of HIP is needed when a host
// compiler includes it (FB_DNSH_HD is `inline` there, `__host__ __device__ inline` under hipcc -- as
// fb_zeek_fmt.h does it).
//
// A tag is the masked hash with bit 63 set (0 is the empty slot); a key's home slot is tag & (slots - 1).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define FB_DNSH_HD __host__ __device__ inline
#else
#define FB_DNSH_HD inline
#endif

namespace fbk {

constexpr unsigned long long kDnsTagUsed = 1ull << 63;

// dword k of a name of `len` bytes, the bytes past the length zeroed (the parse leaves them unspecified)
FB_DNSH_HD uint32_t name_dword(const uint32_t* nm, uint32_t k, uint32_t len) {
    const uint32_t w = nm[k], rest = len - 4u * k;
    return rest >= 4u ? w : (w & ((1u << (8u * rest)) - 1u));
}
FB_DNSH_HD unsigned long long name_tag(const uint32_t* nm, uint32_t len, unsigned long long hash_mask) {
    unsigned long long h = 0x9E3779B97F4A7C15ull ^ len;
    const uint32_t nd = (len + 3u) >> 2;
    for (uint32_t k = 0; k < nd; ++k) {
        h ^= name_dword(nm, k, len);
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 31;
    }
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    return (h & hash_mask) | kDnsTagUsed;
}
// (4 address words, family): a v4 and a v6 key with equal words differ in the family
FB_DNSH_HD unsigned long long dns_addr_tag(const uint32_t w[4], uint32_t family, unsigned long long hash_mask) {
    unsigned long long h = 0x9E3779B97F4A7C15ull ^ family;
    for (int j = 0; j < 4; j += 2) {
        h ^= (unsigned long long)w[j] | ((unsigned long long)w[j + 1] << 32);
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 31;
    }
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    return (h & hash_mask) | kDnsTagUsed;
}

}  // namespace fbk
