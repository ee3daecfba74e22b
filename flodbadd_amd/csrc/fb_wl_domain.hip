// fb_wl_domain.hip -- the names of the DNS tracker matched against the whitelist's domain patterns
// (fb_set_whitelist_dom): domain_matches (src/whitelists.rs:602-679) of every (name, pattern)
// pair, once per name.  Names are far fewer than flows and their ids never change, so the string work happens
// here, when a name first appears, and the per-flow pass (fb_whitelist.hip, kDom) only looks ids up.  The
// classification, the tables and the byte comparison are fb_wl_domain.h's -- one definition for this kernel and
// for the host.
//
// One wavefront per name.  The store's 256 B per id are one dword per lane; the lower-cased bytes go to LDS.
// Two wave scans of the per-lane (hash, power) element give the hash of every prefix and of every suffix of the
// name.  The candidates -- the whole name (exact, prefix), and at every dot what follows it (suffix) and what
// precedes it (prefix) -- take one lane each, byte positions lane, lane + 64, ...; a candidate bisects its
// kind's table to the run of its (hash, length) and compares bytes with every pattern of the run.  The general
// patterns are scanned, lane, lane + 64, ...  Every hit goes through a chain of LDS atomicMin over the row's
// eight words, which leaves the least eight ids ascending whatever order the lanes arrive in; an id that falls
// off the end sets the overflow flag.
#include "fb_internal.h"

namespace fbk {

namespace {

constexpr uint32_t kNamesPerBlock = 4u;  // one per wavefront of a 256-thread workgroup
constexpr uint32_t kNameDwords = FB_DNS_MAX_NAME / 4u;
static_assert(kNameDwords == 64u, "one dword of the name per lane");

__device__ __forceinline__ WlDomHash shfl_up(const WlDomHash& v, uint32_t d) {
    return {__shfl_up(v.h, d), __shfl_up(v.p, d)};
}
__device__ __forceinline__ WlDomHash shfl_down(const WlDomHash& v, uint32_t d) {
    return {__shfl_down(v.h, d), __shfl_down(v.p, d)};
}

// ctr[0]: names with a non-empty row, ctr[1]: names with the overflow flag (of the ids this launch matched).
__global__ __launch_bounds__(256) void k_wl_name_match(const WlDomTables T, const uint32_t* names, const uint16_t* name_len,
                                                       uint32_t first, uint32_t last, uint32_t* rows, uint8_t* flags,
                                                       unsigned long long* ctr) {
    __shared__ uint32_t s_name[kNamesPerBlock][kNameDwords];
    __shared__ unsigned long long s_pre[kNamesPerBlock][FB_DNS_MAX_NAME + 1u];  // hash of name[:k]
    __shared__ unsigned long long s_suf[kNamesPerBlock][FB_DNS_MAX_NAME + 1u];  // hash of name[k:]
    __shared__ uint32_t s_row[kNamesPerBlock][FB_WL_NAME_MATCHES + 1u];         // the row, then the overflow word
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const WlDomHash one = {0ull, 1ull};
    // (every wavefront of a workgroup makes the same number of trips: the barriers are the workgroup's)
    for (unsigned long long base = (unsigned long long)first + (unsigned long long)blockIdx.x * kNamesPerBlock; base <= last;
         base += (unsigned long long)gridDim.x * kNamesPerBlock) {
        const unsigned long long id = base + wave;
        const bool live = id <= last;
        uint32_t L = 0u;
        if (live) {
            L = min((uint32_t)name_len[id], FB_DNS_MAX_NAME);
            const uint32_t w = names[id * kNameDwords + lane];
            uint32_t b[4], lw = 0u;
            WlDomHash e = one;
            for (uint32_t j = 0; j < 4u; ++j) {
                b[j] = 4u * lane + j < L ? wl_dom_lower((w >> (8u * j)) & 0xFFu) : 0u;
                lw |= b[j] << (8u * j);
                if (4u * lane + j < L) e = wl_dom_join(e, wl_dom_byte(b[j]));
            }
            s_name[wave][lane] = lw;
            if (lane <= FB_WL_NAME_MATCHES) s_row[wave][lane] = lane < FB_WL_NAME_MATCHES ? kWlDomNone : 0u;
            WlDomHash pre = e, suf = e;  // inclusive scans: lanes 0 .. lane, lanes lane .. 63
            for (uint32_t d = 1u; d < 64u; d <<= 1) {
                const WlDomHash u = shfl_up(pre, d), v = shfl_down(suf, d);
                if (lane >= d) pre = wl_dom_join(u, pre);
                if (lane + d < 64u) suf = wl_dom_join(suf, v);
            }
            WlDomHash x = shfl_up(pre, 1u), y = shfl_down(suf, 1u);  // exclusive
            if (lane == 0u) x = one;
            if (lane == 63u) y = one;
            for (uint32_t j = 0; j < 4u; ++j) {
                s_pre[wave][4u * lane + j] = x.h;
                if (4u * lane + j < L) x = wl_dom_join(x, wl_dom_byte(b[j]));
            }
            for (uint32_t j = 4u; j-- > 0u;) {
                if (4u * lane + j < L) y = wl_dom_join(wl_dom_byte(b[j]), y);
                s_suf[wave][4u * lane + j] = y.h;
            }
            if (lane == 63u) {
                s_pre[wave][FB_DNS_MAX_NAME] = x.h;
                s_suf[wave][FB_DNS_MAX_NAME] = 0ull;
            }
        }
        __syncthreads();
        if (live) {
            const uint8_t* name = reinterpret_cast<const uint8_t*>(s_name[wave]);
            uint32_t* row = s_row[wave];
            auto hit = [&](uint32_t pid) {
                uint32_t v = pid;  // each word keeps the lesser and passes the greater on
                for (uint32_t s = 0; s < FB_WL_NAME_MATCHES && v != kWlDomNone; ++s) {
                    const uint32_t old = atomicMin(&row[s], v);
                    v = old > v ? old : v;
                }
                if (v != kWlDomNone) row[FB_WL_NAME_MATCHES] = 1u;
            };
            if (lane == 0u) {
                wl_dom_lookup(T, kWlDomExact, s_pre[wave][L], name, 0u, L, hit);
                wl_dom_lookup(T, kWlDomPrefix, s_pre[wave][L], name, 0u, L, hit);
            }
            for (uint32_t k = lane; k < L; k += 64u) {
                if (name[k] != '.') continue;
                wl_dom_lookup(T, kWlDomSuffix, s_suf[wave][k + 1u], name, k + 1u, L - k - 1u, hit);
                wl_dom_lookup(T, kWlDomPrefix, s_pre[wave][k], name, 0u, k, hit);
            }
            for (uint32_t g = lane; g < T.ng; g += 64u)
                if (wl_dom_general(T, g, name, L)) hit(T.gpid[g]);
        }
        __syncthreads();
        if (live) {
            if (lane < FB_WL_NAME_MATCHES) {
                const uint32_t v = s_row[wave][lane];
                rows[id * FB_WL_NAME_MATCHES + lane] = v == kWlDomNone ? 0u : v;
            }
            if (lane == 0u) {
                const bool over = s_row[wave][FB_WL_NAME_MATCHES] != 0u;
                flags[id] = over ? 1u : 0u;
                if (s_row[wave][0] != kWlDomNone) atomicAdd(ctr, 1ull);
                if (over) atomicAdd(ctr + 1, 1ull);
            }
        }
        __syncthreads();
    }
}

// The rows of the given ids: a zero row for id 0 and for an id past `upto` (the ids whose rows are valid).
__global__ __launch_bounds__(256) void k_wl_name_rows(const uint32_t* ids, unsigned long long n, const uint32_t* rows,
                                                      const uint8_t* flags, uint32_t upto, uint32_t* out_rows,
                                                      uint8_t* out_flags) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * FB_WL_NAME_MATCHES) return;
    const unsigned long long k = i / FB_WL_NAME_MATCHES;
    const uint32_t j = (uint32_t)(i % FB_WL_NAME_MATCHES), id = ids[k];
    const bool have = id != 0u && id <= upto;
    out_rows[i] = have ? rows[(unsigned long long)id * FB_WL_NAME_MATCHES + j] : 0u;
    if (j == 0u) out_flags[k] = have ? flags[id] : 0u;
}

}  // namespace

#ifndef FB_WLD_GRID
#define FB_WLD_GRID 4096ull
#endif
hipError_t launch_wl_name_match(const WlDomTables& t, const uint32_t* names, const uint16_t* name_len, uint32_t first,
                                uint32_t last, uint32_t* rows, uint8_t* flags, unsigned long long* ctr, hipStream_t s) {
    if (first == 0u || last < first) return hipSuccess;
    if (!names || !name_len || !rows || !flags || !ctr || !t.off) return hipErrorInvalidValue;
    const unsigned long long blocks = ((unsigned long long)(last - first) + kNamesPerBlock) / kNamesPerBlock;
    hipLaunchKernelGGL(k_wl_name_match, dim3((uint32_t)std::min<unsigned long long>(blocks, FB_WLD_GRID)), dim3(256), 0, s, t,
                       names, name_len, first, last, rows, flags, ctr);
    return hipGetLastError();
}

hipError_t launch_wl_name_rows(const uint32_t* ids, unsigned long long n, const uint32_t* rows, const uint8_t* flags,
                               uint32_t upto, uint32_t* out_rows, uint8_t* out_flags, hipStream_t s) {
    if (n == 0ull) return hipSuccess;
    const unsigned long long threads = n * FB_WL_NAME_MATCHES;
    hipLaunchKernelGGL(k_wl_name_rows, dim3((uint32_t)((threads + 255ull) / 256ull)), dim3(256), 0, s, ids, n, rows, flags, upto,
                       out_rows, out_flags);
    return hipGetLastError();
}

}  // namespace fbk
