// fb_domains.hip -- the domain pass over every flow of the table (fb_flow_domains): the reference's
// populate_domain_names (src/capture.rs:1307-1411) as update_sessions_internal runs it between populate_l7
// and the blacklist pass (src/capture.rs:1824-1848), restricted to the passive resolutions: the reference
// also asks its active resolver for reverse lookups, which is network I/O.
//
// The reference walks current_sessions only (src/capture.rs:1322-1331), looks each side's address up in
// dns_resolutions, and writes src_domain / dst_domain where the lookup gave a name that is neither "Unknown"
// nor "Resolving" and differs from the stored one (src/capture.rs:1381-1396); a session with either side
// written gets last_modified = now (src/capture.rs:1397-1399).  Nothing is ever unset.  Here a name is its
// id in the tracker's store (fb_dnstrack.hip), so "differs" is one integer compare, and the two excluded
// strings are compared against the store's bytes only when a write is about to happen.
//
// The ids live in a per-slot plane of their own: FlowSlot and the update kernels are
// untouched, and a zero pair (no pass has seen the flow) is the reference's insert state, no domains.
#include "fb_internal.h"

namespace fbk {

// name id `id` is the literal "Unknown" or "Resolving"
__device__ __forceinline__ bool dns_name_excluded(const DnsTables& t, uint32_t id) {
    const uint32_t len = t.name_len[id];
    const uint32_t* w = t.names + (size_t)id * (FB_DNS_MAX_NAME / 4u);
    if (len == 7u) return w[0] == 0x6E6B6E55u && w[1] == 0x006E776Fu;                         // "Unkn" "own"
    if (len == 9u) return w[0] == 0x6F736552u && w[1] == 0x6E69766Cu && w[2] == 0x00000067u;  // "Reso" "lvin" "g"
    return false;
}

// k_flow_blacklist's geometry: one lane per table slot, 256-thread workgroups striding over the table.
// Per occupied current slot one 128-B line of the table and the old pair; each side is one probe run of
// the resolutions table (dns_lookup, shared with fb_dns_lookup_dev).  The pair is stored only when it
// changed.  kStamp (a pass time is set, fb_set_pass_time): the changed flows get `now` in the stamp plane;
// the unstamped instance holds no such store.  Counters: PassCounters (fb_internal.h).
template <bool kStamp>
__global__ __launch_bounds__(256) void k_flow_domains(const DnsTables t, const FlowSlot* T, unsigned long long cap,
                                                      const uint8_t* status, uint2* dom, unsigned long long* stats,
                                                      unsigned long long* mod, unsigned long long now) {
    PassCounters<kDomCounters> cnt;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < cap; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        const bool occ = i < cap && T[i].tag >= 2u;
        bool cur = false, set_s = false, set_d = false;
        uint2 d = make_uint2(0u, 0u);
        if (occ) {
            const uint32_t sb = status ? status[i] : 0u;
            cur = sb == 0u || (sb & kAgeCurrent) != 0u;
            d = dom[i];
            if (cur) {
                const uint32_t* k = T[i].key;
                const uint32_t src[4] = {k[0], k[1], k[2], k[3]}, dst[4] = {k[4], k[5], k[6], k[7]};
                const uint32_t fam = (k[9] >> 8) & 0xFFu;
                const uint32_t ns = dns_lookup(t, src, fam), nd = dns_lookup(t, dst, fam);
                if (ns != 0u && ns != d.x && !dns_name_excluded(t, ns)) d.x = ns, set_s = true;
                if (nd != 0u && nd != d.y && !dns_name_excluded(t, nd)) d.y = nd, set_d = true;
                if (set_s || set_d) {
                    dom[i] = d;
                    if (kStamp) mod[i] = now;
                }
            }
        }
        cnt.add(0, occ);
        cnt.add(1, cur);
        cnt.add(2, set_s);
        cnt.add(3, set_d);
        cnt.add(4, set_s || set_d);
        cnt.add(5, occ && (d.x | d.y) != 0u);
    }
    cnt.flush(stats);
}

hipError_t launch_flow_domains(const DnsTables& t, const FlowSlot* table, unsigned long long cap, const uint8_t* status,
                               uint2* dom, unsigned long long* stats, hipStream_t s, unsigned long long* mod,
                               unsigned long long now) {
    if (!table || !dom || !stats || cap == 0ull || !t.atag || t.aslots == 0ull) return hipErrorInvalidValue;
    const dim3 g(sweep_grid(cap, 1024ull));
    const auto k = mod ? k_flow_domains<true> : k_flow_domains<false>;
    hipLaunchKernelGGL(k, g, dim3(256), 0, s, t, table, cap, status, dom, stats, mod, now);
    return hipGetLastError();
}

}  // namespace fbk
