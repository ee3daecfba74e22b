// fb_l7.hip -- the L7 pass over every flow of the table (fb_flow_l7): process attribution against the installed
// socket snapshot, the reference's populate_l7 (src/capture.rs:1414-1495) with one cycle of its resolver task
// (src/l7.rs:208-500) folded in, as update_sessions_internal runs it between the status update and the domain
// pass (src/capture.rs:1815-1822).
//
// The reference scans the socket list per session (resolve_l7_data, src/l7.rs:1020-1135): sessions x sockets.
// Here the snapshot is two sorted tables (fb_l7_index.h) and a session's match is ten point lookups at the
// most -- l7_match, the one definition the pass, fb_l7_lookup_dev and the host test program share.
//
// The elements live in a per-slot plane of their own: FlowSlot and the update kernels are
// untouched, and a zero element (no pass has seen the flow) is the reference's insert state, l7 = None.
#include "fb_internal.h"
#include "fb_l7_index.h"

namespace fbk {

// k_flow_domains' geometry: one lane per table slot, 256-thread workgroups striding over the table.  Per
// occupied slot the tag, the status byte and the old element; a looked-up flow reads its 128-B line (the
// key) and runs l7_match: the two exact bisections advance together, then -- only in the lanes whose exact
// phase missed -- the eight fuzzy ones.  The element is stored only when it changed.  kStamp (a pass time is
// set, fb_set_pass_time): the flows that got a process get `now` in the stamp plane; the unstamped instance
// holds no such store.  Counters: PassCounters (fb_internal.h).
template <bool kStamp>
__global__ __launch_bounds__(256) void k_flow_l7(const L7Tables t, const FlowSlot* T, unsigned long long cap,
                                                 const uint8_t* status, uint2* l7, uint32_t max_retries,
                                                 unsigned long long* stats, unsigned long long* mod,
                                                 unsigned long long now) {
    PassCounters<kL7Counters> cnt;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < cap; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        const bool occ = i < cap && T[i].tag >= 2u;
        bool cur = false, look = false, exact = false, fuzzy = false, failed = false;
        uint2 e = make_uint2(0u, 0u);
        if (occ) {
            const uint32_t sb = status ? status[i] : 0u;
            cur = sb == 0u || (sb & kAgeCurrent) != 0u;
            e = l7[i];
            look = cur && e.x == 0u && (e.y & 0xFFu) != FB_L7_FAILED;
            if (look) {
                uint32_t key[10];
#pragma unroll
                for (int j = 0; j < 10; ++j) key[j] = T[i].key[j];
                const L7Match m = l7_match(t, key);
                const uint2 old = e;
                l7_apply(m, max_retries, e.x, e.y);
                exact = m.source == FB_L7_EXACT;
                fuzzy = m.source == FB_L7_FUZZY;
                failed = (e.y & 0xFFu) == FB_L7_FAILED;
                if (e.x != old.x || e.y != old.y) l7[i] = e;
                if (kStamp && m.pid != 0u) mod[i] = now;
            }
        }
        cnt.add(0, occ);
        cnt.add(1, cur);
        cnt.add(2, look);
        cnt.add(3, exact);
        cnt.add(4, fuzzy);
        cnt.add(5, failed);
        cnt.add(6, occ && e.x != 0u);
        cnt.add(7, exact || fuzzy);
    }
    cnt.flush(stats);
}

// fb_l7_lookup_dev: l7_match of n caller-supplied keys, one lane per key.
__global__ __launch_bounds__(256) void k_l7_lookup(const L7Tables t, const uint32_t* keys, unsigned long long n,
                                                   uint2* out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t key[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) key[j] = keys[i * 10ull + j];
    const L7Match m = l7_match(t, key);
    out[i] = make_uint2(m.pid, m.source);
}

hipError_t launch_flow_l7(const L7Tables& t, const FlowSlot* table, unsigned long long cap, const uint8_t* status,
                          uint2* l7, uint32_t max_retries, unsigned long long* stats, hipStream_t s,
                          unsigned long long* mod, unsigned long long now) {
    if (!table || !l7 || !stats || cap == 0ull || max_retries > 255u) return hipErrorInvalidValue;
    if ((t.n_pairs && !t.pairs) || (t.n_locals && !t.locals)) return hipErrorInvalidValue;
    const dim3 g(sweep_grid(cap, 1024ull));
    const auto k = mod ? k_flow_l7<true> : k_flow_l7<false>;
    hipLaunchKernelGGL(k, g, dim3(256), 0, s, t, table, cap, status, l7, max_retries, stats, mod, now);
    return hipGetLastError();
}

hipError_t launch_l7_lookup(const L7Tables& t, const fb_session_key* keys, unsigned long long n, fb_l7_rec* out,
                            hipStream_t s) {
    if (n == 0ull) return hipSuccess;
    if (!keys || !out || n > 0xFFFFFFFFull * 256ull) return hipErrorInvalidValue;
    if ((t.n_pairs && !t.pairs) || (t.n_locals && !t.locals)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_l7_lookup, dim3((uint32_t)((n + 255ull) / 256ull)), dim3(256), 0, s, t,
                       reinterpret_cast<const uint32_t*>(keys), n, reinterpret_cast<uint2*>(out));
    return hipGetLastError();
}

}  // namespace fbk
