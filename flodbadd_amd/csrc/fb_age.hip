// fb_age.hip -- session aging on a timed context (fb_flow_age): the reference's update_sessions_status
// (src/capture.rs:1497-1551, constants src/sessions.rs:10-15) over the whole table in one pass --
// every flow's SessionStatus {active, added, activated, deactivated}, its membership of
// current_sessions, and the removal of the flows whose last activity is older than the retention span.
//
// The status lives in a plane of its own, one byte per table slot (fb_internal.h, kAge*): FlowSlot,
// the time plane and the update kernels are untouched.  A zero byte is a flow no aging call has seen
// since its insert and stands for the reference's insert status (src/packets.rs:497-502: active, added,
// activated) and a member of current_sessions (src/packets.rs:532).
#include "fb_internal.h"

namespace fbk {

namespace {

// Sum of a per-thread flag over the workgroup's waves: lane 0 of each wave leaves the wave's count.
__device__ __forceinline__ void wave_count(bool f, uint32_t* dst) {
    const unsigned long long m = __ballot(f);
    if ((threadIdx.x & 63u) == 0u) *dst = (uint32_t)__popcll(m);
}

}  // namespace

// One workgroup per partition, one slot per thread (k_flow_grow's geometry).
//
// Status (every occupied slot): reads the slot's tag and the start / last activity times of its time
// record, writes one byte.  The comparisons are the reference's (capture.rs:1514-1536) with the span
// moved to the time's side and the sums taken in 128 bits, so neither a capture time after `now` nor a
// span near 2^64 wraps:
//   active      last  + activity  >= now        (last_activity >= now - CONNECTION_ACTIVITY_TIMEOUT)
//   added       start + activity  >= now
//   current     now <  last + current           (strict)
//   expired     now >  last + retention         (strict)
//   activated   !previous.active && active;  deactivated  previous.active && !active
//
// Purge (A.purge): a partition none of whose flows expired is not written.  Any other is rebuilt IN
// PLACE: every thread loads its whole slot, time record, character-call entry and new status byte into
// registers; after a barrier the survivors claim a position by linear probing from their unchanged home
// slot on an LDS array (k_flow_grow with k = 0), and after a second barrier write their registers there;
// every position nobody claimed gets a zeroed slot and a zero status byte (its time record and
// character-call entry stay stale, as after fb_flow_clear: an insert rewrites them).  In place is safe
// because every read of the partition completes before the first barrier (the loads are waited for in
// front of it) and every destination has exactly one writer: position j is written by the
// one survivor whose claim took j, or, unclaimed, by thread j.  No other workgroup touches the partition.
__global__ __launch_bounds__(kFlowSlots) void k_flow_age(AgeArgs A) {
    __shared__ uint32_t claim[kFlowSlots];
    __shared__ uint32_t cnt[kFlowSlots / 64u][kAgeCounters];
    const uint32_t p = blockIdx.x, i = threadIdx.x, wave = i >> 6;
    const size_t g = (size_t)p * kFlowSlots + i;
    claim[i] = 0u;
    const bool occ = A.table[g].tag >= 2u;
    uint32_t nb = 0u;
    bool expired = false;
    if (occ) {
        const unsigned long long start = A.plane[g].start_time_ns, last = A.plane[g].last_activity_ns;
        const uint32_t old = A.status[g];
        typedef unsigned __int128 u128;
        const bool prev_active = (old & kAgeAged) ? (old & kAgeActive) != 0u : true;
        const bool active = (u128)last + A.activity >= (u128)A.now;
        const bool added = (u128)start + A.activity >= (u128)A.now;
        const bool current = (u128)A.now < (u128)last + A.current;
        expired = (u128)A.now > (u128)last + A.retention;
        nb = kAgeAged | (active ? kAgeActive : 0u) | (added ? kAgeAdded : 0u) |
             ((!prev_active && active) ? kAgeActivated : 0u) | ((prev_active && !active) ? kAgeDeactivated : 0u) |
             (current ? kAgeCurrent : 0u);
    }
    wave_count(occ, &cnt[wave][0]);
    wave_count(nb & kAgeActive, &cnt[wave][1]);
    wave_count(nb & kAgeAdded, &cnt[wave][2]);
    wave_count(nb & kAgeActivated, &cnt[wave][3]);
    wave_count(nb & kAgeDeactivated, &cnt[wave][4]);
    wave_count(nb & kAgeCurrent, &cnt[wave][5]);
    wave_count(expired, &cnt[wave][6]);
    __syncthreads();
    uint32_t n_expired = 0u;
    for (uint32_t w = 0; w < kFlowSlots / 64u; ++w) n_expired += cnt[w][6];
    const bool rebuild = A.purge && n_expired != 0u;  // uniform over the workgroup
    if (i < kAgeCounters) {  // one atomic per counter per workgroup
        unsigned long long t = 0ull;
        for (uint32_t w = 0; w < kFlowSlots / 64u; ++w) t += cnt[w][i];
        if (i == 6u && !A.purge) t = 0ull;  // `purged`: nothing is removed without the flag
        if (t) atomicAdd(A.stats + i, t);
        if (i == 0u) {  // occupancy after the call
            const unsigned long long rem = t - (A.purge ? n_expired : 0u);
            if (rem) {
                atomicAdd(A.stats + 7, rem);
                atomicMax(A.stats + 8, rem);
            }
        }
    }
    if (!rebuild) {
        if (occ) A.status[g] = (uint8_t)nb;
        if (A.purge) A.remap[g] = occ ? (uint32_t)g : ~0u;
        return;
    }
    // ---- rebuild the partition in place ----
    const bool keep = occ && !expired;
    uint4 sl[8], cc = make_uint4(0u, 0u, 0u, 0u);
    const uint4* tsrc = reinterpret_cast<const uint4*>(A.plane + g);
    const uint4 tm0 = tsrc[0], tm1 = tsrc[1], tm2 = tsrc[2], tm3 = tsrc[3];  // (named: an array went to LDS)
    {
        const uint4* s = reinterpret_cast<const uint4*>(A.table + g);
#pragma unroll
        for (int k = 0; k < 8; ++k) sl[k] = s[k];
        if (A.char_call) cc = A.char_call[g];
    }
    // every load above has returned its data before this thread arrives at the barrier, so no thread's
    // write below can reach a slot that is still to be read (the barrier's own workgroup-scope fence
    // does not wait for loads whose values are not used yet)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    uint32_t j = ~0u;
    if (keep) {
        // key words 0-9 follow tag and segment_count: sl[0].zw, sl[1], sl[2]
        const uint32_t key[10] = {sl[0].z, sl[0].w, sl[1].x, sl[1].y, sl[1].z, sl[1].w, sl[2].x, sl[2].y, sl[2].z, sl[2].w};
        j = (uint32_t)flow_hash_words(key) & (kFlowSlots - 1u);
        while (atomicCAS(&claim[j], 0u, 1u) != 0u) j = (j + 1u) & (kFlowSlots - 1u);  // <= 512 survivors: terminates
    }
    __syncthreads();
    if (keep) {
        const size_t d = (size_t)p * kFlowSlots + j;
        uint4* s = reinterpret_cast<uint4*>(A.table + d);
        uint4* t = reinterpret_cast<uint4*>(A.plane + d);
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = sl[k];
        t[0] = tm0;
        t[1] = tm1;
        t[2] = tm2;
        t[3] = tm3;
        if (A.char_call) A.char_call[d] = cc;
        A.status[d] = (uint8_t)nb;
    }
    if (claim[i] == 0u) {  // nobody's destination: an empty slot
        uint4* s = reinterpret_cast<uint4*>(A.table + g);
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = make_uint4(0u, 0u, 0u, 0u);
        A.status[g] = 0u;
    }
    A.remap[g] = keep ? (uint32_t)((size_t)p * kFlowSlots + j) : ~0u;
}

hipError_t launch_flow_age(const AgeArgs& a, uint32_t parts, hipStream_t s) {
    if (!a.table || !a.plane || !a.status || !a.stats || (a.purge && !a.remap) || parts == 0u)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_flow_age, dim3(parts), dim3(kFlowSlots), 0, s, a);
    return hipGetLastError();
}

}  // namespace fbk
