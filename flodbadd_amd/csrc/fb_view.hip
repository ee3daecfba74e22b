// fb_view.hip -- the view export (fb_flow_export_view_dev): one sweep over the table that selects flows
// and writes, per selected flow, one 256-B fb_flow_view -- its flow record, its time record and its element
// of every per-slot plane, joined on the device.
//
// It is what the reference's incremental getters need (get_sessions / get_current_sessions /
// get_blacklisted_sessions / get_whitelist_exceptions with `incremental`, src/capture.rs:1578-1760): they
// return the sessions of one collection whose last_modified is newer than the getter's last full fetch
// (`<= last_fetch_ts -> skip`).  Here last_modified = max(last_activity_ns, stamp): the packet path's part
// is already in the time plane, the passes' part is the stamp plane (fb_capi.hip kPlaneMod, written by the
// stamped instances of the three pass kernels).
//
// The two sides of the kernel have different shapes:
//   predicate  one lane per slot, like every sweep: the 128-B table line (tag and key), then only what
//              the query needs -- one plane element for the set, 8 B of the 64-B time record and the 8-B
//              stamp for FB_VIEW_MODIFIED_SINCE;
//   copy-out   256 B per selected flow gathered from six arrays.  One lane storing its own record
//              issues sixteen 16-B stores 256 B apart from its neighbours' (every store instruction of
//              the wave touches 64 lines).  Instead the selected flows of a step take consecutive
//              ranks (ballot + LDS sums, as sweep_compact), each lane builds its record into LDS at its
//              rank, and the whole workgroup then writes the step's records -- one contiguous range of
//              the output -- in 16-B columns: consecutive lanes, consecutive 16 B.
// LDS rows are 272 B apart (68 words): the sixteen lanes of one 16-B write phase then fall on sixteen
// different 4-bank groups instead of all on the same one.  A round stages kViewStage records (34 KiB),
// so a full step of 256 selected flows takes two rounds and four workgroups fit a CU.
// Nothing here waits on another workgroup: the only inter-workgroup traffic is one atomicAdd per step.
#include "fb_internal.h"

namespace fbk {

namespace {

constexpr uint32_t kViewStage = 128;            // records staged per round
constexpr uint32_t kViewRow = 272;              // LDS bytes per staged record (256 + one 16-B column)
constexpr uint32_t kViewCols = sizeof(fb_flow_view) / 16u;

// The view record of slot i.  (The predicate, view_take, is in fb_internal.h: fb_learn.hip selects by it too.)
__device__ __forceinline__ void view_of(const ViewArgs& a, unsigned long long i, fb_flow_view& v) {
    v.rec = flow_rec_at(a.table, a.time, i);
    if (a.time) {
        v.time = a.time[i];
    } else {
        v.time = fb_flow_time();
    }
    v.time.slot = (uint32_t)i;
    v.stamp_ns = a.mod ? a.mod[i] : 0ull;
    const unsigned long long act = a.time ? v.time.last_activity_ns : 0ull;
    v.last_modified_ns = act > v.stamp_ns ? act : v.stamp_ns;
    v.bl_mask = a.bl ? a.bl[i] : 0ull;
    if (a.an) {
        v.an = a.an[i];
    } else {
        v.an = fb_an_rec();
    }
    v.status = a.status ? a.status[i] : (uint8_t)0;
    v.wl_state = a.wl ? a.wl[i] : (uint8_t)0;
#pragma unroll
    for (int k = 0; k < 14; ++k) v.reserved[k] = 0u;
}

// The sweep's step, as sweep_compact: the ranks of the step's selected slots (slot order) and the output
// position of rank 0 (one atomic per workgroup and step; the count is added whether or not it fits).
struct StepRanks {
    uint32_t rank;            // of this lane's slot among the step's selected ones (when taken)
    uint32_t total;           // selected slots of the step
    unsigned long long base;  // output position of rank 0
};
__device__ __forceinline__ StepRanks step_ranks(bool taken, unsigned long long* d_n, uint32_t (&sh)[4],
                                                unsigned long long& s_base) {
    const unsigned long long m = __ballot(taken);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) sh[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    StepRanks r;
    r.total = sh[0] + sh[1] + sh[2] + sh[3];
    if (threadIdx.x == 0) s_base = r.total ? atomicAdd(d_n, (unsigned long long)r.total) : 0ull;
    r.rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) r.rank += sh[w];
    __syncthreads();
    r.base = s_base;
    return r;
}

}  // namespace

template <bool kStaged>
__global__ __launch_bounds__(256) void k_flow_view(const ViewArgs a, fb_flow_view* out, unsigned long long out_cap,
                                                   unsigned long long* d_n) {
    __shared__ uint32_t sh[4];
    __shared__ unsigned long long s_base;
    __shared__ uint4 s_stage[kStaged ? kViewStage * kViewRow / 16u : 1u];
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < a.cap; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        const bool taken = i < a.cap && a.table[i].tag >= 2u && view_take(a, i);
        const StepRanks r = step_ranks(taken, d_n, sh, s_base);
        if (!kStaged) {
            if (taken && r.base + r.rank < out_cap) view_of(a, i, out[r.base + r.rank]);
            continue;
        }
        // the records that fit the output: ranks [0, fit)
        const unsigned long long room = r.base < out_cap ? out_cap - r.base : 0ull;
        const uint32_t fit = (uint32_t)(room < r.total ? room : r.total);
        for (uint32_t first = 0; first < fit; first += kViewStage) {  // (uniform over the workgroup)
            const uint32_t n = fit - first < kViewStage ? fit - first : kViewStage;
            if (taken && r.rank >= first && r.rank < first + n)
                view_of(a, i, *reinterpret_cast<fb_flow_view*>(reinterpret_cast<char*>(s_stage) +
                                                               (size_t)(r.rank - first) * kViewRow));
            __syncthreads();
            uint4* dst = reinterpret_cast<uint4*>(out + r.base + first);
            for (uint32_t c = threadIdx.x; c < n * kViewCols; c += 256u)
                dst[c] = s_stage[(c / kViewCols) * (kViewRow / 16u) + (c % kViewCols)];
            __syncthreads();
        }
    }
}

hipError_t launch_flow_view(const ViewArgs& a, fb_flow_view* out, unsigned long long out_cap, unsigned long long* d_n,
                            bool staged, hipStream_t s) {
    if (!view_args_valid(a) || !d_n || (out_cap && !out)) return hipErrorInvalidValue;
    const dim3 g(sweep_grid(a.cap, 1024ull));
    hipLaunchKernelGGL(staged ? k_flow_view<true> : k_flow_view<false>, g, dim3(256), 0, s, a, out, out_cap, d_n);
    return hipGetLastError();
}

}  // namespace fbk
