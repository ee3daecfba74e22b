// fb_zeek.hip -- the Zeek conn.log export (fb_format_zeek_dev): one text line per fb_flow_view record,
// formatted on the device (format_sessions_zeek, src/sessions.rs:694-774; the format itself is
// fb_zeek_fmt.h).
//
// Three launches, no host round trip:
//   length  one lane per record: zeek_line_len into line_off[i + 1], and the two per-record counters
//           (ts_inexact, hist_mismatch) by one atomic per wave that has any;
//   scan    rocPRIM's inclusive scan over line_off[1 .. n] in place (line_off[0] = 0), which makes it the
//           exclusive scan of the lengths with the total in line_off[n];
//   write   one lane per record again, through zeek_line_write -- the same walker as the length pass.
// The write-out follows fb_view.hip.  A lane that stored its own ~150-byte line byte by byte would touch a
// cache line of its own on every store of the wave.  The lines of one workgroup step (256 consecutive
// records) are one contiguous range of the text, so the lanes format into LDS at their step-local offsets,
// shifted by the range's misalignment so that LDS column c is the 16-B aligned global column c, and the
// whole workgroup writes the range in 16-B columns; the partial first and last column go out byte by byte.
// Histories are unbounded, so a step's bytes may exceed the staging budget (FB_ZEEK_STAGE_BYTES: with it
// the kernel's LDS stays under 40 KiB and four workgroups fit a CU's 160 KiB); such a step -- and every
// step under FB_DEBUG_ZEEK_DIRECT -- stores straight to global memory.  On either path a history of
// FB_ZEEK_COOP_HIST characters or more is left out by its lane and copied by the whole wave, 64
// consecutive bytes per store.
// Lines that do not fit text_cap entirely are not written: line ends grow with the index, so the written
// lines are a prefix, a step writes [off[base], off[base + fitting)) and nothing at or past text_cap.
#include <rocprim/device/device_scan.hpp>

#include "fb_internal.h"
#include "fb_zeek_fmt.h"

namespace fbk {

namespace {

constexpr uint32_t kZeekStage = FB_ZEEK_STAGE_BYTES;
static_assert(kZeekStage % 16u == 0u && kZeekStage + 16u + 64u <= 40u * 1024u, "four workgroups per CU");
static_assert(FB_ZEEK_STEP == 256, "one lane per record of a step");

struct Hist {
    const uint8_t* p;
    uint32_t len;
    bool mismatch;
};
// The history of a record: the blob's range of its slot (the blob decides; rec.hist_len only counts as a
// mismatch), empty without a blob or for a slot the offsets do not cover.  The offsets are indexed by the
// record's slot, or (fb_format_zeek_hist_dev) by its position i in the views.
__device__ __forceinline__ Hist hist_of(const ZeekArgs& a, const fb_flow_rec& r, unsigned long long i) {
    Hist h = {nullptr, 0u, false};
    if (!a.hist) return h;
    const unsigned long long at = a.by_record ? i : (unsigned long long)r.slot;
    if (at >= a.n_slots) {
        h.mismatch = true;
        return h;
    }
    const unsigned long long o0 = a.hist_off[at], o1 = a.hist_off[at + 1ull];
    if (o1 > o0 && o1 - o0 <= 0xFFFFFFFFull) {
        h.p = a.hist + o0;
        h.len = (uint32_t)(o1 - o0);
    }
    h.mismatch = h.len != r.hist_len;
    return h;
}

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return (unsigned long long)hi << 32 | lo;
}

}  // namespace

__global__ __launch_bounds__(256) void k_zeek_len(const ZeekArgs a) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < a.n; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        bool inexact = false, mismatch = false;
        if (i < a.n) {
            const fb_flow_view v = a.views[i];  // (a copy: every load of the record issues before the first use)
            const Hist h = hist_of(a, v.rec, i);
            a.off[i + 1ull] = fbzeek::zeek_line_len(v, h.len);
            inexact = fbzeek::zeek_inexact(v);
            mismatch = h.mismatch;
        }
        const unsigned long long mi = __ballot(inexact), mm = __ballot(mismatch);
        if ((threadIdx.x & 63u) == 0u) {
            if (mi) atomicAdd(reinterpret_cast<unsigned long long*>(&a.stats->ts_inexact), (unsigned long long)__popcll(mi));
            if (mm) atomicAdd(reinterpret_cast<unsigned long long*>(&a.stats->hist_mismatch), (unsigned long long)__popcll(mm));
        }
    }
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.off[0] = 0ull;
}

template <bool kStaged>
__global__ __launch_bounds__(256) void k_zeek_write(const ZeekArgs a) {
    __shared__ uint32_t sh[4];
    __shared__ uint4 s_stage[kStaged ? (kZeekStage + 16u) / 16u : 1u];
    uint8_t* const stage = reinterpret_cast<uint8_t*>(s_stage);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < a.n; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        const bool in = i < a.n;
        const unsigned long long start = in ? a.off[i] : 0ull, end = in ? a.off[i + 1ull] : 0ull;
        const bool fits = in && end <= a.cap;  // (line ends grow with i: the fitting lines are a prefix)
        const unsigned long long m = __ballot(fits);
        if (lane == 0u) sh[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        const uint32_t nfit = sh[0] + sh[1] + sh[2] + sh[3];
        __syncthreads();
        if (nfit == 0u) continue;  // (uniform over the workgroup)
        if (threadIdx.x == 0u)
            atomicAdd(reinterpret_cast<unsigned long long*>(&a.stats->lines_written), (unsigned long long)nfit);
        // the step's range of the text
        const unsigned long long r0 = a.off[base], bytes = a.off[base + nfit] - r0;
        const bool staged = kStaged && bytes <= kZeekStage;
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(a.text + r0) & 15u);

        // every fitting lane formats its line, all but a long history
        uint8_t* line = nullptr;
        Hist h = {nullptr, 0u, false};
        uint32_t hist_at = 0u;
        bool coop = false;
        if (fits) {
            const fb_flow_view v = a.views[i];  // (a copy: every load of the record issues before the first use)
            line = staged ? stage + mis + (uint32_t)(start - r0) : a.text + start;
            h = hist_of(a, v.rec, i);
            coop = h.len >= FB_ZEEK_COOP_HIST;
            fbzeek::zeek_line_write(v, coop ? nullptr : h.p, h.len, line, &hist_at);
        }
        // long histories: the wave copies them, one after the other
        for (unsigned long long todo = __ballot(coop); todo; todo &= todo - 1ull) {
            const int src = __ffsll((long long)todo) - 1;
            const uint8_t* from = reinterpret_cast<const uint8_t*>(shfl64(reinterpret_cast<uintptr_t>(h.p), src));
            uint8_t* to = reinterpret_cast<uint8_t*>(shfl64(reinterpret_cast<uintptr_t>(line + hist_at), src));
            const uint32_t len = (uint32_t)__shfl((int)h.len, src);
            for (uint32_t k = lane; k < len; k += 64u) to[k] = from[k];
        }
        if (!staged) continue;  // (uniform)
        __syncthreads();
        // LDS byte b is the byte of global address g + b, g 16-B aligned; the range is [mis, mis + bytes)
        uint8_t* const g = a.text + r0 - mis;
        const uint32_t lim = mis + (uint32_t)bytes;
        for (uint32_t c = threadIdx.x; c < (lim + 15u) / 16u; c += 256u) {
            const uint32_t lo = c * 16u, hi = lo + 16u;
            if (lo >= mis && hi <= lim) {
                *reinterpret_cast<uint4*>(g + lo) = s_stage[c];
            } else {
                for (uint32_t b = lo > mis ? lo : mis; b < (hi < lim ? hi : lim); ++b) g[b] = stage[b];
            }
        }
        __syncthreads();
    }
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        a.stats->lines = a.n;
        a.stats->bytes = a.off[a.n];
    }
}

hipError_t zeek_scan_tmp_bytes(unsigned long long n, size_t* bytes) {
    unsigned long long* p = nullptr;
    *bytes = 0;
    return rocprim::inclusive_scan(nullptr, *bytes, p, p, (size_t)n, rocprim::plus<unsigned long long>(),
                                   (hipStream_t) nullptr);
}

hipError_t launch_zeek(const ZeekArgs& a, bool staged, void* tmp, size_t tmp_bytes, hipStream_t s) {
    if (!a.views || !a.off || !a.stats || a.n == 0ull || (a.cap && !a.text) || (a.hist && !a.hist_off))
        return hipErrorInvalidValue;
    const dim3 g(sweep_grid(a.n, 2048ull));
    hipLaunchKernelGGL(k_zeek_len, g, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::inclusive_scan(tmp, tmp_bytes, a.off + 1, a.off + 1, (size_t)a.n, rocprim::plus<unsigned long long>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(staged ? k_zeek_write<true> : k_zeek_write<false>, g, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace fbk
