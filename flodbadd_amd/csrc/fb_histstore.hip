// fb_histstore.hip -- the device-resident session history (fb_hist_store_*): every flow's
// SessionStats.history (src/packets.rs:187-198, 410-426) as a chain of 64-byte blocks in one pool.
//
// A character is the 4-bit history code of the update (1 + its FB_HIST_CHARS index), two to a byte, the
// low nibble first.  A block is a u32 `next` link and 60 payload bytes (FB_HIST_BLOCK_CHARS codes); blocks
// are named by a 1-based id (0: none), so links survive a reallocation of the pool.  The per-slot plane
// element {head, tail, len, reserved} (kPlaneHist, fb_capi.hip) follows its flow through growths and purges
// like every other plane; the blocks never move.
//
// Allocation: a free stack of ids with a bump cursor above it.  A kernel that allocates takes ids from one
// virtual sequence -- index v < F is free_stack[F - 1 - v], the rest bump + (v - F) + 1 -- through one atomic
// per workgroup on ctl.cursor after a workgroup prefix sum; F and bump are constant while it runs, and the
// one-thread commit kernel after it folds the cursor into them and reports the counters to the host-mapped
// mailbox.  The purge's free sweep is the only kernel that pushes ids, so alloc and free never share a kernel.
//
// Append: the last update's history runs (launch_flow_history's output: one run per flow) are found by their
// heads.  A head lane measures its run up to FB_HIST_COOP_RUN characters; a run that reaches it is measured
// and packed by its whole wave.  A run writes whole bytes: the first byte of a run that starts at an odd
// position keeps its low nibble (a read-modify-write no other lane shares: one run per flow per call), the
// last byte of a run that ends at an even position gets a zero high nibble.
#include <rocprim/device/device_scan.hpp>

#include <string.h>

#include <deque>
#include <memory>
#include <new>

#include "fb_host.h"
#include "fb_internal.h"

namespace fbk {

namespace {

constexpr uint32_t kBlkChars = FB_HIST_BLOCK_CHARS, kBlkBytes = kBlkChars / 2u;
struct HsBlock {
    uint32_t next;
    uint8_t b[kBlkBytes];
};
static_assert(sizeof(HsBlock) == 64 && kBlkChars == 120u, "one block per 64 B");
static_assert(FB_HIST_COOP_RUN >= 2u && FB_HIST_COOP_RUN <= kBlkChars, "a lane's run starts at most one block");

struct HsCtl {
    uint32_t free_n;   // F: ids on the free stack
    uint32_t bump;     // ids ever taken from the bump cursor (the high-water mark)
    uint32_t cursor;   // the running kernel's position in the virtual sequence
    uint32_t bad;      // ids a kernel refused (outside the pool): the host bound was broken
    unsigned long long chars;
};
struct HsMailbox {
    unsigned long long in_use, high_water, free_n, chars, seq;  // seq written last
};

struct HsPool {
    HsBlock* blk;
    uint32_t cap;  // blocks: ids 1 .. cap
    uint32_t* free_stack;
    HsCtl* ctl;
};

__device__ __forceinline__ uint32_t blocks_of(uint32_t len) { return (len + kBlkChars - 1u) / kBlkChars; }

__device__ __forceinline__ uint32_t code_of_char(uint8_t ch) {
    constexpr char kChars[] = FB_HIST_CHARS;
    uint32_t code = 0u;
#pragma unroll
    for (uint32_t k = 0; k < sizeof(kChars) - 1u; ++k) code = ch == (uint8_t)kChars[k] ? k + 1u : code;
    return code;
}
__device__ __forceinline__ uint8_t char_of_code(uint32_t code) {
    constexpr unsigned long long kLo = 0x5266466848735300ull;  // "\0SsHhFfR", byte k = code k
    constexpr unsigned long long kHi = 0x2D61413C3E72ull;      // "r><Aa-", byte k = code 8 + k
    return (uint8_t)(((code < 8u) ? kLo : kHi) >> (8u * (code & 7u)));
}

// id of index v of the virtual sequence (F, bump: the control words as the kernel found them)
__device__ __forceinline__ uint32_t id_of(const HsPool& P, uint32_t F, uint32_t bump, uint32_t v) {
    return v < F ? P.free_stack[F - 1u - v] : bump + (v - F) + 1u;
}
__device__ __forceinline__ HsBlock* block_at(const HsPool& P, uint32_t id) {
    if (id == 0u || id > P.cap) {
        atomicAdd(&P.ctl->bad, 1u);
        return nullptr;
    }
    return P.blk + (id - 1u);
}

// One run of r characters (hist[0 .. r)) appended to the flow of plane element *pe, whose new blocks are the
// virtual indices v0 ..; lanes l0, l0 + stride, .. share the bytes and the links, lane l0 == 0 writes the element.
__device__ __forceinline__ void append_run(const HsPool& P, uint32_t F, uint32_t bump, const uint8_t* hist, uint32_t r,
                                           uint4* pe, const uint4 e, uint32_t v0, uint32_t l0, uint32_t stride) {
    const uint32_t len = e.z, nb0 = blocks_of(len), need = blocks_of(len + r) - nb0;
    const uint32_t B1 = (len + r - 1u) / 2u;
    for (uint32_t B = len / 2u + l0; B <= B1; B += stride) {
        const uint32_t ord = B / kBlkBytes;
        HsBlock* const blk = block_at(P, ord < nb0 ? e.y : id_of(P, F, bump, v0 + (ord - nb0)));
        if (!blk) continue;
        uint8_t* const bp = blk->b + B % kBlkBytes;
        const uint32_t q0 = 2u * B, q1 = q0 + 1u;
        const uint32_t lo = q0 < len ? (uint32_t)*bp & 15u : code_of_char(hist[q0 - len]);
        const uint32_t hi = q1 >= len + r ? 0u : code_of_char(hist[q1 - len]);
        *bp = (uint8_t)(lo | hi << 4);
    }
    for (uint32_t j = l0; j < need; j += stride)
        if (HsBlock* const blk = block_at(P, id_of(P, F, bump, v0 + j)))
            blk->next = j + 1u < need ? id_of(P, F, bump, v0 + j + 1u) : 0u;
    if (l0 != 0u) return;
    uint4 o = e;
    if (need) {
        const uint32_t first = id_of(P, F, bump, v0);
        if (len == 0u) {
            o.x = first;
        } else if (HsBlock* const t = block_at(P, e.y)) {
            t->next = first;
        }
        o.y = id_of(P, F, bump, v0 + need - 1u);
    }
    o.z = len + r;
    *pe = o;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, (int)d);
        if (lane >= d) v += t;
    }
    return v;
}

}  // namespace

struct HsAppendArgs {
    const uint8_t* hist;
    const uint32_t* hslot;
    const uint32_t* n;
    uint4* plane;
    unsigned long long tcap;
    HsPool P;
};

__global__ __launch_bounds__(256) void k_hs_append(const HsAppendArgs a) {
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_base;
    const uint32_t n = *a.n;
    // (only the commit kernel changes them; F never passes the stack's size)
    const uint32_t F = a.P.ctl->free_n < a.P.cap ? a.P.ctl->free_n : a.P.cap, bump = a.P.ctl->bump;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {  // (uniform)
        const uint32_t p = base + threadIdx.x;
        const uint32_t slot = p < n ? a.hslot[p] : ~0u;
        const bool head = p < n && slot < a.tcap && (p == 0u || a.hslot[p - 1u] != slot);
        uint32_t r = 0u;
        if (head)
            for (r = 1u; r < FB_HIST_COOP_RUN && p + r < n && a.hslot[p + r] == slot;) ++r;
        const bool coop = head && r == FB_HIST_COOP_RUN;
        // a run that reached the threshold: its wave finds the end, 64 positions per step
        for (unsigned long long todo = __ballot(coop); todo; todo &= todo - 1ull) {
            const int src = __ffsll((long long)todo) - 1;
            const uint32_t q0 = (uint32_t)__shfl((int)p, src) + FB_HIST_COOP_RUN, ss = (uint32_t)__shfl((int)slot, src);
            uint32_t q = q0;
            for (;;) {
                const uint32_t i = q + lane;
                const unsigned long long same = __ballot(i < n && a.hslot[i] == ss);
                if (same == ~0ull) {
                    q += 64u;
                    continue;
                }
                q += (uint32_t)__ffsll((long long)~same) - 1u;
                break;
            }
            if ((int)lane == src) r = FB_HIST_COOP_RUN + (q - q0);
        }
        const uint4 e = head ? a.plane[slot] : make_uint4(0u, 0u, 0u, 0u);
        const uint32_t need = head ? blocks_of(e.z + r) - blocks_of(e.z) : 0u;
        // the workgroup's share of the virtual sequence: prefix sum, one atomic
        const uint32_t incl = wave_incl_scan(need, lane);
        if (lane == 63u) s_w[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0u) {
            const uint32_t total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
            s_base = total ? atomicAdd(&a.P.ctl->cursor, total) : 0u;
        }
        __syncthreads();
        uint32_t v0 = s_base + incl - need;
        for (uint32_t w = 0; w < wave; ++w) v0 += s_w[w];
        __syncthreads();  // (s_w, s_base: free for the next step)
        if (head && !coop) append_run(a.P, F, bump, a.hist + p, r, a.plane + slot, e, v0, 0u, 1u);
        for (unsigned long long todo = __ballot(coop); todo; todo &= todo - 1ull) {
            const int src = __ffsll((long long)todo) - 1;
            const uint32_t sp = (uint32_t)__shfl((int)p, src), ss = (uint32_t)__shfl((int)slot, src);
            const uint32_t sr = (uint32_t)__shfl((int)r, src), sv = (uint32_t)__shfl((int)v0, src);
            const uint4 se = make_uint4((uint32_t)__shfl((int)e.x, src), (uint32_t)__shfl((int)e.y, src),
                                        (uint32_t)__shfl((int)e.z, src), (uint32_t)__shfl((int)e.w, src));
            append_run(a.P, F, bump, a.hist + sp, sr, a.plane + ss, se, sv, lane, 64u);
        }
    }
}

// After a kernel that allocated (n: its characters, or null), after the free sweep and after a clear: the
// cursor folded into F and the bump cursor, the counters reported to the host, seq last.
__global__ void k_hs_commit(HsCtl* ctl, const uint32_t* n, uint32_t reset, HsMailbox* mbox, unsigned long long seq) {
    if (reset) {
        ctl->free_n = 0u;
        ctl->bump = 0u;
        ctl->chars = 0ull;
    }
    const uint32_t used = ctl->cursor;
    if (used <= ctl->free_n) {
        ctl->free_n -= used;
    } else {
        ctl->bump += used - ctl->free_n;
        ctl->free_n = 0u;
    }
    ctl->cursor = 0u;
    if (n) ctl->chars += *n;
    __hip_atomic_store(&mbox->in_use, (unsigned long long)(ctl->bump - ctl->free_n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&mbox->high_water, (unsigned long long)ctl->bump, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&mbox->free_n, (unsigned long long)ctl->free_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&mbox->chars, ctl->chars, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&mbox->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The purge's free sweep, over the plane as it was before the move: the chain of every removed flow
// (remap == ~0u, head != 0) goes onto the free stack.  A lane's chain has ceil(len / 120) blocks: the wave
// reserves its lanes' positions with one atomic, then every lane walks its own chain.
__global__ __launch_bounds__(256) void k_hs_free_sweep(const uint4* plane, const uint32_t* remap, unsigned long long tcap,
                                                       HsPool P, unsigned long long* chars_freed) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < tcap; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        if (i < tcap && remap[i] == ~0u) e = plane[i];
        const uint32_t nb = e.x ? blocks_of(e.z) : 0u;
        const uint32_t incl = wave_incl_scan(nb, lane);
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
        if (total == 0u) continue;  // (uniform over the wave)
        uint32_t at = 0u;
        if (lane == 63u) at = atomicAdd(&P.ctl->free_n, total);
        at = (uint32_t)__shfl((int)at, 63) + incl - nb;
        uint32_t id = e.x;
        for (uint32_t k = 0; k < nb && id != 0u && id <= P.cap; ++k) {
            if (at + k < P.cap) P.free_stack[at + k] = id;
            id = P.blk[id - 1u].next;
        }
        if (nb) atomicAdd(chars_freed, (unsigned long long)e.z);
    }
}
__global__ void k_hs_chars_sub(HsCtl* ctl, unsigned long long* chars_freed) {
    ctl->chars -= *chars_freed;
    *chars_freed = 0ull;
}

struct HsReadArgs {
    const uint4* plane;
    unsigned long long tcap;
    const char* slots;  // null: slot i = i
    unsigned long long stride;
    unsigned long long n;
    unsigned long long* off;
    uint8_t* chars;
    unsigned long long cap;
    HsPool P;
};
__device__ __forceinline__ unsigned long long slot_of(const HsReadArgs& a, unsigned long long i) {
    return a.slots ? (unsigned long long)*reinterpret_cast<const uint32_t*>(a.slots + i * a.stride) : i;
}

__global__ __launch_bounds__(256) void k_hs_lengths(const HsReadArgs a) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < a.n; i += stride) {
        const unsigned long long s = slot_of(a, i);
        a.off[i + 1ull] = s < a.tcap ? (unsigned long long)a.plane[s].z : 0ull;
    }
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.off[0] = 0ull;
}

// One chain of `len` characters decoded to out[0 .. len): lanes l0, l0 + stride, .. take the bytes of a block.
__device__ __forceinline__ void gather_chain(const HsPool& P, uint32_t id, uint32_t len, uint8_t* out, uint32_t l0,
                                             uint32_t stride) {
    for (uint32_t done = 0u; done < len && id != 0u && id <= P.cap; done += kBlkChars) {
        const HsBlock* const blk = P.blk + (id - 1u);
        const uint32_t m = len - done < kBlkChars ? len - done : kBlkChars;
        for (uint32_t B = l0; 2u * B < m; B += stride) {
            const uint32_t v = blk->b[B];
            out[done + 2u * B] = char_of_code(v & 15u);
            if (2u * B + 1u < m) out[done + 2u * B + 1u] = char_of_code(v >> 4);
        }
        id = blk->next;
    }
}

__global__ __launch_bounds__(256) void k_hs_gather(const HsReadArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < a.n; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        uint32_t id = 0u, len = 0u;
        unsigned long long o0 = 0ull;
        if (i < a.n) {
            o0 = a.off[i];
            const unsigned long long o1 = a.off[i + 1ull], s = slot_of(a, i);
            if (s < a.tcap && o1 > o0 && o1 <= a.cap) {  // a range that ends past cap is not written at all
                const uint4 e = a.plane[s];
                id = e.x;
                len = (uint32_t)(o1 - o0 < (unsigned long long)e.z ? o1 - o0 : e.z);
            }
        }
        const bool coop = len >= FB_HIST_COOP_GATHER;
        if (len && !coop) gather_chain(a.P, id, len, a.chars + o0, 0u, 1u);
        for (unsigned long long todo = __ballot(coop); todo; todo &= todo - 1ull) {
            const int src = __ffsll((long long)todo) - 1;
            const unsigned long long so = (unsigned long long)(uint32_t)__shfl((int)(uint32_t)o0, src) |
                                          (unsigned long long)(uint32_t)__shfl((int)(uint32_t)(o0 >> 32), src) << 32;
            gather_chain(a.P, (uint32_t)__shfl((int)id, src), (uint32_t)__shfl((int)len, src), a.chars + so, lane, 64u);
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------
struct HistStore {
    DevBuf<HsBlock> pool;
    DevBuf<uint32_t> free_stack;  // [capacity]
    DevBuf<HsCtl> ctl;
    DevBuf<unsigned long long> chars_freed;
    PinnedBuf<HsMailbox> mbox;
    uint64_t cap = 0, max_blocks = 0;
    bool can_grow = true;
    // scratch of an append: the last update's runs (launch_flow_history's output)
    DevBuf<uint8_t> h_chars;
    DevBuf<uint32_t> h_slots, h_n;
    uint64_t h_cap = 0;
    StreamScratch scan_tmp;  // lengths: rocPRIM's scan storage
    uint64_t seq = 0;        // reports issued (appends, free sweeps, clears)
    std::deque<std::pair<uint64_t, uint64_t>> inflight;  // (seq, block bound) of the appends not yet reported
    uint64_t appends = 0;

    HsPool dev() const { return {pool.get(), (uint32_t)cap, free_stack.get(), ctl.get()}; }
};

static int hs_report(HistStore* h, const uint32_t* n, uint32_t reset, hipStream_t s) {
    hipLaunchKernelGGL(k_hs_commit, dim3(1), dim3(1), 0, s, h->ctl.get(), n, reset, h->mbox.dev(),
                       (unsigned long long)++h->seq);
    HIP_TRY(hipGetLastError());
    return FB_OK;
}

int histstore_create(HistStore** out, const fb_hist_store_config* cfg, bool can_grow, uint64_t rec_slots) {
    const uint64_t kMaxId = 0xFFFFFFFEull;
    std::unique_ptr<HistStore> h(new (std::nothrow) HistStore());
    if (!h) return set_err(FB_ERR_NOMEM, "history store");
    h->max_blocks = cfg->max_blocks ? std::min<uint64_t>(cfg->max_blocks, kMaxId) : kMaxId;
    h->cap = std::min<uint64_t>(cfg->block_capacity ? cfg->block_capacity : 1ull << 20, h->max_blocks);
    h->can_grow = can_grow;
    if (alloc_each(h->pool, h->cap, h->free_stack, h->cap, h->ctl, 1, h->chars_freed, 1, h->h_n, 1) != hipSuccess ||
        h->mbox.alloc(1, hipHostMallocMapped) != hipSuccess)
        return set_err(FB_ERR_NOMEM, "history store (%llu blocks)", (unsigned long long)h->cap);
    memset(h->mbox.get(), 0, sizeof(HsMailbox));
    HIP_TRY(hipMemset(h->ctl, 0, sizeof(HsCtl)));
    HIP_TRY(hipMemset(h->chars_freed, 0, 8));
    if (const int rc = histstore_scratch(h.get(), rec_slots)) return rc;
    *out = h.release();
    return FB_OK;
}
void histstore_free(HistStore* h) { delete h; }

// The append's run scratch holds `rec_slots` record slots (the caller has drained what used the old one).
int histstore_scratch(HistStore* h, uint64_t rec_slots) {
    if (rec_slots <= h->h_cap) return FB_OK;
    if (alloc_each(h->h_chars, rec_slots, h->h_slots, rec_slots) != hipSuccess) {
        h->h_cap = 0;
        return set_err(FB_ERR_NOMEM, "history store run scratch (%llu record slots)", (unsigned long long)rec_slots);
    }
    h->h_cap = rec_slots;
    return FB_OK;
}
uint64_t histstore_scratch_slots(const HistStore* h) { return h->h_cap; }
uint8_t* histstore_run_chars(HistStore* h) { return h->h_chars; }
uint32_t* histstore_run_slots(HistStore* h) { return h->h_slots; }
uint32_t* histstore_run_count(HistStore* h) { return h->h_n; }

// Before an append whose runs need at most `bound` new blocks: the last reported blocks in use plus the bounds
// of the appends still in flight plus this one stay within the pool -- else the exact usage is read (a device
// wait) and the pool grown x2 until it holds them, ids unchanged.  FB_ERR_TABLE_FULL, nothing changed, when it
// may not grow.  `drain` waits for whatever else may use the pool.
int histstore_admit(HistStore* h, uint64_t bound, hipStream_t s) {
    const volatile HsMailbox* m = h->mbox;
    const uint64_t seen = __atomic_load_n(&m->seq, __ATOMIC_ACQUIRE);
    uint64_t in_use = m->in_use;
    while (!h->inflight.empty() && h->inflight.front().first <= seen) h->inflight.pop_front();
    uint64_t ahead = 0;
    for (const auto& f : h->inflight) ahead += f.second;
    if (in_use + ahead + bound <= h->cap) return FB_OK;
    HIP_TRY(hipStreamSynchronize(s));
    HsCtl ctl;
    HIP_TRY(hipMemcpy(&ctl, h->ctl, sizeof(ctl), hipMemcpyDeviceToHost));
    h->inflight.clear();
    in_use = (uint64_t)ctl.bump - ctl.free_n;
    if (in_use + bound <= h->cap) return FB_OK;
    uint64_t want = h->cap;
    while (want < in_use + bound && want < h->max_blocks) want = std::min<uint64_t>(want * 2ull, h->max_blocks);
    if (!h->can_grow || want < in_use + bound)
        return set_err(FB_ERR_TABLE_FULL, "history store: %llu blocks in use + %llu for this update > %llu%s",
                       (unsigned long long)in_use, (unsigned long long)bound, (unsigned long long)h->cap,
                       h->can_grow ? " (max_blocks)" : " (FB_CFG_FIXED_TABLE)");
    DevBuf<HsBlock> pool;
    DevBuf<uint32_t> fs;
    if (alloc_each(pool, want, fs, want) != hipSuccess)
        return set_err(FB_ERR_NOMEM, "history store (%llu blocks)", (unsigned long long)want);
    HIP_TRY(hipDeviceSynchronize());  // a gather on another stream may still read the old pool
    HIP_TRY(hipMemcpy(pool, h->pool, std::min<uint64_t>(ctl.bump, h->cap) * sizeof(HsBlock), hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(fs, h->free_stack, std::min<uint64_t>(ctl.free_n, h->cap) * 4ull, hipMemcpyDeviceToDevice));
    h->pool.swap(pool);
    h->free_stack.swap(fs);
    h->cap = want;
    return FB_OK;
}

// The runs in the scratch (written on `s` by launch_flow_history) appended; `bound`: what histstore_admit took.
int histstore_append(HistStore* h, uint4* plane, uint64_t tcap, uint32_t rec_slots, uint64_t bound, hipStream_t s) {
    HsAppendArgs a;
    a.hist = h->h_chars;
    a.hslot = h->h_slots;
    a.n = h->h_n;
    a.plane = plane;
    a.tcap = tcap;
    a.P = h->dev();
    hipLaunchKernelGGL(k_hs_append, dim3(sweep_grid(rec_slots, 2048ull)), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    const int rc = hs_report(h, h->h_n, 0u, s);
    if (rc) return rc;
    h->inflight.emplace_back(h->seq, bound);
    ++h->appends;
    return FB_OK;
}

int histstore_free_sweep(HistStore* h, const uint4* plane, const uint32_t* remap, uint64_t tcap, hipStream_t s) {
    hipLaunchKernelGGL(k_hs_free_sweep, dim3(sweep_grid(tcap, 2048ull)), dim3(256), 0, s, plane, remap,
                       (unsigned long long)tcap, h->dev(), h->chars_freed.get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_hs_chars_sub, dim3(1), dim3(1), 0, s, h->ctl.get(), h->chars_freed.get());
    HIP_TRY(hipGetLastError());
    return hs_report(h, nullptr, 0u, s);
}

int histstore_clear(HistStore* h, hipStream_t s) { return hs_report(h, nullptr, 1u, s); }

static HsReadArgs read_args(const HistStore* h, const uint4* plane, uint64_t tcap, const void* d_slots, uint64_t stride,
                            uint64_t n, uint64_t* d_off) {
    HsReadArgs a;
    a.plane = plane;
    a.tcap = plane ? tcap : 0ull;
    a.slots = static_cast<const char*>(d_slots);
    a.stride = stride;
    a.n = n;
    a.off = reinterpret_cast<unsigned long long*>(d_off);
    a.chars = nullptr;
    a.cap = 0ull;
    a.P = h->dev();
    return a;
}

int histstore_lengths(HistStore* h, const uint4* plane, uint64_t tcap, const void* d_slots, uint64_t stride, uint64_t n,
                      uint64_t* d_off, hipStream_t s) {
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_off, 0, 8, s));
        return FB_OK;
    }
    unsigned long long* const off = reinterpret_cast<unsigned long long*>(d_off);
    size_t want = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, want, off, off, (size_t)n, rocprim::plus<unsigned long long>(), s));
    int rc = h->scan_tmp.acquire(want, s, "history store scan scratch");
    if (rc) return rc;
    hipLaunchKernelGGL(k_hs_lengths, dim3(sweep_grid(n, 2048ull)), dim3(256), 0, s,
                       read_args(h, plane, tcap, d_slots, stride, n, d_off));
    HIP_TRY(hipGetLastError());
    size_t have = h->scan_tmp.capacity();
    HIP_TRY(rocprim::inclusive_scan(h->scan_tmp.get(), have, off + 1, off + 1, (size_t)n,
                                    rocprim::plus<unsigned long long>(), s));
    return h->scan_tmp.release(s);
}

int histstore_gather(HistStore* h, const uint4* plane, uint64_t tcap, const void* d_slots, uint64_t stride, uint64_t n,
                     const uint64_t* d_off, uint8_t* d_chars, uint64_t cap, hipStream_t s) {
    if (n == 0 || cap == 0) return FB_OK;
    HsReadArgs a = read_args(h, plane, tcap, d_slots, stride, n, const_cast<uint64_t*>(d_off));
    a.chars = d_chars;
    a.cap = cap;
    hipLaunchKernelGGL(k_hs_gather, dim3(sweep_grid(n, 2048ull)), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return FB_OK;
}

__global__ __launch_bounds__(256) void k_hs_count_flows(const uint4* plane, unsigned long long tcap,
                                                        unsigned long long* out) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < tcap; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        const unsigned long long m = __ballot(i < tcap && plane[i].z != 0u);
        if ((threadIdx.x & 63u) == 0u && m) atomicAdd(out, (unsigned long long)__popcll(m));
    }
}

// Synchronous: the control words as they are once `s` has run everything issued.
int histstore_info(HistStore* h, const uint4* plane, uint64_t tcap, fb_hist_store_info* out, hipStream_t s) {
    unsigned long long flows = 0ull;
    if (plane) {  // (chars_freed is zero between the free sweeps; it goes back to zero here)
        hipLaunchKernelGGL(k_hs_count_flows, dim3(sweep_grid(tcap, 2048ull)), dim3(256), 0, s, plane,
                           (unsigned long long)tcap, h->chars_freed.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&flows, h->chars_freed, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemsetAsync(h->chars_freed, 0, 8, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    out->flows = flows;
    HsCtl ctl;
    HIP_TRY(hipMemcpy(&ctl, h->ctl, sizeof(ctl), hipMemcpyDeviceToHost));
    if (ctl.bad)
        return set_err(FB_ERR_INTERNAL, "history store: %u block ids outside the pool were refused", ctl.bad);
    out->blocks_capacity = h->cap;
    out->blocks_high_water = ctl.bump;
    out->blocks_free = ctl.free_n;
    out->blocks_in_use = (uint64_t)ctl.bump - ctl.free_n;
    out->chars = ctl.chars;
    out->appends = h->appends;
    return FB_OK;
}

}  // namespace fbk
