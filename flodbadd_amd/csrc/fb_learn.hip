// fb_learn.hip -- endpoint learning (fb_flow_learn_endpoints_dev): the distinct endpoints of the flows a
// view query selects, each with a deterministic representative session -- what Whitelists::new_from_sessions
// (src/whitelists.rs:103-177) builds a custom whitelist from.  DESIGN.md 3.17 has the argument; one call is
//
//   select     one sweep: view_take (the view export's predicate) per occupied slot; a selected slot gets
//              the 64-bit tag of its fingerprint -- (dst_ip, family, dst_port, protocol, dst name id) and, while
//              a process-name table is installed (kProc), the flow's verbatim process name id
//              --, the others tag 0; the counts the index is sized by
//   insert     every selected flow -> an entry of the endpoint index (open addressing over the tags),
//              concurrent inserts in ROUNDS exactly as fb_dnstrack.hip's: claim by atomicCAS on the tag, the
//              winner writes the key and then the number of this launch as the slot's stamp, and a flow that
//              meets a slot claimed in this launch stays there for the next round -- no lane waits on
//              another lane's store.  Where a flow resolves it adds one to the entry's sessions and lowers
//              the entry's first order word to its own
//   least      IPv6 sources are wider than one word: two more atomicMin passes (address words 2-3, then the
//              port), each among the flows that equalled the previous winner.  (IPv4: source << 16 | port
//              is the whole order, in the insert.)  Table keys are unique, so exactly one flow of a group
//              equals all its entry's winners: the least session under Session's derived Ord
//   flag/scan  that flow flags its slot; an exclusive scan over the flags numbers the endpoints in slot order
//   emit       the flagged slots write their records at their ranks
//
// The scan, not the view export's per-step atomic, places the records: the output is in ascending rep_slot
// order over the whole table and two calls write the same bytes, which one atomic per workgroup and step
// (slot order inside a step only) does not give.
#include <cstring>  // (rocPRIM's texture-cache iterator needs memset declared)

#include <rocprim/device/device_scan.hpp>

#include "fb_host.h"
#include "fb_internal.h"

namespace fbk {

namespace {

constexpr unsigned long long kTagUsed = 1ull << 63;
constexpr uint32_t kEntNone = ~0u - 1u, kEntUnresolved = ~0u;  // LearnSlots::ent
// fingerprint words: six, or -- kProc -- eight (the process name id and a zero word: the tag hashes pairs)
template <bool kProc>
struct Fp {
    static constexpr uint32_t kWords = kProc ? 8u : 6u;
};
constexpr unsigned long long kMinIndexSlots = 64;
// the call's counter words
enum Ctr : uint32_t { cFlows, cSelected, cSelectedV6, cUnresolved, cExhausted, kCtrWords = 8 };

struct LearnSlots {  // per table slot
    unsigned long long* tag;  // 0: not selected
    uint32_t* pos;            // the flow's probe position; after the rounds: 1 = the representative of its entry
    uint32_t* ent;            // its index entry; kEntUnresolved before, kEntNone: not selected
    uint32_t* rank;           // exclusive scan of the flags
};
struct LearnIndex {
    unsigned long long* tag;  // [slots] 0: empty
    uint32_t* stamp;          // [slots] the launch that claimed the slot (0: none)
    uint32_t* cnt;            // [slots] flows resolved to it
    uint32_t* key;            // [slots * fingerprint words]
    unsigned long long* min;  // [slots * 3] the least order words of the entry's flows (~0: none yet)
    unsigned long long slots; // a power of two
};

__device__ __forceinline__ unsigned long long ld64(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The fingerprint of a slot: the four destination words, dst_port | protocol << 16 | family << 24, the name id
// -- and, eight words, the process name id.
template <uint32_t kFpWords>
__device__ __forceinline__ void fingerprint(const FlowSlot& t, uint32_t name_id, uint32_t proc_name_id,
                                            uint32_t (&f)[kFpWords]) {
    f[0] = t.key[4], f[1] = t.key[5], f[2] = t.key[6], f[3] = t.key[7];
    f[4] = (t.key[8] >> 16) | (t.key[9] & 0xFFFFu) << 16;
    f[5] = name_id;
    if constexpr (kFpWords > 6u) f[6] = proc_name_id, f[7] = 0u;
}
template <uint32_t kFpWords>
__device__ __forceinline__ unsigned long long fp_tag(const uint32_t (&f)[kFpWords], unsigned long long hash_mask) {
    unsigned long long h = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (uint32_t j = 0; j < kFpWords; j += 2) {
        h ^= (unsigned long long)f[j] | ((unsigned long long)f[j + 1] << 32);
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 31;
    }
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    return (h & hash_mask) | kTagUsed;
}
// A flow's place in Session's derived Ord inside its group (protocol and destination equal): the source
// address, then the source port -- one word for IPv4, three for IPv6.
__device__ __forceinline__ void order_words(const FlowSlot& t, unsigned long long (&k)[3]) {
    const uint32_t sport = t.key[8] & 0xFFFFu;
    if (((t.key[9] >> 8) & 0xFFu) == 10u) {
        k[0] = (unsigned long long)t.key[0] << 32 | t.key[1];
        k[1] = (unsigned long long)t.key[2] << 32 | t.key[3];
        k[2] = sport;
    } else {
        k[0] = (unsigned long long)t.key[0] << 16 | sport;
        k[1] = k[2] = ~0ull;
    }
}

template <bool kProc>
__global__ __launch_bounds__(256) void k_learn_select(const ViewArgs a, const uint2* dom, const WlProcNames P,
                                                      unsigned long long hash_mask, const LearnSlots sl,
                                                      unsigned long long* ctr) {
    constexpr uint32_t kFpWords = Fp<kProc>::kWords;
    PassCounters<3> pc;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < a.cap; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        const bool occupied = i < a.cap && a.table[i].tag >= 2u;
        const bool taken = occupied && view_take(a, i);
        unsigned long long tag = 0ull;
        bool v6 = false;
        if (taken) {
            uint32_t f[kFpWords];
            fingerprint(a.table[i], dom ? dom[i].y : 0u, kProc ? wl_flow_name_id(P, i) : 0u, f);
            tag = fp_tag(f, hash_mask);
            v6 = (f[4] >> 24) == 10u;
        }
        if (i < a.cap) {
            sl.tag[i] = tag;
            sl.ent[i] = taken ? kEntUnresolved : kEntNone;
            sl.pos[i] = 0u;
        }
        pc.add(cFlows, occupied);
        pc.add(cSelected, taken);
        pc.add(cSelectedV6, v6);
    }
    pc.flush(ctr);
}

// One insert round (launch number `launch`, from 1): one lane per table slot.
template <bool kProc>
__global__ __launch_bounds__(256) void k_learn_round(const FlowSlot* table, const uint2* dom, const WlProcNames P,
                                                     unsigned long long cap, const LearnSlots sl, const LearnIndex ix,
                                                     uint32_t launch, unsigned long long* ctr) {
    constexpr uint32_t kFpWords = Fp<kProc>::kWords;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= cap || sl.ent[i] != kEntUnresolved) return;
    const unsigned long long tag = sl.tag[i], mask = ix.slots - 1ull;
    uint32_t f[kFpWords];
    fingerprint(table[i], dom ? dom[i].y : 0u, kProc ? wl_flow_name_id(P, i) : 0u, f);
    unsigned long long pos = launch == 1u ? (tag & mask) : (unsigned long long)sl.pos[i];
    for (unsigned long long step = 0; step < ix.slots; ++step) {
        unsigned long long g = ld64(ix.tag + pos);
        bool hit = false;
        if (g == 0ull) {
            g = atomicCAS(ix.tag + pos, 0ull, tag);
            if (g == 0ull) {  // claimed: the key, then the stamp that publishes it to the next launch
                uint32_t* k = ix.key + pos * kFpWords;
#pragma unroll
                for (uint32_t j = 0; j < kFpWords; ++j) k[j] = f[j];
                ix.stamp[pos] = launch;
                hit = true;
            }
        }
        if (!hit && g == tag) {
            const uint32_t stamp = __hip_atomic_load(ix.stamp + pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (stamp == 0u || stamp >= launch) {  // claimed in this launch: not comparable yet
                sl.pos[i] = (uint32_t)pos;
                atomicAdd(ctr + cUnresolved, 1ull);
                return;
            }
            const uint32_t* k = ix.key + pos * kFpWords;
            hit = true;
#pragma unroll
            for (uint32_t j = 0; j < kFpWords; ++j) hit &= k[j] == f[j];
        }
        if (hit) {
            unsigned long long o[3];
            order_words(table[i], o);
            atomicMin(ix.min + pos * 3ull, o[0]);
            atomicAdd(ix.cnt + pos, 1u);
            sl.ent[i] = (uint32_t)pos;
            return;
        }
        pos = (pos + 1ull) & mask;
    }
    atomicAdd(ctr + cExhausted, 1ull);  // (the index has twice the selected flows: it cannot fill)
}

// IPv6 groups: order word `w` (1, 2) among the flows that equal their entry's winners of the words before it.
__global__ __launch_bounds__(256) void k_learn_least(const FlowSlot* table, unsigned long long cap, const LearnSlots sl,
                                                     const LearnIndex ix, uint32_t w) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= cap) return;
    const uint32_t e = sl.ent[i];
    if (e >= kEntNone || ((table[i].key[9] >> 8) & 0xFFu) != 10u) return;
    unsigned long long o[3];
    order_words(table[i], o);
    const unsigned long long* m = ix.min + (unsigned long long)e * 3ull;
    for (uint32_t j = 0; j < w; ++j)
        if (o[j] != m[j]) return;
    atomicMin(ix.min + (unsigned long long)e * 3ull + w, o[w]);
}

// flag[i] (in sl.pos) = slot i holds the representative of its entry.
__global__ __launch_bounds__(256) void k_learn_flag(const FlowSlot* table, unsigned long long cap, const LearnSlots sl,
                                                    const LearnIndex ix) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= cap) return;
    const uint32_t e = sl.ent[i];
    uint32_t flag = 0u;
    if (e < kEntNone) {
        unsigned long long o[3];
        order_words(table[i], o);
        const unsigned long long* m = ix.min + (unsigned long long)e * 3ull;
        flag = (o[0] == m[0] && o[1] == m[1] && o[2] == m[2]) ? 1u : 0u;
    }
    sl.pos[i] = flag;
}

template <bool kProc>
__global__ __launch_bounds__(256) void k_learn_emit(const FlowSlot* table, unsigned long long cap, const LearnSlots sl,
                                                    const LearnIndex ix, fb_learned_endpoint* out,
                                                    unsigned long long out_cap, unsigned long long* d_n) {
    constexpr uint32_t kFpWords = Fp<kProc>::kWords;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= cap) return;
    const uint32_t flag = sl.pos[i], rank = sl.rank[i];
    if (i == cap - 1ull) *d_n = (unsigned long long)rank + flag;
    if (!flag || rank >= out_cap) return;
    const FlowSlot& t = table[i];
    const uint32_t e = sl.ent[i];
    const uint32_t* k = ix.key + (unsigned long long)e * kFpWords;
    // the record as four 16-B stores: dst_ip | rep_src_ip | ports, protocol, family, name id, slot | sessions,
    // process name id (the entry's: its flows share it)
    uint4* o = reinterpret_cast<uint4*>(out + rank);
    o[0] = make_uint4(k[0], k[1], k[2], k[3]);
    o[1] = make_uint4(t.key[0], t.key[1], t.key[2], t.key[3]);
    o[2] = make_uint4((k[4] & 0xFFFFu) | (t.key[8] & 0xFFFFu) << 16, k[4] >> 16, k[5], (uint32_t)i);
    o[3] = make_uint4(ix.cnt[e], kProc ? k[6] : 0u, 0u, 0u);
}

inline dim3 grid_for(unsigned long long n) { return dim3((uint32_t)std::max(1ull, (n + 255ull) / 256ull)); }
inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

int learn_endpoints(const ViewArgs& a, const uint2* dom, const WlProcNames& names, unsigned long long hash_mask,
                    StreamScratch& per_slot, StreamScratch& index, fb_learned_endpoint* out, unsigned long long out_cap,
                    unsigned long long* d_n, fb_learn_stats* stats, hipStream_t s) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!view_args_valid(a) || !d_n || (out_cap && !out)) return set_err(FB_ERR_INVAL, "bad arguments");
    const bool proc = names.n != 0u;  // a name table is installed: the eight-word fingerprint
    if (proc && (!names.match_id || !names.name_id)) return set_err(FB_ERR_INVAL, "bad arguments");
    const unsigned long long key_b = 4ull * (proc ? Fp<true>::kWords : Fp<false>::kWords);
    const unsigned long long cap = a.cap;
    // per table slot: tag (8 B), pos, ent, rank (4 B each); then the counters and the scan's storage
    size_t scan_b = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)cap,
                                    rocprim::plus<uint32_t>(), s));
    const size_t slot_b = round_up(cap * 20ull, 256), ctr_b = 256;
    int rc = per_slot.acquire(slot_b + ctr_b + scan_b, s, "endpoint learning scratch");
    if (rc) return rc;
    uint8_t* p = static_cast<uint8_t*>(per_slot.get());
    LearnSlots sl;
    sl.tag = reinterpret_cast<unsigned long long*>(p);
    sl.pos = reinterpret_cast<uint32_t*>(p + cap * 8ull);
    sl.ent = sl.pos + cap;
    sl.rank = sl.ent + cap;
    unsigned long long* ctr = reinterpret_cast<unsigned long long*>(p + slot_b);
    void* scan_tmp = p + slot_b + ctr_b;
    const dim3 g = grid_for(cap), b(256);
    unsigned long long h[kCtrWords] = {};
    auto read_ctr = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(h, ctr, kCtrWords * 8ull, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return FB_OK;
    };

    HIP_TRY(hipMemsetAsync(ctr, 0, kCtrWords * 8ull, s));
    hipLaunchKernelGGL(proc ? k_learn_select<true> : k_learn_select<false>, dim3(sweep_grid(cap, 1024ull)), b, 0, s, a,
                       dom, names, hash_mask, sl, ctr);
    HIP_TRY(hipGetLastError());
    rc = read_ctr();
    if (rc) return rc;
    const unsigned long long flows = h[cFlows], selected = h[cSelected], selected_v6 = h[cSelectedV6];
    unsigned long long rounds = 0, endpoints = 0;
    if (selected == 0) {
        HIP_TRY(hipMemsetAsync(d_n, 0, 8, s));
        HIP_TRY(hipStreamSynchronize(s));
    } else {
        // the index: at least twice the selected flows, so it stays at most half full
        LearnIndex ix;
        ix.slots = kMinIndexSlots;
        while (ix.slots < 2ull * selected) ix.slots <<= 1;
        // per index slot: tag 8 | min 24 | stamp 4 | cnt 4 | key 24 (32 with the process name id)
        rc = index.acquire(ix.slots * (40ull + key_b), s, "endpoint index");
        if (rc) return rc;
        uint8_t* q = static_cast<uint8_t*>(index.get());
        ix.tag = reinterpret_cast<unsigned long long*>(q);
        ix.min = ix.tag + ix.slots;
        ix.stamp = reinterpret_cast<uint32_t*>(ix.min + 3ull * ix.slots);
        ix.cnt = ix.stamp + ix.slots;
        ix.key = ix.cnt + ix.slots;
        HIP_TRY(hipMemsetAsync(ix.tag, 0, ix.slots * 8ull, s));
        HIP_TRY(hipMemsetAsync(ix.min, 0xFF, ix.slots * 24ull, s));
        HIP_TRY(hipMemsetAsync(ix.stamp, 0, ix.slots * 8ull, s));  // stamps and counts
        unsigned long long unresolved = selected;
        while (unresolved) {
            if (rounds >= ix.slots + 2ull)  // never spins: the bound a converging insert cannot reach
                return set_err(FB_ERR_INTERNAL, "endpoint index: insert did not converge in %llu rounds", rounds);
            HIP_TRY(hipMemsetAsync(ctr + cUnresolved, 0, 8, s));
            hipLaunchKernelGGL(proc ? k_learn_round<true> : k_learn_round<false>, g, b, 0, s, a.table, dom, names, cap,
                               sl, ix, (uint32_t)(++rounds), ctr);
            HIP_TRY(hipGetLastError());
            rc = read_ctr();
            if (rc) return rc;
            if (h[cExhausted] || h[cUnresolved] > unresolved)
                return set_err(FB_ERR_INTERNAL, "endpoint index: insert did not converge (round %llu)", rounds);
            unresolved = h[cUnresolved];
        }
        for (uint32_t w = 1; selected_v6 && w <= 2u; ++w) {
            hipLaunchKernelGGL(k_learn_least, g, b, 0, s, a.table, cap, sl, ix, w);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_learn_flag, g, b, 0, s, a.table, cap, sl, ix);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::exclusive_scan(scan_tmp, scan_b, sl.pos, sl.rank, 0u, (size_t)cap, rocprim::plus<uint32_t>(), s));
        hipLaunchKernelGGL(proc ? k_learn_emit<true> : k_learn_emit<false>, g, b, 0, s, a.table, cap, sl, ix, out,
                           out_cap, d_n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&endpoints, d_n, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        rc = index.release(s);
        if (rc) return rc;
    }
    rc = per_slot.release(s);
    if (rc) return rc;
    if (stats) {
        stats->flows = flows;
        stats->selected = selected;
        stats->endpoints = endpoints;
        stats->written = std::min<unsigned long long>(endpoints, out_cap);
        stats->rounds = rounds;
    }
    return FB_OK;
}

}  // namespace fbk
