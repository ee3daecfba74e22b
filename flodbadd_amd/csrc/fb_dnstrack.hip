// fb_dnstrack.hip -- the DNS tracker (fb_dns_track_*): DnsPacketProcessor's pending_dns_queries and
// dns_resolutions (src/dns.rs:16-121) in device memory, brought forward in packet order from the arrays
// fb_dns_parse_dev leaves there.  DESIGN.md 3.14 has the argument; in short, one call is
//
//   classify     per message: accepted query / response / neither; the counts the growth rule needs
//   intern       every accepted query's name -> name id, concurrent inserts in ROUNDS (below)
//   sort         the setters' keys (transaction id << 32 | index): rocPRIM radix sort, 49 bits
//   take         a response reads its predecessor in sorted order: same id and a query -> that query's
//                name; same id and a response -> none; another id -> the carried pending[id]
//   carry        the last setter of each id's run writes pending[id] (its own kernel: the head of a run
//                reads what the tail of the same run overwrites)
//   resolve      every kept answer of a matched response -> a slot of the address table (rounds), then
//                one 64-bit atomicMax of order << 24 | name id: the last writer in packet order wins
//
// Rounds.  An insert of a wide key claims an empty slot by atomicCAS on its tag; the winner then writes
// the key beside it.  No lane ever waits for that store: a slot whose stamp says "claimed in this launch"
// cannot be compared yet, so the item stays where it is and the host launches the next round after reading
// one counter.  A stamp is the number of the launch that claimed the slot (the tracker counts its launches),
// so "published" is stamp != 0 && stamp < this launch -- whatever a racing read of the stamp returns, the old
// zero or the new number, it says "not yet".  Every round resolves or advances every item, so the loop ends
// after at most (longest probe run + 1) rounds; with 64-bit tags that is one or two.
//
// Name ids are deterministic: the names a call adds are numbered in the order of their first message.  Who
// wins a slot is not (any of the messages that carry the name may), so the winner only leaves a provisional
// reference to its message -- the bytes are compared where fb_dns_parse_dev wrote them --, every message
// that resolves to the slot lowers first[slot] to its index, and a scan over the "I am the first" flags
// numbers the new names before their bytes are copied into the store.
#include <cstring>  // (rocPRIM's texture-cache iterator needs memset declared)
#include <new>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fb_dns_hash.h"
#include "fb_host.h"
#include "fb_internal.h"

namespace fbk {

namespace {

constexpr uint32_t kNameDwords = FB_DNS_MAX_NAME / 4u;
constexpr uint32_t kIds = 65536u;                  // transaction ids
constexpr unsigned long long kNoTime = ~0ull;      // a pending query stored without a capture time
constexpr uint32_t kProvisional = 0x80000000u;     // meta ref: | the message that claimed the slot (this call)
constexpr uint32_t kKindNone = 0u, kKindQuery = 1u, kKindResponse = 2u;
constexpr unsigned long long kNonSetter = 1ull << 48;  // sort key of a message that is no setter
// the call's counter words
enum Ctr : uint32_t { cMsgs, cQueries, cResponses, cAddrBound, cMatched, cAddrItems, cUnresolved, cNamesNew,
                      cAddrsNew, cExhausted, cCount, kCtrWords = 16 };

__device__ __forceinline__ unsigned long long ld64(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// (name_dword, name_tag and dns_addr_tag: fb_dns_hash.h)
__device__ __forceinline__ bool name_equal(const uint32_t* a, const uint32_t* b, uint32_t len) {
    const uint32_t nd = (len + 3u) >> 2;
    for (uint32_t k = 0; k < nd; ++k)
        if (name_dword(a, k, len) != name_dword(b, k, len)) return false;
    return true;
}

struct NameIndex {  // the name store's index: open addressing over the tags
    unsigned long long* tag;   // [slots] 0: empty
    unsigned long long* meta;  // [slots] stamp << 32 | ref (a name id, or kProvisional | message)
    uint32_t* first;           // [slots] the first message of this call that carries the slot's new name
    unsigned long long slots;  // a power of two
};
struct TrackArgs {
    const fb_dns_msg* msgs;
    const uint32_t* names;  // the call's names, dwords
    const fb_ip* addrs;
    const fb_batch_stats* stats;
    const unsigned long long* ts;
    uint32_t n;
    uint8_t* kind;                 // [n]
    unsigned long long* key;       // [n] sort input
    unsigned long long* ntag;      // [n] an accepted query's name tag
    uint32_t* npos;                // [n] ... its probe position
    uint32_t* nslot;               // [n] ... its slot once resolved, ~0u before
    uint32_t* name_id;             // [n] ... its name id
    uint32_t* flag;                // [n] this message is the first of a new name
    uint32_t* rank;                // [n] exclusive scan of flag
    uint32_t* taken;               // [n]
    uint32_t* apos;                // [n * FB_DNS_MAX_ADDRS] an answer's probe position
    uint32_t* aslot;               // [n * FB_DNS_MAX_ADDRS] its slot once resolved; ~0u: unresolved, ~0u - 1: no item
    unsigned long long* ctr;       // [kCtrWords]
    unsigned long long hash_mask;
};

// *ctr += the wave's sum of v (v <= 15, every lane of the wave calls it): four ballots, one atomic
__device__ __forceinline__ void wave_add(unsigned long long* ctr, uint32_t v) {
    uint32_t sum = 0u;
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) sum += (uint32_t)__popcll(__ballot((v >> b) & 1u)) << b;
    if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(ctr, (unsigned long long)sum);
}

__global__ __launch_bounds__(256) void k_dns_classify(const TrackArgs a, const NameIndex ix) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t cnt = a.stats ? (uint32_t)min((unsigned long long)a.n, a.stats->n_dns) : a.n;
    uint32_t kind = kKindNone, na = 0u;
    if (i < cnt) {
        const fb_dns_msg m = a.msgs[i];
        if (m.status == FB_DNS_OK) {
            if (m.flags & FB_DNS_QUERY) {
                if ((m.flags & FB_DNS_HAS_QUESTION) && !(m.flags & FB_DNS_REVERSE)) kind = kKindQuery;
            } else {
                kind = kKindResponse;
                na = min((uint32_t)m.n_addrs, FB_DNS_MAX_ADDRS);
            }
        }
        if (kind == kKindQuery) {
            const uint32_t len = min((uint32_t)m.name_len, FB_DNS_MAX_NAME - 1u);
            const unsigned long long tag = name_tag(a.names + (size_t)i * kNameDwords, len, a.hash_mask);
            a.ntag[i] = tag;
            a.npos[i] = (uint32_t)(tag & (ix.slots - 1ull));
        }
    }
    if (i < a.n) {
        a.kind[i] = (uint8_t)kind;
        a.key[i] = kind == kKindNone ? (kNonSetter | i) : ((unsigned long long)a.msgs[i].id << 32 | i);
        a.nslot[i] = ~0u;
        a.name_id[i] = 0u;
        a.flag[i] = 0u;
        a.taken[i] = 0u;
    }
    // one atomic per wave and counter (a per-lane add of a varying value is one atomic per lane: the first
    // measurement had 262,144 of them on one word, 6.5 ms of a 7.2-ms call)
    if (i == 0u) atomicAdd(a.ctr + cMsgs, (unsigned long long)cnt);
    wave_add(a.ctr + cQueries, kind == kKindQuery ? 1u : 0u);
    wave_add(a.ctr + cResponses, kind == kKindResponse ? 1u : 0u);
    wave_add(a.ctr + cAddrBound, na);
}

// One insert round of the names (launch number `launch`).
__global__ __launch_bounds__(256) void k_dns_name_round(const TrackArgs a, const NameIndex ix, const uint32_t* store,
                                                        const uint16_t* store_len, uint32_t launch) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n || a.kind[i] != kKindQuery || a.nslot[i] != ~0u) return;
    const unsigned long long tag = a.ntag[i], mask = ix.slots - 1ull;
    const uint32_t len = min((uint32_t)a.msgs[i].name_len, FB_DNS_MAX_NAME - 1u);
    const uint32_t* mine = a.names + (size_t)i * kNameDwords;
    unsigned long long pos = a.npos[i];
    for (unsigned long long step = 0; step < ix.slots; ++step) {
        unsigned long long g = ld64(ix.tag + pos);
        if (g == 0ull) {
            g = atomicCAS(ix.tag + pos, 0ull, tag);
            if (g == 0ull) {  // claimed: leave the reference, resolved
                ix.meta[pos] = (unsigned long long)launch << 32 | kProvisional | i;
                atomicMin(ix.first + pos, i);
                a.nslot[i] = (uint32_t)pos;
                return;
            }
        }
        if (g == tag) {
            const unsigned long long m = ld64(ix.meta + pos);
            const uint32_t stamp = (uint32_t)(m >> 32), ref = (uint32_t)m;
            if (stamp == 0u || stamp >= launch) {  // claimed in this launch: not comparable yet
                a.npos[i] = (uint32_t)pos;
                atomicAdd(a.ctr + cUnresolved, 1ull);
                return;
            }
            const bool prov = (ref & kProvisional) != 0u;
            const uint32_t j = ref & ~kProvisional;
            const uint32_t olen = prov ? min((uint32_t)a.msgs[j].name_len, FB_DNS_MAX_NAME - 1u) : store_len[j];
            const uint32_t* other = prov ? a.names + (size_t)j * kNameDwords : store + (size_t)j * kNameDwords;
            if (olen == len && name_equal(mine, other, len)) {
                if (prov) atomicMin(ix.first + pos, i);
                a.nslot[i] = (uint32_t)pos;
                return;
            }
        }
        pos = (pos + 1ull) & mask;
    }
    atomicAdd(a.ctr + cExhausted, 1ull);  // (the growth rule keeps the index at most half full)
}

__global__ __launch_bounds__(256) void k_dns_name_flag(const TrackArgs a, const NameIndex ix) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n || a.kind[i] != kKindQuery) return;
    const uint32_t s = a.nslot[i];
    if (s == ~0u) return;
    if (((uint32_t)ix.meta[s] & kProvisional) && ix.first[s] == i) a.flag[i] = 1u;
}
// The first message of each new name numbers it, copies its bytes into the store and replaces the slot's
// provisional reference.
__global__ __launch_bounds__(256) void k_dns_name_publish(const TrackArgs a, const NameIndex ix, uint32_t* store,
                                                          uint16_t* store_len, uint32_t used, uint32_t launch) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n || !a.flag[i]) return;
    const uint32_t id = used + a.rank[i] + 1u, len = min((uint32_t)a.msgs[i].name_len, FB_DNS_MAX_NAME - 1u);
    const uint32_t nd = (len + 3u) >> 2;
    const uint32_t* mine = a.names + (size_t)i * kNameDwords;
    uint32_t* dst = store + (size_t)id * kNameDwords;
    for (uint32_t k = 0; k < kNameDwords; ++k) dst[k] = k < nd ? name_dword(mine, k, len) : 0u;
    store_len[id] = (uint16_t)len;
    const uint32_t s = a.nslot[i];
    ix.meta[s] = (unsigned long long)launch << 32 | id;
    ix.first[s] = ~0u;
    atomicAdd(a.ctr + cNamesNew, 1ull);
}
__global__ __launch_bounds__(256) void k_dns_name_ids(const TrackArgs a, const NameIndex ix) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n || a.kind[i] != kKindQuery) return;
    const uint32_t s = a.nslot[i];
    if (s != ~0u) a.name_id[i] = (uint32_t)ix.meta[s] & kDnsIdMask;
}

// take: sorted[p] = id << 32 | index of the setters (the others behind them)
__global__ __launch_bounds__(256) void k_dns_take(const TrackArgs a, const unsigned long long* sorted,
                                                  const uint32_t* pend_name) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const unsigned long long k = p < a.n ? sorted[p] : kNonSetter;
    const uint32_t i = (uint32_t)k;
    uint32_t t = 0u, na = 0u;
    if (!(k & kNonSetter) && a.kind[i] == kKindResponse) {
        if (p > 0u && (sorted[p - 1u] >> 32) == (k >> 32)) {
            const uint32_t j = (uint32_t)sorted[p - 1u];
            t = a.kind[j] == kKindQuery ? a.name_id[j] : 0u;
        } else {
            t = pend_name[(uint32_t)(k >> 32)];
        }
        a.taken[i] = t;
        na = t ? min((uint32_t)a.msgs[i].n_addrs, FB_DNS_MAX_ADDRS) : 0u;
    }
    wave_add(a.ctr + cMatched, t ? 1u : 0u);
    wave_add(a.ctr + cAddrItems, na);
}
// carry: the last setter of an id's run leaves pending[id]
__global__ __launch_bounds__(256) void k_dns_carry(const TrackArgs a, const unsigned long long* sorted,
                                                   uint32_t* pend_name, unsigned long long* pend_time) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.n) return;
    const unsigned long long k = sorted[p];
    if (k & kNonSetter) return;
    if (p + 1u < a.n && (sorted[p + 1u] >> 32) == (k >> 32)) return;
    const uint32_t i = (uint32_t)k, id = (uint32_t)(k >> 32);
    if (a.kind[i] == kKindQuery) {
        pend_name[id] = a.name_id[i];
        pend_time[id] = a.ts ? a.ts[a.msgs[i].pkt_index] : kNoTime;
    } else {
        pend_name[id] = 0u;
        pend_time[id] = kNoTime;
    }
}

struct AddrTable {
    unsigned long long* tag;   // [slots]
    uint32_t* stamp;           // [slots] the launch that claimed the slot
    uint32_t* key;             // [slots * 5]
    unsigned long long* val;   // [slots] order << kDnsIdBits | name id
    unsigned long long slots;
};
__global__ __launch_bounds__(256) void k_dns_addr_init(const TrackArgs a, const AddrTable t) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= a.n * FB_DNS_MAX_ADDRS) return;
    const uint32_t i = x / FB_DNS_MAX_ADDRS, j = x % FB_DNS_MAX_ADDRS;
    const bool item = a.kind[i] == kKindResponse && a.taken[i] != 0u && j < min((uint32_t)a.msgs[i].n_addrs, FB_DNS_MAX_ADDRS);
    a.aslot[x] = item ? ~0u : ~0u - 1u;
    if (item) {
        const fb_ip ip = a.addrs[x];
        a.apos[x] = (uint32_t)(dns_addr_tag(ip.addr, ip.family, a.hash_mask) & (t.slots - 1ull));
    }
}
// One insert round of the answers; a resolved item writes its resolution.
__global__ __launch_bounds__(256) void k_dns_addr_round(const TrackArgs a, const AddrTable t, uint32_t launch,
                                                        unsigned long long order0) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= a.n * FB_DNS_MAX_ADDRS || a.aslot[x] != ~0u) return;
    const uint32_t i = x / FB_DNS_MAX_ADDRS;
    const fb_ip ip = a.addrs[x];
    const unsigned long long tag = dns_addr_tag(ip.addr, ip.family, a.hash_mask), mask = t.slots - 1ull;
    const unsigned long long v = (order0 + i) << kDnsIdBits | a.taken[i];
    unsigned long long pos = a.apos[x];
    for (unsigned long long step = 0; step < t.slots; ++step) {
        unsigned long long g = ld64(t.tag + pos);
        bool hit = false;
        if (g == 0ull) {
            g = atomicCAS(t.tag + pos, 0ull, tag);
            if (g == 0ull) {
                uint32_t* k = t.key + pos * 5ull;
                k[0] = ip.addr[0], k[1] = ip.addr[1], k[2] = ip.addr[2], k[3] = ip.addr[3], k[4] = ip.family;
                t.stamp[pos] = launch;
                atomicAdd(a.ctr + cAddrsNew, 1ull);
                hit = true;
            }
        }
        if (!hit && g == tag) {
            const uint32_t stamp = __hip_atomic_load(t.stamp + pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (stamp == 0u || stamp >= launch) {
                a.apos[x] = (uint32_t)pos;
                atomicAdd(a.ctr + cUnresolved, 1ull);
                return;
            }
            const uint32_t* k = t.key + pos * 5ull;
            hit = k[0] == ip.addr[0] && k[1] == ip.addr[1] && k[2] == ip.addr[2] && k[3] == ip.addr[3] && k[4] == ip.family;
        }
        if (hit) {
            atomicMax(t.val + pos, v);
            a.aslot[x] = (uint32_t)pos;
            return;
        }
        pos = (pos + 1ull) & mask;
    }
    atomicAdd(a.ctr + cExhausted, 1ull);
}

// Rebuilds after a growth: every stored key is distinct, so an insert is a claim of the first empty slot.
__global__ __launch_bounds__(256) void k_dns_name_rebuild(const NameIndex ix, const uint32_t* store, const uint16_t* store_len,
                                                          uint32_t used, unsigned long long hash_mask, uint32_t launch) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x + 1u;
    if (id > used) return;
    const unsigned long long tag = name_tag(store + (size_t)id * kNameDwords, store_len[id], hash_mask), mask = ix.slots - 1ull;
    unsigned long long pos = tag & mask;
    for (unsigned long long step = 0; step < ix.slots; ++step, pos = (pos + 1ull) & mask) {
        if (ld64(ix.tag + pos) != 0ull || atomicCAS(ix.tag + pos, 0ull, tag) != 0ull) continue;
        ix.meta[pos] = (unsigned long long)launch << 32 | id;
        return;
    }
}
__global__ __launch_bounds__(256) void k_dns_addr_rebuild(const AddrTable old, const AddrTable nw, uint32_t launch) {
    const unsigned long long o = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (o >= old.slots) return;
    const unsigned long long tag = old.tag[o], mask = nw.slots - 1ull;
    if (tag == 0ull) return;
    unsigned long long pos = tag & mask;
    for (unsigned long long step = 0; step < nw.slots; ++step, pos = (pos + 1ull) & mask) {
        if (ld64(nw.tag + pos) != 0ull || atomicCAS(nw.tag + pos, 0ull, tag) != 0ull) continue;
        for (uint32_t k = 0; k < 5u; ++k) nw.key[pos * 5ull + k] = old.key[o * 5ull + k];
        nw.val[pos] = old.val[o];
        nw.stamp[pos] = launch;
        return;
    }
}

__global__ __launch_bounds__(256) void k_dns_expire(uint32_t* pend_name, unsigned long long* pend_time,
                                                    unsigned long long now, uint32_t drop, unsigned long long* count) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= kIds || pend_name[id] == 0u) return;
    if (!drop) {
        atomicAdd(count, 1ull);
        return;
    }
    const unsigned long long t = pend_time[id];
    if (t == kNoTime || now < t || now - t < FB_DNS_EXPIRY_NS) return;
    pend_name[id] = 0u;
    pend_time[id] = kNoTime;
    atomicAdd(count, 1ull);
}
__global__ __launch_bounds__(256) void k_dns_export_resolutions(const AddrTable t, fb_dns_resolution* out,
                                                                unsigned long long out_cap, unsigned long long* d_n) {
    sweep_compact(
        t.slots, out_cap, d_n, [=](unsigned long long i) { return t.tag[i] != 0ull; },
        [=](unsigned long long i, unsigned long long pos, bool) {
            fb_dns_resolution r;
            const uint32_t* k = t.key + i * 5ull;
            r.ip.addr[0] = k[0], r.ip.addr[1] = k[1], r.ip.addr[2] = k[2], r.ip.addr[3] = k[3];
            r.ip.family = k[4];
            r.ip.reserved[0] = r.ip.reserved[1] = r.ip.reserved[2] = 0u;
            const unsigned long long v = t.val[i];
            r.name_id = (uint32_t)v & kDnsIdMask;
            r.reserved = 0u;
            r.order = v >> kDnsIdBits;
            out[pos] = r;
        });
}
// 64 lanes per id: one dword each
__global__ __launch_bounds__(256) void k_dns_names(const uint32_t* store, const uint16_t* store_len, uint32_t used,
                                                   const uint32_t* ids, unsigned long long n, uint32_t* out, uint16_t* len) {
    const unsigned long long x = (unsigned long long)blockIdx.x * 256u + threadIdx.x, r = x / kNameDwords;
    if (r >= n) return;
    const uint32_t k = (uint32_t)(x % kNameDwords), id = ids[r];
    const bool known = id >= 1u && id <= used;
    out[x] = known ? store[(size_t)id * kNameDwords + k] : 0u;
    if (k == 0u) len[r] = known ? store_len[id] : (uint16_t)0;
}
__global__ __launch_bounds__(256) void k_dns_lookup(const DnsTables t, const fb_ip* ips, unsigned long long n, uint32_t* out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const fb_ip ip = ips[i];
    out[i] = dns_lookup(t, ip.addr, ip.family);
}

inline dim3 grid_for(unsigned long long n) { return dim3((uint32_t)std::max(1ull, (n + 255ull) / 256ull)); }
unsigned long long pow2_at_least(unsigned long long v) {
    unsigned long long p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

// The host's handle.  Capacities: `name_cap` ids fit the store and `addr_cap` addresses the table; both
// indexes have twice that many slots (a power of two), so they stay at most half full.
namespace {
// The owners of what the kernels see as a NameIndex / an AddrTable, and of the name store: each made whole
// (alloc_group) or not at all.
struct NameIndexBuf {
    DevBuf<unsigned long long> tag, meta;
    DevBuf<uint32_t> first;
    unsigned long long slots = 0;
    NameIndex view() const { return {tag, meta, first, slots}; }
};
struct AddrTableBuf {
    DevBuf<unsigned long long> tag;
    DevBuf<uint32_t> stamp, key;
    DevBuf<unsigned long long> val;
    unsigned long long slots = 0;
    AddrTable view() const { return {tag, stamp, key, val, slots}; }
};
struct NameStore {
    DevBuf<uint32_t> names;  // [(cap + 1) * kNameDwords]
    DevBuf<uint16_t> len;    // [cap + 1]
};
}  // namespace

struct DnsTrack {
    unsigned long long hash_mask = ~0ull;
    uint32_t launch = 1;  // the next launch's number (stamps)
    // names
    NameStore store;
    NameIndexBuf ix;
    uint64_t name_cap = 0, names = 0;
    // resolutions
    AddrTableBuf at;
    uint64_t addr_cap = 0, addrs = 0;
    // pending
    DevBuf<uint32_t> pend_name;            // [kIds]
    DevBuf<unsigned long long> pend_time;  // [kIds]
    uint64_t messages = 0, writes = 0;
    // per-call scratch, for `scratch_n` messages: `a` and `sorted` point into it
    uint32_t scratch_n = 0;
    DevBuf<uint8_t> scratch;
    TrackArgs a = {};
    unsigned long long* sorted = nullptr;
    DevBuf<uint8_t> sort_tmp;
    DevBuf<unsigned long long> d_ctr;
};

namespace {

bool alloc_name_index(NameIndexBuf& ix, uint64_t cap) {
    const unsigned long long slots = pow2_at_least(2ull * cap);
    const hipError_t e = alloc_group(ix, [&](NameIndexBuf& n) {
        n.slots = slots;
        return alloc_each(n.tag, slots, n.meta, slots, n.first, slots);
    });
    return e == hipSuccess && hipMemset(ix.tag, 0, slots * 8ull) == hipSuccess &&
           hipMemset(ix.meta, 0, slots * 8ull) == hipSuccess && hipMemset(ix.first, 0xFF, slots * 4ull) == hipSuccess;
}
bool alloc_addr_table(AddrTableBuf& t, uint64_t cap) {
    const unsigned long long slots = pow2_at_least(2ull * cap);
    const hipError_t e = alloc_group(t, [&](AddrTableBuf& n) {
        n.slots = slots;
        return alloc_each(n.tag, slots, n.stamp, slots, n.key, slots * 5ull, n.val, slots);
    });
    return e == hipSuccess && hipMemset(t.tag, 0, slots * 8ull) == hipSuccess &&
           hipMemset(t.stamp, 0, slots * 4ull) == hipSuccess && hipMemset(t.val, 0, slots * 8ull) == hipSuccess;
}
bool alloc_store(NameStore& st, uint64_t cap) {
    const hipError_t e = alloc_group(st, [&](NameStore& n) {
        return alloc_each(n.names, (cap + 1ull) * kNameDwords, n.len, cap + 1ull);
    });
    return e == hipSuccess && hipMemset(st.len, 0, (cap + 1ull) * 2ull) == hipSuccess;
}

// The stamps are 32-bit launch numbers; a tracker that has used them up restamps what it holds.
int stamps_reset(DnsTrack* t, hipStream_t s);

// The store and the index take `want` names: grown (ids stay, the index is rebuilt from the stored names)
// when they do not.  FB_ERR_TABLE_FULL, the state untouched, when that is impossible.
int grow_names(DnsTrack* t, uint64_t want, hipStream_t s) {
    if (want <= t->name_cap) return FB_OK;
    if (want > FB_DNS_MAX_NAMES) return set_err(FB_ERR_TABLE_FULL, "DNS name store: %llu names pass the 24-bit ids", (unsigned long long)want);
    const uint64_t cap = std::min<uint64_t>(FB_DNS_MAX_NAMES, std::max<uint64_t>(2ull * t->name_cap, pow2_at_least(want)));
    NameStore store;
    NameIndexBuf ix;
    if (!alloc_store(store, cap)) return set_err(FB_ERR_TABLE_FULL, "DNS name store cannot grow to %llu names", (unsigned long long)cap);
    if (!alloc_name_index(ix, cap))
        return set_err(FB_ERR_TABLE_FULL, "DNS name index cannot grow to %llu names", (unsigned long long)cap);
    HIP_TRY(hipMemcpyAsync(store.names, t->store.names, (t->names + 1ull) * FB_DNS_MAX_NAME, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(store.len, t->store.len, (t->names + 1ull) * 2ull, hipMemcpyDeviceToDevice, s));
    if (t->names)
        hipLaunchKernelGGL(k_dns_name_rebuild, grid_for(t->names), dim3(256), 0, s, ix.view(), store.names.get(),
                           store.len.get(), (uint32_t)t->names, t->hash_mask, t->launch++);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    t->store = std::move(store);
    t->ix = std::move(ix);
    t->name_cap = cap;
    return FB_OK;
}
int grow_addrs(DnsTrack* t, uint64_t want, hipStream_t s) {
    if (want <= t->addr_cap) return FB_OK;
    if (want > (1ull << 28)) return set_err(FB_ERR_TABLE_FULL, "DNS resolutions: %llu addresses pass the limit", (unsigned long long)want);
    const uint64_t cap = std::min<uint64_t>(1ull << 28, std::max<uint64_t>(2ull * t->addr_cap, pow2_at_least(want)));
    AddrTableBuf nw;
    if (!alloc_addr_table(nw, cap)) return set_err(FB_ERR_TABLE_FULL, "DNS resolutions cannot grow to %llu addresses", (unsigned long long)cap);
    hipLaunchKernelGGL(k_dns_addr_rebuild, grid_for(t->at.slots), dim3(256), 0, s, t->at.view(), nw.view(), t->launch++);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    t->at = std::move(nw);
    t->addr_cap = cap;
    return FB_OK;
}

int ensure_scratch(DnsTrack* t, uint32_t n) {
    if (n <= t->scratch_n) return FB_OK;
    t->scratch_n = 0;
    const uint64_t m = pow2_at_least(std::max<uint32_t>(n, 1024u));
    // 8-B arrays first: key, ntag, sorted; then the 4-B ones; kind last
    const uint64_t bytes = m * (3ull * 8 + 7ull * 4 + 2ull * FB_DNS_MAX_ADDRS * 4 + 1);
    if (t->scratch.alloc(bytes) != hipSuccess) return set_err(FB_ERR_NOMEM, "DNS tracker scratch for %u messages", n);
    uint8_t* p = t->scratch;
    auto take = [&](uint64_t b) {
        uint8_t* q = p;
        p += b;
        return q;
    };
    TrackArgs& a = t->a;
    a.key = reinterpret_cast<unsigned long long*>(take(m * 8));
    a.ntag = reinterpret_cast<unsigned long long*>(take(m * 8));
    t->sorted = reinterpret_cast<unsigned long long*>(take(m * 8));
    a.npos = reinterpret_cast<uint32_t*>(take(m * 4));
    a.nslot = reinterpret_cast<uint32_t*>(take(m * 4));
    a.name_id = reinterpret_cast<uint32_t*>(take(m * 4));
    a.flag = reinterpret_cast<uint32_t*>(take(m * 4));
    a.rank = reinterpret_cast<uint32_t*>(take(m * 4));
    a.taken = reinterpret_cast<uint32_t*>(take(m * 4));
    take(m * 4);
    a.apos = reinterpret_cast<uint32_t*>(take(m * FB_DNS_MAX_ADDRS * 4));
    a.aslot = reinterpret_cast<uint32_t*>(take(m * FB_DNS_MAX_ADDRS * 4));
    a.kind = take(m);
    t->scratch_n = (uint32_t)m;
    return FB_OK;
}
// rocPRIM's temporary storage for the sort and the scan of n items
int ensure_sort_tmp(DnsTrack* t, uint32_t n) {
    size_t sort_b = 0, scan_b = 0;
    HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_b, t->a.key, t->sorted, (size_t)n, 0u, 49u, (hipStream_t) nullptr));
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_b, t->a.flag, t->a.rank, 0u, (size_t)n, rocprim::plus<uint32_t>(),
                                    (hipStream_t) nullptr));
    const size_t want = std::max(sort_b, scan_b);
    if (want > t->sort_tmp.size() && t->sort_tmp.alloc(want) != hipSuccess)
        return set_err(FB_ERR_NOMEM, "DNS tracker sort scratch");
    return FB_OK;
}

int read_ctr(DnsTrack* t, unsigned long long* h, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(h, t->d_ctr, kCtrWords * 8ull, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FB_OK;
}

int stamps_reset(DnsTrack* t, hipStream_t s) {
    // every slot is republished under launch 1 by a rebuild into fresh tables of the same size
    const uint64_t nc = t->name_cap, ac = t->addr_cap;
    t->launch = 1;
    t->name_cap = 0;
    int rc = grow_names(t, nc, s);
    if (rc) {
        t->name_cap = nc;
        return rc;
    }
    t->addr_cap = 0;
    rc = grow_addrs(t, ac, s);
    if (rc) t->addr_cap = ac;
    return rc;
}

}  // namespace

int dnstrack_create(DnsTrack** out, const fb_dns_track_config* cfg) {
    *out = nullptr;
    uint64_t nc = 65536, ac = 262144, hm = ~0ull;
    if (cfg) {
        if (cfg->flags || cfg->reserved) return set_err(FB_ERR_INVAL, "fb_dns_track_config: flags and reserved must be 0");
        if (cfg->name_capacity > FB_DNS_MAX_NAMES || cfg->addr_capacity > (1ull << 28))
            return set_err(FB_ERR_INVAL, "fb_dns_track_config: capacity above the limit");
        if (cfg->name_capacity) nc = cfg->name_capacity;
        if (cfg->addr_capacity) ac = cfg->addr_capacity;
        if (cfg->hash_mask) hm = cfg->hash_mask;
    }
    DnsTrack* t = new (std::nothrow) DnsTrack;
    if (!t) return set_err(FB_ERR_NOMEM, "DNS tracker");
    t->hash_mask = hm;
    const bool ok = alloc_store(t->store, nc) && alloc_name_index(t->ix, nc) && alloc_addr_table(t->at, ac) &&
                    alloc_each(t->pend_name, kIds, t->pend_time, kIds, t->d_ctr, kCtrWords) == hipSuccess &&
                    hipMemset(t->pend_name, 0, kIds * 4ull) == hipSuccess &&
                    hipMemset(t->pend_time, 0xFF, kIds * 8ull) == hipSuccess &&
                    hipMemset(t->store.names, 0, FB_DNS_MAX_NAME) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        dnstrack_free(t);
        return set_err(FB_ERR_NOMEM, "DNS tracker tables (%llu names, %llu addresses)", (unsigned long long)nc, (unsigned long long)ac);
    }
    t->name_cap = nc;
    t->addr_cap = ac;
    *out = t;
    return FB_OK;
}

void dnstrack_free(DnsTrack* t) { delete t; }

int dnstrack_clear(DnsTrack* t, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(t->ix.tag, 0, t->ix.slots * 8ull, s));
    HIP_TRY(hipMemsetAsync(t->ix.meta, 0, t->ix.slots * 8ull, s));
    HIP_TRY(hipMemsetAsync(t->ix.first, 0xFF, t->ix.slots * 4ull, s));
    HIP_TRY(hipMemsetAsync(t->store.len, 0, (t->name_cap + 1ull) * 2ull, s));
    HIP_TRY(hipMemsetAsync(t->at.tag, 0, t->at.slots * 8ull, s));
    HIP_TRY(hipMemsetAsync(t->at.stamp, 0, t->at.slots * 4ull, s));
    HIP_TRY(hipMemsetAsync(t->at.val, 0, t->at.slots * 8ull, s));
    HIP_TRY(hipMemsetAsync(t->pend_name, 0, kIds * 4ull, s));
    HIP_TRY(hipMemsetAsync(t->pend_time, 0xFF, kIds * 8ull, s));
    HIP_TRY(hipStreamSynchronize(s));
    t->names = t->addrs = t->messages = 0;
    t->launch = 1;
    ++t->writes;
    return FB_OK;
}

int dnstrack_track(DnsTrack* t, const fb_dns_msg* msgs, const char* names, const fb_ip* addrs, uint32_t n,
                   const fb_batch_stats* stats, const unsigned long long* ts, uint32_t* taken, fb_dns_track_stats* out,
                   hipStream_t s) {
    if (out) memset(out, 0, sizeof(*out));
    if (t->messages + n >= kDnsMaxOrder) return set_err(FB_ERR_INVAL, "DNS tracker: the message count would pass 2^40");
    if (n == 0) return FB_OK;
    if (t->launch > 0xF0000000u) {
        const int rc = stamps_reset(t, s);
        if (rc) return rc;
    }
    int rc = ensure_scratch(t, n);
    if (!rc) rc = ensure_sort_tmp(t, n);
    if (rc) return rc;
    TrackArgs a = t->a;
    a.msgs = msgs;
    a.names = reinterpret_cast<const uint32_t*>(names);
    a.addrs = addrs;
    a.stats = stats;
    a.ts = ts;
    a.n = n;
    a.ctr = t->d_ctr;
    a.hash_mask = t->hash_mask;
    const dim3 g = grid_for(n), ga = grid_for((unsigned long long)n * FB_DNS_MAX_ADDRS), b(256);
    unsigned long long h[kCtrWords] = {};
    // classify against the index as it is; the counts bound what the call can add, so the tables grow --
    // or the call fails -- before anything is written.  (A growth moves the index: classify again, since
    // the probe positions depend on its size.)
    for (int pass = 0; pass < 2; ++pass) {
        HIP_TRY(hipMemsetAsync(t->d_ctr, 0, kCtrWords * 8ull, s));
        hipLaunchKernelGGL(k_dns_classify, g, b, 0, s, a, t->ix.view());
        HIP_TRY(hipGetLastError());
        rc = read_ctr(t, h, s);
        if (rc) return rc;
        if (pass == 1 || (t->names + h[cQueries] <= t->name_cap && t->addrs + h[cAddrBound] <= t->addr_cap)) break;
        rc = grow_names(t, t->names + h[cQueries], s);
        if (!rc) rc = grow_addrs(t, t->addrs + h[cAddrBound], s);
        if (rc) return rc;
    }
    // intern the names
    uint64_t name_rounds = 0, addr_rounds = 0;
    unsigned long long unresolved = h[cQueries];
    while (unresolved) {
        HIP_TRY(hipMemsetAsync(t->d_ctr + cUnresolved, 0, 8, s));
        hipLaunchKernelGGL(k_dns_name_round, g, b, 0, s, a, t->ix.view(), t->store.names.get(), t->store.len.get(), t->launch++);
        HIP_TRY(hipGetLastError());
        rc = read_ctr(t, h, s);
        if (rc) return rc;
        ++name_rounds;
        if (h[cExhausted] || name_rounds > t->ix.slots + 2ull || h[cUnresolved] > unresolved)
            return set_err(FB_ERR_INTERNAL, "DNS name index: insert did not converge (round %llu)", (unsigned long long)name_rounds);
        unresolved = h[cUnresolved];
    }
    if (h[cQueries]) {
        hipLaunchKernelGGL(k_dns_name_flag, g, b, 0, s, a, t->ix.view());
        HIP_TRY(hipGetLastError());
        size_t tmp = t->sort_tmp.size();
        HIP_TRY(rocprim::exclusive_scan(t->sort_tmp.get(), tmp, a.flag, a.rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), s));
        hipLaunchKernelGGL(k_dns_name_publish, g, b, 0, s, a, t->ix.view(), t->store.names.get(), t->store.len.get(), (uint32_t)t->names, t->launch++);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_dns_name_ids, g, b, 0, s, a, t->ix.view());
        HIP_TRY(hipGetLastError());
    }
    // pending: sort the setters, take, carry
    {
        size_t tmp = t->sort_tmp.size();
        HIP_TRY(rocprim::radix_sort_keys(t->sort_tmp.get(), tmp, a.key, t->sorted, (size_t)n, 0u, 49u, s));
    }
    hipLaunchKernelGGL(k_dns_take, g, b, 0, s, a, t->sorted, t->pend_name.get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_dns_carry, g, b, 0, s, a, t->sorted, t->pend_name.get(), t->pend_time.get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_dns_addr_init, ga, b, 0, s, a, t->at.view());
    HIP_TRY(hipGetLastError());
    rc = read_ctr(t, h, s);
    if (rc) return rc;
    // resolutions
    unresolved = h[cAddrItems];
    while (unresolved) {
        HIP_TRY(hipMemsetAsync(t->d_ctr + cUnresolved, 0, 8, s));
        hipLaunchKernelGGL(k_dns_addr_round, ga, b, 0, s, a, t->at.view(), t->launch++, (unsigned long long)t->messages);
        HIP_TRY(hipGetLastError());
        rc = read_ctr(t, h, s);
        if (rc) return rc;
        ++addr_rounds;
        if (h[cExhausted] || addr_rounds > t->at.slots + 2ull || h[cUnresolved] > unresolved)
            return set_err(FB_ERR_INTERNAL, "DNS resolutions: insert did not converge (round %llu)", (unsigned long long)addr_rounds);
        unresolved = h[cUnresolved];
    }
    if (taken) HIP_TRY(hipMemcpyAsync(taken, a.taken, n * 4ull, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    t->names += h[cNamesNew];
    t->addrs += h[cAddrsNew];
    t->messages += n;
    if (h[cAddrItems]) ++t->writes;
    if (out) {
        out->messages = h[cMsgs];
        out->queries = h[cQueries];
        out->responses = h[cResponses];
        out->matched = h[cMatched];
        out->resolutions = h[cAddrItems];
        out->names_new = h[cNamesNew];
        out->addrs_new = h[cAddrsNew];
        out->rounds = std::max(name_rounds, addr_rounds);
    }
    return FB_OK;
}

// fb_debug_set FB_DEBUG_DNS_LAUNCH: the next launch's number, so that a test reaches stamps_reset without
// 2^32 launches.  Never backwards: a slot stamped above the launch that reads it says "not yet" for ever.
int dnstrack_set_launch(DnsTrack* t, uint64_t launch) {
    if (launch == 0 || launch > 0xFFFFFFFFull) return set_err(FB_ERR_INVAL, "DNS tracker launch number %llu: 1 .. 2^32 - 1", (unsigned long long)launch);
    if (launch < t->launch)
        return set_err(FB_ERR_INVAL, "DNS tracker launch number %llu is below the current one, %u", (unsigned long long)launch, t->launch);
    t->launch = (uint32_t)launch;
    return FB_OK;
}

int dnstrack_expire(DnsTrack* t, unsigned long long now, uint64_t* dropped, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(t->d_ctr + cCount, 0, 8, s));
    hipLaunchKernelGGL(k_dns_expire, grid_for(kIds), dim3(256), 0, s, t->pend_name.get(), t->pend_time.get(), now, 1u, t->d_ctr + cCount);
    HIP_TRY(hipGetLastError());
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, t->d_ctr + cCount, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (dropped) *dropped = h;
    return FB_OK;
}

int dnstrack_info(DnsTrack* t, fb_dns_track_info* out, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(t->d_ctr + cCount, 0, 8, s));
    hipLaunchKernelGGL(k_dns_expire, grid_for(kIds), dim3(256), 0, s, t->pend_name.get(), t->pend_time.get(), 0ull, 0u, t->d_ctr + cCount);
    HIP_TRY(hipGetLastError());
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, t->d_ctr + cCount, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memset(out, 0, sizeof(*out));
    out->names = t->names;
    out->addrs = t->addrs;
    out->name_capacity = t->name_cap;
    out->addr_capacity = t->addr_cap;
    out->pending = h;
    out->messages = t->messages;
    out->writes = t->writes;
    return FB_OK;
}

int dnstrack_export_resolutions(DnsTrack* t, fb_dns_resolution* out, uint64_t cap, uint64_t* d_n, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(d_n, 0, 8, s));
    hipLaunchKernelGGL(k_dns_export_resolutions, dim3(sweep_grid(t->at.slots, 1024ull)), dim3(256), 0, s, t->at.view(), out,
                       (unsigned long long)cap, (unsigned long long*)d_n);
    HIP_TRY(hipGetLastError());
    return FB_OK;
}

int dnstrack_export_pending(DnsTrack* t, uint32_t* name_id, uint64_t* time, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(name_id, t->pend_name, kIds * 4ull, hipMemcpyDeviceToDevice, s));
    if (time) HIP_TRY(hipMemcpyAsync(time, t->pend_time, kIds * 8ull, hipMemcpyDeviceToDevice, s));
    return FB_OK;
}

int dnstrack_names(DnsTrack* t, const uint32_t* ids, uint64_t n, char* out, uint16_t* len, hipStream_t s) {
    if (n == 0) return FB_OK;
    hipLaunchKernelGGL(k_dns_names, grid_for(n * kNameDwords), dim3(256), 0, s, t->store.names.get(), t->store.len.get(), (uint32_t)t->names, ids,
                       (unsigned long long)n, reinterpret_cast<uint32_t*>(out), len);
    HIP_TRY(hipGetLastError());
    return FB_OK;
}

DnsTables dnstrack_tables(const DnsTrack* t) {
    DnsTables d;
    d.atag = t->at.tag;
    d.akey = t->at.key;
    d.aval = t->at.val;
    d.aslots = t->at.slots;
    d.hash_mask = t->hash_mask;
    d.names = t->store.names;
    d.name_len = t->store.len;
    d.n_names = (uint32_t)t->names;
    return d;
}

int dnstrack_lookup(DnsTrack* t, const fb_ip* ips, uint64_t n, uint32_t* name_id, hipStream_t s) {
    if (n == 0) return FB_OK;
    hipLaunchKernelGGL(k_dns_lookup, grid_for(n), dim3(256), 0, s, dnstrack_tables(t), ips, (unsigned long long)n, name_id);
    HIP_TRY(hipGetLastError());
    return FB_OK;
}

}  // namespace fbk
