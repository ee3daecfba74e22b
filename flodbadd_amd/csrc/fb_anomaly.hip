// fb_anomaly.hip -- the anomaly pass over every flow of the table (fb_flow_anomaly): the reference's
// SessionAnalyzer (src/analyzer.rs) as far as it is per session -- compute_features (716-793), the
// forest's score against the two thresholds (586-592) and generate_anomaly_diagnostic (356-487).
//
// The forest itself is the project's own definition (the reference's forest crate is not
// part of its sources): fb_if_node trees the host trains and installs, walked here in f64.  Every
// result must be reproducible bit for bit by a host restatement, so the whole translation unit is
// compiled without floating-point contraction: each product, sum, difference and quotient below is one
// IEEE operation of its own (hipcc would otherwise fuse a * b + c).
#include <math.h>

#include "fb_internal.h"

#pragma clang fp contract(off)

namespace fbk {

// ---- the forest, host side ---------------------------------------------------------------------------
// The rules fb_if_validate documents; they are what bounds forest_walk's loop and its LDS indices.
bool forest_valid(const fb_if_node* nodes, uint64_t n_nodes, const uint32_t* first, uint32_t n_trees) {
    if (!nodes || !first || n_trees == 0u || n_trees > FB_IF_MAX_TREES) return false;
    if (first[0] != 0u || first[n_trees] != n_nodes) return false;
    for (uint32_t t = 0; t < n_trees; ++t) {
        if (first[t + 1] <= first[t] || first[t + 1] > n_nodes) return false;
        const uint32_t n = first[t + 1] - first[t];
        if (n > FB_IF_MAX_TREE_NODES) return false;
        const fb_if_node* tr = nodes + first[t];
        int depth[FB_IF_MAX_TREE_NODES];
        for (uint32_t i = 0; i < n; ++i) depth[i] = i == 0u ? 0 : -1;  // -1: no path from the root
        for (uint32_t i = 0; i < n; ++i) {
            const fb_if_node& nd = tr[i];
            if (!isfinite(nd.value)) return false;
            for (int j = 0; j < FB_AN_FEATURES; ++j)
                if (!isfinite(nd.normal[j])) return false;
            if (depth[i] > FB_IF_MAX_DEPTH) return false;
            if (nd.left == FB_IF_LEAF) continue;
            if (nd.left <= i || nd.left >= n || nd.right <= i || nd.right >= n) return false;
            if (depth[i] == FB_IF_MAX_DEPTH) return false;  // its leaves would lie deeper than the cap
            if (depth[i] >= 0) {
                depth[nd.left] = std::max(depth[nd.left], depth[i] + 1);
                depth[nd.right] = std::max(depth[nd.right], depth[i] + 1);
            }
        }
    }
    return true;
}

// ---- features ----------------------------------------------------------------------------------------
constexpr uint32_t kStateDstService = 1u << 15;               // hist_state: FB_SESSION_DST_SERVICE
constexpr uint32_t kStateSelfDst = FB_SESSION_SELF_DST << 20;  // hist_state: the stored is_self_dst

// compute_features for one occupied slot; tm: the flow's time record on a timed context, else null.
__device__ __forceinline__ void an_features(const FlowSlot& s, const FlowTime* tm, const uint32_t* service_code,
                                            double (&x)[FB_AN_FEATURES]) {
    const unsigned long long out = s.cnt[0], in = s.cnt[1], bytes = in + out, pkts = s.cnt[2] + s.cnt[3];
    x[0] = 0.0;
    x[1] = 0.0;
    x[4] = 0.0;
    if (tm) {
        const unsigned long long t = tm->end_time_ns != FB_SEEN_NONE ? tm->end_time_ns : tm->last_activity_ns;
        const long long ms = (long long)(t - tm->start_time_ns) / 1000000ll;  // num_milliseconds: toward zero
        x[1] = (double)ms / 1000.0;
        const uint32_t div = tm->segment_interarrival_div;
        if (div) x[4] = ((double)tm->total_segment_interarrival_ms / 1000.0) / (double)div;
    }
    x[2] = (double)bytes;
    x[3] = (double)pkts;
    x[5] = out ? (double)in / (double)out : 0.0;
    x[6] = pkts ? (double)bytes / (double)pkts : 0.0;
    x[7] = ((s.hist_state & kStateDstService) && service_code) ? (double)service_code[s.key[8] >> 16] : 0.0;
    x[8] = (s.hist_state & kStateSelfDst) ? 1.0 : 0.0;
    x[9] = 0.0;
}

// ---- the walk ----------------------------------------------------------------------------------------
// One tree at a time is staged in LDS, field by field (structure of arrays): word f * kIfStride + n is
// 8-byte field f of node n -- fields 0-9 the normal, 10 the value, 11 left | right << 32.  A ds_read_b64
// of field f by lanes at nodes n, n' then conflicts only when n = n' mod 32 (bank (2 (f * 257 + n)) mod 64);
// the root is a broadcast.  The stride of 257 (not 256) spreads the staging stores, whose consecutive lanes
// hold consecutive fields of one node, over the banks.  Two buffers: 2 * 12 * 257 * 8 = 49,344 B, three
// workgroups per CU.
constexpr uint32_t kIfFields = 12, kIfStride = 257, kIfUnits = 12;  // kIfUnits * 256 >= 255 nodes * 12 fields
static_assert(sizeof(fb_if_node) == 8 * kIfFields, "a node is twelve 8-byte fields");
static_assert(kIfUnits * 256u >= FB_IF_MAX_TREE_NODES * kIfFields && kIfStride > FB_IF_MAX_TREE_NODES, "staging covers a tree");

struct AnModel {
    const fb_if_node* nodes;
    const uint32_t* first;  // [n_trees + 1]
    const uint32_t* service_code;  // [65536] or null (zeros)
    uint32_t n_trees;
    fb_an_params prm;
};

__device__ __forceinline__ double if_walk_tree(const unsigned long long* tr, const double (&x)[FB_AN_FEATURES]) {
    uint32_t n = 0u;
#pragma unroll 1
    for (uint32_t step = 0; step < FB_IF_MAX_DEPTH; ++step) {  // a leaf is at most FB_IF_MAX_DEPTH below the root
        const unsigned long long lr = tr[11u * kIfStride + n];
        if ((uint32_t)lr == FB_IF_LEAF) break;
        double s = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < FB_AN_FEATURES; ++j) s = s + x[j] * __longlong_as_double((long long)tr[j * kIfStride + n]);
        n = s < __longlong_as_double((long long)tr[10u * kIfStride + n]) ? (uint32_t)lr : (uint32_t)(lr >> 32);
    }
    return __longlong_as_double((long long)tr[10u * kIfStride + n]);
}

// The sum of the leaf values of x's walk through every tree, in tree order.  Called by all 256 threads of
// the workgroup (it holds barriers); a lane that is not `active` stages trees but walks none.  Tree t + 1
// is loaded into registers before tree t is walked and stored into the other buffer after it, so the
// loads are in flight during the walk; one barrier per tree.
__device__ __forceinline__ double forest_path_sum(const AnModel& m, bool active, const double (&x)[FB_AN_FEATURES]) {
    __shared__ unsigned long long s_tree[2][kIfFields * kIfStride];
    unsigned long long r[kIfUnits];
    auto load = [&](uint32_t t) -> uint32_t {
        const uint32_t f0 = m.first[t], units = (m.first[t + 1] - f0) * kIfFields;
        const unsigned long long* g = reinterpret_cast<const unsigned long long*>(m.nodes + f0);
#pragma unroll
        for (uint32_t k = 0; k < kIfUnits; ++k) {
            const uint32_t e = k * 256u + threadIdx.x;
            r[k] = e < units ? g[e] : 0ull;
        }
        return units;
    };
    auto store = [&](uint32_t buf, uint32_t units) {
#pragma unroll
        for (uint32_t k = 0; k < kIfUnits; ++k) {
            const uint32_t e = k * 256u + threadIdx.x;
            const uint32_t node = e / kIfFields, field = e - node * kIfFields;
            if (e < units) s_tree[buf][field * kIfStride + node] = r[k];
        }
    };
    uint32_t units = load(0u);
    store(0u, units);
    __syncthreads();
    double sum = 0.0;
    for (uint32_t t = 0; t < m.n_trees; ++t) {
        const bool more = t + 1u < m.n_trees;
        if (more) units = load(t + 1u);
        if (active) sum = sum + if_walk_tree(s_tree[t & 1u], x);
        if (more) store((t + 1u) & 1u, units);
        __syncthreads();
    }
    return sum;
}

// generate_anomaly_diagnostic's per-feature decision as fb_an_diag codes.
__device__ __forceinline__ uint32_t an_diag(const fb_an_params& p, const double (&x)[FB_AN_FEATURES]) {
    uint32_t mask = 0u;
#pragma unroll
    for (uint32_t i = 0; i < FB_AN_FEATURES; ++i) {
        const bool categorical = i == 0u || i == 6u || i == 8u;  // FEATURE_DEFS, src/analyzer.rs:369-380
        const double mean = p.mean[i], sd = p.std[i], dev = fabs(x[i] - mean);
        uint32_t code = FB_AN_DIAG_NONE;
        if (!categorical && sd > 1e-6) {
            const double z = (x[i] - mean) / sd;
            code = z >= 2.5 ? FB_AN_DIAG_HIGH : (z <= -2.5 ? FB_AN_DIAG_LOW : FB_AN_DIAG_NONE);
        } else if (sd <= 1e-6 && dev > 1e-6) {
            code = FB_AN_DIAG_DEVIATES;
        }
        mask |= code << (2u * i);
    }
    return mask;
}

// ---- the pass ----------------------------------------------------------------------------------------
// k_flow_blacklist's geometry: one lane per table slot, 256-thread workgroups striding over the table.
// Per occupied slot the 128-B table line, the 64-B time record (timed contexts) and the 16-B record, read
// and -- when it changed -- written; the forest comes from L2, staged once per step of 256 slots.  A step
// without an occupied slot stages nothing.  Counters: PassCounters, fb_an_stats' first seven fields.
// kStamp (a pass time is set, fb_set_pass_time): the flows whose level or diagnostic codes changed -- the two
// fields the criticality string shows -- get `now` in the stamp plane; a new path_sum alone does not stamp
// (DESIGN.md 7).  The unstamped instance holds no such store.
template <bool kStamp>
__global__ __launch_bounds__(256) void k_flow_anomaly(const AnModel m, const FlowSlot* T, const FlowTime* plane,
                                                      unsigned long long cap, fb_an_rec* recs,
                                                      unsigned long long* stats, unsigned long long* mod,
                                                      unsigned long long now) {
    PassCounters<kAnCounters> cnt;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < cap; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        const bool occ = i < cap && T[i].tag >= 2u;
        if (__syncthreads_count(occ) == 0) continue;  // (uniform over the workgroup)
        double x[FB_AN_FEATURES] = {};
        if (occ) an_features(T[i], plane ? plane + i : nullptr, m.service_code, x);
        const double sum = forest_path_sum(m, occ, x);
        uint32_t level = 0u, old_level = 0u;
        bool changed = false;
        if (occ) {
            level = sum <= m.prm.abnormal_cut ? FB_AN_ABNORMAL : (sum <= m.prm.suspicious_cut ? FB_AN_SUSPICIOUS : FB_AN_NORMAL);
            const uint32_t diag = (level >= FB_AN_SUSPICIOUS && m.prm.has_stats) ? an_diag(m.prm, x) : 0u;
            const fb_an_rec old = recs[i];
            old_level = old.level;
            changed = __double_as_longlong(old.path_sum) != __double_as_longlong(sum) || old.diag != diag ||
                      old.level != level;
            if (changed) {
                fb_an_rec nw;
                nw.path_sum = sum;
                nw.diag = diag;
                nw.level = (uint8_t)level;
                nw.reserved[0] = nw.reserved[1] = nw.reserved[2] = 0u;
                recs[i] = nw;
            }
            if (kStamp && (old.diag != diag || old.level != level)) mod[i] = now;
        }
        cnt.add(0, occ);
        cnt.add(1, level == FB_AN_NORMAL);
        cnt.add(2, level == FB_AN_SUSPICIOUS);
        cnt.add(3, level == FB_AN_ABNORMAL);
        cnt.add(4, changed);
        cnt.add(5, occ && old_level < FB_AN_SUSPICIOUS && level >= FB_AN_SUSPICIOUS);
        cnt.add(6, occ && old_level >= FB_AN_SUSPICIOUS && level < FB_AN_SUSPICIOUS);
    }
    cnt.flush(stats);
}

// fb_if_score_dev: the same walk over caller-supplied vectors.
__global__ __launch_bounds__(256) void k_if_score(const AnModel m, const double* feat, unsigned long long n,
                                                  double* path_sum) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < n; base += stride) {
        const unsigned long long i = base + threadIdx.x;
        double x[FB_AN_FEATURES] = {};
        if (i < n) {
#pragma unroll
            for (uint32_t j = 0; j < FB_AN_FEATURES; ++j) x[j] = feat[i * FB_AN_FEATURES + j];
        }
        const double sum = forest_path_sum(m, i < n, x);
        if (i < n) path_sum[i] = sum;
    }
}

// Every flow's feature vector and slot.
__global__ __launch_bounds__(256) void k_flow_features(const FlowSlot* T, const FlowTime* plane,
                                                       const uint32_t* service_code, unsigned long long cap,
                                                       double* feat, uint32_t* slot, unsigned long long out_cap,
                                                       unsigned long long* d_n) {
    sweep_compact(
        cap, out_cap, d_n, [=](unsigned long long i) { return T[i].tag >= 2u; },
        [=](unsigned long long i, unsigned long long pos, bool) {
            double x[FB_AN_FEATURES];
            an_features(T[i], plane ? plane + i : nullptr, service_code, x);
#pragma unroll
            for (uint32_t j = 0; j < FB_AN_FEATURES; ++j) feat[pos * FB_AN_FEATURES + j] = x[j];
            slot[pos] = (uint32_t)i;
        });
}

// The flows whose level is at least min_level; out_recs (may be null): the record beside each.
__global__ __launch_bounds__(256) void k_flow_export_anomalous(const FlowSlot* T, const fb_an_rec* recs,
                                                               unsigned long long cap, uint32_t min_level,
                                                               fb_flow_rec* out, fb_an_rec* out_recs,
                                                               unsigned long long out_cap, unsigned long long* d_n,
                                                               const FlowTime* plane) {
    sweep_compact(
        cap, out_cap, d_n, [=](unsigned long long i) { return T[i].tag >= 2u && recs[i].level >= min_level; },
        [=](unsigned long long i, unsigned long long pos, bool) {
            out[pos] = flow_rec_at(T, plane, i);
            if (out_recs) out_recs[pos] = recs[i];
        });
}

#ifndef FB_AN_GRID
#define FB_AN_GRID 2048ull  // (not tuned: every step of 256 slots stages the forest, whatever the grid)
#endif
static AnModel model_of(const AnForest& f) {
    AnModel m;
    m.nodes = f.nodes;
    m.first = f.first;
    m.service_code = f.service_code;
    m.n_trees = f.n_trees;
    m.prm = f.prm;
    return m;
}

hipError_t launch_flow_anomaly(const AnForest& f, const FlowSlot* table, const FlowTime* plane, unsigned long long cap,
                               fb_an_rec* recs, unsigned long long* stats, hipStream_t s, unsigned long long* mod,
                               unsigned long long now) {
    if (!f.nodes || !f.first || !f.n_trees || !table || !recs || !stats || cap == 0ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mod ? k_flow_anomaly<true> : k_flow_anomaly<false>, dim3(sweep_grid(cap, FB_AN_GRID)), dim3(256), 0,
                       s, model_of(f), table, plane, cap, recs, stats, mod, now);
    return hipGetLastError();
}

hipError_t launch_if_score(const AnForest& f, const double* feat, unsigned long long n, double* path_sum, hipStream_t s) {
    if (!f.nodes || !f.first || !f.n_trees || !feat || !path_sum || n == 0ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_if_score, dim3(sweep_grid(n, FB_AN_GRID)), dim3(256), 0, s, model_of(f), feat, n, path_sum);
    return hipGetLastError();
}

hipError_t launch_flow_features(const FlowSlot* table, const FlowTime* plane, const uint32_t* service_code,
                                unsigned long long cap, double* feat, uint32_t* slot, unsigned long long out_cap,
                                unsigned long long* d_n, hipStream_t s) {
    if (!table || !d_n || (out_cap && (!feat || !slot))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_flow_features, dim3(sweep_grid(cap, 1024ull)), dim3(256), 0, s, table, plane, service_code, cap,
                       feat, slot, out_cap, d_n);
    return hipGetLastError();
}

hipError_t launch_flow_export_anomalous(const FlowSlot* table, const fb_an_rec* recs, unsigned long long cap,
                                        uint32_t min_level, fb_flow_rec* out, fb_an_rec* out_recs,
                                        unsigned long long out_cap, unsigned long long* d_n, const FlowTime* plane,
                                        hipStream_t s) {
    if (!table || !recs || !d_n || (out_cap && !out)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_flow_export_anomalous, dim3(sweep_grid(cap, 1024ull)), dim3(256), 0, s, table, recs, cap,
                       min_level, out, out_recs, out_cap, d_n, plane);
    return hipGetLastError();
}

}  // namespace fbk
