// wl_match_host.cpp -- a stand-alone host program over fb_wl_match.h, for the CPU tests
// (tests/test_wlprocspace_oracle.py builds it with the address and undefined-behaviour sanitizers): the header a
// plain C++ compiler sees is the one fb_set_whitelist and the whitelist pass's kernels include, so the index
// build and wl_eval run here exactly as they do there.
//   wl_match_host IN
// IN (tests/wlprocspace.py, write_corpus): u64 n_endpoints, n_names, has_plane, n_flows; n_endpoints
//     fb_wl_endpoint records (40 B); match_id[n_names], name_id[n_names] (u32); per flow 16 u32: the ten
//     session_key words, the L7 element's process_id, then dst_asn as {some, as_number, owner id, country id}, 0.
// Prints the state byte of every flow as two hex digits on one line ("invalid" when the list is refused), then
// the index's groups, rules and whether it has process ids.
// The index arrays are searched from heap blocks of exactly their size, so a probe outside one is an overflow
// the sanitizer reports; the program itself checks the order the searches rely on (exit code 6).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../flodbadd_amd/csrc/fb_wl_match.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

struct FlowAsn {
    const uint32_t* w;  // the flow's words 11..14
    bool operator()(const uint32_t*, bool, uint32_t& as_number, uint32_t& owner, uint32_t& country) const {
        if (!w[0]) return false;
        as_number = w[1], owner = w[2], country = w[3];
        return true;
    }
};

template <class T>
static std::vector<T> exact(const std::vector<T>& v) {  // a block of exactly v.size() elements
    std::vector<T> o(v);
    o.shrink_to_fit();
    return o;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint64_t head[4];
    if (!read_all(in, head, sizeof head)) return 3;
    std::vector<fb_wl_endpoint> eps(head[0]);
    std::vector<uint32_t> match_id(head[1]), name_id(head[1]), flows(head[3] * 16);
    if (!read_all(in, eps.data(), eps.size() * sizeof(fb_wl_endpoint)) || !read_all(in, match_id.data(), match_id.size() * 4) ||
        !read_all(in, name_id.data(), name_id.size() * 4) || !read_all(in, flows.data(), flows.size() * 4))
        return 3;
    fclose(in);

    fbk::WlIndex ix;
    if (!fbk::build_whitelist_index(eps.data(), eps.size(), ix)) {
        puts("invalid");
        return 0;
    }
    // the order the searches rely on: addresses ascending, inside a run the keys -- (key, process) pairs --
    // strictly ascending; group keys strictly ascending; the rule offsets ascending and complete
    const size_t n4 = ix.a4.size(), n6 = ix.a6.size();
    if ((ix.with_proc ? ix.kp4.size() : ix.k4.size()) != n4 || (ix.with_proc ? ix.kp6.size() : ix.k6.size()) != n6) return 6;
    for (size_t i = 1; i < n4; ++i) {
        if (ix.a4[i - 1] > ix.a4[i]) return 6;
        if (ix.a4[i - 1] == ix.a4[i] && (ix.with_proc ? ix.kp4[i - 1] >= ix.kp4[i] : ix.k4[i - 1] >= ix.k4[i])) return 6;
    }
    for (size_t i = 1; i < n6; ++i) {
        const uint32_t a[4] = {ix.a6[i - 1].x, ix.a6[i - 1].y, ix.a6[i - 1].z, ix.a6[i - 1].w};
        const uint32_t b[4] = {ix.a6[i].x, ix.a6[i].y, ix.a6[i].z, ix.a6[i].w};
        if (fbk::wl_ip_lt(b, a, true)) return 6;
        if (!fbk::wl_ip_lt(a, b, true) && (ix.with_proc ? ix.kp6[i - 1] >= ix.kp6[i] : ix.k6[i - 1] >= ix.k6[i])) return 6;
    }
    if (ix.gbeg.size() != ix.gkey.size() + 1 || ix.gbeg.back() != ix.rules.size()) return 6;
    for (size_t g = 0; g < ix.gkey.size(); ++g) {
        if (g && (ix.gkey[g - 1] & ~fbk::kWlGroupFlags) >= (ix.gkey[g] & ~fbk::kWlGroupFlags)) return 6;
        if (ix.gbeg[g] > ix.gbeg[g + 1]) return 6;
    }

    const std::vector<uint32_t> a4 = exact(ix.a4), k4 = exact(ix.k4), k6 = exact(ix.k6), gkey = exact(ix.gkey),
                                gbeg = exact(ix.gbeg);
    const std::vector<unsigned long long> kp4 = exact(ix.kp4), kp6 = exact(ix.kp6);
    const std::vector<fbk::WlU4> a6 = exact(ix.a6);
    const std::vector<fbk::WlRule> rules = exact(ix.rules);
    const fbk::WlTables W = {a4.data(), k4.data(), a6.data(), k6.data(), gkey.data(), gbeg.data(), rules.data(), nullptr,
                             nullptr, kp4.data(), kp6.data(), (uint32_t)n4, (uint32_t)n6, (uint32_t)gkey.size(),
                             (uint32_t)rules.size(), 0u};
    std::vector<fb_l7_rec> plane(head[3]);
    for (uint64_t i = 0; i < head[3]; ++i) plane[i] = fb_l7_rec{flows[i * 16 + 10], 0, 0, 0};
    const fbk::WlProcNames P = {head[2] ? plane.data() : nullptr, match_id.data(), name_id.data(), (uint32_t)head[1]};
    for (uint64_t i = 0; i < head[3]; ++i) {
        const uint32_t* f = flows.data() + i * 16;
        const FlowAsn asn = {f + 11};
        const uint32_t b = ix.with_proc ? fbk::wl_eval<true>(W, asn, W.gkey, W.gbeg, W.rules, f, fbk::wl_flow_match_id(P, i), P.n != 0u)
                                        : fbk::wl_eval<false>(W, asn, W.gkey, W.gbeg, W.rules, f, 0u, false);
        printf("%02x", b);
    }
    printf("\n%zu %zu %d\n", gkey.size(), rules.size(), ix.with_proc ? 1 : 0);
    return 0;
}
