// wl_domain_host.cpp -- a stand-alone host program over fb_wl_domain.h, for the CPU tests
// (tests/test_wldomspace_oracle.py builds it with the address and undefined-behaviour sanitizers): the header a
// plain C++ compiler sees is the one fb_set_whitelist_dom and the name-match kernel include, so the pattern
// classification, the index build, the table searches and the byte comparisons run here exactly as they do there.
//   wl_domain_host IN
// IN (tests/wldomspace.py, write_corpus): u64 n_patterns, n_names; pattern_off[n_patterns + 1] (u64); the pattern
//     bytes; per name a u32 length and FB_DNS_MAX_NAME bytes.
// Prints "invalid" when the patterns are refused; else the patterns per kind on one line, then per name its row
// and flags byte as nine hex words.  The run is repeated under the hash masks {all bits, 0xF, bit 63 alone}: rows
// that differ between masks end the program with exit code 7.  The tables are searched from heap blocks of exactly
// their size, so a probe outside one is an overflow the sanitizer reports; the program itself checks the order
// the searches rely on (exit code 6).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../flodbadd_amd/csrc/fb_wl_domain.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

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
    uint64_t head[2];
    if (!read_all(in, head, sizeof head)) return 3;
    std::vector<uint64_t> off(head[0] + 1u);
    if (!read_all(in, off.data(), off.size() * 8u)) return 3;
    std::vector<uint8_t> blob(off.back());
    if (!read_all(in, blob.data(), blob.size())) return 3;
    std::vector<uint32_t> len(head[1]);
    std::vector<uint8_t> names(head[1] * FB_DNS_MAX_NAME);
    for (uint64_t i = 0; i < head[1]; ++i)
        if (!read_all(in, &len[i], 4) || !read_all(in, names.data() + i * FB_DNS_MAX_NAME, FB_DNS_MAX_NAME)) return 3;
    fclose(in);

    const unsigned long long masks[3] = {~0ull, 0xFull, 1ull << 63};
    std::vector<uint32_t> first;
    for (int m = 0; m < 3; ++m) {
        fbk::WlDomIndex ix;
        if (!fbk::build_wl_dom_index(blob.data(), off.data(), head[0], masks[m], ix)) {
            puts("invalid");
            return 0;
        }
        for (uint32_t k = 0; k < fbk::kWlDomHashed; ++k)  // ascending by (hash, length, id)
            for (size_t i = 1; i < ix.pid[k].size(); ++i) {
                const bool lt = ix.hash[k][i - 1] != ix.hash[k][i] ? ix.hash[k][i - 1] < ix.hash[k][i]
                                : ix.len[k][i - 1] != ix.len[k][i] ? ix.len[k][i - 1] < ix.len[k][i]
                                                                   : ix.pid[k][i - 1] < ix.pid[k][i];
                if (!lt) return 6;
            }
        for (size_t i = 1; i < ix.gpid.size(); ++i)
            if (ix.gpid[i - 1] >= ix.gpid[i]) return 6;
        // the tables as the device holds them: blocks of exactly their size
        const std::vector<uint8_t> b = exact(ix.blob);
        const std::vector<uint32_t> o = exact(ix.off), gp = exact(ix.gpid), gs = exact(ix.gstar);
        std::vector<unsigned long long> h[fbk::kWlDomHashed];
        std::vector<uint32_t> l[fbk::kWlDomHashed], p[fbk::kWlDomHashed];
        fbk::WlDomTables T = ix.tables();
        T.blob = b.data(), T.off = o.data(), T.gpid = gp.data(), T.gstar = gs.data();
        for (uint32_t k = 0; k < fbk::kWlDomHashed; ++k) {
            h[k] = exact(ix.hash[k]), l[k] = exact(ix.len[k]), p[k] = exact(ix.pid[k]);
            T.hash[k] = h[k].data(), T.len[k] = l[k].data(), T.pid[k] = p[k].data();
        }
        if (m == 0)
            printf("%u %u %u %u %u\n", ix.count[0], ix.count[1], ix.count[2], ix.count[3], ix.count[4]);
        std::vector<uint32_t> out;
        for (uint64_t i = 0; i < head[1]; ++i) {
            if (len[i] > FB_DNS_MAX_NAME) return 3;
            const std::vector<uint8_t> nm(names.begin() + i * FB_DNS_MAX_NAME, names.begin() + i * FB_DNS_MAX_NAME + len[i]);
            uint32_t row[FB_WL_NAME_MATCHES];
            uint8_t flags = 0;
            fbk::wl_dom_match_name(T, nm.data(), len[i], row, &flags);
            out.insert(out.end(), row, row + FB_WL_NAME_MATCHES);
            out.push_back(flags);
        }
        if (m == 0) first = out;
        else if (out != first) return 7;
    }
    for (size_t i = 0; i < first.size(); ++i) printf("%x%c", first[i], (i + 1) % (FB_WL_NAME_MATCHES + 1u) ? ' ' : '\n');
    return 0;
}
