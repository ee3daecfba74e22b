// dns_hash_host.cpp -- a stand-alone host program over fb_dns_hash.h, for the CPU tests (tests/dnstrackspace.py
// builds it with the address and undefined-behaviour sanitizers): the header a plain C++ compiler sees is the
// one the tracker's kernels include.
//   dns_hash_host IN OUT
// IN:  u64 n_names, u64 n_addrs, u64 hash_mask; u16 name_len[n_names]; n_names rows of 256 bytes (the name,
//      then whatever the caller put past name_len); n_addrs records of 5 u32 (4 address words, family).
// OUT: u64 name_tag per name, then u64 dns_addr_tag per address.
// Every name is hashed from a buffer of exactly (len + 3) / 4 dwords, so a tag function that read a dword
// past the name is an overflow the sanitizer reports.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../flodbadd_amd/csrc/fb_dns_hash.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint64_t head[3];
    if (!read_all(in, head, sizeof head)) return 3;
    const uint64_t n_names = head[0], n_addrs = head[1], mask = head[2];
    std::vector<uint16_t> len(n_names);
    std::vector<uint8_t> rows(n_names * 256);
    std::vector<uint32_t> addrs(n_addrs * 5);
    if (!read_all(in, len.data(), n_names * 2) || !read_all(in, rows.data(), rows.size()) ||
        !read_all(in, addrs.data(), addrs.size() * 4))
        return 3;
    fclose(in);

    std::vector<uint64_t> tags;
    for (uint64_t i = 0; i < n_names; ++i) {
        if (len[i] > 255) return 5;
        std::vector<uint32_t> name((len[i] + 3u) / 4u);
        if (!name.empty()) memcpy(name.data(), rows.data() + i * 256, name.size() * 4);
        tags.push_back(fbk::name_tag(name.data(), len[i], mask));
    }
    for (uint64_t i = 0; i < n_addrs; ++i) {
        uint32_t w[4] = {addrs[i * 5], addrs[i * 5 + 1], addrs[i * 5 + 2], addrs[i * 5 + 3]};
        tags.push_back(fbk::dns_addr_tag(w, addrs[i * 5 + 4], mask));
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    if (!tags.empty()) fwrite(tags.data(), 8, tags.size(), out);
    return fclose(out) == 0 ? 0 : 4;
}
