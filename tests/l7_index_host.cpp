// l7_index_host.cpp -- a stand-alone host program over fb_l7_index.h, for the CPU tests (tests/test_l7_abi.py
// builds it with the address and undefined-behaviour sanitizers): the header a plain C++ compiler sees is the
// one fb_set_l7_sockets and the L7 pass's kernels include, so the index build and l7_match run here exactly as
// they do there.
//   l7_index_host IN OUT
// IN:  u64 n_sockets, u64 n_keys; n_sockets fb_l7_socket records (48 B); n_keys fb_session_key records (40 B).
// OUT: u64 status (0 ok, 1 the snapshot is invalid), u64 n_pairs, u64 n_locals; then per key u32 process_id,
//      u32 source.
// The tables are searched from heap blocks of exactly their size, so a probe outside a table is an overflow the
// sanitizer reports; the program itself checks that both tables are strictly ascending (exit code 6).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../flodbadd_amd/csrc/fb_l7_index.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

template <uint32_t W>
static bool ascending(const std::vector<fbk::L7Entry<W>>& v) {
    for (size_t i = 1; i < v.size(); ++i)
        if (fbk::l7_cmp<W>(v[i - 1].k, v[i].k) >= 0) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint64_t head[2];
    if (!read_all(in, head, sizeof head)) return 3;
    std::vector<fb_l7_socket> socks(head[0]);
    std::vector<uint32_t> keys(head[1] * 10);
    if (!read_all(in, socks.data(), socks.size() * sizeof(fb_l7_socket)) || !read_all(in, keys.data(), keys.size() * 4))
        return 3;
    fclose(in);

    std::vector<fbk::L7Pair> pairs;
    std::vector<fbk::L7Local> locals;
    std::vector<uint64_t> out = {0, 0, 0};
    if (!fbk::build_l7_index(socks.data(), socks.size(), pairs, locals)) {
        out[0] = 1;
    } else {
        if (!ascending(pairs) || !ascending(locals)) return 6;
        pairs.shrink_to_fit();
        locals.shrink_to_fit();
        out[1] = pairs.size();
        out[2] = locals.size();
        const fbk::L7Tables t = {pairs.data(), locals.data(), (uint32_t)pairs.size(), (uint32_t)locals.size()};
        for (uint64_t i = 0; i < head[1]; ++i) {
            const fbk::L7Match m = fbk::l7_match(t, keys.data() + i * 10);
            out.push_back((uint64_t)m.pid | (uint64_t)m.source << 32);
        }
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(out.data(), 8, out.size(), o);
    return fclose(o) == 0 ? 0 : 4;
}
