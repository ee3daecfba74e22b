// zeek_fmt_host.cpp -- a stand-alone host program over fb_zeek_fmt.h, for the CPU tests (tests/zeekref.py
// builds it with the address and undefined-behaviour sanitizers): the header a plain C++ compiler sees is the
// one the kernel includes.
//   zeek_fmt_host IN OUT
// IN:  u64 n, u64 n_slots, u64 has_blob; n fb_flow_view; with a blob: u64 off[n_slots + 1], then the characters.
// OUT: per record u32 zeek_line_len, u32 bytes zeek_line_write stored, u32 zeek_inexact; then the text.
// Every line is written into a buffer of exactly zeek_line_len bytes, so a walker that stored more than it
// counted is an overflow the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../flodbadd_amd/csrc/fb_zeek_fmt.h"

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint64_t head[3];
    if (!read_all(in, head, sizeof head)) return 3;
    const uint64_t n = head[0], n_slots = head[1];
    const bool blob = head[2] != 0;
    std::vector<fb_flow_view> views(n);
    if (!read_all(in, views.data(), n * sizeof(fb_flow_view))) return 3;
    std::vector<uint64_t> off;
    std::vector<uint8_t> chars;
    if (blob) {
        off.resize(n_slots + 1);
        if (!read_all(in, off.data(), off.size() * 8)) return 3;
        chars.resize(off[n_slots]);
        if (!read_all(in, chars.data(), chars.size())) return 3;
    }
    fclose(in);

    std::vector<uint32_t> meta;
    std::vector<uint8_t> text;
    for (uint64_t i = 0; i < n; ++i) {
        const fb_flow_view& v = views[i];
        const uint8_t* h = nullptr;
        uint32_t hl = 0;
        if (blob && v.rec.slot < n_slots) {
            h = chars.data() + off[v.rec.slot];
            hl = (uint32_t)(off[v.rec.slot + 1] - off[v.rec.slot]);
        }
        const uint32_t len = fbzeek::zeek_line_len(v, hl);
        std::vector<uint8_t> line(len);
        const uint32_t wrote = fbzeek::zeek_line_write(v, h, hl, line.data());
        meta.push_back(len);
        meta.push_back(wrote);
        meta.push_back(fbzeek::zeek_inexact(v) ? 1u : 0u);
        text.insert(text.end(), line.begin(), line.end());
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    if (!meta.empty()) fwrite(meta.data(), 4, meta.size(), out);
    if (!text.empty()) fwrite(text.data(), 1, text.size(), out);
    return fclose(out) == 0 ? 0 : 4;
}
