// fb_zeek_fmt.h -- one Zeek conn.log line from one fb_flow_view: the single definition of the text
// format_sessions_zeek (src/sessions.rs:694-774) writes, for the kernel (fb_zeek.hip) and for host
// programs alike.  Plain C++: nothing of HIP is needed when a host compiler includes it (FB_ZK_HD is
// `inline` there, `__host__ __device__ inline` under hipcc -- the idea of flow_hash_words in
// fb_internal.h, without that header's HIP includes).
//
// A line is 21 tab-separated fields and a '\n' (DESIGN.md 3.15 has the rules and their exactness range):
//   ts uid id.orig_h id.orig_p id.resp_h id.resp_p proto service duration orig_bytes resp_bytes conn_state
//   local_orig local_resp missed_bytes history orig_pkts orig_ip_bytes resp_pkts resp_ip_bytes tunnel_parents
// zeek_line_len and zeek_line_write run the same field walker (zeek_walk) over two sinks, one that counts
// and one that stores, so the length pass and the write pass cannot disagree.
#pragma once

#include <stdint.h>

#include "../../include/flodbadd_gpu.h"

#if defined(__HIPCC__)
#define FB_ZK_HD __host__ __device__ inline
#else
#define FB_ZK_HD inline
#endif

namespace fbzeek {

// Decimal digits of x: how many, and stored so that they end at `end` -- no digit buffer in between, so
// nothing of a line lives in scratch memory.  A value that fits 32 bits never sees a 64-bit division; a
// larger one sheds nine digits per 64-bit division.
FB_ZK_HD uint32_t dec_len(uint64_t x) {
    uint32_t k = 1;
    for (; x >> 32; x /= 1000000000ull) k += 9;  // (x >= 2^32 > 10^9: the quotient is never 0)
    for (uint32_t y = (uint32_t)x; y >= 10u; y /= 10u) ++k;
    return k;
}
FB_ZK_HD void dec_store(uint64_t x, uint8_t* end) {
    while (x >> 32) {  // (the fixed nine digits are inner ones)
        const uint64_t q = x / 1000000000ull;
        uint32_t r = (uint32_t)(x - q * 1000000000ull);
        for (int k = 0; k < 9; ++k) {
            *--end = (uint8_t)('0' + r % 10u);
            r /= 10u;
        }
        x = q;
    }
    uint32_t y = (uint32_t)x;
    do {
        *--end = (uint8_t)('0' + y % 10u);
        y /= 10u;
    } while (y);
}

// The sinks.  `dec` takes a decimal number, `fixed` one of exactly k digits (zero-padded), `bytes` a run of
// characters, `hist` the history field (kept apart: a writer may leave it to someone else, see
// zeek_line_write).
struct CountSink {
    uint32_t n = 0;
    FB_ZK_HD void put(char) { ++n; }
    FB_ZK_HD void bytes(const char*, uint32_t k) { n += k; }
    FB_ZK_HD void dec(uint64_t x) { n += dec_len(x); }
    FB_ZK_HD void fixed(uint32_t, uint32_t k) { n += k; }
    FB_ZK_HD void hist(const uint8_t*, uint32_t k) { n += k; }
};
struct WriteSink {
    uint8_t* out;
    uint32_t n = 0;
    uint32_t hist_at = 0;  // where the history field starts
    FB_ZK_HD explicit WriteSink(uint8_t* o) : out(o) {}
    FB_ZK_HD void put(char c) { out[n++] = (uint8_t)c; }
    FB_ZK_HD void bytes(const char* p, uint32_t k) {
        for (uint32_t i = 0; i < k; ++i) out[n + i] = (uint8_t)p[i];
        n += k;
    }
    FB_ZK_HD void dec(uint64_t x) {
        n += dec_len(x);
        dec_store(x, out + n);
    }
    FB_ZK_HD void fixed(uint32_t v, uint32_t k) {
        for (uint32_t i = k; i-- > 0u; v /= 10u) out[n + i] = (uint8_t)('0' + v % 10u);
        n += k;
    }
    FB_ZK_HD void hist(const uint8_t* p, uint32_t k) {
        hist_at = n;
        if (p)
            for (uint32_t i = 0; i < k; ++i) out[n + i] = p[i];
        n += k;
    }
};

// us < 10^6 as six digits; `trim` drops trailing zeros (us != 0 then).
template <class Sink>
FB_ZK_HD void put_micros(Sink& s, uint32_t us, bool trim) {
    uint32_t k = 6;
    for (; trim && us % 10u == 0u && k > 1u; us /= 10u) --k;
    s.fixed(us, k);
}

FB_ZK_HD char hex_digit(uint32_t v) { return (char)(v < 10u ? '0' + v : 'a' + (v - 10u)); }

template <class Sink>
FB_ZK_HD void put_hex_group(Sink& s, uint32_t g) {  // 16 bits, lowercase, no leading zeros
    bool on = false;
    for (int sh = 12; sh >= 0; sh -= 4) {
        const uint32_t d = (g >> sh) & 15u;
        if (d || on || sh == 0) {
            s.put(hex_digit(d));
            on = true;
        }
    }
}

template <class Sink>
FB_ZK_HD void put_v4(Sink& s, uint32_t a) {
    for (int sh = 24; sh >= 0; sh -= 8) {
        s.dec((a >> sh) & 255u);
        if (sh) s.put('.');
    }
}

// An address as Rust's Display prints it: family 2, the dotted quad of word 0; family 10, Ipv6Addr's
// rules -- an IPv4-mapped address as ::ffff:a.b.c.d, otherwise lowercase groups without leading zeros
// with the first longest run of two or more zero groups as "::" (so :: and ::1 come out as such).
template <class Sink>
FB_ZK_HD void put_ip(Sink& s, const uint32_t w[4], uint32_t family) {
    if (family != 10u) {
        put_v4(s, w[0]);
        return;
    }
    if (w[0] == 0u && w[1] == 0u && w[2] == 0x0000FFFFu) {
        s.bytes("::ffff:", 7);
        put_v4(s, w[3]);
        return;
    }
    uint32_t g[8];
    for (int k = 0; k < 4; ++k) {
        g[2 * k] = w[k] >> 16;
        g[2 * k + 1] = w[k] & 0xFFFFu;
    }
    int best = 0, best_len = 0, cur = 0, cur_len = 0;
    for (int k = 0; k < 8; ++k) {
        if (g[k] == 0u) {
            if (cur_len == 0) cur = k;
            if (++cur_len > best_len) {
                best = cur;
                best_len = cur_len;
            }
        } else {
            cur_len = 0;
        }
    }
    if (best_len < 2) best_len = 0;
    for (int k = 0; k < 8; ++k) {
        if (best_len && k == best) {
            s.bytes("::", 2);
            k += best_len - 1;
            continue;
        }
        if (k && !(best_len && k == best + best_len)) s.put(':');
        put_hex_group(s, g[k]);
    }
}

// fb_flow_hash (fb_flow.hip; restated here so that this header stands without the HIP ones -- the uid
// test pins the two against each other).
FB_ZK_HD uint64_t key_hash(const fb_session_key& key) {
    const uint32_t w[10] = {key.src_ip[0], key.src_ip[1], key.src_ip[2], key.src_ip[3], key.dst_ip[0],
                            key.dst_ip[1], key.dst_ip[2], key.dst_ip[3],
                            (uint32_t)key.src_port | (uint32_t)key.dst_port << 16,
                            (uint32_t)key.protocol | (uint32_t)key.family << 8};
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int j = 0; j < 10; j += 2) {
        h ^= (uint64_t)w[j] | ((uint64_t)w[j + 1] << 32);
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 31;
    }
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    return h;
}

FB_ZK_HD uint64_t uid_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The session uid: a = fb_flow_hash(key), b = mix(a ^ start_time_ns), the sixteen bytes a then b big-endian
// with the version nibble set to 4 and the variant bits to 10, as 8-4-4-4-12 lowercase hex.
template <class Sink>
FB_ZK_HD void put_uid(Sink& s, const fb_session_key& key, uint64_t start_ns) {
    uint64_t a = key_hash(key);
    uint64_t b = uid_mix(a ^ start_ns);
    a = (a & ~0xF000ull) | 0x4000ull;                               // byte 6: (v & 0x0F) | 0x40
    b = (b & ~0xC000000000000000ull) | 0x8000000000000000ull;       // byte 8: (v & 0x3F) | 0x80
    for (int k = 0; k < 32; ++k) {
        const uint64_t v = k < 16 ? a : b;
        s.put(hex_digit((uint32_t)(v >> (60 - 4 * (k & 15))) & 15u));
        if (k == 7 || k == 11 || k == 15 || k == 19) s.put('-');
    }
}

// Is the record outside the range in which the integer ts / duration text equals the reference's f64
// text?  ts: 2^14 <= secs < 2^33; duration: |us| < 2^52.
FB_ZK_HD bool zeek_inexact(const fb_flow_view& v) {
    const uint64_t secs = v.time.start_time_ns / 1000000000ull;
    if (secs < (1ull << 14) || secs >= (1ull << 33)) return true;
    if (v.time.end_time_ns == FB_SEEN_NONE) return false;
    const int64_t us = (int64_t)(v.time.end_time_ns - v.time.start_time_ns) / 1000;
    return (us < 0 ? 0ull - (uint64_t)us : (uint64_t)us) >= (1ull << 52);
}

// The field walker: every character of the line of `v`, in order, into `s`.
template <class Sink>
FB_ZK_HD void zeek_walk(Sink& s, const fb_flow_view& v, const uint8_t* hist, uint32_t hist_len) {
    const fb_flow_rec& r = v.rec;
    // 1 ts: secs[.us], us as six digits without trailing zeros
    const uint64_t start = v.time.start_time_ns;
    const uint32_t sub_us = (uint32_t)(start % 1000000000ull) / 1000u;
    s.dec(start / 1000000000ull);
    if (sub_us) {
        s.put('.');
        put_micros(s, sub_us, true);
    }
    s.put('\t');
    // 2 uid
    put_uid(s, r.key, start);
    s.put('\t');
    // 3-6 endpoints
    put_ip(s, r.key.src_ip, r.key.family);
    s.put('\t');
    s.dec(r.key.src_port);
    s.put('\t');
    put_ip(s, r.key.dst_ip, r.key.family);
    s.put('\t');
    s.dec(r.key.dst_port);
    s.put('\t');
    // 7 proto, 8 service
    s.bytes(r.key.protocol == 6 ? "tcp" : "udp", 3);
    s.bytes("\t-\t", 3);
    // 9 duration: [-]secs.micros of the difference truncated to whole microseconds
    if (v.time.end_time_ns == FB_SEEN_NONE) {
        s.put('-');
    } else {
        const int64_t us = (int64_t)(v.time.end_time_ns - start) / 1000;
        const uint64_t mag = us < 0 ? 0ull - (uint64_t)us : (uint64_t)us;
        if (us < 0) s.put('-');
        s.dec(mag / 1000000ull);
        s.put('.');
        put_micros(s, (uint32_t)(mag % 1000000ull), false);
    }
    s.put('\t');
    // 10, 11 orig_bytes, resp_bytes
    s.dec(r.outbound_bytes);
    s.put('\t');
    s.dec(r.inbound_bytes);
    s.put('\t');
    // 12 conn_state
    switch (r.conn_state) {
        case FB_CONN_SF: s.bytes("SF", 2); break;
        case FB_CONN_S0: s.bytes("S0", 2); break;
        case FB_CONN_REJ: s.bytes("REJ", 3); break;
        case FB_CONN_S1: s.bytes("S1", 2); break;
        default: s.put('-'); break;
    }
    // 13 local_orig, 14 local_resp, 15 missed_bytes
    s.bytes("\t-\t-\t0\t", 7);
    // 16 history
    s.hist(hist, hist_len);
    s.put('\t');
    // 17-20 packet counters, 21 tunnel_parents
    s.dec(r.orig_pkts);
    s.put('\t');
    s.dec(r.orig_ip_bytes);
    s.put('\t');
    s.dec(r.resp_pkts);
    s.put('\t');
    s.dec(r.resp_ip_bytes);
    s.bytes("\t-\n", 3);
}

// Bytes of the line of `v` with a history of hist_len characters ('\n' included).
FB_ZK_HD uint32_t zeek_line_len(const fb_flow_view& v, uint32_t hist_len) {
    CountSink s;
    zeek_walk(s, v, (const uint8_t*)0, hist_len);
    return s.n;
}

// Stores the line at `out` and returns its bytes.  hist == NULL with hist_len != 0 leaves the hist_len
// bytes of the history field untouched for the caller to fill; *hist_at (when given) is their offset.
FB_ZK_HD uint32_t zeek_line_write(const fb_flow_view& v, const uint8_t* hist, uint32_t hist_len, uint8_t* out,
                                  uint32_t* hist_at = 0) {
    WriteSink s(out);
    zeek_walk(s, v, hist, hist_len);
    if (hist_at) *hist_at = s.hist_at;
    return s.n;
}

}  // namespace fbzeek
