"""The Zeek export's test corpus and its expectations.

corpus() builds fb_flow_view records (FLOW_VIEW_DTYPE) and their histories ({slot: str}) over the cases the
format has: both families and protocols, the IPv6 text forms, extreme ports and counters, every conn_state,
the end_time and microsecond edge cases, the ends of the exact ts range, a few records outside it, and
history lengths around the kernel's thresholds.  host_format() runs the stand-alone host program
(tests/zeek_fmt_host.cpp: fb_zeek_fmt.h under g++ with the address and undefined-behaviour sanitizers) over
records; expected_lines() is the Python side -- format_sessions_zeek's float path, with the integer text
(int_ts / int_duration, written here from the rules, not from the header) for the records the float path
does not cover."""
import functools
import ipaddress
import os
import shutil
import subprocess
import tempfile

import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.sessions import format_sessions_zeek, ip_to_words, pack_histories, views_to_sessions

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = N.FB_SEEN_NONE
T0 = 1752800000
V6_TEXT = ["::", "::1", "::ffff:1.2.3.4", "::ffff:255.255.255.255", "0:0:0:1:2:3:4:5", "1:2:0:0:0:3:4:5",
           "1:2:3:4:5:0:0:0", "1:0:0:2:3:0:0:4", "1:0:0:2:0:0:0:3", "1:2:3:0:4:5:6:7", "0:1:2:3:4:5:6:7",
           "1:2:3:4:5:6:7:0", "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "::1.2.3.4", "::ffff:0:1", "64:ff9b::102:304",
           "2001:db8:a0b:12f0::1", "fe80::1ff:fe23:4567:890a", "0:0:1::", "a:b:c:d:e:f:0:0"]
COUNTERS = [0, 9, 10, 99, 1 << 32, 5 * 10 ** 9, 10 ** 9, (1 << 32) - 1, 10 ** 18, 10 ** 18 + 7, (1 << 64) - 1]
HIST_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 5000]


def history_of(length, seed=0):
    rng = np.random.default_rng(1000 + seed)
    return "".join(N.FB_HIST_CHARS[k] for k in rng.integers(0, len(N.FB_HIST_CHARS), length))


def record(src="192.168.1.10", dst="93.184.216.34", sport=51234, dport=443, proto=6, start=T0 * 10 ** 9 + 123456789,
           end=NONE, counters=(1200, 3400, 5, 7, 1500, 3800), conn_state=0, hist_len=0):
    """One view record; the slot is assigned by finish()."""
    v = np.zeros(1, dtype=N.FLOW_VIEW_DTYPE)
    s, fam = ip_to_words(src)
    d, fam_d = ip_to_words(dst)
    assert fam == fam_d
    r = v[0]["rec"]
    r["src_ip"], r["dst_ip"], r["family"], r["protocol"] = s, d, fam, proto
    r["src_port"], r["dst_port"] = sport, dport
    for f, c in zip(("outbound_bytes", "inbound_bytes", "orig_pkts", "resp_pkts", "orig_ip_bytes", "resp_ip_bytes"),
                    counters):
        r[f] = c
    r["conn_state"], r["hist_len"] = conn_state, hist_len
    r["end_seen"] = NONE
    start, end = start & ((1 << 64) - 1), end & ((1 << 64) - 1)
    t = v[0]["time"]
    t["start_time_ns"], t["last_activity_ns"], t["end_time_ns"], t["last_segment_end_ns"] = start, start, end, NONE
    v[0]["last_modified_ns"] = start
    return v


def finish(records, seed=7):
    """Concatenate records, give them distinct, scattered slots and histories of their hist_len ->
    (views, {slot: history}, n_slots)."""
    views = np.concatenate(records)
    n = len(views)
    n_slots = 3 * n + 2
    slots = np.random.default_rng(seed).permutation(n_slots)[:n].astype(np.uint32)
    views["rec"]["slot"], views["time"]["slot"] = slots, slots
    hist = {int(s): history_of(int(h), k) for k, (s, h) in enumerate(zip(slots, views["rec"]["hist_len"])) if h}
    return views, hist, n_slots


def extreme_record():
    """Every field at its longest: FB_ZEEK_FIXED_MAX bytes without a history."""
    full = "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff"
    start = (1 << 64) - 1
    return record(full, "eeee:eeee:eeee:eeee:eeee:eeee:eeee:eeee", 65535, 65535, 6, start, (1 << 63) - 1,
                  ((1 << 64) - 1,) * 6, 3, 0)


@functools.lru_cache(maxsize=None)
def corpus():
    recs = []
    for proto in (6, 17):
        recs.append(record(proto=proto))
        recs.append(record("2001:db8::1", "2001:db8::2", proto=proto))
    other = "2001:db8:1:2:3:4:5:6"
    for a in V6_TEXT:
        recs.append(record(a, other))
        recs.append(record(other, a, proto=17))
    for a in ("0.0.0.0", "255.255.255.255", "10.0.0.1", "1.20.255.0"):
        recs.append(record(a, "8.8.8.8"))
    for p in (0, 1, 9, 10, 65535):
        recs.append(record(sport=p, dport=65535 - p))
    for k in range(len(COUNTERS)):
        recs.append(record(counters=[COUNTERS[(k + j) % len(COUNTERS)] for j in range(6)]))
    for cs in range(6):
        recs.append(record(conn_state=cs, end=T0 * 10 ** 9 + 5 * 10 ** 9))
    base = T0 * 10 ** 9 + 123456789
    for end in (base, base + 999, base + 1000, base + 1, base - 1, base - 999, base - 1000, base - 1500,
                base - 3500000000, base + 3500000000, base + 86400 * 10 ** 9, base + 1000000000):
        recs.append(record(end=end, conn_state=1))
    for secs in (1 << 14, (1 << 33) - 1, T0):
        for us in [0, 1, 100000, 999999, 10, 123450] + [15625 * k for k in (1, 3, 7, 33, 63)]:
            for ns in (0, 999):
                recs.append(record(start=secs * 10 ** 9 + us * 1000 + ns))
    # outside the exact range: counted in ts_inexact, excluded from the float comparison
    for start in (0, 999, 1000, ((1 << 14) - 1) * 10 ** 9 + 5000, (1 << 33) * 10 ** 9, (1 << 34) * 10 ** 9 + 5000000,
                  (1 << 64) - 1):
        recs.append(record(start=start))
    recs.append(record(end=base + (1 << 52) * 1000, conn_state=1))
    recs.append(record(end=base - (1 << 52) * 1000 - 5, conn_state=1))
    recs.append(extreme_record())
    for k, h in enumerate(HIST_LENS + HIST_LENS[:6]):
        recs.append(record(sport=40000 + k, hist_len=h, conn_state=k % 6,
                           src="2001:db8::5" if k % 2 else "10.1.2.3", dst="2001:db8::6" if k % 2 else "10.3.2.1"))
    # seeded combinations of the above, so that neighbouring lines differ in every field
    rng = np.random.default_rng(3)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]  # noqa: E731
    for k in range(140):
        v6 = bool(k % 3 == 0)
        start = int(rng.integers(1 << 14, 1 << 33)) * 10 ** 9 + int(rng.integers(0, 10 ** 6)) * 1000 * int(k % 5 != 0)
        end = NONE if k % 4 == 0 else start + int(rng.integers(-10 ** 10, 10 ** 13))
        recs.append(record(pick(V6_TEXT) if v6 else str(ipaddress.IPv4Address(int(rng.integers(0, 1 << 32)))),
                           pick(V6_TEXT) if v6 else "10.0.0.%d" % (k % 256), int(rng.integers(0, 65536)),
                           int(rng.integers(0, 65536)), 6 if k % 2 else 17, start, end,
                           [pick(COUNTERS) if j == k % 6 else int(rng.integers(0, 10 ** int(rng.integers(1, 19))))
                            for j in range(6)], k % 6, int(rng.integers(0, 40)) if k % 2 else 0))
    return finish(recs)


def inexact(view):
    secs = int(view["time"]["start_time_ns"]) // 10 ** 9
    if not (1 << 14) <= secs < (1 << 33):
        return True
    end = int(view["time"]["end_time_ns"])
    return end != NONE and abs(_micros(int(view["time"]["start_time_ns"]), end)) >= 1 << 52


def _micros(start, end):
    d = ((end - start + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)
    return -(-d // 1000) if d < 0 else d // 1000


def int_ts(start):
    secs, us = start // 10 ** 9, start % 10 ** 9 // 1000
    return str(secs) if us == 0 else ("%d.%06d" % (secs, us)).rstrip("0")


def int_duration(start, end):
    if end == NONE:
        return "-"
    us = _micros(start, end)
    return "%s%d.%06d" % ("-" if us < 0 else "", abs(us) // 10 ** 6, abs(us) % 10 ** 6)


def expected_lines(views, histories):
    """The lines of `views`, in their order, without newlines: format_sessions_zeek over views_to_sessions of
    each record; the ts and duration of a record outside the exact range are the integer text."""
    out = []
    for k in range(len(views)):
        line = format_sessions_zeek(views_to_sessions(views[k:k + 1], histories))[1]
        if inexact(views[k]):
            f = line.split("\t")
            start, end = int(views[k]["time"]["start_time_ns"]), int(views[k]["time"]["end_time_ns"])
            f[0], f[8] = int_ts(start), int_duration(start, end)
            line = "\t".join(f)
        out.append(line)
    return out


def expected_text(views, histories):
    """(text bytes, line_off) of the whole export."""
    lines = [(l + "\n").encode("ascii") for l in expected_lines(views, histories)]
    off = np.zeros(len(lines) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(l) for l in lines], dtype=np.uint64)
    return b"".join(lines), off


@functools.lru_cache(maxsize=None)
def host_program():
    """The stand-alone host program, built once per run with the sanitizers (host code, its own main)."""
    d = tempfile.mkdtemp(prefix="zeekfmt")
    exe = os.path.join(d, "zeek_fmt_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "zeek_fmt_host.cpp")], check=True)
    return exe


def host_format(views, histories=None, n_slots=0):
    """The host program over `views` -> (zeek_line_len per record, bytes written per record, inexact flag per
    record, the text).  histories None: no blob."""
    d = tempfile.mkdtemp(prefix="zeekrun")
    src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(src, "wb") as f:
        if histories is None:
            np.array([len(views), 0, 0], dtype=np.uint64).tofile(f)
            views.tofile(f)
        else:
            chars, off = pack_histories(histories, n_slots)
            np.array([len(views), n_slots, 1], dtype=np.uint64).tofile(f)
            views.tofile(f)
            off.tofile(f)
            chars.tofile(f)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    try:
        subprocess.run([host_program(), src, dst], check=True, env=env)
        with open(dst, "rb") as f:
            raw = f.read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    head = np.frombuffer(raw[:12 * len(views)], dtype=np.uint32).reshape(-1, 3)
    return head[:, 0].copy(), head[:, 1].copy(), head[:, 2].astype(bool), raw[12 * len(views):]
