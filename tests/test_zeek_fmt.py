"""CPU-side checks of the Zeek export: the line format of fb_zeek_fmt.h -- the header the kernel includes, here
under g++ with the sanitizers in a stand-alone program -- against format_sessions_zeek, the exactness range of
the integer ts / duration text, the uid, and the C ABI of fb_format_zeek_dev."""
import os
import re
import subprocess

import numpy as np

import zeekref
from flodbadd_amd import _native as N
from flodbadd_amd.sessions import (ZEEK_FIELDS, ZEEK_HEADER, Session, SessionInfo, format_sessions_zeek, pack_histories,
                                   rust_ip_str, session_uid, views_to_sessions)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_OFFSETS = {"lines": 0, "bytes": 8, "lines_written": 16, "ts_inexact": 24, "hist_mismatch": 32, "reserved": 40}
CONSTANTS = {"FB_ZEEK_FIXED_MAX": 312, "FB_ZEEK_STEP": 256, "FB_ZEEK_STAGE_BYTES": 40000, "FB_ZEEK_COOP_HIST": 64,
             "FB_DEBUG_ZEEK_DIRECT": 4, "FB_DEBUG_VIEW_DIRECT": 3, "FB_ABI_VERSION": 4}


def _split(text, lens):
    out, at = [], 0
    for n in lens.tolist():
        out.append(text[at:at + n])
        at += n
    assert at == len(text)
    return out


def test_host_formatter_equals_the_restatement():
    views, hist, n_slots = zeekref.corpus()
    assert 200 <= len(views) <= 600
    lens, wrote, flagged, text = zeekref.host_format(views, hist, n_slots)
    assert (lens == wrote).all()                      # zeek_line_len == the bytes zeek_line_write stored
    lines = _split(text, wrote)
    want = zeekref.expected_lines(views, hist)
    for k, (got, exp) in enumerate(zip(lines, want)):
        assert got == (exp + "\n").encode("ascii"), (k, got, exp)
    # the records outside the exact range are the ones the corpus put there, and they are counted
    assert flagged.tolist() == [zeekref.inexact(v) for v in views]
    assert 5 <= int(flagged.sum()) <= 20
    # every line: 21 fields, one newline at its end
    for l in lines:
        assert l.count(b"\t") == 20 and l.count(b"\n") == 1 and l.endswith(b"\t-\n")
    # the histories are the blob's, whole
    for v, l in zip(views, lines):
        assert l.split(b"\t")[15].decode() == hist.get(int(v["rec"]["slot"]), "")


def test_no_blob_and_uncovered_slots_give_empty_histories():
    views, hist, n_slots = zeekref.corpus()
    lens, wrote, _, text = zeekref.host_format(views)
    assert (lens == wrote).all()
    assert all(l.split(b"\t")[15] == b"" for l in _split(text, wrote))
    cut = int(np.sort(views["rec"]["slot"])[len(views) // 2])  # offsets that cover only the slots below `cut`
    low = {s: h for s, h in hist.items() if s < cut}
    _, wrote, _, text = zeekref.host_format(views, low, cut)
    for v, l in zip(views, _split(text, wrote)):
        assert l.split(b"\t")[15].decode() == low.get(int(v["rec"]["slot"]), "")


def test_fixed_max_is_reached_by_the_extreme_record_and_exceeded_by_none():
    views, hist, n_slots = zeekref.corpus()
    lens, _, _, _ = zeekref.host_format(views)        # without histories: the fixed part of every line
    assert int(lens.max()) == N.FB_ZEEK_FIXED_MAX
    ext, _, _ = zeekref.finish([zeekref.extreme_record()])
    lens, wrote, _, text = zeekref.host_format(ext)
    assert lens.tolist() == [N.FB_ZEEK_FIXED_MAX] and wrote.tolist() == [N.FB_ZEEK_FIXED_MAX]
    f = text.decode().rstrip("\n").split("\t")
    assert [len(x) for x in f] == [18, 36, 39, 5, 39, 5, 3, 1, 18, 20, 20, 3, 1, 1, 1, 0, 20, 20, 20, 20, 1]
    # random records never exceed it
    rng = np.random.default_rng(11)
    raw = rng.integers(0, 256, size=(2000, N.FLOW_VIEW_DTYPE.itemsize), dtype=np.uint8)
    rnd = raw.view(N.FLOW_VIEW_DTYPE).reshape(-1).copy()
    rnd["rec"]["family"][::2] = 10
    lens, wrote, _, _ = zeekref.host_format(rnd)
    assert (lens == wrote).all() and int(lens.max()) <= N.FB_ZEEK_FIXED_MAX


def _sweep_views(start, end):
    v = np.zeros(len(start), dtype=N.FLOW_VIEW_DTYPE)
    v["rec"]["family"], v["rec"]["protocol"] = 2, 17
    v["time"]["start_time_ns"], v["time"]["end_time_ns"] = start, end
    return v


def test_integer_ts_equals_the_shortest_round_trip_float_text():
    """>= 10^5 seeded (secs, us) draws in [2^14, 2^33) x [0, 10^6): the header's integer text against repr()."""
    rng = np.random.default_rng(20250717)
    n = 120000
    secs = np.concatenate([rng.integers(1 << 14, 1 << 33, n // 2), (2.0 ** rng.uniform(14, 33, n // 2)).astype(np.int64)])
    secs = np.clip(secs, 1 << 14, (1 << 33) - 1).astype(np.uint64)
    us = rng.integers(0, 10 ** 6, n).astype(np.uint64)
    us[::7] = us[::7] // 1000 * 1000                  # short fractions too
    us[::11] = 0
    start = secs * np.uint64(10 ** 9) + us * np.uint64(1000) + rng.integers(0, 1000, n).astype(np.uint64)
    lens, wrote, flagged, text = zeekref.host_format(_sweep_views(start, np.full(n, N.FB_SEEN_NONE, dtype=np.uint64)))
    assert not flagged.any()
    got = [l.split(b"\t", 1)[0].decode() for l in _split(text, wrote)]
    bad = 0
    for g, s, u in zip(got, secs.tolist(), us.tolist()):
        r = repr(float(s) + float(u) / 1e6)
        bad += g != (r[:-2] if r.endswith(".0") else r)
    assert bad == 0


def test_integer_duration_equals_the_six_digit_float_text():
    """>= 10^5 seeded draws of |us| < 2^52, both signs and every magnitude: the header's text against '%.6f'."""
    rng = np.random.default_rng(20250718)
    n = 120000
    mag = np.concatenate([rng.integers(0, 1 << 52, n // 2), (2.0 ** rng.uniform(0, 52, n // 2)).astype(np.int64)])
    mag = np.clip(mag, 0, (1 << 52) - 1)
    us = mag * rng.choice([-1, 1], n)
    d = us * 1000 + np.sign(us) * rng.integers(0, 1000, n)          # truncation toward zero drops this
    start = np.full(n, 6 * 10 ** 18, dtype=np.uint64)
    end = (start.astype(object) + d.astype(object)) % (1 << 64)
    lens, wrote, flagged, text = zeekref.host_format(_sweep_views(start, np.array(end, dtype=np.uint64)))
    assert not flagged.any()
    got = [l.split(b"\t")[8].decode() for l in _split(text, wrote)]
    bad = sum(g != "%.6f" % (float(u) / 1e6) for g, u in zip(got, us.tolist()))
    assert bad == 0


def test_rust_ip_text():
    want = {"::": "::", "::1": "::1", "::ffff:1.2.3.4": "::ffff:1.2.3.4", "0:0:0:1:2:3:4:5": "::1:2:3:4:5",
            "1:2:0:0:0:3:4:5": "1:2::3:4:5", "1:2:3:4:5:0:0:0": "1:2:3:4:5::", "1:0:0:2:3:0:0:4": "1::2:3:0:0:4",
            "1:0:0:2:0:0:0:3": "1:0:0:2::3", "1:2:3:0:4:5:6:7": "1:2:3:0:4:5:6:7", "::1.2.3.4": "::102:304",
            "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff": "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff",
            "2001:0DB8::00a0": "2001:db8::a0", "1.2.3.4": "1.2.3.4"}
    for text, exp in want.items():
        assert rust_ip_str(text) == exp
    assert set(want) >= set(zeekref.V6_TEXT[:3])


def test_header_and_pack_histories():
    assert ZEEK_HEADER.split("\t") == ZEEK_FIELDS and len(ZEEK_FIELDS) == 21
    assert ZEEK_FIELDS[0] == "ts" and ZEEK_FIELDS[15] == "history" and ZEEK_FIELDS[20] == "tunnel_parents"
    assert format_sessions_zeek([]) == [ZEEK_HEADER]
    chars, off = pack_histories({3: "Sh", 0: "A", 5: ""}, 6)
    assert chars.tobytes() == b"ASh" and off.dtype == np.uint64 and off.tolist() == [0, 1, 1, 1, 3, 3, 3]
    chars, off = pack_histories({}, 2)
    assert len(chars) == 0 and off.tolist() == [0, 0, 0]


def test_uid():
    views, hist, _ = zeekref.corpus()
    _, wrote, _, text = zeekref.host_format(views)
    lines = _split(text, wrote)
    pat = re.compile(r"^[0-9a-f]{8}-[0-9a-f]{4}-4[0-9a-f]{3}-[89ab][0-9a-f]{3}-[0-9a-f]{12}$")
    for v, l in zip(views, lines):
        uid = l.split(b"\t")[1].decode()
        assert pat.match(uid), uid                    # version nibble 4, variant bits 10
        # session_uid (the library's host-side fb_flow_hash) is the formatter's uid field
        assert session_uid(Session.from_key(v["rec"]), int(v["time"]["start_time_ns"])) == uid
    k = views[:1].copy()
    s = Session.from_key(k[0]["rec"])
    t = int(k[0]["time"]["start_time_ns"])
    k["rec"]["padding"] = 0xBEEF                      # a copy of the key: its padding is not part of it
    k["rec"]["slot"] = 12345                          # nor is the slot
    _, w2, _, t2 = zeekref.host_format(k)
    assert t2.split(b"\t")[1].decode() == session_uid(s, t)
    assert session_uid(s, t) != session_uid(s, t + 1)
    assert session_uid(s, t) != session_uid(s.reversed(), t)
    info = views_to_sessions(views[:1])[0]
    assert isinstance(SessionInfo.uid, property) and "uid" not in SessionInfo.__dataclass_fields__
    assert info.uid == session_uid(s, t)


def test_stats_struct_and_constants_match_the_header(tmp_path):
    dt = N.ZEEK_STATS_DTYPE
    assert list(dt.names) == list(STATS_OFFSETS) and dt.itemsize == 64
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s/include/flodbadd_gpu.h"' % ROOT, "int main(void) {",
           'printf("%zu\\n", sizeof(fb_zeek_stats));']
    want = [64]
    for f in dt.names:
        assert dt.fields[f][1] == STATS_OFFSETS[f], f
        src.append('printf("%%zu\\n", offsetof(fb_zeek_stats, %s));' % f)
        want.append(STATS_OFFSETS[f])
    for c, v in CONSTANTS.items():
        src.append('printf("%%u\\n", (unsigned)%s);' % c)
        want.append(v)
        assert getattr(N, c) == v
    src.append("return 0; }")
    c = tmp_path / "zeek.c"
    c.write_text("\n".join(src) + "\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "zeek"), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "zeek")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want


def test_symbol_is_exported_and_rejects_null_arguments():
    lib = N.gpu_lib()
    assert hasattr(lib, "fb_format_zeek_dev")
    assert lib.fb_format_zeek_dev(None, None, 0, None, None, 0, None, 0, None, None, None) == N.FB_ERR_INVAL
    x = np.zeros(64, dtype=np.uint64)                 # (never dereferenced: the context is checked first)
    assert lib.fb_format_zeek_dev(None, N.ptr(x), 0, None, None, 0, None, 0, N.ptr(x), N.ptr(x), None) == N.FB_ERR_INVAL
