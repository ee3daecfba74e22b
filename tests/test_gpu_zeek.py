"""The Zeek conn.log export on the GPU (fb_format_zeek_dev, flodbadd_amd/csrc/fb_zeek.hip; export_zeek and
get_sessions_zeek of the capture).

The kernel's text is compared byte for byte with tests/zeekref.py's expectation -- format_sessions_zeek over
views_to_sessions of the same records, the Python restatement with the float path -- on the CPU tests' corpus
and on inputs built around the kernel's own thresholds (the 256-record step, the staging budget
FB_ZEEK_STAGE_BYTES, the cooperative-copy length FB_ZEEK_COOP_HIST, every alignment of a step's range), staged
and direct.  No tolerance applies anywhere: the output is text.  The text buffer is followed by a 64-byte guard
region that must come back untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import framegen as fg
import joinref
import zeekref
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture
from flodbadd_amd.sessions import SessionFilter, format_sessions_zeek, pack_histories, views_to_sessions

pytestmark = pytest.mark.gpu

S = 10 ** 9
T0 = 1_752_800_000 * S
FILL, GUARD = 0xA5, 64
STAGE, STEP, COOP = N.FB_ZEEK_STAGE_BYTES, N.FB_ZEEK_STEP, N.FB_ZEEK_COOP_HIST


@pytest.fixture(scope="module")
def cap():
    c = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 10, timed=True)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _plain_pool():
    return np.concatenate([zeekref.record(sport=20000 + 7 * k, counters=(k, 2 * k, 3, 4, 50 * k, 6), proto=(6, 17)[k % 2],
                                          conn_state=k % 6, end=zeekref.NONE if k % 3 else T0 + k * 1000)
                           for k in range(64)])


def make(n, hist_lens=None, seed=1, v4=False):
    """n records cycled from the corpus (v4: from short IPv4 records instead, 256 of which leave room under the
    staging budget), with the given history lengths (default: none) -> (views, {slot: str}, n_slots)."""
    base = _plain_pool() if v4 else zeekref.corpus()[0]
    v = base[np.arange(n) % len(base)].copy()
    v["rec"]["hist_len"] = 0 if hist_lens is None else np.asarray(hist_lens, dtype=np.uint32)
    return zeekref.finish([v], seed)


def run(cap, views, hist=None, n_slots=0, text_cap=None, direct=False, shift=0):
    """fb_format_zeek_dev over host-made records -> (the text_cap bytes of the text buffer, the guard region
    after it, line_off, stats).  The text buffer starts `shift` bytes into its allocation and is filled with
    FILL, guard included; line_off and the stats are filled too, so what comes back was written."""
    lib = N.gpu_lib()
    n = len(views)
    N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_ZEEK_DIRECT, int(direct)))
    d_views = N.DeviceBuffer(max(n, 1) * N.FLOW_VIEW_DTYPE.itemsize)
    if n:
        d_views.upload(views)
    d_hist = d_hoff = None
    hist_bytes = 0
    if hist is not None:
        chars, off = pack_histories(hist, n_slots)
        hist_bytes = len(chars)
        d_hist, d_hoff = N.DeviceBuffer(max(hist_bytes, 1)), N.DeviceBuffer(off.nbytes).upload(off)
        if hist_bytes:
            d_hist.upload(chars)
    if text_cap is None:
        text_cap = n * N.FB_ZEEK_FIXED_MAX + hist_bytes
    d_text, d_off, d_stats = N.DeviceBuffer(shift + text_cap + GUARD), N.DeviceBuffer(8 * (n + 1)), N.DeviceBuffer(64)
    for b in (d_text, d_off, d_stats):
        b.memset(FILL)
    try:
        N.check(lib.fb_format_zeek_dev(cap.ctx, d_views.ptr, n, d_hist.ptr if d_hist else None,
                                       d_hoff.ptr if d_hoff else None, n_slots, C.c_void_p(d_text.ptr.value + shift),
                                       text_cap, d_off.ptr, d_stats.ptr, None))
    finally:
        lib.fb_debug_set(cap.ctx, N.FB_DEBUG_ZEEK_DIRECT, 0)
    raw = d_text.download(np.zeros(shift + text_cap + GUARD, dtype=np.uint8))
    assert (raw[:shift] == FILL).all()
    off = d_off.download(np.zeros(n + 1, dtype=np.uint64))
    st = d_stats.download(np.zeros(1, dtype=N.ZEEK_STATS_DTYPE))
    assert not st[0]["reserved"].any()
    return raw[shift:shift + text_cap], raw[shift + text_cap:], off, {k: int(st[0][k]) for k in N.ZEEK_STATS_FIELDS}


def check_full(cap, views, hist, n_slots, want=None, **kw):
    """Both paths over the input with room for everything: the expected text, offsets and counters."""
    text, off = want if want is not None else zeekref.expected_text(views, hist or {})
    outs = []
    for direct in (False, True):
        got, guard, goff, st = run(cap, views, hist, n_slots, direct=direct, **kw)
        assert (guard == FILL).all()
        assert goff.tolist() == off.tolist()
        assert got[:len(text)].tobytes() == text
        assert (got[len(text):] == FILL).all()
        assert st["lines"] == st["lines_written"] == len(views) and st["bytes"] == len(text)
        assert st["ts_inexact"] == sum(zeekref.inexact(v) for v in views)
        outs.append((got.tobytes(), st))
    assert outs[0] == outs[1]
    return off, outs[0][1]


# ---- 1. the corpus ---------------------------------------------------------------------------------------
def test_corpus_equals_the_host_expectation(cap):
    views, hist, n_slots = zeekref.corpus()
    off, st = check_full(cap, views, hist, n_slots)
    assert st["hist_mismatch"] == 0 and 5 <= st["ts_inexact"] <= 20
    assert int(np.diff(off.astype(np.int64)).max()) > 5000                # the 5,000-character history is in
    # the extreme record is FB_ZEEK_FIXED_MAX bytes on the device too
    ext, _, _ = zeekref.finish([zeekref.extreme_record()])
    off, _ = check_full(cap, ext, None, 0)
    assert off.tolist() == [0, N.FB_ZEEK_FIXED_MAX]


def test_no_blob_mismatches_and_uncovered_slots(cap):
    views, hist, n_slots = zeekref.corpus()
    # no blob: every history field empty, nothing counted
    _, _, off, st = run(cap, views)
    text, want_off = zeekref.expected_text(views, {})
    assert off.tolist() == want_off.tolist() and st["hist_mismatch"] == 0 and st["bytes"] == len(text)
    # hist_len that disagrees with the blob: the blob decides the text, the record is counted
    bad = views.copy()
    with_hist = np.flatnonzero(bad["rec"]["hist_len"] > 0)[:3]
    bad["rec"]["hist_len"][with_hist] += 1
    bad["rec"]["hist_len"][np.flatnonzero(views["rec"]["hist_len"] == 0)[:2]] = 4
    got, _, off, st = run(cap, bad, hist, n_slots)
    text, want_off = zeekref.expected_text(views, hist)
    assert got[:len(text)].tobytes() == text and off.tolist() == want_off.tolist() and st["hist_mismatch"] == 5
    # offsets that cover only the low slots: the others have an empty history and count as mismatches
    cut = int(np.sort(views["rec"]["slot"])[len(views) // 2])
    low = {s: h for s, h in hist.items() if s < cut}
    got, _, off, st = run(cap, views, low, cut)
    text, want_off = zeekref.expected_text(views, low)
    assert got[:len(text)].tobytes() == text and off.tolist() == want_off.tolist()
    assert st["hist_mismatch"] == int((views["rec"]["slot"] >= cut).sum())


# ---- 2. staged against direct, around what can go wrong ------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_sizes_around_the_wave_and_the_step(cap, n):
    lens = [(k * 5) % 23 for k in range(n)]
    views, hist, n_slots = make(n, lens)
    check_full(cap, views, hist, n_slots)


def test_zero_records(cap):
    for direct in (False, True):
        got, guard, off, st = run(cap, np.zeros(0, dtype=N.FLOW_VIEW_DTYPE), text_cap=32, direct=direct)
        assert off.tolist() == [0] and set(st.values()) == {0} and (got == FILL).all() and (guard == FILL).all()


def _step_bytes(views):
    """Bytes of the lines of `views` without their histories."""
    return len(zeekref.expected_text(views, {})[0])


@pytest.mark.parametrize("spread", [False, True], ids=["one-history", "spread"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_a_step_at_the_staging_budget(cap, delta, spread):
    """The first step's 256 lines total FB_ZEEK_STAGE_BYTES + delta: the padding is one long history (copied by
    the wave) or many short ones; a second, partial step follows."""
    n = STEP + 40
    plain, _, _ = make(n, v4=True)
    pad = STAGE + delta - _step_bytes(plain[:STEP])
    assert pad > 4000
    lens = np.zeros(n, dtype=np.int64)
    if spread:
        lens[:STEP] = pad // STEP
        lens[:pad % STEP] += 1
        assert 0 < lens[:STEP].max() < COOP
    else:
        lens[7] = pad
    lens[STEP + 3] = 70
    views, hist, n_slots = make(n, lens, v4=True)
    off, _ = check_full(cap, views, hist, n_slots)
    assert int(off[STEP]) == STAGE + delta


@pytest.mark.parametrize("long", [1500, 5000], ids=["staged", "over-budget"])
def test_long_histories_first_and_last_in_a_step(cap, long):
    n = 2 * STEP + 10
    lens = np.array([(k * 3) % 11 for k in range(n)], dtype=np.int64)
    lens[[0, STEP - 1, STEP, 2 * STEP - 1, 2 * STEP, n - 1]] = [long, long, long + 1, COOP, COOP - 1, long]
    views, hist, n_slots = make(n, lens, v4=True)
    off, _ = check_full(cap, views, hist, n_slots)
    assert (int(off[STEP]) <= STAGE) == (long == 1500)


def test_every_alignment_of_a_steps_range(cap):
    """The second step's range starts at every residue mod 16 (a first record of growing length in front), and
    the text buffer itself starts at every residue."""
    n = STEP + 70
    seen = set()
    plain, _, _ = make(n)
    base = zeekref.expected_lines(plain, {})
    for j in range(16):
        lens = np.zeros(n, dtype=np.int64)
        lens[0] = j
        views, hist, n_slots = make(n, lens)
        lines = list(base)
        if j:
            f = lines[0].split("\t")
            f[15] = hist[int(views["rec"]["slot"][0])]
            lines[0] = "\t".join(f)
        text = "".join(l + "\n" for l in lines).encode("ascii")
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(l) + 1 for l in lines])
        got_off, _ = check_full(cap, views, hist, n_slots, want=(text, off), shift=(5 * j + 3) % 16)
        seen.add(int(got_off[STEP]) % 16)
    assert seen == set(range(16))


# ---- 3. capacity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [False, True], ids=["staged", "direct"])
def test_text_cap_bounds_what_is_written(cap, direct):
    n = STEP + 44
    views, hist, n_slots = make(n, [(k * 7) % 19 for k in range(n)], v4=True)   # (a first step under the budget)
    text, off = zeekref.expected_text(views, hist)
    assert off[STEP] <= STAGE
    off = off.tolist()
    caps = [(0, 0)]
    for k in (1, 100, STEP - 1, STEP, STEP + 1, n):
        caps += [(off[k] - 1, k - 1), (off[k], k)]
    caps.append((off[n] + 100, n))
    for text_cap, written in caps:
        got, guard, goff, st = run(cap, views, hist, n_slots, text_cap=text_cap, direct=direct, shift=text_cap % 16)
        assert (guard == FILL).all(), text_cap
        assert goff.tolist() == off                                  # complete whatever fits
        assert st["lines"] == n and st["bytes"] == len(text) and st["lines_written"] == written, (text_cap, st)
        assert got[:off[written]].tobytes() == text[:off[written]]
        assert (got[off[written]:] == FILL).all()                    # a line that does not fit is not begun


# ---- 4. refusals ---------------------------------------------------------------------------------------------
def test_refusals(cap):
    lib = N.gpu_lib()
    views, hist, n_slots = make(4, [1, 2, 3, 4])
    d_v = N.DeviceBuffer(5 * 256).upload(views)
    d_o, d_s, d_t = N.DeviceBuffer(64), N.DeviceBuffer(64), N.DeviceBuffer(4096)
    args = lambda c, v=d_v.ptr, h=None, ho=None, t=d_t.ptr, o=d_o.ptr, s=d_s.ptr: (  # noqa: E731
        c, v, 4, h, ho, n_slots, t, 4096, o, s, None)
    assert lib.fb_format_zeek_dev(*args(cap.ctx)) == N.FB_OK
    N.check(lib.fb_stream_sync(None))
    assert lib.fb_format_zeek_dev(*args(None)) == N.FB_ERR_INVAL
    assert lib.fb_format_zeek_dev(*args(cap.ctx, v=None)) == N.FB_ERR_INVAL
    assert lib.fb_format_zeek_dev(*args(cap.ctx, o=None)) == N.FB_ERR_INVAL
    assert lib.fb_format_zeek_dev(*args(cap.ctx, s=None)) == N.FB_ERR_INVAL
    assert lib.fb_format_zeek_dev(*args(cap.ctx, t=None)) == N.FB_ERR_INVAL
    assert lib.fb_format_zeek_dev(*args(cap.ctx, h=d_t.ptr)) == N.FB_ERR_INVAL          # a blob without offsets
    assert lib.fb_format_zeek_dev(*args(cap.ctx, v=C.c_void_p(d_v.ptr.value + 8))) == N.FB_ERR_INVAL
    untimed = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 10)
    try:
        assert lib.fb_format_zeek_dev(*args(untimed.ctx)) == N.FB_ERR_INVAL
        assert lib.fb_debug_set(untimed.ctx, N.FB_DEBUG_ZEEK_DIRECT, 1) == N.FB_OK
        assert lib.fb_debug_set(untimed.ctx, N.FB_DEBUG_ZEEK_DIRECT + 1, 1) == N.FB_ERR_INVAL
    finally:
        untimed.close()


# ---- 5. end to end -------------------------------------------------------------------------------------------
FLAGS = (fg.SYN, fg.SYN | fg.ACK, fg.ACK, fg.PSH | fg.ACK, fg.FIN | fg.ACK, fg.RST)


def _flow_frames(k, first, count):
    """`count` frames of flow k, its flag cycle continued from packet `first`; every fourth flow is UDP, every
    fifth IPv6; odd packets travel the other way, handshake packets the way their flags say."""
    v6 = k % 5 == 0
    a = "2001:db8::%x" % (k + 1) if v6 else "10.%d.%d.%d" % (k >> 16 & 255, k >> 8 & 255, k & 255)
    b = "2001:db8:1::1" if v6 else "93.184.216.34"
    out = []
    for j in range(first, first + count):
        flags = FLAGS[(k + j) % len(FLAGS)]
        # (a SYN names its sender the originator, a SYN-ACK its receiver: keep both on the client's side)
        fwd = j % 2 == 0 if k % 4 == 3 or not flags & fg.SYN else flags == fg.SYN
        src, sp, dst, dp = (a, 40000 + k % 7, b, 443) if fwd else (b, 443, a, 40000 + k % 7)
        if k % 4 == 3:
            out.append(fg.udp_frame(src, sp, dst, dp, 20 + j))
        else:
            out.append(fg.tcp_frame(src, sp, dst, dp, flags, 10 * (j % 3)))
    return out


def _batch(flows, first, t0):
    frames = [f for k in flows for f in _flow_frames(k, first, 2 + k % 3)]
    buf, offs = fg.pack(frames)
    return buf, offs, t0 + np.arange(len(frames), dtype=np.uint64) * 1237


def _same_log(cap):
    log = cap.export_zeek()
    want = format_sessions_zeek(cap.get_sessions())[1:]
    assert sorted(log.lines()) == sorted(want)
    assert len(log) == len(want) == log.stats["lines"] == log.stats["lines_written"]
    assert log.line_off[-1] == len(log.text) == log.stats["bytes"] and log.stats["ts_inexact"] == 0
    return log


def test_capture_end_to_end(tmp_path):
    day = 86400 * S
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=512, timed=True, track_history=True)
    try:
        buf, offs, ts = _batch(range(300), 0, T0)
        assert len(ts) > 800
        cap.process_frames(buf, offs, ts=ts)
        assert cap.table_info()["capacity"] == 512
        first = cap.get_sessions_zeek(now_ns=T0 + 10 * S)              # a full fetch: moves this getter's timestamp
        assert len(first) == 300 and cap._zeek_fetch_ts == T0 + 10 * S and set(cap._fetch_ts.values()) == {0}
        buf, offs, ts = _batch(range(150, 700), 2, T0 + 2 * day)       # 150 known flows go on, 400 new ones
        assert len(ts) > 1500
        cap.process_frames(buf, offs, ts=ts)
        assert cap.table_info()["capacity"] > 512 and cap.flow_count() == 700
        log = _same_log(cap)                                           # after the growth
        assert any(l.split("\t")[15] for l in log.lines()) and any(not l.split("\t")[15] for l in log.lines())
        assert {l.split("\t")[6] for l in log.lines()} == {"tcp", "udp"}
        # incremental: exactly the flows the second batch touched, and get_sessions' state is left alone
        inc = cap.get_sessions_zeek(incremental=True)
        touched = [i for i in cap.get_sessions() if i.stats.last_activity_ns > T0 + 10 * S]
        assert len(touched) == 550 and sorted(inc.lines()) == sorted(format_sessions_zeek(touched)[1:])
        assert cap._zeek_fetch_ts == T0 + 10 * S and set(cap._fetch_ts.values()) == {0}
        cap.reset_fetch_timestamps()
        assert cap._zeek_fetch_ts == 0 and len(cap.get_sessions_zeek(incremental=True)) == 700
        # the file form
        p = tmp_path / "conn.log"
        log.write(str(p))
        assert p.read_text().split("\n")[:-1] == [format_sessions_zeek([])[0]] + log.lines()
        # an aging purge: the flows only the first batch saw are a day past retention
        ag = cap.update_sessions_status(T0 + 2 * day + 100 * S)
        assert ag["purged"] == 150 and cap.flow_count() == 550
        _same_log(cap)
        # the uid does not depend on the slot: the survivors kept theirs through the purge's moves
        uids = {l.split("\t")[1] for l in log.lines()}
        assert {l.split("\t")[1] for l in cap.export_zeek().lines()} < uids
    finally:
        cap.close()


def test_capture_without_histories_and_untimed():
    buf, offs, ts = _batch(range(40), 0, T0)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 10, timed=True)
    try:
        cap.process_frames(buf, offs, ts=ts)
        log = _same_log(cap)                                           # (get_sessions has no histories either)
        assert len(log) == 40 and all(l.split("\t")[15] == "" for l in log.lines())
        assert log.stats["hist_mismatch"] == 0
    finally:
        cap.close()
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 10)
    try:
        cap.process_frames(buf, offs)
        with pytest.raises(N.FbError) as e:
            cap.export_zeek()
        assert e.value.code == N.FB_ERR_INVAL
    finally:
        cap.close()


# ---- 6. unchanged behaviour ----------------------------------------------------------------------------------
def test_session_info_is_what_it_was():
    """The uid property changes neither SessionInfo equality nor views_to_sessions' output: one small table
    against flows_to_sessions over the separate exports."""
    buf, offs, ts = _batch(range(60), 0, T0)
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 10, timed=True, track_history=True)
    try:
        cap.process_frames(buf, offs, ts=ts)
        got = views_to_sessions(cap.export_view(), cap.histories, whitelist=False, blacklist=False)
        want = joinref.sessions(cap, "sessions")
        assert len(got) == 60 and got == want and cap.get_sessions() == want
        joinref.assert_same(got, want)
        assert "uid" not in got[0].__dict__ and len({i.uid for i in got}) == 60
    finally:
        cap.close()
