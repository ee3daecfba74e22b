"""The frame decode (process_frame, fb_parse.hip) on every parse instance, against the C oracle, bit
for bit, on the enumerated corpora of tests/framespace.py: (a) every cut of 42 header shapes at every
start alignment, the bytes behind each caplen being the valid continuation of its headers; (b) every
length field swept around the sizes that matter, the protocol byte and the EtherType; (c) one-frame
batches whose frame ends at frames_bytes with its continuation in memory right behind.  What the
decode owes them: a field is used only when pnet's length rules put it inside caplen, the aligned
loads at (o + 10) & ~3 and their realignment by (o + 10) & 3 are right for every o, the dependent load
for IPv4 options likewise, and no load's range check against frames_bytes loses a byte in range or
lets one past it in.  tests/test_framespace_oracle.py pins the reference on the same corpora.

  instance                          entry point                                      filter
  dense                             fb_parse_classify_dev                            All, GlobalOnly, LocalOnly
  dense, look-back fallback forced  the same after fb_debug_set(FB_DEBUG_DENSE_      All
                                    STEAL_POLLS, 0): the count-only re-classification
  plain segmented                   fb_parse_classify_seg_dev                        All, GlobalOnly, LocalOnly
  several batches, one launch       fb_parse_classify_seg_batches_dev (MULTI): five   All
                                    batches of unequal size, each with a frame
                                    buffer of its own (the alignments shift)
  resident queue                    fb_seg_queue_*, depth 1 and 4, twice round        GlobalOnly
  fused parse + upsert (kPartOut)   fb_process_seg_dev / fb_process_seg_async_dev,    All
                                    session records on and off; the table too
  ingest ring                       fb_ring_push_block, batches of 1,000 frames       All
                                    (repacked: the alignments change again)

(a) and (b) go through all of them, (a) with both IPv4 addresses on the LAN through the first and the
third as well (LocalOnly then keeps sessions); IPv6 LAN prefixes and own IPs are configured, so the
classifier's table lookups are live.  (c) goes through fb_parse_classify_seg_batches_dev (32 cases a
launch, each descriptor with its own frames_bytes, offsets and outputs), fb_parse_classify_seg_dev
and fb_parse_classify_dev (one call per case, buffers allocated once, results down once per path),
and again with d_frames 1, 2 and 3 bytes off the allocation's alignment: the kernels address the
frames through a raw buffer resource whose base is d_frames itself, every offset -- the "dword-aligned"
(o + 10) & ~3 included -- is relative to that base and so is the realignment shift, and the range
check compares offsets with frames_bytes, never addresses; a misaligned base only makes the loads
unaligned in memory, which the decode already relies on for IPv4 options.  So d_frames needs no
alignment, and the tests pin that.

Compared, with no tolerance: records as bytes, DNS side records, classes, segment words, every stats
field with error == 0, and the output bytes outside the records left untouched."""
import ctypes as C

import numpy as np
import pytest

import framespace as fsp
from flodbadd_amd import _native as N
from flodbadd_amd.capture import FlodbaddGpuCapture, IngestRing, lan_v6_table, own_ip_table
from flodbadd_amd.sessions import SessionFilter
from oracle import coracle
from test_gpu_dense import _Dense
from test_gpu_flagspace import _check_tables
from test_gpu_fuzz_paths import _check_fused, _fused
from test_gpu_parity import rows_sorted
from test_gpu_queue import _Batch, _Queue, _verify
from test_gpu_ring import _oracle_batches
from test_gpu_segmented import _check, _run_batches

pytestmark = pytest.mark.gpu

FILTERS = [SessionFilter.All, SessionFilter.GlobalOnly, SessionFilter.LocalOnly]
STAT_KEYS = [k for k in N.STATS_FIELDS if not k.startswith("reserved")]
SESSION, DNS, DROP, FILTERED = 0, 1, 2, 3
CFG_KW = dict(lan_v6=lan_v6_table(fsp.LAN), own_ips=own_ip_table(fsp.OWN))
# the batches of the one-launch test, in frames: one shorter than 64, one no multiple of 64, all unequal
SPLITS = {"cuts": [0, 37, 1001, 7784, 20001, 38328], "fields": [0, 37, 1000, 3333, 7000, 9378]}


def _capture(flt=SessionFilter.All, **kw):
    return FlodbaddGpuCapture(0, session_filter=flt, lan_v6=fsp.LAN, own_ips=fsp.OWN, **kw)


@pytest.fixture(scope="module")
def corpus():
    """name -> (frames, offsets), read-only: (a), (b), and (a) with both IPv4 addresses on the LAN."""
    c = {"cuts": fsp.cuts(fsp.shapes())[:2], "fields": fsp.fields()[:2], "cuts_lan": fsp.cuts(fsp.shapes(lan_v4=True))[:2]}
    for fr, of in c.values():
        fr.setflags(write=False)
        of.setflags(write=False)
    for k, bounds in SPLITS.items():
        assert bounds[-1] == len(c[k][1]) - 1
    return c


def _dense_check(cap, frames, offs, flt, reps=1):
    b = _Dense(frames, offs, flt=int(flt))
    b.ref = coracle.parse_classify(fsp.cfg(flt), frames, offs)  # (under the LAN prefixes and own IPs)
    for _ in range(reps):
        b.run(cap)
        b.check()
    return b.ref


# ---- (a) and (b): dense ----------------------------------------------------------------------------
@pytest.mark.parametrize("flt", FILTERS, ids=lambda f: f.name)
@pytest.mark.parametrize("name", ["cuts", "fields", "cuts_lan"])
def test_framespace_dense(corpus, name, flt):
    cap = _capture(flt, flow_capacity=0)
    try:
        cls = _dense_check(cap, *corpus[name], flt)[2]
    finally:
        cap.close()
    seen = set(cls.tolist())
    if name == "cuts_lan":  # each real filter keeps some sessions and filters others
        assert seen == ({SESSION, DNS, DROP} if flt == SessionFilter.All else {SESSION, DNS, DROP, FILTERED})
    else:
        assert {DNS, DROP} <= seen


@pytest.mark.parametrize("name", ["cuts", "fields"])
def test_framespace_dense_lookback_fallback_forced(corpus, name):
    """FB_DEBUG_DENSE_STEAL_POLLS = 0: a look-back that meets an unpublished predecessor classifies
    that tile's frames itself, count-only -- the same decode, a second time, into the same sums."""
    cap = _capture(flow_capacity=0)
    N.check(N.gpu_lib().fb_debug_set(cap.ctx, N.FB_DEBUG_DENSE_STEAL_POLLS, 0))
    try:
        _dense_check(cap, *corpus[name], SessionFilter.All, reps=3)
    finally:
        cap.close()


# ---- (a) and (b): plain segmented, and several batches in one launch ---------------------------------
@pytest.mark.parametrize("flt", FILTERS, ids=lambda f: f.name)
@pytest.mark.parametrize("name", ["cuts", "fields", "cuts_lan"])
def test_framespace_seg(corpus, name, flt):
    cap = _capture(flt, flow_capacity=0)
    try:
        _check(cap, *corpus[name], int(flt), **CFG_KW)
    finally:
        cap.close()


def _split(frames, offs, bounds):
    """The corpus cut at the frame indices `bounds`, every batch with a frame buffer of its own."""
    return [(np.ascontiguousarray(frames[offs[a]: offs[b]]), (offs[a: b + 1] - offs[a]).astype(np.uint32))
            for a, b in zip(bounds[:-1], bounds[1:])]


@pytest.mark.parametrize("name", ["cuts", "fields"])
def test_framespace_seg_batches_one_launch(corpus, name):
    frames, offs = corpus[name]
    bounds = SPLITS[name]
    sizes = np.diff(bounds)
    assert len(sizes) >= 4 and len(set(sizes.tolist())) == len(sizes) and sizes.min() < 64 and (sizes % 64 != 0).sum() >= 2
    if name == "cuts":  # the batches start at other alignments than the corpus gave their frames
        assert {int(offs[b]) % 4 for b in bounds[:-1]} == {0, 1, 2, 3}
    batches = _split(frames, offs, bounds)
    cap = _capture(flow_capacity=0)
    try:
        for (fr, of), res in zip(batches, _run_batches(cap, batches)):
            _check(cap, fr, of, 2, res=res, **CFG_KW)
    finally:
        cap.close()


# ---- (a) and (b): the resident queue -------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 4])
def test_framespace_queue(corpus, depth):
    """Both corpora through k_parse_seg_queue, each submitted twice round the ring."""
    flt = SessionFilter.GlobalOnly
    cap = _capture(flt, flow_capacity=0)
    batches = [_Batch(*corpus["cuts"]), _Batch(*corpus["fields"], with_cls=False), _Batch(*corpus["cuts_lan"])]
    cap.parse_classify(*corpus["fields"])  # (the configuration is on the device before the queue captures it)
    q = _Queue(cap, depth=depth)
    try:
        for rnd in range(2):
            for b in batches:
                b.reset()
            tickets = [q.submit(b) for b in batches]
            for t in tickets:
                q.wait(t)
            for b in batches:
                _verify(b, flt, cfg=fsp.cfg(flt))
                assert int(b.result()[3][0]["error"]) == 0
    finally:
        q.close()
        cap.close()


# ---- (a) and (b): fused parse + upsert, records on and off -------------------------------------------
@pytest.mark.parametrize("records", [True, False], ids=["records", "table_only"])
@pytest.mark.parametrize("asyn", [False, True], ids=["sync", "async"])
def test_framespace_fused_parse_and_upsert(corpus, asyn, records):
    cap = _capture(flow_capacity=1 << 15, track_history=True)
    flows = coracle.Flows()
    try:
        if not records:
            N.check(N.gpu_lib().fb_set_session_records(cap.ctx, 0))
        for k in ("cuts", "fields", "cuts"):
            ref = coracle.parse_classify(fsp.cfg(2), *corpus[k])
            r_st = ref[3].copy()
            flows.update(ref[0], r_st)
            _check_fused(_fused(cap, *corpus[k], asyn=asyn), ref, r_st, records, k)
        gf = _check_tables(cap, flows, "fused")
        assert len(gf) > 30 and (gf["hist_len"] > 1).any()
    finally:
        cap.close()


# ---- (a) and (b): the ingest ring ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cuts", "fields"])
def test_framespace_ring(gpu_capture, corpus, name):
    """fb_ring_push_block, cut into batches of 1,000 frames: totals, DNS payloads and the table as in
    test_gpu_fuzz_paths.test_fuzz_ring."""
    frames, offs = corpus[name]
    n, per = len(offs) - 1, 1000
    gpu_capture.clear_all_sessions()
    ring = IngestRing(gpu_capture, slots=3, max_packets=per, max_bytes=4 << 20)
    try:
        ring.push_block(frames, offs)
        ring.sync()
        tot, nb, nf = ring.stats()
        dns = ring.poll_dns()
    finally:
        ring.close()
    flows = coracle.Flows()
    r_tot, r_dns = _oracle_batches(frames, offs, per, flows)
    assert nf == n and nb == (n + per - 1) // per
    for k in STAT_KEYS:
        assert tot[k] == int(r_tot[0][k]), k
    assert [(s, p, pl) for s, p, _, pl in dns] == r_dns and len(r_dns) == {"cuts": 160, "fields": 1737}[name]
    assert rows_sorted(gpu_capture.export_flows()) == rows_sorted(flows.export_sorted())
    gpu_capture.clear_all_sessions()


# ---- (c): the frame ends at frames_bytes, its continuation right behind ------------------------------
OUT_STRIDE, DNS_STRIDE, CLS_STRIDE = 64, 32, 8  # the dense path's per-case output slots (records 56 B, DNS 16 B)


class _Ends:
    """Corpus (c) on the device: the physical buffer `mem` (uploaded once), one offsets pair per case
    and per-case output slots, all allocated once; a case is (where d_frames points in `mem`, a, c).
    The three run_* methods launch every case and bring the results down once."""

    def __init__(self, mem, cases):
        self.mem, self.cases, n = mem, cases, len(cases)
        self.d_mem = N.DeviceBuffer(len(mem)).upload(mem)
        offs = np.array([[a, a + c] for _, a, c in cases], dtype=np.uint32)
        self.d_off = N.DeviceBuffer(offs.nbytes).upload(offs)
        self.d_seg_out, self.d_seg = N.DeviceBuffer(n * N.SEG_BYTES), N.DeviceBuffer(n * 4)
        self.d_out, self.d_dns = N.DeviceBuffer(n * OUT_STRIDE), N.DeviceBuffer(n * DNS_STRIDE)
        self.d_cls, self.d_st = N.DeviceBuffer(n * CLS_STRIDE), N.DeviceBuffer(n * N.STATS_DTYPE.itemsize)
        # the oracle sees the batch's bytes only: mem[at : at + a + c]
        cfg = fsp.cfg(2)
        self.r_cls = np.zeros(n, dtype=np.uint8)
        self.r_rec, self.r_dns = np.zeros((n, 56), dtype=np.uint8), np.zeros((n, 16), dtype=np.uint8)
        self.r_st = np.zeros(n, dtype=N.STATS_DTYPE)
        for i, (at, a, c) in enumerate(cases):
            assert at + a + c + fsp.END_SLACK <= len(mem)  # the allocation reaches 80 B past every frames_bytes
            out, dns, cls, st = coracle.parse_classify(cfg, mem[at: at + a + c], offs[i])
            self.r_cls[i], self.r_st[i] = cls[0], st[0]
            if len(out):
                self.r_rec[i] = out.view(np.uint8)
            if len(dns):
                self.r_dns[i] = dns.view(np.uint8)
        assert set(self.r_cls.tolist()) == {SESSION, DNS, DROP}

    def _p(self, buf, off):
        return C.c_void_p(buf.ptr.value + off)

    def _reset(self):
        self.d_seg_out.memset(0xA5)
        self.d_out.memset(0x5A)
        self.d_dns.memset(0x5A)
        for b in (self.d_seg, self.d_cls, self.d_st):
            b.memset(0xEE)

    def _down(self, seg):
        n = len(self.cases)
        N.check(N.gpu_lib().fb_stream_sync(None))
        cls = self.d_cls.download(np.zeros(n * CLS_STRIDE, dtype=np.uint8))[::CLS_STRIDE]
        st = self.d_st.download(np.zeros(n, dtype=N.STATS_DTYPE))
        if seg:
            return (cls, st, self.d_seg.download(np.zeros(n, dtype=np.uint32)),
                    self.d_seg_out.download(np.zeros(n * N.SEG_BYTES, dtype=np.uint8)).reshape(n, N.SEG_BYTES))
        return (cls, st, self.d_out.download(np.zeros(n * OUT_STRIDE, dtype=np.uint8)).reshape(n, OUT_STRIDE),
                self.d_dns.download(np.zeros(n * DNS_STRIDE, dtype=np.uint8)).reshape(n, DNS_STRIDE))

    def run_batches(self, cap, per=32):
        """fb_parse_classify_seg_batches_dev, `per` cases a launch, a descriptor per case."""
        self._reset()
        lib, sz = N.gpu_lib(), N.STATS_DTYPE.itemsize
        for i0 in range(0, len(self.cases), per):
            part = self.cases[i0: i0 + per]
            desc = np.zeros(len(part), dtype=N.SEG_BATCH_DTYPE)
            for j, (at, a, c) in enumerate(part):
                i = i0 + j
                desc[j] = (self.d_mem.ptr.value + at, a + c, self.d_off.ptr.value + 8 * i, 1, 0,
                           self.d_seg_out.ptr.value + i * N.SEG_BYTES, self.d_seg.ptr.value + 4 * i,
                           self.d_cls.ptr.value + CLS_STRIDE * i, self.d_st.ptr.value + sz * i)
            N.check(lib.fb_parse_classify_seg_batches_dev(cap.ctx, N.ptr(desc), len(part), None))
        return self._down(seg=True)

    def run_seg(self, cap):
        """fb_parse_classify_seg_dev, one call per case."""
        self._reset()
        lib, sz = N.gpu_lib(), N.STATS_DTYPE.itemsize
        for i, (at, a, c) in enumerate(self.cases):
            N.check(lib.fb_parse_classify_seg_dev(cap.ctx, self._p(self.d_mem, at), a + c, self._p(self.d_off, 8 * i), 1,
                                                  self._p(self.d_seg_out, i * N.SEG_BYTES), self._p(self.d_seg, 4 * i),
                                                  self._p(self.d_cls, CLS_STRIDE * i), self._p(self.d_st, sz * i), None))
        return self._down(seg=True)

    def run_dense(self, cap):
        """fb_parse_classify_dev, one call per case."""
        self._reset()
        lib, sz = N.gpu_lib(), N.STATS_DTYPE.itemsize
        for i, (at, a, c) in enumerate(self.cases):
            N.check(lib.fb_parse_classify_dev(cap.ctx, self._p(self.d_mem, at), a + c, self._p(self.d_off, 8 * i), 1,
                                              self._p(self.d_out, OUT_STRIDE * i), self._p(self.d_dns, DNS_STRIDE * i),
                                              self._p(self.d_cls, CLS_STRIDE * i), self._p(self.d_st, sz * i), None))
        return self._down(seg=False)

    def _first_bad(self, bad):
        i = int(np.flatnonzero(bad)[0])
        return "%d of %d cases differ, first %d: d_frames = mem + %d, a = %d, c = %d, oracle class %d" % (
            (int(bad.sum()), len(self.cases), i) + tuple(self.cases[i]) + (int(self.r_cls[i]),))

    def _check_common(self, cls, st):
        assert not (cls != self.r_cls).any(), "classes: " + self._first_bad(cls != self.r_cls)
        for k in STAT_KEYS:
            want = np.zeros(len(st), dtype=np.uint64) if k == "error" else self.r_st[k]
            assert not (st[k] != want).any(), "stats.%s: %s" % (k, self._first_bad(st[k] != want))

    def check_seg(self, res):
        cls, st, seg, raw = res
        self._check_common(cls, st)
        want_seg = ((self.r_cls == SESSION).astype(np.uint32) | ((self.r_cls == DNS).astype(np.uint32) << 16))
        assert not (seg != want_seg).any(), "segment words: " + self._first_bad(seg != want_seg)
        want = np.full(raw.shape, 0xA5, dtype=np.uint8)  # a record at the segment's head or a DNS record at its tail
        s, d = self.r_cls == SESSION, self.r_cls == DNS
        want[s, :56] = self.r_rec[s]
        want[d, N.SEG_BYTES - 16:] = self.r_dns[d]
        bad = (raw != want).any(axis=1)
        assert not bad.any(), "segment bytes: " + self._first_bad(bad)

    def check_dense(self, res):
        cls, st, out, dns = res
        self._check_common(cls, st)
        w_out, w_dns = np.full(out.shape, 0x5A, dtype=np.uint8), np.full(dns.shape, 0x5A, dtype=np.uint8)
        s, d = self.r_cls == SESSION, self.r_cls == DNS
        w_out[s, :56] = self.r_rec[s]
        w_dns[d, :16] = self.r_dns[d]
        bad = (out != w_out).any(axis=1) | (dns != w_dns).any(axis=1)
        assert not bad.any(), "records: " + self._first_bad(bad)


@pytest.fixture(scope="module")
def ends():
    mem, cases = fsp.buffer_ends(fsp.shapes())
    assert len(cases) == 3184
    return _Ends(mem, [(base, a, c) for _, a, c, base in cases])


@pytest.fixture(scope="module")
def ends_misaligned():
    """Four shapes of (c) (IPv4 / TCP, IHL 15, IPv6 / TCP, a DNS divert) with d_frames = a 256-B
    aligned address + k, k = 1..3, and pad a = 0: the same batches as the a = 0 cases, at a base
    pointer of every other alignment."""
    sh = fsp.shapes()
    mem, cases = [], []
    for name in ("v4_ihl5_tcp5", "v4_ihl15_tcp5", "v6_tcp5", "dns_v4_tcp_dst"):
        for k in (1, 2, 3):
            at = len(mem) * fsp.END_REGION + k
            mem.append((b"\xff" * k + sh[name]).ljust(fsp.END_REGION, b"\xff"))
            cases += [(at, 0, c) for c in range(len(sh[name]) + 1)]
    return _Ends(np.frombuffer(b"".join(mem), dtype=np.uint8).copy(), cases)


@pytest.mark.parametrize("path", ["seg_batches", "seg", "dense"])
@pytest.mark.parametrize("which", ["ends", "ends_misaligned"])
def test_framespace_buffer_ends(request, which, path):
    """Every case of (c) (3,184; and 906 at misaligned base pointers), none left out: the class, the
    record or DNS record, the segment word and the stats of each equal the oracle's for the batch's own
    bytes, and nothing else in its output slot is written."""
    e = request.getfixturevalue(which)
    cap = _capture(flow_capacity=0)
    try:
        if path == "dense":
            e.check_dense(e.run_dense(cap))
        else:
            e.check_seg(e.run_batches(cap) if path == "seg_batches" else e.run_seg(cap))
    finally:
        cap.close()
