"""Run-space corpora for the history ordering (test helper, no tests): small, deterministic batches in
which every (bucketing chunk, partition) group -- a "run" of fb_hist.hip -- has a chosen length, so
each of the launcher's data-dependent paths is reached by construction and not by sampling.

Which path a partition takes depends only on how many records each (chunk, partition) group holds and
on whether K1 listed the group for k_flow_combine.  fb_flow_update_seg_dev takes a segmented buffer
that need not come from a parse: d_seg[s] = n_session | n_dns << 16, records at the front of each
64-slot segment.  A record's slot fixes its chunk (slot // kFlowChunk) and its record-in-chunk, so a
batch can be hundreds of chunks long and hold a few thousand records (`place`).

Flows.  Flow f is 10.(f>>16).(f>>8).(f) talking to flagseq.SERVER on flagseq.ONE_SVC (both directions
share one key; all 13 history characters are reachable).  `pool(parts)` buckets the first flow ids by
the partition of the key the oracle's parse gives them (keyspace.flow_hash / part_of): no hash inversion.
A flow id with the UDP bit is the UDP flow of the same addresses and ports: another key, and records
without a history character (code 0: the ~0 keys of wave_sort_run, the bitmap paths' skipped entries).

Strings.  TCP packet j of flow f (counted over all update calls, in slot order) carries the character
CYCLE13[(f + j * step(f)) % 13], step(f) = 1 + f % 12: consecutive characters of a flow always differ
and two characters of a flow are equal only 13 packets apart, so any transposition inside a flow, and
any character filed under a neighbouring flow, changes a string.  `closed_form` restates the strings.

`census` restates the dispatch conditions of fb_hist.hip (and K1's hot rule) -- never the ordering --
and names, per partition, the kernel that handles it and, per run, its class; the corpora's coverage is
asserted on it (tests/test_runspace_oracle.py) before anything runs on a GPU.  `CONSTANTS` are the
thresholds it uses; `source_constants` reads the same values out of the sources."""
import functools
import os
import re

import numpy as np

import flagseq as fs
import framegen as fg
import keyspace as ks

CONSTANTS = {
    "kFlowChunk": 20480, "kFlowSlots": 512, "kCombMin": 64, "kCombSlots": 256, "kHistCap": 4096, "kHistRuns": 512,
    "kRunSort": 16, "kWaveSortMax": 512, "kHistSplitEntries": 8192, "kHistBlockEntries": 4096, "kHistMaxBlocks": 128,
    "kHistBlockChunks": 4, "kHistListCap": 256,
}
CH, SLOTS, CAP = CONSTANTS["kFlowChunk"], CONSTANTS["kFlowSlots"], CONSTANTS["kHistCap"]
SEG = 64  # FB_SEG_FRAMES

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flodbadd_amd", "csrc")
_DEFINE, _CONST = r"^#define %s (\d+)\b", r"^constexpr uint32_t %s = (\w+);"
# constant -> (file, the macro whose default it is bound to; None: a literal constexpr)
_SOURCES = {
    "kFlowChunk": ("fb_internal.h", "FB_FLOW_CHUNK"), "kFlowSlots": ("fb_internal.h", "FB_FLOW_SLOTS"),
    "kCombMin": ("fb_flow.hip", "FB_COMB_MIN"), "kCombSlots": ("fb_flow.hip", "FB_COMB_SLOTS"),
    "kHistCap": ("fb_hist.hip", "FB_HIST_CAP"), "kHistSplitEntries": ("fb_hist.hip", "FB_HIST_SPLIT_ENTRIES"),
    "kHistBlockEntries": ("fb_hist.hip", "FB_HIST_BLOCK_ENTRIES"),
    "kHistRuns": ("fb_hist.hip", None), "kRunSort": ("fb_hist.hip", None), "kWaveSortMax": ("fb_hist.hip", None),
    "kHistMaxBlocks": ("fb_hist.hip", None), "kHistBlockChunks": ("fb_hist.hip", None), "kHistListCap": ("fb_hist.hip", None),
}


def source_constants(csrc=CSRC):
    """CONSTANTS as the sources under `csrc` state them: `constexpr uint32_t kX = <literal>;`, or
    `constexpr uint32_t kX = FB_X;` with `#define FB_X <literal>` (the build passes no -D for them)."""
    out, text = {}, {}
    for name, (fn, macro) in _SOURCES.items():
        if fn not in text:
            with open(os.path.join(csrc, fn)) as f:
                text[fn] = f.read()
        m = re.findall(_CONST % name, text[fn], flags=re.M)
        assert len(m) == 1, "%s: %d definitions of %s" % (fn, len(m), name)
        if macro is None:
            out[name] = int(m[0])
        else:
            assert m[0] == macro, (name, m[0])
            d = re.findall(_DEFINE % macro, text[fn], flags=re.M)
            assert len(d) == 1, "%s: %d defaults of %s" % (fn, len(d), macro)
            out[name] = int(d[0])
    return out


# ---- flows, characters ----------------------------------------------------------------------------
UDP = 1 << 31  # flow id bit: the UDP flow of the same addresses and ports
HIST_CHARS = "SsHhFfRr><Aa-"
# flagseq symbols of S s H h F f R r > < A a - (tests/test_runspace_oracle.py asserts them through the oracle)
CYCLE13 = np.array([fs.SYN, fs.REV | fs.SYN, fs.SYN | fs.ACK, fs.REV | fs.SYN | fs.ACK, fs.FIN | fs.ACK,
                    fs.REV | fs.FIN | fs.ACK, fs.RST, fs.REV | fs.RST, fs.PAY | fs.ACK, fs.REV | fs.PAY | fs.ACK,
                    fs.ACK, fs.REV | fs.ACK, 0], dtype=np.uint8)


def step(flow):
    return 1 + (np.asarray(flow, dtype=np.int64) & 0xFFFFFF) % 12


def char_index(flow, j):
    f = np.asarray(flow, dtype=np.int64) & 0xFFFFFF
    return (f + np.asarray(j, dtype=np.int64) * step(f)) % 13


_TEMPLATES = []


def frames(flow, sym):
    """One frame per item: flow (UDP bit: a UDP datagram, sym ignored) and flagseq symbol -> (frames u8,
    offsets u32[n + 1]).  numpy-patched framegen templates, as flagseq.frames."""
    if not _TEMPLATES:
        t = np.zeros((3, 60), dtype=np.uint8)
        for k, f in enumerate((fg.tcp_frame("10.0.0.0", fs.ONE_SVC[0], fs.SERVER, fs.ONE_SVC[1], 0, 0),
                               fg.tcp_frame("10.0.0.0", fs.ONE_SVC[0], fs.SERVER, fs.ONE_SVC[1], 0, 6),
                               fg.udp_frame("10.0.0.0", fs.ONE_SVC[0], fs.SERVER, fs.ONE_SVC[1], 0))):
            assert len(f) == (54, 60, 42)[k]
            t[k, :len(f)] = np.frombuffer(f, dtype=np.uint8)
        _TEMPLATES.append(t)
    flow = np.asarray(flow, dtype=np.int64)
    sym = np.asarray(sym, dtype=np.uint8)
    udp = (flow & UDP) != 0
    kind = np.where(udp, 2, ((sym & fs.PAY) != 0).astype(np.intp))
    rev = ((sym & fs.REV) != 0) & ~udp
    fr = _TEMPLATES[0][kind]
    fr[:, 27], fr[:, 28], fr[:, 29] = (flow >> 16) & 0xFF, (flow >> 8) & 0xFF, flow & 0xFF
    sw = fr[rev]
    sw[:, 26:30], sw[:, 30:34] = fr[rev, 30:34], fr[rev, 26:30]
    sw[:, 34:36], sw[:, 36:38] = fr[rev, 36:38], fr[rev, 34:36]
    fr[rev] = sw
    fr[~udp, 47] = sym[~udp] & 0x1F
    ln = np.array([54, 60, 42])[kind]
    offs = np.zeros(len(flow) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum(ln)
    return np.ascontiguousarray(fr[np.arange(60)[None, :] < ln[:, None]]), offs


def parse(flow, sym):
    """The oracle's fb_pkt_out records of frames(flow, sym): every frame yields one session record."""
    from oracle import coracle
    fr, of = frames(flow, sym)
    recs, dns, _, _ = coracle.parse_classify(coracle.make_cfg(2), fr, of)
    assert len(recs) == len(flow) and len(dns) == 0
    return recs


def keys_of(flows):
    """[n, 10] key words of flow ids."""
    return ks.words_of(parse(flows, np.full(len(flows), fs.SYN, dtype=np.uint8)))


@functools.lru_cache(maxsize=None)
def pool(parts, n=1 << 16):
    """(tcp, udp): per partition of a `parts`-partition table, the flow ids among the first n whose TCP
    key (and, with the UDP bit, whose UDP key) falls into it, ascending."""
    f = np.arange(n, dtype=np.int64)
    out = []
    for ids in (f, f | UDP):
        p = ks.part_of(ks.flow_hash(keys_of(ids)), parts)
        out.append([ids[p == q].tolist() for q in range(parts)])
    return tuple(out)


# ---- update calls ---------------------------------------------------------------------------------
class Call:
    """One update call: the oracle's records (pkt_index = the record slot), their strictly increasing
    record slots, the slot count of the batch (a multiple of 64), and per record its flow id and symbol."""

    def __init__(self, recs, slots, n_slots, flow, sym):
        self.recs, self.slots, self.n_slots, self.flow, self.sym = recs, slots, n_slots, flow, sym
        for a in (recs, slots, flow, sym):
            a.setflags(write=False)

    @property
    def keys(self):
        return ks.words_of(self.recs)

    @property
    def codes(self):
        """K1's history code: 0 for no character, else 1 + the FB_HIST_CHARS index."""
        has = (self.recs["meta"] & 1) != 0
        idx = np.array([HIST_CHARS.find(chr(c)) for c in range(256)])[self.recs["hist_char"]]
        assert (idx[has] >= 0).all()
        return np.where(has, idx + 1, 0)


def build(calls):
    """[(flow ids in slot order, slots, n_slots)] -> [Call]: packet j of a flow counts on over the calls."""
    seen, out = {}, []
    for flow, slots, n_slots in calls:
        flow, slots = np.asarray(flow, dtype=np.int64), np.asarray(slots, dtype=np.int64)
        assert len(flow) == len(slots) and n_slots % SEG == 0
        order = np.argsort(flow, kind="stable")
        fsrt = flow[order]
        first = np.r_[0, np.flatnonzero(np.diff(fsrt)) + 1]
        j = np.zeros(len(flow), dtype=np.int64)
        lens = np.diff(np.r_[first, len(flow)])
        base = np.array([seen.get(int(x), 0) for x in fsrt[first]], dtype=np.int64)
        j[order] = np.arange(len(flow)) - np.repeat(first, lens) + np.repeat(base, lens)
        for x, ln, b in zip(fsrt[first].tolist(), lens.tolist(), base.tolist()):
            seen[x] = b + ln
        sym = CYCLE13[char_index(flow, j)]
        recs = parse(flow, sym).copy()
        check_slots(slots, n_slots)
        recs["pkt_index"] = slots
        out.append(Call(recs, slots, int(n_slots), flow, sym))
    return out


def closed_form(calls):
    """{flow id: its history string over the calls} from CYCLE13 alone (UDP flows: "")."""
    n = {}
    for c in calls:
        f, k = np.unique(c.flow, return_counts=True)
        for x, y in zip(f.tolist(), k.tolist()):
            n[x] = n.get(x, 0) + y
    return {f: "" if f & UDP else "".join(HIST_CHARS[i] for i in char_index(f, np.arange(k))) for f, k in n.items()}


# ---- placement ------------------------------------------------------------------------------------
def check_slots(slots, n_slots):
    """The segmented layout packs a segment's records at its front: a slot list is strictly increasing,
    inside the batch, and fills every segment it uses from the segment's first slot."""
    s = np.asarray(slots, dtype=np.int64)
    assert n_slots % SEG == 0 and 0 < n_slots < (1 << 27)
    assert (np.diff(s) > 0).all() and (len(s) == 0 or (s[0] >= 0 and s[-1] < n_slots))
    seg, first = np.unique(s // SEG, return_index=True)
    cnt = np.diff(np.r_[first, len(s)])
    assert (s[first] % SEG == 0).all() and (s[first + cnt - 1] % SEG == cnt - 1).all(), \
        "a used segment must be filled from its first slot, without gaps"


def place(recs, slots, n_slots):
    """Records at chosen record slots -> (out bytes u8[n_slots * 56], d_seg words u32[n_slots / 64]) in the
    segmented layout (include/flodbadd_gpu.h); pkt_index = the slot; the other bytes stay zero."""
    from flodbadd_amd import _native as N
    check_slots(slots, n_slots)
    r = np.ascontiguousarray(recs, dtype=N.PKT_OUT_DTYPE).copy()
    r["pkt_index"] = slots
    out = np.zeros(n_slots, dtype=N.PKT_OUT_DTYPE)
    out[np.asarray(slots, dtype=np.int64)] = r
    seg = np.bincount(np.asarray(slots, dtype=np.int64) // SEG, minlength=n_slots // SEG).astype(np.uint32)
    return out.view(np.uint8), seg


def dense(recs):
    """The same records without gaps, for the dense entry points (pkt_index stays the placed slot)."""
    from flodbadd_amd import _native as N
    return np.ascontiguousarray(recs, dtype=N.PKT_OUT_DTYPE).copy()


# ---- the census -----------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def _wave_class(wl):
    # fb_hist.hip:228-230 / 672-674: sort_net<16> if wl > 8, <8> if wl > 4, <4> if wl > 1, else no network
    return "reg16" if wl > 8 else "reg8" if wl > 4 else "reg4" if wl > 1 else "single"


def _general(read, comb, c_lo, c_hi, K):
    """k_hist_general<false> over the chunks [c_lo, c_hi) of one partition (fb_hist.hip:745-770): chunk
    rounds of kHistRuns runs, in each batches of whole runs up to kHistCap entries, a longer run alone."""
    runs, batches, rounds = {}, [], 0
    for c0 in range(c_lo, c_hi, K["kHistRuns"]):  # :745
        rounds += 1
        nr = min(K["kHistRuns"], c_hi - c0)
        ln = [read.get(c0 + r, 0) for r in range(nr)]
        rp = np.r_[0, np.cumsum(ln)]
        r = 0
        while r < nr:
            if ln[r] > K["kHistCap"]:  # :754 long_run; :716 a combined run in entry windows
                runs[c0 + r] = ("long_combined" if comb.get(c0 + r) else "long_plain", ln[r])
                r += 1
                continue
            r1 = int(np.searchsorted(rp, rp[r] + K["kHistCap"], side="right")) - 1  # :759-765
            r1 = min(max(r1, r + 1), nr)
            if rp[r1] > rp[r]:
                batches.append((c0 + r, c0 + r1, int(rp[r1] - rp[r])))
            for w0 in range(r, r1, 64):  # run r0 + tid is thread tid's (:661): a wave holds 64 runs
                wl = max([ln[x] for x in range(w0, min(w0 + 64, r1))
                          if not comb.get(c0 + x) and ln[x] <= K["kRunSort"]] + [0])  # :669-671
                for x in range(w0, min(w0 + 64, r1)):
                    L = ln[x]
                    if L == 0:
                        continue
                    if comb.get(c0 + x):
                        cls = "combined"  # :653 e_sort is in record order already
                    elif L <= K["kRunSort"]:
                        cls = _wave_class(wl)
                    elif L <= K["kWaveSortMax"]:  # :664-665, :684-687
                        cls = "wave1" if L <= 64 else "wave2" if L <= 128 else "wave4" if L <= 256 else "wave8"
                    else:
                        cls = "bitmap"  # :689
                    runs[c0 + x] = (cls, L)
            r = r1
    return runs, batches, rounds


def census(slots, keys, codes, parts, n_slots, hot=True, overflow_ok=False, K=CONSTANTS):
    """The dispatch of one update call's history, restated from the conditions alone.

    slots / keys ([n, 10] key words) / codes (0: no character) per record, parts: the table's partitions,
    n_slots: the batch's record slots; hot=False: a timed context (flow_update sets p.hot = nullptr, no
    group is combined).  Returns {"chunks", "nblk", "partitions": {p: {...}}} with, per partition that
    holds records: "kernel" ("uniform", "general", or "idle": no characters, both kernels return at
    once), "blocks" (1: not split) and "block_chunks", "read" / "applied" entries, "rounds", "batches"
    [(first chunk, end chunk, entries)] and "runs" {chunk: (class, entries to read)}."""
    slots = np.asarray(slots, dtype=np.int64)
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 10)
    codes = np.asarray(codes)
    chunks = max(1, _ceil(n_slots, K["kFlowChunk"]))  # fb_capi.hip flow_update: chunks
    part = ks.part_of(ks.flow_hash(keys), parts)
    chunk = slots // K["kFlowChunk"]
    kid = np.unique(keys.view("V40").ravel(), return_inverse=True)[1]
    nblk = min(K["kHistMaxBlocks"], _ceil(chunks, K["kHistBlockChunks"]))  # fb_hist.hip:841-842
    out = {"chunks": chunks, "nblk": nblk, "partitions": {}}
    for p in np.unique(part).tolist():
        sel = part == p
        read, applied, comb, overflow = {}, {}, {}, set()
        for c in np.unique(chunk[sel]).tolist():
            g = sel & (chunk == c)
            m = int(g.sum())
            cnt_c = min(K["kFlowChunk"], n_slots - K["kFlowChunk"] * c)
            hot_min = max(K["kCombMin"], 4 * _ceil(cnt_c, parts))  # fb_flow.hip:277 (cnt: the chunk's slots)
            read[c] = applied[c] = m
            if hot and m >= hot_min:  # fb_flow.hip:284
                mult = np.bincount(kid[g])
                mult = mult[mult > 0]
                if not (mult >= 2).any():  # fb_flow.hip:959: no key met twice, the group stays plain
                    pass
                elif len(mult) > K["kCombSlots"]:  # keys past a full table stay plain entries (fb_flow.hip:803, 927):
                    if not overflow_ok:            # which keys those are is a race, so the applied entries are not known
                        raise ValueError("hot group (chunk %d, partition %d) holds %d distinct keys" % (c, p, len(mult)))
                    overflow.add(c)
                    comb[c], applied[c] = True, None
                else:
                    comb[c] = True
                    applied[c] = int((mult == 1).sum() + (mult >= 2).sum())  # :1068 cursor + n_comb
        info = {"read": sum(read.values()), "applied": None if overflow else sum(applied.values())}
        waves = [sum(read.get(c, 0) for c in range(w, w + 64)) for w in range(0, K["kHistRuns"], 64)]
        if not (codes[sel] != 0).any():  # fb_hist.hip:180, :420
            info.update(kernel="idle", blocks=1, block_chunks=[(0, chunks)], rounds=0, batches=[], runs={})
        elif (chunks <= K["kHistRuns"] and not comb and max(read.values()) <= K["kRunSort"] and
              info["applied"] <= K["kHistCap"] and max(waves) <= (K["kHistCap"] // K["kHistRuns"]) * 64):  # :191
            runs = {}
            for c, L in read.items():  # :225-230: the network is chosen by the wave's longest run
                runs[c] = (_wave_class(max(read.get(x, 0) for x in range(c - c % 64, c - c % 64 + 64))), L)
            info.update(kernel="uniform", blocks=1, block_chunks=[(0, chunks)], rounds=1, batches=[], runs=runs)
        else:
            nb = 1
            if nblk > 1 and info["read"] > K["kHistSplitEntries"]:  # :202 (the 256-entry list cap: not restated)
                nb = min(max(_ceil(info["read"], K["kHistBlockEntries"]), 2), nblk)  # :204, :781
            cbs = _ceil(chunks, nb)  # :423
            blocks = [(b * cbs, min(chunks, (b + 1) * cbs)) for b in range(nb) if b * cbs < chunks]  # :424-425
            runs, batches, rounds = {}, [], 0
            for lo, hi in blocks:
                r, b, k = _general(read, comb, lo, hi, K)
                runs.update(r)
                batches += b
                rounds += k
            for c in overflow:
                runs[c] = ("overflow", read[c])
            info.update(kernel="general", blocks=nb, block_chunks=blocks, rounds=rounds, batches=batches, runs=runs)
        out["partitions"][p] = info
    return out


def census_of(call, parts, **kw):
    return census(call.slots, call.keys, call.codes, parts, call.n_slots, **kw)


def classes(cen):
    return {cls for i in cen["partitions"].values() for cls, _ in i["runs"].values()}


def lengths(cen, cls=None, kernel=None):
    """The run lengths of a census (of one class / one kernel)."""
    return {L for i in cen["partitions"].values() if kernel in (None, i["kernel"])
            for k, L in i["runs"].values() if cls in (None, k)}


# ---- corpus construction --------------------------------------------------------------------------
def rr(flows, length, udp=(), every=5):
    """A run's flows in record order: round-robin over `flows`, every `every`-th record one of `udp`."""
    out = []
    for i in range(length):
        if udp and i % every == every - 1:
            out.append(udp[(i // every) % len(udp)])
        else:
            out.append(flows[(i - i // every if udp else i) % len(flows)])
    return out


def _weave(a, b):
    """b's items spread evenly between a's."""
    out, k = [], max(len(a) // max(len(b), 1), 1)
    for i, x in enumerate(a):
        out.append(x)
        if i % k == k - 1 and i // k < len(b):
            out.append(b[i // k])
    return out + list(b[len(a) // k:])


def merge(runs, forced=()):
    """Interleave the runs of one chunk evenly (record i of a run of n at (i + 1/2) / n of the chunk), then
    for each forced (position, run) -- negative positions from the end -- swap the nearest record of that
    run into the position.  Returns (flow per position, run index per position)."""
    frac = np.concatenate([(np.arange(len(r)) + 0.5) / max(len(r), 1) for r in runs]) if runs else np.zeros(0)
    rid = np.concatenate([np.full(len(r), k, dtype=np.int64) for k, r in enumerate(runs)]) if runs else np.zeros(0, np.int64)
    flow = np.concatenate([np.asarray(r, dtype=np.int64) for r in runs]) if runs else np.zeros(0, np.int64)
    order = np.lexsort((rid, frac))
    flow, rid = flow[order], rid[order]
    done = []
    for pos, k in forced:
        pos %= len(flow)
        at = np.setdiff1d(np.flatnonzero(rid == k), done)
        done.append(pos)
        q = int(at[np.argmin(np.abs(at - pos))])
        flow[[pos, q]], rid[[pos, q]] = flow[[q, pos]], rid[[q, pos]]
    return flow, rid


def chunk_slots(c, m, tail=0):
    """m records of chunk c: the first m - tail from the chunk's first slot on, the last `tail` (a
    multiple of 64) at the chunk's end."""
    assert tail % SEG == 0 and m <= CH and (tail == 0 or (m - tail) <= CH - tail)
    return np.r_[c * CH + np.arange(m - tail), c * CH + CH - tail + np.arange(tail)].astype(np.int64)


def _call(chunks, n_slots):
    """{chunk: (flow per position, tail)} -> (flow, slots, n_slots)."""
    fl, sl = [], []
    for c in sorted(chunks):
        f, tail = chunks[c]
        fl.append(np.asarray(f, dtype=np.int64))
        sl.append(chunk_slots(c, len(f), tail))
    return np.concatenate(fl), np.concatenate(sl), n_slots


def _nflows(L):
    return L if L < 3 else min(L, 3 + L % 6)


# ladder: run lengths per partition role and chunk (16 partitions; two full chunks and one of 4,096 records, every
# slot taken, so the dense and fused layouts see the same chunks as the placed one)
LADDER_PARTS = 16
LADDER = {0: [3, 9, 16],          # every run <= 16: k_hist_uniform
          1: [5000, 4, 8],        # a long run, then small ones: register sorts inside k_hist_general
          2: [4095, 1, 17],       # 4095 + 1 = kHistCap: the batch is cut on the run boundary
          3: [4096, 2, 63],
          4: [5, 4097, 64],
          5: [65, 127, 128],
          6: [129, 255, 256],
          7: [257, 511, 512],
          8: [513, 0, 0],
          9: [0, 3300, 0]}
LADDER_FLOWS = {5000: 40, 4097: 3, 4096: 7, 4095: 12, 3300: 25}
LADDER_EDGES = [0, 4095, 4096, 8191, 8192, CH - 1]  # long_run's record windows start at multiples of kHistCap
LADDER_WAVE_FLOW, LADDER_STRIDE_FLOW = 0, 1  # (indices into partition 1's pool) > 64 consecutive / 64 apart


def _ladder_run(T, U, p, L):
    nf = LADDER_FLOWS.get(L, _nflows(L))
    if L == 5000:  # flow 0: 70 consecutive entries (a full-wave ballot on one slot); flow 1: every 64th entry
        rest = rr(T[p][2:nf], L, U[p][:2])
        out = [T[p][LADDER_WAVE_FLOW]] * 70 + rest[70:]
        for i in range(134, L, 64):
            out[i] = T[p][LADDER_STRIDE_FLOW]
        return out
    return rr(T[p][:nf], L, U[p][:2] if L >= 17 else ())


LADDER_FILL = [10, 11, 12, 13, 14, 15]  # partitions that fill the chunks: the dense layouts then cut the same chunks
LADDER_SLOTS = 2 * CH + 4096


@functools.lru_cache(maxsize=None)
def ladder():
    T, U = pool(LADDER_PARTS)
    chunks = {}
    for c in range(3):
        ps = [p for p in LADDER if LADDER[p][c]]
        runs = [_ladder_run(T, U, p, LADDER[p][c]) for p in ps]
        room = min(CH, LADDER_SLOTS - c * CH) - sum(len(r) for r in runs)
        for k, p in enumerate(LADDER_FILL):  # 1,052 / 1,053 a partition in chunk 0, 2,029 in chunk 1, 505 / 506 in chunk 2
            runs.append(rr(T[p][:30], room // 6 + (k < room % 6), U[p][:2]))
        long_p = [k for k, p in enumerate(ps) if LADDER[p][c] in (5000, 4097)]
        flow, _ = merge(runs, [(e, long_p[0]) for e in LADDER_EDGES] if long_p else [])
        chunks[c] = (flow, 0)
    first = _call(chunks, LADDER_SLOTS)
    # the second call continues every flow of the first (two packets each, one run per partition)
    home = {f: p for p in range(LADDER_PARTS) for f in T[p][:64]}
    used = {}
    for f in np.unique(first[0]).tolist():
        if not f & UDP:
            used.setdefault(home[f], []).append(f)
    flow, _ = merge([rr(used[p], 2 * len(used[p])) for p in sorted(used)])
    return build([first, _call({0: (flow, 0)}, 4096)])


# waves: what needs a wave's 64 chunks (16 partitions, 256 full chunks and a 64-slot tail)
WAVES_PARTS, WAVES_CHUNKS = 16, 257
WAVES = {0: [8] * 64 + [1, 2, 3, 4] * 16 + [16, 9, 5, 1] * 16 + [1] * 64 + [0],  # uniform: 512 / reg4 / reg16 / single
         1: [9] + [8] * 63 + [0] * 193,                                        # a wave's share of 513: general
         2: [16] * 256 + [1]}                                                  # 4097 applied entries in runs <= 16
WAVES_FLOWS = {0: 5, 1: 9, 2: 16}


@functools.lru_cache(maxsize=None)
def waves():
    T, _ = pool(WAVES_PARTS)
    at = {p: 0 for p in WAVES}
    chunks = {}
    for c in range(WAVES_CHUNKS):
        runs = []
        for p in WAVES:
            fl = T[p][:WAVES_FLOWS[p]]
            runs.append([fl[(at[p] + i) % len(fl)] for i in range(WAVES[p][c])])
            at[p] += WAVES[p][c]
        chunks[c] = (merge(runs)[0], 0)
    return build([_call(chunks, (WAVES_CHUNKS - 1) * CH + SEG)])


# combined: 256 partitions; the hot threshold is 320 in a full chunk and 64 in the 4,096-slot tail chunk
COMBINED_PARTS, COMBINED_POOL = 256, 1 << 17
COMBINED_GROUPS = ["on_threshold", "below_threshold", "one_key", "keys_256", "half_once", "long", "overflow",
                   "tail_on", "tail_below"]


@functools.lru_cache(maxsize=None)
def combined():
    """-> ([Call], {group name: (chunk, partition)})."""
    T, U = pool(COMBINED_PARTS, COMBINED_POOL)
    by_size = sorted(range(COMBINED_PARTS), key=lambda p: -len(T[p]))
    P = dict(zip(COMBINED_GROUPS, by_size))  # (the overflow group needs 300 flows of one partition)
    assert len(T[P["overflow"]]) >= 300 and len(T[P["keys_256"]]) >= 256 and len(T[P["half_once"]]) >= 210
    t = lambda name, k: T[P[name]][:k]  # noqa: E731
    c0 = [rr(t("on_threshold", 10), 320, U[P["on_threshold"]][:1], every=8),   # 320 records: hot
          rr(t("below_threshold", 10), 319, U[P["below_threshold"]][:1], every=8),  # 319: plain (wave8)
          rr(t("one_key", 1), 400),
          rr(t("keys_256", 256), 512),
          _weave(rr(t("half_once", 110), 220), t("half_once", 210)[110:])]      # 110 keys twice, 100 keys once
    c1 = [rr(t("long", 6), 4100, U[P["long"]][:1], every=10),
          rr(t("overflow", 300), 600)]
    c2 = [rr(t("tail_on", 4), 64), rr(t("tail_below", 4), 63)]
    where = dict(zip(COMBINED_GROUPS, [(0, P[g]) for g in COMBINED_GROUPS[:5]] + [(1, P[g]) for g in COMBINED_GROUPS[5:7]] +
                     [(2, P[g]) for g in COMBINED_GROUPS[7:]]))
    chunks = {0: (merge(c0)[0], 0), 1: (merge(c1)[0], 0), 2: (merge(c2)[0], 0)}
    return build([_call(chunks, 2 * CH + 4096)]), where


# blocks: 16 partitions, 12 chunks (nblk = 3)
BLOCKS_PARTS, BLOCKS_CHUNKS = 16, 12
BLOCKS = {0: [1025] * 12,                                  # 12,300 entries to read: split
          1: [683] * 8 + [682] * 4,                        # 8,192: not split
          2: [683] * 9 + [682] * 3,                        # 8,193: split
          3: [300] * 5 + [5200] + [300] * 6}               # chunk 5 is hot (combined), the others plain: split
BLOCKS_FIRST_ONLY, BLOCKS_LAST_ONLY = 20, 21  # (indices into partition 0's pool)


@functools.lru_cache(maxsize=None)
def blocks():
    T, U = pool(BLOCKS_PARTS)
    chunks = {}
    for c in range(BLOCKS_CHUNKS):
        runs = []
        for p in BLOCKS:
            r = rr(T[p][:20] if p != 3 else T[p][:10], BLOCKS[p][c], U[p][:2], every=7)
            if p == 0 and c < 4:
                r[5::50] = [T[0][BLOCKS_FIRST_ONLY]] * len(r[5::50])
            if p == 0 and c >= 8:
                r[5::50] = [T[0][BLOCKS_LAST_ONLY]] * len(r[5::50])
            runs.append(r)
        chunks[c] = (merge(runs)[0], 0)
    return build([_call(chunks, BLOCKS_CHUNKS * CH)])


# rounds: 16 partitions, 514 chunks: more than kHistRuns, the second chunk round
ROUNDS_PARTS, ROUNDS_CHUNKS = 16, 514
ROUNDS_AT = [0, 1, 511, 512, 513]
ROUNDS = {0: [8, 16, 4, 12, 2],     # every run <= 16: uniform by everything but the chunk count
          1: [5, 3, 7, 600, 9],
          2: [1, 0, 0, 17, 0]}


@functools.lru_cache(maxsize=None)
def rounds():
    T, U = pool(ROUNDS_PARTS)
    chunks = {}
    for k, c in enumerate(ROUNDS_AT):
        runs = [rr(T[p][:4 if p == 0 else 12], ROUNDS[p][k], U[p][:1] if ROUNDS[p][k] >= 17 else ()) for p in ROUNDS]
        chunks[c] = (merge(runs)[0], 0)
    return build([_call(chunks, ROUNDS_CHUNKS * CH)])


# scramble: K1 scatters a chunk's records in the order its wavefronts reach their LDS atomics -- thread t takes
# the chunk's slots t, t + 1024, ..., so slot k belongs to iteration k // 1024 of wavefront (k % 1024) // 64 -- and
# that order is record order unless wavefronts race.  Here they are made to: the first half of every run sits in
# the last iteration's slots of wavefronts 0..7, which have a record (ballast, of other partitions) in every
# earlier iteration, and the second half in the same iteration's slots of wavefronts 8..15, which have none
# and get there first.  The runs then reach fb_hist.hip out of record order, and every sort has work to do.
SCRAMBLE_PARTS, SCRAMBLE_ITER = 16, 19
SCRAMBLE = {0: [4, 0], 1: [8, 0], 2: [16, 0],            # uniform: sort_net<4>, <8>, <16>
            3: [4, 17], 4: [8, 17], 5: [16, 17],         # the same networks inside k_hist_general, beside a wavefront's run
            6: [40, 0], 7: [100, 0], 8: [200, 0], 9: [400, 0],  # wave_sort_run<1>, <2>, <4>, <8>
            10: [0, 600]}                                # the bitmap rank
SCRAMBLE_BALLAST = [13, 14, 15]


@functools.lru_cache(maxsize=None)
def scramble():
    T, _ = pool(SCRAMBLE_PARTS)
    flow, slots = [], []
    for c in range(2):
        jw = np.arange(SCRAMBLE_ITER)[:, None] * 1024 + np.arange(512)[None, :]  # iterations 0..18 of wavefronts 0..7
        ballast = np.sort(jw.reshape(-1))
        early, late, at = [], [], SCRAMBLE_ITER * 1024
        for p in SCRAMBLE:
            r = rr(T[p][:3], SCRAMBLE[p][c])
            early += r[:len(r) // 2]
            late += r[len(r) // 2:]
        assert len(early) <= 512 and len(late) <= 512
        pos = np.r_[ballast, at + np.arange(len(early)), at + 512 + np.arange(len(late))]
        fl = np.r_[[T[SCRAMBLE_BALLAST[i % 3]][(i // 3) % 20] for i in range(len(ballast))], early, late]
        flow.append(np.asarray(fl, dtype=np.int64))
        slots.append(c * CH + pos)
    return build([(np.concatenate(flow), np.concatenate(slots), 2 * CH)])


# overfull: one partition of 512 slots and 600 flows
OVERFULL_FLOWS = 600


@functools.lru_cache(maxsize=None)
def overfull():
    count = [2 + (f * 7) % 39 for f in range(OVERFULL_FLOWS)]
    flow = [f for j in range(40) for f in range(OVERFULL_FLOWS) if j < count[f]]  # position-major
    assert min(count) == 2 and max(count) == 40 and len(flow) <= CH
    return build([_call({0: (flow, 0)}, _ceil(len(flow), SEG) * SEG)])
