"""A plain Python restatement of the device history store (flodbadd_amd/csrc/fb_histstore.hip): chains of
blocks of FB_HIST_BLOCK_CHARS 4-bit codes (1 + the FB_HIST_CHARS index, two to a byte, the low nibble first)
behind a 1-based id, a per-flow element [head, tail, len], a free stack of ids with a bump cursor above it.
An append takes its ids from one virtual sequence -- the first F off the top of the stack, the rest from the
bump cursor -- and commits afterwards; a purge pushes the removed flows' chains; the two never mix."""

HIST_CHARS = "SsHhFfRr><Aa-"
BLOCK_CHARS = 120
BLOCK_BYTES = BLOCK_CHARS // 2


def blocks_of(length):
    return (length + BLOCK_CHARS - 1) // BLOCK_CHARS


class HistStoreRef:
    def __init__(self):
        self.next = [None]       # next[id], id 0 unused
        self.bytes = [None]      # bytes[id]: bytearray(60)
        self.flows = {}          # key -> [head, tail, len]
        self.free = []           # the free stack, top last
        self.bump = 0            # ids ever taken from the bump cursor
        self.chars = 0

    # ---- allocation -------------------------------------------------------------------------------------
    def _id_of(self, v, F, bump):
        return self.free[F - 1 - v] if v < F else bump + (v - F) + 1

    def append(self, runs):
        """runs: [(key, str)] with one run per key -- one update's characters."""
        assert len({k for k, _ in runs}) == len(runs)
        F, bump, cursor = len(self.free), self.bump, 0
        for key, run in runs:
            if not run:
                continue
            e = self.flows.setdefault(key, [0, 0, 0])
            ln, nb0 = e[2], blocks_of(e[2])
            need = blocks_of(ln + len(run)) - nb0
            ids = [self._id_of(cursor + j, F, bump) for j in range(need)]
            cursor += need
            for i in ids:  # (a bump id extends the pool; a reused block keeps its stale payload)
                while len(self.next) <= i:
                    self.next.append(0)
                    self.bytes.append(bytearray(BLOCK_BYTES))
            for B in range(ln // 2, (ln + len(run) - 1) // 2 + 1):  # whole bytes, as the kernel writes them
                blk = B // BLOCK_BYTES
                bid = e[1] if blk < nb0 else ids[blk - nb0]
                q0, q1 = 2 * B, 2 * B + 1
                lo = self.bytes[bid][B % BLOCK_BYTES] & 15 if q0 < ln else HIST_CHARS.index(run[q0 - ln]) + 1
                hi = 0 if q1 >= ln + len(run) else HIST_CHARS.index(run[q1 - ln]) + 1
                self.bytes[bid][B % BLOCK_BYTES] = lo | hi << 4
            for j, i in enumerate(ids):
                self.next[i] = ids[j + 1] if j + 1 < need else 0
            if need:
                if ln == 0:
                    e[0] = ids[0]
                else:
                    self.next[e[1]] = ids[0]
                e[1] = ids[-1]
            e[2] = ln + len(run)
            self.chars += len(run)
        # the commit: what the cursor consumed folded into F and the bump cursor
        if cursor <= F:
            del self.free[F - cursor:]
        else:
            self.bump += cursor - F
            self.free = []

    def purge(self, keys):
        """The removed flows' chains go onto the free stack."""
        for key in keys:
            e = self.flows.pop(key, None)
            if not e:
                continue
            i, n = e[0], 0
            while i:
                self.free.append(i)
                i, n = self.next[i], n + 1
            assert n == blocks_of(e[2])
            self.chars -= e[2]

    def clear(self):
        self.__init__()

    # ---- reading ----------------------------------------------------------------------------------------
    def gather(self, key):
        e = self.flows.get(key)
        if not e:
            return ""
        out, i = [], e[0]
        while i and len(out) < e[2]:
            for b in self.bytes[i]:
                out += [b & 15, b >> 4]
            i = self.next[i]
        return "".join(HIST_CHARS[c - 1] for c in out[:e[2]])

    def info(self):
        return dict(blocks_high_water=self.bump, blocks_free=len(self.free), blocks_in_use=self.bump - len(self.free),
                    chars=self.chars, flows=sum(1 for e in self.flows.values() if e[2]))
