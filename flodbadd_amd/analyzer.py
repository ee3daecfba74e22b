"""Host side of the anomaly pass (src/analyzer.rs): the model the device walks, and everything around it
that covers at most 300 samples -- training, feature statistics, percentile thresholds, the strings.

The reference scores sessions with the `extended-isolation-forest` crate, which is not part of its
sources, and hashes names with per-call random keys; so the forest is DEFINED here: the
Extended Isolation Forest of Hariri et al. with the reference's hyper-parameters, split tests folded to
`x . normal < b`, and every dot product accumulated left to right from 0.0 with separately rounded
products and sums -- the arithmetic of fb_anomaly.hip, so `Forest.path_sums` equals the device bit for bit.
"""
import math
import struct

import numpy as np

from . import _native as N
from .sessions import service_name

NUM_FEATURES = N.FB_AN_FEATURES
MAX_SAMPLES = 300                       # IsolationForestModel.max_samples, src/analyzer.rs:136
DEFAULT_SUSPICIOUS_PERCENTILE, DEFAULT_ABNORMAL_PERCENTILE = 0.93, 0.95  # src/analyzer.rs:72-73
DEFAULT_SUSPICIOUS_THRESHOLD, DEFAULT_ABNORMAL_THRESHOLD = 0.75, 0.80    # src/analyzer.rs:74-75
WARMUP_DELAY_S = 30                     # src/analyzer.rs:77
MAX_TREE_DEPTH = 6                      # src/analyzer.rs:284
LEVELS = {N.FB_AN_NORMAL: "normal", N.FB_AN_SUSPICIOUS: "suspicious", N.FB_AN_ABNORMAL: "abnormal"}
# FEATURE_DEFS, src/analyzer.rs:369-380: (name, categorical).  The table calls index 6 DestService and
# index 7 AvgPacketSize although compute_features puts them the other way round; kept as it is.
FEATURE_DEFS = [("Process", True), ("Duration", False), ("Bytes", False), ("Packets", False),
                ("SegmentInterarrival", False), ("InOutRatio", False), ("DestService", True),
                ("AvgPacketSize", False), ("SelfDestination", True), ("MissedData", False)]


def fnv1a64(text):
    h = 0xCBF29CE484222325
    for b in text.encode():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def service_code(name):
    """The feature value of a destination service name: FNV-1a-64 % 1,000,000 (the reference's SipHash with
    random keys is not reproducible; src/analyzer.rs:766-774)."""
    return fnv1a64(name) % N.FB_AN_MAX_SERVICE_CODE


_SERVICE_CODES = None


def default_service_codes():
    """uint32[65536]: the code of every port's service name (data/service_names.json), or of its decimal
    number where only a run-time table would name it -- the strings flows_to_sessions puts in dst_service."""
    global _SERVICE_CODES
    if _SERVICE_CODES is None:
        _SERVICE_CODES = np.array([service_code(service_name(p) or str(p)) for p in range(65536)], dtype=np.uint32)
    return _SERVICE_CODES


def sanitize(v):
    return 0.0 if (math.isnan(v) or math.isinf(v)) else v


def compute_features(info):
    """compute_features (src/analyzer.rs:716-793) of a SessionInfo -> [float] * 10."""
    st = info.stats
    if st.start_time_ns is not None:
        t = st.end_time_ns if st.end_time_ns is not None else st.last_activity_ns
        d = t - st.start_time_ns
        ms = -((-d) // 1000000) if d < 0 else d // 1000000  # num_milliseconds truncates toward zero
        duration, interarrival = sanitize(ms / 1000.0), sanitize(st.segment_interarrival)
    else:
        duration, interarrival = 0.0, 0.0  # no clock on an untimed capture
    # (the counters as f64 first, then one division: `as f64` of the reference, and what the device does;
    # Python's int / int would round the exact quotient instead, which differs above 2^53)
    nbytes, pkts = float(st.inbound_bytes + st.outbound_bytes), float(st.orig_pkts + st.resp_pkts)
    ratio = float(st.inbound_bytes) / float(st.outbound_bytes) if st.outbound_bytes > 0 else 0.0
    return [0.0, duration, sanitize(nbytes), sanitize(pkts), interarrival, sanitize(ratio),
            sanitize(nbytes / pkts if pkts > 0 else 0.0),
            float(service_code(info.dst_service)) if info.dst_service is not None else 0.0,
            1.0 if info.is_self_dst else 0.0, 0.0]


def c_factor(n):
    """Average path length of an unsuccessful search in a binary search tree of n points."""
    if n > 2:
        return 2.0 * (math.log(n - 1) + 0.5772156649) - 2.0 * (n - 1) / n
    return 1.0 if n == 2 else 0.0


def dot_unfused(x, w):
    s = 0.0
    for a, b in zip(x, w):
        s = s + float(a) * float(b)
    return s


class Forest:
    """nodes: IF_NODE_DTYPE, tree t = nodes[first[t]:first[t + 1]]; sample_size: what the trees were grown on."""

    def __init__(self, nodes, first, sample_size):
        self.nodes = np.ascontiguousarray(nodes, dtype=N.IF_NODE_DTYPE)
        self.first = np.ascontiguousarray(first, dtype=np.uint32)
        self.sample_size = int(sample_size)

    @property
    def n_trees(self):
        return len(self.first) - 1

    def valid(self):
        """fb_if_validate: the rules fb_set_anomaly_model installs a forest under (host code, needs no GPU)."""
        return N.gpu_lib().fb_if_validate(N.ptr(self.nodes), len(self.nodes), N.ptr(self.first), self.n_trees) == N.FB_OK

    def path_sums(self, X):
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, NUM_FEATURES)
        total = np.zeros(len(X))
        with np.errstate(all="ignore"):
            for t in range(self.n_trees):
                tr = self.nodes[self.first[t]:self.first[t + 1]]
                at = np.zeros(len(X), dtype=np.int64)
                for _ in range(N.FB_IF_MAX_DEPTH):
                    inner = tr["left"][at] != N.FB_IF_LEAF
                    if not inner.any():
                        break
                    s = np.zeros(len(X))
                    for j in range(NUM_FEATURES):
                        s = s + X[:, j] * tr["normal"][at, j]
                    nxt = np.where(s < tr["value"][at], tr["left"][at], tr["right"][at]).astype(np.int64)
                    at = np.where(inner, nxt, at)
                total = total + tr["value"][at]
        return total

    def score(self, X):
        """2^(-(mean path length) / c(sample_size)), for display and for the percentile thresholds."""
        c = c_factor(self.sample_size)
        return np.array([2.0 ** (-(p / self.n_trees) / c) if c > 0.0 else 0.5 for p in self.path_sums(X).tolist()])


def dedup_rows(data):
    """src/analyzer.rs:254-262: rows deduplicated by bit pattern, first occurrence kept."""
    seen, out = set(), []
    for row in data:
        key = struct.pack("<%dd" % NUM_FEATURES, *[float(v) for v in row])
        if key not in seen:
            seen.add(key)
            out.append([float(v) for v in row])
    return out


def train_forest(data, seed):
    """An Extended Isolation Forest over the deduplicated rows with the reference's hyper-parameters
    (src/analyzer.rs:276-291).  Raises ValueError on fewer than 2 unique rows (no model)."""
    rows = np.array(dedup_rows(data), dtype=np.float64).reshape(-1, NUM_FEATURES)
    n = len(rows)
    if n < 2:
        raise ValueError("%d unique samples: no forest" % n)
    sample_size = min(128, n)
    n_trees = 10 if n < 10 else (15 if n < 50 else 25)
    rng = np.random.default_rng(seed)
    nodes, first = [], [0]

    def grow(tree, X, depth):
        idx = len(tree)
        tree.append(None)
        if depth >= MAX_TREE_DEPTH or len(X) <= 1:
            tree[idx] = ([0.0] * NUM_FEATURES, depth + c_factor(len(X)), N.FB_IF_LEAF, N.FB_IF_LEAF)
            return idx
        normal = rng.standard_normal(NUM_FEATURES)           # extension level 9: every coordinate drawn
        point = rng.uniform(X.min(axis=0), X.max(axis=0))    # the intercept, inside the node's box
        b = dot_unfused(point, normal)
        left = np.array([dot_unfused(x, normal) < b for x in X], dtype=bool)
        li = grow(tree, X[left], depth + 1)
        ri = grow(tree, X[~left], depth + 1)
        tree[idx] = (normal.tolist(), b, li, ri)
        return idx

    for _ in range(n_trees):
        tree = []
        grow(tree, rows[rng.choice(n, sample_size, replace=False)], 0)
        nodes += tree
        first.append(len(nodes))
    arr = np.zeros(len(nodes), dtype=N.IF_NODE_DTYPE)
    for k, (normal, value, li, ri) in enumerate(nodes):
        arr[k] = (normal, value, li, ri)
    return Forest(arr, first, sample_size)


def feature_stats(data):
    """compute_feature_stats_bulk (src/analyzer.rs:317-353) -> (mean[10], std[10], has_stats): the sums run
    in row order; has_stats is its `counts > 1` (without it no feature has statistics)."""
    rows = [[float(v) for v in r] for r in data]
    cnt = len(rows)
    mean, std = [0.0] * NUM_FEATURES, [0.0] * NUM_FEATURES
    if cnt == 0:
        return mean, std, False
    for i in range(NUM_FEATURES):
        s = 0.0
        for r in rows:
            s += r[i]
        mean[i] = s / float(cnt)
    if cnt > 1:
        for i in range(NUM_FEATURES):
            q = 0.0
            for r in rows:
                d = r[i] - mean[i]
                q += d * d
            std[i] = math.sqrt(q / (float(cnt) - 1.0))
    return mean, std, cnt > 1


def compute_dynamic_thresholds(scores, suspicious_percentile=DEFAULT_SUSPICIOUS_PERCENTILE,
                               abnormal_percentile=DEFAULT_ABNORMAL_PERCENTILE):
    """src/analyzer.rs:880-969 over the scores of recent_data -> (suspicious, abnormal) score thresholds."""
    s = sorted(float(v) for v in scores)
    n = len(s)
    if n == 0:
        return DEFAULT_SUSPICIOUS_THRESHOLD, DEFAULT_ABNORMAL_THRESHOLD
    eps = 1e-6
    si = max(int(math.ceil(n * suspicious_percentile)) - 1, 0)
    ai = max(int(math.ceil(n * abnormal_percentile)) - 1, 0)
    sus = max(s[si] + eps, DEFAULT_SUSPICIOUS_THRESHOLD)
    abn = max(max(s[ai] + eps, sus + eps), DEFAULT_ABNORMAL_THRESHOLD)
    return sus, abn


def path_cut(threshold, sample_size, n_trees):
    """score >= threshold (src/analyzer.rs:586-592) as a bound on the path sum: path_sum <= cut.  The cut IS
    the project's boundary: the device has no pow."""
    return -math.log2(threshold) * c_factor(sample_size) * n_trees


def diagnostic_string(mask):
    """generate_anomaly_diagnostic's text (src/analyzer.rs:425-470) from the device's fb_an_diag codes."""
    out = []
    for i, (name, categorical) in enumerate(FEATURE_DEFS):
        code = (int(mask) >> (2 * i)) & 3
        if code == N.FB_AN_DIAG_HIGH:
            out.append(name + ":UnusuallyHigh")
        elif code == N.FB_AN_DIAG_LOW:
            out.append(name + ":UnusuallyLow")
        elif code == N.FB_AN_DIAG_DEVIATES:
            out.append(name + (":Unusual" if categorical else ":DeviatesFromNorm"))
    return "/".join(out) if out else "OverallScoreHigh"


def merge_criticality(existing, level, diag=""):
    """analyze_session's tag merge (src/analyzer.rs:630-653): the old anomaly: tags go, the others stay,
    the new tag is added, all sorted and deduplicated.  level: "normal" / "suspicious" / "abnormal"."""
    tag = "anomaly:%s/%s" % (level, diag) if diag else "anomaly:%s" % level
    tags = [t.strip() for t in existing.split(",") if t.strip() and not t.strip().startswith("anomaly:")]
    return ",".join(sorted(set(tags + [tag])))


def anomaly_tag_of(rec):
    """(level name, diagnostic text) of one fb_an_rec whose level is not 0."""
    lvl = int(rec["level"])
    return LEVELS[lvl], (diagnostic_string(rec["diag"]) if lvl >= N.FB_AN_SUSPICIOUS else "")


class SessionAnalyzer:
    """The analyzer's state around the device pass: the recent_data FIFO (at most 300 vectors, appended in
    the caller's order), the thresholds, the warm-up clock (the caller's `now`), the trained model."""

    def __init__(self, seed=0):
        self.recent_data = []
        self.seed = seed
        self.forest = None
        self.stats = None                     # feature_stats of recent_data at training
        self.suspicious_threshold = DEFAULT_SUSPICIOUS_THRESHOLD
        self.abnormal_threshold = DEFAULT_ABNORMAL_THRESHOLD
        self.test_thresholds = False
        self.warmup_disabled = False
        self.started_ns = None

    def set_test_thresholds(self, suspicious, abnormal):
        """src/analyzer.rs:1823: fixed thresholds; training no longer replaces them."""
        self.suspicious_threshold, self.abnormal_threshold, self.test_thresholds = float(suspicious), float(abnormal), True

    def disable_warmup_for_testing(self):
        self.warmup_disabled = True

    def add_session_data(self, vectors):
        for v in vectors:
            self.recent_data.append([float(x) for x in v])
        del self.recent_data[:max(len(self.recent_data) - MAX_SAMPLES, 0)]

    def warming_up(self, now_ns):
        """The first call starts the clock; warm-up lasts WARMUP_DELAY_S of the caller's time."""
        if self.warmup_disabled:
            return False
        if now_ns is None:
            return False
        if self.started_ns is None:
            self.started_ns = int(now_ns)
        return int(now_ns) - self.started_ns < WARMUP_DELAY_S * 10 ** 9

    def train(self):
        """Train on recent_data -> True, or False (no model) on fewer than 2 unique vectors."""
        try:
            self.forest = train_forest(self.recent_data, self.seed)
        except ValueError:
            self.forest = None
            return False
        self.stats = feature_stats(self.recent_data)
        if not self.test_thresholds:
            self.suspicious_threshold, self.abnormal_threshold = compute_dynamic_thresholds(
                self.forest.score(self.recent_data))
        return True
