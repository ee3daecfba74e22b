"""CPU-side checks of the anomaly pass: the C-ABI structs, constants and symbols, the forest validation
(host code of the library), the restatement in tests/anref.py against the reference's criticality-merging
tests (tests/golden/anomaly_kats.json), and flodbadd_amd/analyzer.py against that restatement -- the walk
bit for bit, the statistics, the thresholds, the strings."""
import ipaddress
import json
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import anforests as F
import anref
from flodbadd_amd import _native as N
from flodbadd_amd import analyzer as A
from flodbadd_amd.sessions import Protocol, Session, SessionInfo, SessionStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "anomaly_kats.json")))["cases"]


def bits(values):
    return [struct.pack("<d", float(v)) for v in values]


def ref_path_sums(forest, X):
    trees = anref.trees_of(forest.nodes, forest.first)
    return [anref.path_sum(trees, [float(v) for v in x]) for x in X]


def test_structs_and_constants_match_the_header(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s/include/flodbadd_gpu.h"' % ROOT, "int main(void) {"]
    want = []
    for st, dt in (("fb_if_node", N.IF_NODE_DTYPE), ("fb_an_params", N.AN_PARAMS_DTYPE), ("fb_an_rec", N.AN_REC_DTYPE),
                   ("fb_an_stats", N.AN_STATS_DTYPE)):
        src.append('printf("%%zu\\n", sizeof(%s));' % st)
        want.append(dt.itemsize)
        for f in dt.names:
            src.append('printf("%%zu\\n", offsetof(%s, %s));' % (st, f))
            want.append(dt.fields[f][1])
    for c, v in (("FB_AN_FEATURES", 10), ("FB_IF_MAX_TREES", 64), ("FB_IF_MAX_TREE_NODES", 255), ("FB_IF_MAX_DEPTH", 12),
                 ("FB_IF_LEAF", 0xFFFFFFFF), ("FB_AN_MAX_SERVICE_CODE", 1000000), ("FB_AN_UNSEEN", 0), ("FB_AN_NORMAL", 1),
                 ("FB_AN_SUSPICIOUS", 2), ("FB_AN_ABNORMAL", 3), ("FB_AN_DIAG_HIGH", 1), ("FB_AN_DIAG_LOW", 2),
                 ("FB_AN_DIAG_DEVIATES", 3), ("FB_ABI_VERSION", 4)):
        src.append('printf("%%u\\n", (unsigned)%s);' % c)
        want.append(v)
        assert getattr(N, c) == v
    src.append("return 0; }")
    c = tmp_path / "an.c"
    c.write_text("\n".join(src) + "\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "an"), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "an")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert (N.IF_NODE_DTYPE.itemsize, N.AN_PARAMS_DTYPE.itemsize, N.AN_REC_DTYPE.itemsize, N.AN_STATS_DTYPE.itemsize) == (96, 184, 16, 64)
    assert list(N.AN_STATS_DTYPE.names[:7]) == N.AN_STATS_FIELDS
    assert anref.LEAF == N.FB_IF_LEAF and anref.MAX_DEPTH == N.FB_IF_MAX_DEPTH and anref.NUM == N.FB_AN_FEATURES


def test_symbols_are_exported_and_reject_a_null_context():
    lib = N.gpu_lib()
    for name in ("fb_if_validate", "fb_set_service_codes", "fb_set_anomaly_model", "fb_clear_anomaly_model", "fb_flow_anomaly", "fb_flow_anomaly_dev",
                 "fb_flow_export_anomalous_dev", "fb_flow_features_dev", "fb_if_score_dev"):
        assert hasattr(lib, name), name
    f = F.three_nodes()
    prm = np.zeros(1, dtype=N.AN_PARAMS_DTYPE)
    assert lib.fb_set_anomaly_model(None, N.ptr(f.nodes), len(f.nodes), N.ptr(f.first), 1, N.ptr(prm), None) == N.FB_ERR_INVAL
    assert lib.fb_clear_anomaly_model(None) == N.FB_ERR_INVAL
    assert lib.fb_set_service_codes(None, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_anomaly(None, 0, None, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_anomaly_dev(None, None, 0, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_export_anomalous_dev(None, 2, None, None, 0, None, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_features_dev(None, None, None, 0, None, None) == N.FB_ERR_INVAL
    assert lib.fb_if_score_dev(None, None, 0, None, None) == N.FB_ERR_INVAL
    assert lib.fb_if_validate(None, 0, None, 0) == N.FB_ERR_INVAL and lib.fb_last_error()


# ---- the reference's merge tests -------------------------------------------------------------------
def check_step(out, step):
    for s in step.get("must", []):
        assert s in out, (s, out)
    for s in step.get("must_not", []):
        assert s not in out, (s, out)
    if "any_of" in step:
        assert any(s in out for s in step["any_of"]), out
    for s, n in step.get("count", {}).items():
        assert out.count(s) == n, out
    tags = out.split(",")
    if step.get("sorted"):
        assert tags == sorted(tags)
    if step.get("no_empty_tags"):
        assert all(t.strip() for t in tags)
    assert sum(t.startswith("anomaly:") for t in tags) == 1 and tags == sorted(set(tags))


@pytest.mark.parametrize("merge", [anref.merge, A.merge_criticality], ids=["anref", "analyzer"])
@pytest.mark.parametrize("case", KATS, ids=[c["from"].split()[1] for c in KATS])
def test_merge_reproduces_the_reference_kats(case, merge):
    for diag in ("", "OverallScoreHigh", "Duration:UnusuallyHigh/Bytes:UnusuallyHigh"):
        levels = set.intersection(*(set(s["levels"]) for s in case["steps"]))
        for level in sorted(levels):
            prev, outs = "", []
            for step in case["steps"]:
                text = (prev if step.get("prefix_previous") else "") + step["in"]
                d = diag if level != "normal" else ""
                prev = merge(text, level, d)
                check_step(prev, step)
                outs.append(prev)
                assert prev == anref.merge(text, level, d) == A.merge_criticality(text, level, d)
            if "blacklisted_count" in case:
                assert sum("blacklist:" in o for o in outs) == case["blacklisted_count"]


def test_merge_examples():
    assert A.merge_criticality("", "normal") == "anomaly:normal"
    assert A.merge_criticality("blacklist:b,blacklist:a", "abnormal", "Bytes:UnusuallyHigh") == \
        "anomaly:abnormal/Bytes:UnusuallyHigh,blacklist:a,blacklist:b"
    assert A.merge_criticality("anomaly:suspicious/OverallScoreHigh, blacklist:x ,", "normal") == "anomaly:normal,blacklist:x"
    assert A.merge_criticality("zz:1,anomaly:normal/warming_up,anomaly:abnormal", "suspicious", "OverallScoreHigh") == \
        "anomaly:suspicious/OverallScoreHigh,zz:1"


# ---- the walk ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["trained", "leaf_only", "chain_12", "three_nodes", "trees_64", "nodes_255"])
def test_path_sums_equal_the_restatement_bit_for_bit(name):
    forest = F.ALL[name]()
    assert forest.valid()
    X = np.concatenate([F.vectors(), F.special_vectors()])
    got = forest.path_sums(X)
    assert bits(got) == bits(ref_path_sums(forest, X))
    if name == "leaf_only":
        assert not got.any() and len(forest.nodes) == 1
    if name == "chain_12":
        assert set(got.tolist()) >= {0.5, 12.5} and len(set(got.tolist())) > 6   # both ends of the chain are reached
    if name == "trained":
        assert forest.n_trees == 25 and forest.sample_size == 128 and len(set(got[:300].tolist())) > 100
        assert max(np.diff(forest.first.astype(int))) <= 127
        sc = forest.score(F.vectors())
        c = anref.c(128)
        assert bits(sc) == bits([2.0 ** (-(p / 25) / c) for p in ref_path_sums(forest, F.vectors())])
        assert 0.3 < sc.min() < sc.max() < 0.9


def test_a_nan_goes_right_and_the_unfused_product_goes_left():
    f = F.three_nodes()
    X = F.special_vectors()
    assert f.path_sums(X[4:5])[0] == 2.5 == ref_path_sums(f, X[4:5])[0]      # NaN < b is false
    assert f.path_sums(np.zeros((1, 10)))[0] == 1.25                          # 0 < 100000
    probe, x = F.contraction_probe()
    assert probe.path_sums(x)[0] == 1.0 == ref_path_sums(probe, x)[0]
    # what a fused multiply-add would have computed: exactly 2^-60, not below the offset 2^-61
    from fractions import Fraction
    exact = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(x[0], probe.nodes[0]["normal"]))
    assert exact == Fraction(1, 2 ** 60) and exact >= Fraction(float(probe.nodes[0]["value"]))


def test_training_follows_the_reference_hyper_parameters():
    X = F.vectors()
    for n, trees, sample in ((2, 10, 2), (9, 10, 9), (10, 15, 10), (49, 15, 49), (50, 25, 50), (300, 25, 128)):
        f = A.train_forest(X[:n], seed=3)
        assert (f.n_trees, f.sample_size) == (trees, sample) and f.valid()
        t = anref.trees_of(f.nodes, f.first)
        for tree in t:
            depth = {0: 0}
            for i, (normal, value, left, right) in enumerate(tree):
                if left != anref.LEAF:
                    assert i < left < len(tree) and i < right < len(tree)
                    depth[left] = depth[right] = depth[i] + 1
                else:
                    assert not any(normal)
            assert max(depth.values()) <= A.MAX_TREE_DEPTH and len(tree) <= 127
    dup = np.concatenate([X[:5], X[:5], X[:5]])
    assert A.train_forest(dup, seed=3).sample_size == 5 and len(A.dedup_rows(dup)) == 5
    assert len(A.dedup_rows([[0.0] * 10, [-0.0] + [0.0] * 9])) == 2                  # by bit pattern
    for bad in (X[:0], X[:1], np.concatenate([X[:1]] * 4)):
        with pytest.raises(ValueError):
            A.train_forest(bad, seed=3)
    same = A.train_forest(X, seed=1234)
    assert same.nodes.tobytes() == F.trained().nodes.tobytes() and A.train_forest(X, seed=1235).nodes.tobytes() != same.nodes.tobytes()


# ---- install-time validation -------------------------------------------------------------------------
def test_validation_rejects_every_malformed_forest():
    lib = N.gpu_lib()

    def ok(forest, n_trees=None, n_nodes=None):
        return lib.fb_if_validate(N.ptr(forest.nodes), len(forest.nodes) if n_nodes is None else n_nodes, N.ptr(forest.first),
                                  forest.n_trees if n_trees is None else n_trees) == N.FB_OK

    for name, make in F.ALL.items():
        assert ok(make()), name
    n = [0.0] * 10
    leaf = F.leaf
    bad = {
        "child == parent": F.make([[(n, 0.0, 0, 2), leaf(1), leaf(1)]]),
        "child below parent": F.make([[(n, 0.0, 1, 2), (n, 0.0, 0, 2), leaf(1)]]),
        "left outside the tree": F.make([[(n, 0.0, 3, 2), leaf(1), leaf(1)]]),
        "right outside the tree": F.make([[(n, 0.0, 1, 3), leaf(1), leaf(1)]]),
        "right is the leaf mark": F.make([[(n, 0.0, 1, N.FB_IF_LEAF), leaf(1), leaf(1)]]),
        "child in the next tree": F.make([[(n, 0.0, 1, 2), leaf(1)], [leaf(1)]]),
        "last node internal": F.make([[(n, 0.0, 1, 2), leaf(1), (n, 0.0, 3, 3)]]),
        "256 nodes": F.make([[(n, 0.0, k + 1, 255) for k in range(254)] + [leaf(1), leaf(1)]]),
        "NaN value": F.make([[(n, float("nan"), 1, 2), leaf(1), leaf(1)]]),
        "infinite leaf value": F.make([[(n, 0.0, 1, 2), leaf(1), leaf(float("inf"))]]),
        "infinite normal": F.make([[([0.0] * 9 + [float("-inf")], 0.0, 1, 2), leaf(1), leaf(1)]]),
        "NaN normal in a leaf": F.make([[([float("nan")] + [0.0] * 9, 1.0, N.FB_IF_LEAF, N.FB_IF_LEAF)]]),
    }
    d = N.FB_IF_MAX_DEPTH + 1  # a chain one level deeper than the cap
    bad["depth 13"] = F.make([[(n, 0.0, d + k, k + 1 if k + 1 < d else 2 * d) for k in range(d)] + [leaf(1)] * (d + 1)])
    for what, forest in bad.items():
        assert not ok(forest), what
    good = F.trees_64()
    assert not ok(good, n_trees=0) and ok(good, n_trees=64)
    assert not ok(F.make([[leaf(1)]] * 65))                                               # above the tree cap
    assert not ok(good, n_nodes=len(good.nodes) - 1)                                      # first[n_trees] != n_nodes
    empty = F.make([[leaf(1)], [leaf(1)]])
    empty.first[1] = 0                                                                    # an empty tree
    assert not ok(empty)
    shifted = F.make([[leaf(1)], [leaf(1)]])
    shifted.first[0] = 1
    assert not ok(shifted)
    assert ok(F.chain_12()) and F.chain_12().valid() and not bad["depth 13"].valid()


# ---- statistics, thresholds, strings -----------------------------------------------------------------
def test_feature_stats_equal_the_restatement():
    X = F.vectors()
    for rows in (X, X[:2], X[:1], X[:0], np.concatenate([X[:1]] * 3)):
        m, s, has = A.feature_stats(rows)
        rm, rs, rhas = anref.feature_stats([[float(v) for v in r] for r in rows])
        assert bits(m) == bits(rm) and bits(s) == bits(rs) and has is rhas is (len(rows) > 1)
    m, s, has = A.feature_stats([[1.0] + [0.0] * 9, [3.0] + [0.0] * 9])
    assert m[0] == 2.0 and s[0] == math.sqrt(2.0) and s[1] == 0.0


def test_dynamic_thresholds():
    # twenty scores 0.40, 0.42 .. 0.78: both percentiles fall on index 18 (ceil(18.6) - 1, ceil(19.0) - 1), score
    # 0.76; + 1e-6 is above the suspicious floor 0.75, and the abnormal one is lifted to its floor 0.80
    s20 = [0.40 + 0.02 * k for k in range(20)]
    assert A.compute_dynamic_thresholds(s20[::-1]) == (s20[18] + 1e-6, 0.80) == anref.dynamic_thresholds(s20)
    # the same ranks well above the floors: the abnormal threshold is pushed one more epsilon above the suspicious one
    hi = [0.5] * 18 + [0.85, 0.9]
    assert A.compute_dynamic_thresholds(hi) == (0.85 + 1e-6, 0.85 + 1e-6 + 1e-6) == anref.dynamic_thresholds(hi)
    assert A.compute_dynamic_thresholds(hi, 0.93, 0.96) == (0.85 + 1e-6, 0.9 + 1e-6)       # ceil(19.2) - 1 = 19
    # everything low: the floors
    assert A.compute_dynamic_thresholds([0.3] * 20) == (0.75, 0.80)
    # n = 1: index ceil(0.93) - 1 = 0 for both
    assert A.compute_dynamic_thresholds([0.9]) == (0.9 + 1e-6, 0.9 + 1e-6 + 1e-6) == anref.dynamic_thresholds([0.9])
    # n = 300: 300 * 0.93 = 279.0 and 300 * 0.95 = 285.0 in f64 -> indices 278 and 284
    assert (300 * 0.93, 300 * 0.95) == (279.0, 285.0)
    s300 = [0.80 + k * 1e-4 for k in range(300)]
    assert A.compute_dynamic_thresholds(s300) == (s300[278] + 1e-6, s300[284] + 1e-6) == anref.dynamic_thresholds(s300)
    assert A.compute_dynamic_thresholds([]) == (0.75, 0.80)


def test_cuts_and_c_factor():
    assert A.c_factor(0) == A.c_factor(1) == 0.0 and A.c_factor(2) == 1.0
    for n in (3, 5, 128, 300):
        assert A.c_factor(n) == anref.c(n) == 2.0 * (math.log(n - 1) + 0.5772156649) - 2.0 * (n - 1) / n
    for thr in (0.6, 0.72, 0.75, 0.8, 0.1):
        assert A.path_cut(thr, 128, 25) == anref.cut(thr, 128, 25) == -math.log2(thr) * anref.c(128) * 25
    assert A.path_cut(0.8, 128, 25) < A.path_cut(0.75, 128, 25)   # a higher score threshold is a shorter path
    assert A.path_cut(0.5, 128, 25) == anref.c(128) * 25


def test_diagnostic_codes_and_strings():
    mean = [0.0, 10.0, 1000.0, 10.0, 0.0, 1.0, 100.0, 443951.0, 0.0, 0.0]
    std = [0.0, 2.0, 100.0, 0.0, 1e-6, 0.5, 0.0, 10.0, 0.5, 0.0]
    x = [0.0, 15.0, 749.0, 11.0, 0.5, 2.2, 101.0, 0.0, 1.0, 1e-6]
    mask = anref.diag_mask(x, mean, std, True)
    # 1: z = 2.5 high; 2: z = -2.51 low; 3: no variance, differs; 4: std == 1e-6 is not above it, differs; 5: z = 2.4;
    # 6: "categorical", no variance, differs; 7: numeric by the table's quirk, far below; 8: categorical with variance;
    # 9: |x - mean| == 1e-6 is not above it
    want = {1: 1, 2: 2, 3: 3, 4: 3, 6: 3, 7: 2}
    assert mask == sum(c << (2 * i) for i, c in want.items())
    text = "Duration:UnusuallyHigh/Bytes:UnusuallyLow/Packets:DeviatesFromNorm/SegmentInterarrival:DeviatesFromNorm/" \
           "DestService:Unusual/AvgPacketSize:UnusuallyLow"
    assert A.diagnostic_string(mask) == anref.diag_text(mask) == text
    assert A.diagnostic_string(0) == anref.diag_text(0) == "OverallScoreHigh"
    assert anref.diag_mask(x, mean, std, False) == 0
    assert A.diagnostic_string(3 | 3 << 16) == "Process:Unusual/SelfDestination:Unusual"
    rng = np.random.default_rng(2)
    for m in rng.integers(0, 1 << 20, 200).tolist():
        assert A.diagnostic_string(m) == anref.diag_text(m)
    assert [n for n, _ in A.FEATURE_DEFS] == anref.NAMES and [i for i, (_, c) in enumerate(A.FEATURE_DEFS) if c] == list(anref.CATEGORICAL)


# ---- features ----------------------------------------------------------------------------------------
def info(stats, dst_port=443, service=None, self_dst=False):
    s = Session(Protocol.TCP, ipaddress.ip_address("192.168.1.9"), 40001, ipaddress.ip_address("93.184.216.34"), dst_port)
    return SessionInfo(s, stats, dst_service=service, is_self_dst=self_dst)


def test_features_of_a_session_info():
    codes = anref.service_codes()
    assert codes == A.default_service_codes().tolist() and max(codes) < N.FB_AN_MAX_SERVICE_CODE
    assert A.fnv1a64("") == 0xCBF29CE484222325 and A.fnv1a64("a") == 0xAF63DC4C8601EC8C       # the published FNV-1a vectors
    assert codes[443] == A.service_code("https") == anref.fnv("https") % 1000000
    assert codes[40001] == A.service_code("40001")                                            # a port without a name
    S = 10 ** 9
    timed = SessionStats(inbound_bytes=3001, outbound_bytes=7, orig_pkts=2, resp_pkts=1, start_time_ns=5 * S,
                         last_activity_ns=5 * S + 1_999_999_999, end_time_ns=None, total_segment_interarrival_ms=1001,
                         segment_interarrival_div=3)
    x = A.compute_features(info(timed, service="https", self_dst=True))
    assert x == anref.features(info(timed, service="https", self_dst=True), codes)
    assert x == [0.0, 1.999, 3008.0, 3.0, 1001 / 1000.0 / 3.0, 3001 / 7, 3008 / 3, float(codes[443]), 1.0, 0.0]
    ended = SessionStats(inbound_bytes=10, outbound_bytes=0, start_time_ns=9 * S, last_activity_ns=20 * S, end_time_ns=9 * S - 1_500_000)
    x = A.compute_features(info(ended))
    assert x == anref.features(info(ended), codes) == [0.0, -0.001, 10.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]   # -1.5 ms -> -1
    untimed = SessionStats(inbound_bytes=1 << 53, outbound_bytes=1, orig_pkts=1, resp_pkts=2, segment_count=4)
    x = A.compute_features(info(untimed, dst_port=40001, service="40001"))
    assert x == anref.features(info(untimed, dst_port=40001, service="40001"), codes)
    assert x[1] == x[4] == 0.0 and x[2] == float((1 << 53) + 1) == float(1 << 53) and x[7] == float(codes[40001])
    assert A.sanitize(float("nan")) == A.sanitize(float("inf")) == A.sanitize(float("-inf")) == 0.0 and A.sanitize(-2.5) == -2.5


def test_analyzer_state():
    a = A.SessionAnalyzer(seed=7)
    assert not a.train() and a.forest is None                                     # nothing to train on: no model
    a.add_session_data(F.vectors()[:1])
    a.add_session_data(F.vectors()[:1])
    assert not a.train()                                                           # one unique vector
    a.add_session_data(F.vectors())
    assert len(a.recent_data) == A.MAX_SAMPLES and a.recent_data[0] == F.vectors()[0].tolist()  # the two oldest fell out
    assert a.recent_data[-1] == F.vectors()[-1].tolist()
    assert a.train() and a.forest.n_trees == 25 and a.stats[2] is True
    assert (a.suspicious_threshold, a.abnormal_threshold) == A.compute_dynamic_thresholds(a.forest.score(a.recent_data))
    a.set_test_thresholds(0.60, 0.72)
    assert a.train() and (a.suspicious_threshold, a.abnormal_threshold) == (0.60, 0.72)
    S = 10 ** 9
    assert a.warming_up(100 * S) and a.warming_up(129 * S) and not a.warming_up(130 * S)
    a.disable_warmup_for_testing()
    assert not a.warming_up(101 * S)
    assert not A.SessionAnalyzer().warming_up(None)                                # no clock: no warm-up
