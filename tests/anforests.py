"""Forests and input vectors shared by the anomaly tests (CPU and GPU): hand-built trees in the installed
format (IF_NODE_DTYPE nodes + tree offsets), the trained 25-tree forest, and vectors with the magnitudes
the walk has to survive.  Built once per process (functools.lru_cache) and never modified."""
import functools

import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.analyzer import Forest, train_forest

LEAF = N.FB_IF_LEAF


def make(trees, sample_size=128):
    """trees: [[(normal[10] or None, value, left, right), ...], ...] -> Forest."""
    nodes, first = [], [0]
    for t in trees:
        nodes += t
        first.append(len(nodes))
    arr = np.zeros(len(nodes), dtype=N.IF_NODE_DTYPE)
    for k, (normal, value, left, right) in enumerate(nodes):
        arr[k] = ([0.0] * 10 if normal is None else list(normal), value, left, right)
    return Forest(arr, first, sample_size)


def leaf(value):
    return (None, float(value), LEAF, LEAF)


@functools.lru_cache(None)
def vectors(n=300, seed=5):
    """n session-like vectors: durations, byte and packet counts, ratios, a few service codes."""
    rng = np.random.default_rng(seed)
    X = np.zeros((n, 10))
    X[:, 1] = np.round(rng.exponential(30.0, n), 3)
    X[:, 3] = rng.integers(1, 2000, n).astype(float)
    X[:, 2] = X[:, 3] * rng.integers(40, 1500, n)
    X[:, 4] = rng.choice([0.0, 0.25, 1.5, 7.125], n)
    X[:, 5] = rng.choice([0.0, 0.5, 2.0, 31.0], n) * rng.random(n)
    X[:, 6] = X[:, 2] / X[:, 3]
    X[:, 7] = rng.choice([0.0, 443951.0, 80112.0, 999999.0], n)
    X[:, 8] = (rng.random(n) < 0.1).astype(float)
    X[::17, 2] *= 4096.0   # a few outliers
    X[::23, 1] = -X[::23, 1]
    X.setflags(write=False)
    return X


@functools.lru_cache(None)
def special_vectors():
    """Huge and denormal magnitudes, -0.0, and a NaN (which must go right at every node)."""
    X = np.zeros((8, 10))
    X[0, :] = 1e300
    X[1, :] = -1e300
    X[2, :] = 5e-324
    X[3, :] = -0.0
    X[4, 2] = float("nan")
    X[5, :] = [1e308, -1e308, 1e-310, -1e-310, 0.0, -0.0, 1.0, -1.0, 2.0 ** 52, 3.0]
    X[6, :] = float("nan")
    X[7, :] = [float("inf"), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, float("-inf")]
    X.setflags(write=False)
    return X


@functools.lru_cache(None)
def inputs(n):
    """n vectors for the walk tests: the special ones first (as many as fit), then the session-like ones;
    inputs(n) is a prefix of inputs(1000)."""
    X = np.concatenate([special_vectors(), vectors(1000, seed=9)])[:n].copy()
    X.setflags(write=False)
    return X


@functools.lru_cache(None)
def trained():
    return train_forest(vectors(), seed=1234)


@functools.lru_cache(None)
def leaf_only():
    return make([[leaf(0.0)]], sample_size=1)


@functools.lru_cache(None)
def three_nodes():
    n = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    return make([[(n, 100000.0, 1, 2), leaf(1.25), leaf(2.5)]], sample_size=2)


def _random_tree(rng, depth, scale):
    """A complete tree of `depth` levels of internal nodes in breadth-first order (children 2i + 1, 2i + 2)."""
    inner = (1 << depth) - 1
    out = []
    for i in range(inner):
        normal = rng.standard_normal(10)
        out.append((normal.tolist(), float(rng.standard_normal() * scale), 2 * i + 1, 2 * i + 2))
    for i in range(inner + 1):
        out.append(leaf(depth + 0.125 * (i % 7)))
    return out


@functools.lru_cache(None)
def trees_64():
    rng = np.random.default_rng(64)
    return make([_random_tree(rng, 1 + t % 3, 1e4) for t in range(N.FB_IF_MAX_TREES)])


@functools.lru_cache(None)
def nodes_255():
    t = _random_tree(np.random.default_rng(255), 7, 3e4)
    assert len(t) == N.FB_IF_MAX_TREE_NODES
    return make([t])


@functools.lru_cache(None)
def chain_12():
    """Twelve internal nodes in a chain to the right, a leaf to the left of each: the last leaf is
    FB_IF_MAX_DEPTH below the root.  The splits test feature 3 against rising offsets."""
    d = N.FB_IF_MAX_DEPTH
    tree = []
    for k in range(d):
        n = [0.0] * 10
        n[3] = 1.0
        tree.append((n, 100.0 * (k + 1), d + k, k + 1 if k + 1 < d else 2 * d))
    tree += [leaf(k + 0.5) for k in range(d + 1)]
    return make([tree])


@functools.lru_cache(None)
def contraction_probe():
    """One split whose unfused dot product is 0 (left: 2^-61 is above it) and whose fused one is 2^-60
    (right); the leaves tell which."""
    n = [1.0, 1.0 + 2.0 ** -30] + [0.0] * 8
    x = np.array([[-(1.0 + 2.0 ** -29), 1.0 + 2.0 ** -30] + [0.0] * 8])
    return make([[(n, 2.0 ** -61, 1, 2), leaf(1.0), leaf(2.0)]], sample_size=2), x


ALL = {"leaf_only": leaf_only, "three_nodes": three_nodes, "trained": trained, "trees_64": trees_64,
       "nodes_255": nodes_255, "chain_12": chain_12}
