"""tests/histref.py, the Python restatement of the device history store, against naive string concatenation
over seeded random run sequences, with the store's accounting invariants after every step."""
import random

import pytest

import histref
from histref import BLOCK_CHARS, HIST_CHARS, HistStoreRef, blocks_of


def _check(store, naive):
    for key, want in naive.items():
        assert store.gather(key) == want, key
    info = store.info()
    assert info["blocks_in_use"] == sum(blocks_of(len(s)) for s in naive.values())
    assert info["chars"] == sum(len(s) for s in naive.values())
    assert info["flows"] == sum(1 for s in naive.values() if s)
    # every id is on the free stack or in exactly one chain
    seen = list(store.free)
    for e in store.flows.values():
        i = e[0]
        while i:
            seen.append(i)
            i = store.next[i]
    assert sorted(seen) == list(range(1, store.bump + 1))


def _run_of(rnd, n):
    return "".join(rnd.choice(HIST_CHARS) for _ in range(n))


@pytest.mark.parametrize("seed", range(6))
def test_random_runs_purges_and_reuse(seed):
    rnd = random.Random(seed)
    store, naive = HistStoreRef(), {}
    key_next = 0
    for step in range(60):
        keys = rnd.sample(range(key_next + 12), rnd.randrange(1, 12))
        key_next = max(key_next, max(keys) + 1)
        runs = [(k, _run_of(rnd, rnd.choice([1, 1, 2, 3, 7, 59, 60, 61, 119, 120, 121, 250]))) for k in keys]
        need = sum(blocks_of(len(naive.get(k, "")) + len(r)) - blocks_of(len(naive.get(k, ""))) for k, r in runs)
        free_before, hw_before = len(store.free), store.bump
        store.append(runs)
        for k, r in runs:
            naive[k] = naive.get(k, "") + r
        # reuse comes first: the high-water mark rises only by what the free stack could not give
        assert store.bump == hw_before + max(0, need - free_before)
        assert len(store.free) == max(0, free_before - need)
        _check(store, naive)
        if step % 7 == 6:
            gone = rnd.sample(sorted(naive), len(naive) // 2)
            freed = sum(blocks_of(len(naive[k])) for k in gone)
            free_before = len(store.free)
            store.purge(gone)
            for k in gone:
                del naive[k]
            assert len(store.free) == free_before + freed
            _check(store, naive)
            assert all(store.gather(k) == "" for k in gone)


@pytest.mark.parametrize("target", [1, 2, 119, 120, 121, 239, 240, 241, 361])
def test_block_edges_one_run_and_character_by_character(target):
    rnd = random.Random(target)
    want = _run_of(rnd, target)
    one, steps = HistStoreRef(), HistStoreRef()
    one.append([(0, want)])
    at = 0
    while at < target:  # 119 first, then 1 to 3 characters a time: every start nibble, every exact fill
        n = min(119 if at == 0 else 1 + (at % 3), target - at)
        steps.append([(0, want[at:at + n])])
        at += n
    for s in (one, steps):
        assert s.gather(0) == want and s.info()["blocks_in_use"] == blocks_of(target) == s.bump
    assert blocks_of(BLOCK_CHARS) == 1 and blocks_of(BLOCK_CHARS + 1) == 2 and blocks_of(0) == 0


def test_a_reused_block_does_not_leak_its_old_characters():
    store = HistStoreRef()
    store.append([(0, "S" * 120), (1, "a" * 7)])
    store.purge([0])
    store.append([(2, "F")])          # takes flow 0's block: one nibble written, the high nibble zeroed
    store.append([(2, "f")])          # an odd start: the read-modify-write keeps "F"
    assert store.gather(2) == "Ff" and store.gather(1) == "a" * 7 and store.bump == 2 and store.free == []
    store.clear()
    assert store.info() == dict(blocks_high_water=0, blocks_free=0, blocks_in_use=0, chars=0, flows=0)
    assert histref.BLOCK_BYTES == 60
