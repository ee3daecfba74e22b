"""The process-aware whitelist corpora and their expectation (tests/wlprocspace.py), pinned on the CPU: the census
of the enumerated classes, the literal scan on hand-written cases, and fb_wl_match.h -- the header the kernels
include -- compiled by a plain host compiler with the address and undefined-behaviour sanitizers into a
stand-alone program (tests/wl_match_host.cpp) that must print the expectation's state bytes for every corpus.
tests/test_gpu_wlprocspace.py holds the device to the same bytes."""
import os
import subprocess

import pytest

import wlprocspace as W
from flodbadd_amd.l7 import ProcessNameInterner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_census_every_class_holds_both_verdicts_where_the_rule_allows():
    world = W.WORLDS["semantic"]()
    seen = {}
    for case in W.semantic():
        shape, _, ep_proc = case.label
        for f, b in zip(world.flows, W.expected(world, case, W.N_NAMES)):
            seen.setdefault((shape, ep_proc, f.state), set()).add(b & 3)
    assert set(seen) == {(s, p, f) for s in W.SHAPES for p in W.EP_PROCS for f in W.FLOW_PROCS}
    for (shape, ep_proc, state), verdicts in sorted(seen.items()):
        want = {W.NONCONFORMING} | ({W.CONFORMING} if W.rule_allows_conforming(shape, ep_proc, state) else set())
        assert verdicts == want, (shape, ep_proc, state)
    # without an L7 plane, and without a name table, only process-less endpoints can conform
    for world, n in ((W.WORLDS["semantic_no_plane"](), W.N_NAMES), (W.WORLDS["semantic"](), 0)):
        for case in W.semantic():
            shape, _, ep_proc = case.label
            got = set(b & 3 for b in W.expected(world, case, n))
            assert (W.CONFORMING in got) == (shape != "domain_only" and ep_proc == "none"), (case.name, n)
    # the host-check bit appears, and only on NonConforming flows
    every = [b for c in W.semantic() for b in W.expected(W.WORLDS["semantic"](), c, W.N_NAMES)]
    assert {1, 2, 6} == set(every)
    # the run corpora: every size has a hit and a miss, the staged corpora sit on the thresholds
    rw = W.WORLDS["runs"]()
    for case in W.runs():
        got = set(W.expected(rw, case, W.N_NAMES))
        assert got == ({W.NONCONFORMING} if case.name == "run_0" else {W.CONFORMING, W.NONCONFORMING}), case.name
    assert [c.label for c in W.staging()] == [(512, 512), (513, 513), (512, 513), (513, 512)]
    assert len(W.corpora()) < 400 and all(len(W.WORLDS[w]().flows) <= 128 for w in W.WORLDS)


@pytest.mark.parametrize("k", range(len(W.HAND)))
def test_hand_written_expectations(k):
    ep, proc, installed, want = W.HAND[k]
    case = W.Case("hand", [ep])
    assert W.expected(W.HandWorld(proc), case, W.N_NAMES if installed else 0) == [want]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wlhost") / "wl_match_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Werror", "-o", exe, os.path.join(ROOT, "tests", "wl_match_host.cpp")], check=True)
    return exe


def test_host_program_prints_the_expectation_for_every_corpus(host_program, tmp_path):
    worlds = {}
    for k, (wname, case, n) in enumerate(W.corpora()):
        world = worlds.setdefault(wname, W.WORLDS[wname]())
        path = str(tmp_path / "c.bin")
        W.write_corpus(path, world, case, n, ProcessNameInterner())
        r = subprocess.run([host_program, path], capture_output=True, text=True)
        assert r.returncode == 0, (case.name, n, r.returncode, r.stderr[-2000:])
        lines = r.stdout.split("\n")
        assert lines[0] == "".join("%02x" % b for b in W.expected(world, case, n)), (wname, case.name, n)
        if case.name.startswith("staging_"):  # the index has the groups and rules the corpus claims
            assert tuple(int(x) for x in lines[1].split()[:2]) == case.label, case.name
