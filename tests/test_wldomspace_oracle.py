"""The domain-matching corpora (tests/wldomspace.py) on the CPU: the "dot-candidate" forms the device evaluates against
the literal domain_matches over the whole enumerated space, the classification, the census of the corpora,
Whitelists.compile(domain_patterns=True), and the kernel's own header -- flodbadd_amd/csrc/fb_wl_domain.h built
with the address and undefined-behaviour sanitizers into tests/wl_domain_host.cpp -- which must print the
expectation's rows for every corpus under three hash masks.  tests/test_gpu_wldomspace.py holds the device to the
same rows."""
import os
import subprocess

import numpy as np
import pytest

import wldomspace as D
import wlprocspace as P
from flodbadd_amd import _native as N
from flodbadd_amd.l7 import ProcessNameInterner
from flodbadd_amd.whitelists import Whitelists, classify_domain_pattern, domain_matches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dot_candidate_forms_equal_domain_matches_on_the_whole_space():
    names, pats = D.exhaustive_names(), D.exhaustive_patterns()
    assert (len(names), len(pats)) == (1365, 121) and names[0] == "" and pats[0] == ""
    hits, most = 0, 0
    for n in names:
        mine = [D.dot_candidate_matches(n, p) for p in pats]
        assert mine == [domain_matches(n, p) for p in pats], n
        hits, most = hits + sum(mine), max(most, sum(mine))
    assert (len(names) * len(pats), hits, most) == (165165, 4702, 11)


def test_classification():
    want = {"": "exact", "a.b": "exact", "*.a": "suffix", "*.": "suffix", "*.*": "suffix", "*.a.*": "suffix", "*.a*": "suffix",
            "a.*": "prefix", ".*": "prefix", "a*.*": "prefix", "*": "general", "a*b": "general", "a.*.b": "general", "*a": "general",
            "a*": "general", "**": "never", "a*b*c": "never", "*a*": "never"}
    for p, k in want.items():
        assert classify_domain_pattern(p) == k, p
    assert set(want.values()) == set(D.KINDS)


def test_census_every_kind_has_hits_and_misses_in_the_corpora():
    seen = {}
    for label, pats in D.name_cases():
        if label.startswith("exhaustive"):
            continue
        names = [n for n in D.case_names(label)]
        for p in pats:
            k = classify_domain_pattern(p.lower())
            for n in names:
                seen.setdefault((k, domain_matches(n, p)), 0)
                seen[(k, domain_matches(n, p))] += 1
    for k in D.KINDS:
        assert seen.get((k, False)), k
        assert bool(seen.get((k, True))) == (k != "never"), k
    # the geometry: every length and dot placement the issue names
    lens = {len(n) for n in D.geometry_names()}
    assert {1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 252, 253, 254, 255} <= lens
    assert max(n.count(".") for n in D.geometry_names()) == 126
    assert any(n.startswith(".") for n in D.geometry_names()) and any(n.endswith(".") for n in D.geometry_names())
    # overflow: exactly eight and nine matches
    assert D.expected_row("m.o.example.com", D.OVERFLOW_PATTERNS) == (list(range(2, 10)), 1)
    assert D.expected_row("m.o.example.com", D.OVERFLOW_PATTERNS[2:10] + ["zz.nope"]) == (list(range(1, 9)), 0)
    assert D.expected_row("x.com", ["*.com"] * 12 + ["x.com"]) == (list(range(1, 9)), 1)
    assert len(D.all_names()) <= 1364 + 1200
    # the flow corpora decide something on every route
    wld = D.world()
    doms = {f: D.DOMAINS[f.dst] for f in wld.flows}
    verdicts = {}
    for case in D.flow_cases():
        st, over = D.expected(wld.flows, doms, wld, case, P.N_NAMES)
        if case.label:
            verdicts.setdefault(case.label[2], set()).update(st)
        if case.name == "overflow_9":
            assert over == sum(1 for f in wld.flows if (f.dst, f.proto, f.dport) == (D.A6, "TCP", 443)) and over
        elif case.name == "overflow_8":
            assert over == 0 and st[[f.dst for f in wld.flows].index(D.A6)] == P.CONFORMING
        else:
            assert over == 0 or case.name.startswith("overflow"), case.name
    for pn in ("exact", "exact_case", "suffix", "prefix", "general"):
        assert P.CONFORMING in verdicts[pn] and P.NONCONFORMING in verdicts[pn], pn
    assert verdicts["never"] <= {P.NONCONFORMING, P.NONCONFORMING | P.HOST_CHECK, P.CONFORMING}
    assert P.NONCONFORMING | P.HOST_CHECK in verdicts["suffix"]  # (the endpoints without a pattern id)


def test_compile_with_domain_patterns():
    eps = [{"domain": "*.Example.COM", "port": 443}, {"ip": "1.2.3.4"}, {"domain": "*.example.com", "ip": "5.6.7.8"},
           {"domain": "Straße.de"}, {"domain": "a*b"}, {"domain": "x.*", "process": "curl"}]
    m = {"date": "", "signature": None, "whitelists": [{"name": "w", "extends": None, "endpoints": eps}]}
    c = Whitelists(m).compile("w", domain_patterns=True, process_ids=ProcessNameInterner())
    assert c.patterns == ["*.example.com", "straße.de", "a*b", "x.*"]
    assert c.ep_pattern.dtype == np.uint32 and c.ep_pattern.tolist() == [1, 0, 1, 2, 3, 4]
    assert len(c.rows) == len(eps)  # no expansion
    assert c.pattern_off.dtype == np.uint64 and c.pattern_off.tolist() == [0, 13, 23, 26, 29]
    assert bytes(c.pattern_bytes) == "*.example.comstraße.dea*bx.*".encode("utf-8")
    assert [bool(r["flags"] & N.FB_WL_HAS_DOMAIN) for r in c.rows] == [True, False, True, True, True, True]
    assert c.rows[5]["reserved2"] != 0
    with pytest.raises(ValueError):
        Whitelists(m).compile("w", dns_resolutions={"1.2.3.4": "a.example.com"}, domain_patterns=True)
    # the default mode is what it was: no pattern table, the expansion
    d = Whitelists(m).compile("w", dns_resolutions={"9.9.9.9": "a.example.com"})
    assert d.ep_pattern is None and d.patterns is None and len(d.rows) == len(eps) + 2
    # general patterns past the FB_WL_MAX_GENERAL-th distinct one are left to the host, in list order
    many = [{"domain": "g%d*z" % j} for j in range(N.FB_WL_MAX_GENERAL + 3)] + [{"domain": "g0*z"}, {"domain": "tail.com"}]
    m["whitelists"][0]["endpoints"] = many
    c = Whitelists(m).compile("w", domain_patterns=True)
    ids = c.ep_pattern.tolist()
    assert ids[:N.FB_WL_MAX_GENERAL] == list(range(1, N.FB_WL_MAX_GENERAL + 1))
    assert ids[N.FB_WL_MAX_GENERAL:] == [0, 0, 0, 1, N.FB_WL_MAX_GENERAL + 1]
    assert len(c.patterns) == N.FB_WL_MAX_GENERAL + 1


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wldomhost") / "wl_domain_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Werror", "-o", exe, os.path.join(ROOT, "tests", "wl_domain_host.cpp")], check=True)
    return exe


def run_host(host_program, path):
    r = subprocess.run([host_program, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.split("\n")


def test_host_program_prints_the_expectation_for_every_corpus(host_program, tmp_path):
    path = str(tmp_path / "c.bin")
    for label, pats in D.name_cases():
        names = D.case_names(label)
        D.write_corpus(path, names, pats)
        lines = run_host(host_program, path)
        kinds = [classify_domain_pattern(p.lower()) for p in pats]
        assert lines[0].split() == [str(kinds.count(k)) for k in D.KINDS], label
        rows, flags = D.expected_rows(names, pats)
        got = np.array([[int(x, 16) for x in ln.split()] for ln in lines[1:1 + len(names)]], dtype=np.uint32)
        assert got.shape == (len(names), D.ROW + 1), label
        bad = np.nonzero((got[:, :D.ROW] != rows).any(axis=1) | (got[:, D.ROW] != flags))[0]
        assert len(bad) == 0, (label, [(names[i], got[i].tolist(), rows[i].tolist(), int(flags[i])) for i in bad[:4]])


def test_host_program_refuses_what_the_abi_refuses(host_program, tmp_path):
    path = str(tmp_path / "c.bin")
    D.write_corpus(path, ["gx-z"], ["g%d*z" % j for j in range(N.FB_WL_MAX_GENERAL)])
    assert run_host(host_program, path)[0].split()[3] == str(N.FB_WL_MAX_GENERAL)
    D.write_corpus(path, ["gx-z"], ["g%d*z" % j for j in range(N.FB_WL_MAX_GENERAL + 1)])
    assert run_host(host_program, path)[0] == "invalid"
