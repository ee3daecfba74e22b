"""CPU-side checks of the L7 pass's C ABI: the structs as the header lays them out against the numpy dtypes of
flodbadd_amd/_native.py, the constants, the argument checks that need no device, and the index -- the host
program tests/l7_index_host.cpp, built with the address and undefined-behaviour sanitizers, over every corpus of
tests/l7space.py against the list-scan restatement."""
import os
import subprocess

import numpy as np

import l7space as L
from flodbadd_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OFFSETS = {
    "fb_l7_socket": (N.L7_SOCKET_DTYPE, 48, {"local_ip": 0, "remote_ip": 16, "local_port": 32, "remote_port": 34,
                                             "protocol": 36, "local_family": 37, "remote_family": 38, "reserved0": 39,
                                             "reserved1": 40, "process_id": 44}),
    "fb_l7_rec": (N.L7_REC_DTYPE, 8, {"process_id": 0, "source": 4, "tries": 5, "reserved": 6}),
    "fb_l7_params": (N.L7_PARAMS_DTYPE, 16, {"max_retries": 0, "flags": 4, "reserved": 8}),
    "fb_l7_stats": (N.L7_STATS_DTYPE, 64, {"flows": 0, "current": 8, "looked_up": 16, "exact": 24, "fuzzy": 32,
                                           "failed": 40, "resolved": 48, "changed": 56}),
}
CONSTANTS = {"FB_L7_NONE": 0, "FB_L7_EXACT": 1, "FB_L7_FUZZY": 2, "FB_L7_FAILED": 3, "FB_L7_DEFAULT_MAX_RETRIES": 5,
             "FB_L7_MAX_SOCKETS": 1 << 22, "FB_ABI_VERSION": 4}


def test_structs_and_constants_match_the_header(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s/include/flodbadd_gpu.h"' % ROOT, "int main(void) {"]
    want = []
    for struct, (dt, size, offsets) in OFFSETS.items():
        assert list(dt.names) == list(offsets) and dt.itemsize == size
        src.append('printf("%%zu\\n", sizeof(%s));' % struct)
        want.append(size)
        for f in dt.names:
            assert dt.fields[f][1] == offsets[f], f
            src.append('printf("%%zu\\n", offsetof(%s, %s));' % (struct, f))
            want.append(offsets[f])
    for c, v in CONSTANTS.items():
        src.append('printf("%%u\\n", (unsigned)%s);' % c)
        want.append(v)
        assert getattr(N, c) == v
    src.append("return 0; }")
    c = tmp_path / "l7.c"
    c.write_text("\n".join(src) + "\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "l7"), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "l7")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert N.FB_L7_MAX_SOCKETS >= 1 << 20


def _one():
    a = L.socket_array([L.Sock(L.TCP, L.addr(L.V4, 1, 1), 80, L.addr(L.V4, 1, 2), 4000, 7)])
    return a


def test_invalid_arguments_are_errors():
    lib = N.gpu_lib()
    for name in ("fb_l7_validate", "fb_set_l7_sockets", "fb_flow_l7", "fb_flow_l7_dev", "fb_l7_clear", "fb_l7_lookup_dev"):
        assert hasattr(lib, name), name
    a = _one()
    assert lib.fb_set_l7_sockets(None, N.ptr(a), 1) == N.FB_ERR_INVAL
    assert lib.fb_flow_l7(None, None, None, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_l7_dev(None, None, 0, None) == N.FB_ERR_INVAL
    assert lib.fb_l7_clear(None) == N.FB_ERR_INVAL
    assert lib.fb_l7_lookup_dev(None, None, 0, None, None) == N.FB_ERR_INVAL
    # the snapshot's own checks (fb_set_l7_sockets runs them before it touches the installed snapshot)
    assert lib.fb_l7_validate(N.ptr(a), 1) == 0 and lib.fb_l7_validate(None, 0) == 0
    assert lib.fb_l7_validate(None, 1) == N.FB_ERR_INVAL
    assert lib.fb_l7_validate(N.ptr(a), N.FB_L7_MAX_SOCKETS + 1) == N.FB_ERR_INVAL  # (the count is checked first)
    bad = [("protocol", 1), ("protocol", 0), ("local_family", 0), ("local_family", 4), ("remote_family", 0),
           ("remote_family", 3), ("process_id", 0), ("reserved0", 1), ("reserved1", 1)]
    for f, v in bad:
        b = a.copy()
        b[0][f] = v
        assert lib.fb_l7_validate(N.ptr(b), 1) == N.FB_ERR_INVAL, (f, v)
        assert b"socket 0" in lib.fb_last_error()
    for f in ("local_ip", "remote_ip"):  # an IPv4 address lives in word 0 alone
        b = a.copy()
        b[0][f][2] = 1
        assert lib.fb_l7_validate(N.ptr(b), 1) == N.FB_ERR_INVAL, f
    u = a.copy()
    u[0]["protocol"] = 17
    for fam in (0, 2, 10):  # a UDP socket's remote side is ignored: 0 (none) or a family
        u[0]["remote_family"] = fam
        assert lib.fb_l7_validate(N.ptr(u), 1) == 0, fam
    two = np.concatenate([a, a])
    two[1]["process_id"] = 0
    assert lib.fb_l7_validate(N.ptr(two), 2) == N.FB_ERR_INVAL and b"socket 1" in lib.fb_last_error()
    assert lib.fb_l7_validate(N.ptr(two), 1) == 0


def test_sanitized_index_on_every_corpus():
    """The index build and l7_match of fb_l7_index.h in the sanitized host program: every flow of every corpus
    resolves as the list scan does, the tables hold the distinct keys, and an invalid snapshot is refused."""
    for c in [L.semantic()] + L.shapes() + list(L.ladder()[1:]):
        flows = c.flows or L.ladder()[0]
        status, n_pairs, n_locals, got = L.host_match(L.socket_array(c.socks), flows)
        assert status == 0, c.name
        tcp = [s for s in c.socks if s.proto == L.TCP and s.local[0] == s.remote[0]]
        assert n_pairs == len({(s.local, s.lport, s.remote, s.rport) for s in tcp}), c.name
        assert n_locals == len({(s.proto, s.local, s.lport) for s in c.socks}), c.name
        for f, g in zip(flows, got):
            assert g == L.resolve(c.socks, f), "%s: %s" % (c.name, L.describe(f))
    bad = _one()
    bad[0]["process_id"] = 0
    assert L.host_match(bad, [])[0] == 1
