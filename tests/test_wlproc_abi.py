"""CPU-side checks of the process-aware whitelist ABI: the words that gained a second name
against the header, fb_set_l7_process_names' symbol and the argument errors that need no device, the name
interner, and the host compiler's process ids (Whitelists.compile / from_learned)."""
import os
import subprocess

import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.l7 import ProcessInterner, ProcessNameInterner
from flodbadd_amd.sessions import SessionL7
from flodbadd_amd.whitelists import Whitelists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_second_names_share_the_bytes_of_the_reserved_words(tmp_path):
    checks = [("fb_wl_endpoint", N.WL_ENDPOINT_DTYPE), ("fb_wl_endpoint", N.WL_ENDPOINT_PROC_DTYPE),
              ("fb_learned_endpoint", N.LEARNED_ENDPOINT_DTYPE), ("fb_learned_endpoint", N.LEARNED_ENDPOINT_PROC_DTYPE)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s/include/flodbadd_gpu.h"' % ROOT, "int main(void) {"]
    want = []
    for st, dt in checks:
        src.append('printf("%%zu\\n", sizeof(%s));' % st)
        want.append(dt.itemsize)
        for f in dt.names:
            src.append('printf("%%zu\\n", offsetof(%s, %s));' % (st, f))
            want.append(dt.fields[f][1])
    src.append('printf("%u\\n", (unsigned)FB_ABI_VERSION);')
    want.append(4)  # the change only adds to the ABI
    src.append("return 0; }")
    c = tmp_path / "wlproc.c"
    c.write_text("\n".join(src) + "\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "wlproc"), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "wlproc")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert N.WL_ENDPOINT_PROC_DTYPE.fields["process_match_id"][1] == N.WL_ENDPOINT_DTYPE.fields["reserved2"][1] == 36
    assert N.LEARNED_ENDPOINT_PROC_DTYPE.fields["proc_name_id"][1] == N.LEARNED_ENDPOINT_DTYPE.fields["reserved2"][1] == 52
    assert N.FB_ABI_VERSION == 4
    # the header compiles as C++ too (the anonymous members)
    cc = tmp_path / "wlproc.cpp"
    cc.write_text('#include "%s/include/flodbadd_gpu.h"\nint main() { fb_wl_endpoint e = {}; e.process_match_id = 1; '
                  'fb_learned_endpoint l = {}; l.reserved2[0] = 2; return e.reserved2 == 1 && l.proc_name_id == 2 ? 0 : 1; }\n'
                  % ROOT)
    subprocess.run(["g++", "-o", str(tmp_path / "wlproc_cc"), str(cc)], check=True)
    subprocess.run([str(tmp_path / "wlproc_cc")], check=True)


def test_symbol_is_exported_and_rejects_a_null_context():
    lib = N.gpu_lib()
    assert hasattr(lib, "fb_set_l7_process_names")
    one = np.ones(2, dtype=np.uint32)
    assert lib.fb_set_l7_process_names(None, None, None, 0) == N.FB_ERR_INVAL
    assert lib.fb_set_l7_process_names(None, N.ptr(one), N.ptr(one), 2) == N.FB_ERR_INVAL
    assert b"ctx" in lib.fb_last_error()


def test_name_interner():
    it = ProcessNameInterner()
    a, b, c = it.name_id("curl"), it.name_id("Curl"), it.name_id("nginx")
    assert (a, b, c) == (1, 2, 3) and it.name_id("curl") == 1 and it.names == {1: "curl", 2: "Curl", 3: "nginx"}
    assert it.match_id("curl") == it.match_id("CURL") == it.match_id("Curl") == 1 and it.match_id("nginx") == 2
    assert it.match_id("cürl") != it.match_id("cÜrl")  # ASCII case only (eq_ignore_ascii_case)
    ghost = it.match_id("ghost")                       # an endpoint's name no process has yet ...
    procs = ProcessInterner()
    for name in ("nginx", "Curl", "ghost"):
        procs.intern(SessionL7(10, name, "/bin/" + name, "u"))
    m, v = it.table(procs.processes)
    assert m.dtype == v.dtype == np.uint32 and m.tolist() == [0, 2, 1, ghost]  # ... keeps its id once one has it
    assert v.tolist() == [0, 3, 2, 4] and it.names[4] == "ghost"
    m0, v0 = it.table({})
    assert m0.tolist() == [0] and v0.tolist() == [0]


def model(eps):
    return {"date": "", "signature": None, "whitelists": [{"name": "w", "extends": None, "endpoints": eps}]}


def test_compile_process_ids():
    eps = [{"ip": "1.2.3.4", "process": "Curl"}, {"process": "curl"}, {"ip": "1.2.3.4"},
           {"domain": "*.example.com", "port": 443, "process": "nginx"}]
    w = Whitelists(model(eps))
    plain = w.compile("w", None, {"9.9.9.9": "a.example.com"})
    assert not plain.rows["reserved2"].any()  # without an interner the word stays 0
    it = ProcessNameInterner()
    rows = w.compile("w", None, {"9.9.9.9": "a.example.com"}, process_ids=it).rows
    ids = rows.view(N.WL_ENDPOINT_PROC_DTYPE)["process_match_id"].tolist()
    # rows: 0, 1, 2, then the row expanded from the domain ("same protocol, port and process") and the domain's own
    assert len(rows) == 5 and ids == [it.match_id("curl")] * 2 + [0] + [it.match_id("nginx")] * 2
    assert (rows[3]["flags"], int(rows[3]["addr"][0]), rows[3]["port"]) == (N.FB_WL_HAS_PORT | N.FB_WL_HAS_PROCESS, 0x09090909, 443)
    z = rows.copy()
    z["reserved2"] = 0
    assert z.tobytes() == plain.rows.tobytes()  # nothing else differs


def test_from_learned_process_names():
    recs = np.zeros(3, dtype=N.LEARNED_ENDPOINT_DTYPE)
    recs["family"], recs["protocol"], recs["dst_port"] = 2, 6, 443
    recs["dst_ip"][:, 0] = 0x08080808
    recs["reserved2"][:, 0] = [2, 0, 1]
    names = {1: "curl", 2: "Curl"}
    eps = Whitelists.from_learned(recs, None, names).whitelists["custom_whitelist"].endpoints
    assert [e.process for e in eps] == ["Curl", None, "curl"]
    assert [e.process for e in Whitelists.from_learned(recs).whitelists["custom_whitelist"].endpoints] == [None] * 3
