"""CPU-side checks of the session-aging boundary (fb_flow_age / fb_flow_status_dev): NULL contexts are
errors, the new structs' layouts match the numpy dtypes, and the host decoder reads a zero status byte
as the insert status."""
import os
import subprocess

import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.sessions import SessionStatus, flows_to_sessions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_context_is_an_error():
    lib = N.gpu_lib()
    st = np.zeros(1, dtype=N.AGE_STATS_DTYPE)
    assert lib.fb_flow_age(None, 1, None, N.FB_AGE_PURGE, N.ptr(st), None) == N.FB_ERR_INVAL
    assert lib.fb_flow_age(None, 1, None, 0, None, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_status_dev(None, None, 0, None) == N.FB_ERR_INVAL
    assert lib.fb_last_error()
    assert not st.view(np.uint64).any()  # nothing written


def test_age_struct_layouts_match_the_header(tmp_path):
    checks = [("fb_age_params", N.AGE_PARAMS_DTYPE), ("fb_age_stats", N.AGE_STATS_DTYPE)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s/include/flodbadd_gpu.h"' % ROOT,
           "int main(void) {"]
    want = []
    for st, dt in checks:
        src.append('printf("%%zu\\n", sizeof(%s));' % st)
        want.append(dt.itemsize)
        for f in dt.names:
            src.append('printf("%%zu\\n", offsetof(%s, %s));' % (st, f))
            want.append(dt.fields[f][1])
    src.append('printf("%u %u %u %u %u %u %u\\n", FB_AGE_PURGE, FB_STATUS_ACTIVE, FB_STATUS_ADDED, FB_STATUS_ACTIVATED,'
               ' FB_STATUS_DEACTIVATED, FB_STATUS_CURRENT, FB_STATUS_AGED); return 0; }')
    want += [N.FB_AGE_PURGE, N.STATUS_ACTIVE, N.STATUS_ADDED, N.STATUS_ACTIVATED, N.STATUS_DEACTIVATED,
             N.STATUS_CURRENT, N.STATUS_AGED]
    c = tmp_path / "lay.c"
    c.write_text("\n".join(src) + "\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "lay"), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "lay")], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got == want
    assert N.AGE_PARAMS_DTYPE.itemsize == 32 and N.AGE_STATS_DTYPE.itemsize == 128
    assert N.AGE_STATS_DTYPE.names[:9] == tuple(N.AGE_STATS_FIELDS)


def test_status_byte_decoding():
    """flows_to_sessions(status=...): byte 0 (never aged since insert) is the insert status
    (src/packets.rs:497-502: active, added, activated); other bytes decode bit by bit; without the
    bytes (untimed captures) the status is None."""
    flows = np.zeros(3, dtype=N.FLOW_REC_DTYPE)
    for i in range(3):
        flows[i]["src_ip"][0], flows[i]["dst_ip"][0] = 0x0A000001 + i, 0x08080808
        flows[i]["src_port"], flows[i]["dst_port"], flows[i]["protocol"], flows[i]["family"] = 1000 + i, 443, 6, 2
        flows[i]["end_seen"] = N.FB_SEEN_NONE
        flows[i]["slot"] = (5, 0, 9)[i]
    status = np.zeros(16, dtype=np.uint8)
    status[0] = N.STATUS_AGED | N.STATUS_DEACTIVATED | N.STATUS_CURRENT
    status[9] = N.STATUS_AGED | N.STATUS_ACTIVE | N.STATUS_ACTIVATED
    a, b, c = flows_to_sessions(flows, status=status)  # sorted by src_ip: slots 5, 0, 9
    assert a.status == SessionStatus(True, True, True, False) == SessionStatus.from_byte(0)
    assert b.status == SessionStatus(False, False, False, True)
    assert c.status == SessionStatus(True, False, True, False)
    assert all(i.status is None for i in flows_to_sessions(flows))
