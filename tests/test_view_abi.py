"""CPU-side checks of the view export's C ABI: fb_flow_view and fb_view_query as the header lays them out
against the numpy dtypes of flodbadd_amd/_native.py, the constants, and the new symbols."""
import os
import subprocess

import numpy as np

from flodbadd_amd import _native as N
from flodbadd_amd.sessions import SessionInfo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the issue's table: field -> offset
VIEW_OFFSETS = {"rec": 0, "time": 136, "last_modified_ns": 200, "stamp_ns": 208, "bl_mask": 216, "an": 224,
                "status": 240, "wl_state": 241, "reserved": 242}
QUERY_OFFSETS = {"since_ns": 0, "set": 8, "filter": 12, "flags": 16, "reserved": 20}
CONSTANTS = {"FB_VIEW_ALL": 0, "FB_VIEW_CURRENT": 1, "FB_VIEW_BLACKLISTED": 2, "FB_VIEW_WL_EXCEPTIONS": 3,
             "FB_VIEW_ANOMALOUS": 4, "FB_VIEW_MODIFIED_SINCE": 1, "FB_DEBUG_VIEW_DIRECT": 3, "FB_ABI_VERSION": 4}


def test_structs_and_constants_match_the_header(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s/include/flodbadd_gpu.h"' % ROOT, "int main(void) {",
           'printf("%zu %zu\\n", sizeof(fb_flow_view), sizeof(fb_view_query));']
    want = [256, 24]
    for struct, dt, offsets in (("fb_flow_view", N.FLOW_VIEW_DTYPE, VIEW_OFFSETS),
                                ("fb_view_query", N.VIEW_QUERY_DTYPE, QUERY_OFFSETS)):
        assert list(dt.names) == list(offsets)
        for f in dt.names:
            assert dt.fields[f][1] == offsets[f], f
            src.append('printf("%%zu\\n", offsetof(%s, %s));' % (struct, f))
            want.append(offsets[f])
    # the nested records are the existing ones, and the reserved tail ends the record
    src.append('printf("%zu %zu %zu %zu\\n", sizeof(((fb_flow_view*)0)->rec), sizeof(((fb_flow_view*)0)->time), '
               'sizeof(((fb_flow_view*)0)->an), sizeof(((fb_flow_view*)0)->reserved));')
    want += [136, 64, 16, 14]
    for c, v in CONSTANTS.items():
        src.append('printf("%%u\\n", (unsigned)%s);' % c)
        want.append(v)
        assert getattr(N, c) == v
    src.append("return 0; }")
    c = tmp_path / "view.c"
    c.write_text("\n".join(src) + "\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "view"), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "view")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert N.FLOW_VIEW_DTYPE.itemsize == 256 and N.FLOW_VIEW_DTYPE.itemsize % 16 == 0
    assert N.VIEW_QUERY_DTYPE.itemsize == 24
    assert N.FLOW_VIEW_DTYPE.fields["rec"][0] == N.FLOW_REC_DTYPE
    assert N.FLOW_VIEW_DTYPE.fields["time"][0] == N.FLOW_TIME_DTYPE
    assert N.FLOW_VIEW_DTYPE.fields["an"][0] == N.AN_REC_DTYPE


def test_symbols_are_exported_and_reject_null_arguments():
    lib = N.gpu_lib()
    for name in ("fb_set_pass_time", "fb_flow_modified_dev", "fb_flow_export_view_dev", "fb_flow_export_view"):
        assert hasattr(lib, name), name
    q = np.zeros(1, dtype=N.VIEW_QUERY_DTYPE)
    assert lib.fb_set_pass_time(None, 1) == N.FB_ERR_INVAL
    assert lib.fb_flow_modified_dev(None, None, 0, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_export_view_dev(None, N.ptr(q), None, 0, None, None) == N.FB_ERR_INVAL
    assert lib.fb_flow_export_view(None, N.ptr(q), None, 0, None, None) == N.FB_ERR_INVAL


def test_session_info_has_last_modified():
    assert SessionInfo.__dataclass_fields__["last_modified_ns"].default == 0
