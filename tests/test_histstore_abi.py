"""CPU-side checks of the device history store's C ABI: the two new structs as the header lays them out against
the numpy dtypes of flodbadd_amd/_native.py, the constants, the new symbols in the built library and the new
entry points' argument checks (no device is needed for a NULL context)."""
import os
import subprocess

import numpy as np

from flodbadd_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "fb_hist_store_config": (N.HIST_STORE_CONFIG_DTYPE, 32,
                             {"block_capacity": 0, "max_blocks": 8, "flags": 16, "reserved": 20}),
    "fb_hist_store_info": (N.HIST_STORE_INFO_DTYPE, 64,
                           {"blocks_capacity": 0, "blocks_high_water": 8, "blocks_free": 16, "blocks_in_use": 24,
                            "chars": 32, "flows": 40, "appends": 48, "missed_updates": 56}),
}
NEW_SYMBOLS = ["fb_hist_store_enable", "fb_hist_store_append_dev", "fb_hist_store_lengths_dev",
               "fb_hist_store_gather_dev", "fb_hist_store_info_get", "fb_format_zeek_hist_dev"]


def test_structs_and_constants_match_the_header(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s/include/flodbadd_gpu.h"' % ROOT, "int main(void) {"]
    want = []
    for struct, (dt, size, offsets) in STRUCTS.items():
        assert list(dt.names) == list(offsets) and dt.itemsize == size, struct
        src.append('printf("%%zu\\n", sizeof(%s));' % struct)
        want.append(size)
        for f in dt.names:
            assert dt.fields[f][1] == offsets[f], (struct, f)
            src.append('printf("%%zu\\n", offsetof(%s, %s));' % (struct, f))
            want.append(offsets[f])
    consts = {"FB_ABI_VERSION": N.FB_ABI_VERSION, "FB_HIST_BLOCK_CHARS": N.FB_HIST_BLOCK_CHARS,
              "FB_HIST_COOP_RUN": N.FB_HIST_COOP_RUN, "FB_HIST_COOP_GATHER": N.FB_HIST_COOP_GATHER}
    for c, v in consts.items():
        src.append('printf("%%llu\\n", (unsigned long long)%s);' % c)
        want.append(v)
    src.append('printf("%zu %zu\\n", sizeof(fb_flow_view), sizeof(FB_HIST_CHARS) - 1); return 0; }')
    want += [256, 13]
    c = tmp_path / "histstore.c"
    c.write_text("\n".join(src) + "\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "histstore"), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "histstore")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert N.FB_ABI_VERSION == 4 and N.FB_HIST_BLOCK_CHARS == 120 and N.FLOW_VIEW_DTYPE.itemsize == 256
    # a lane's run starts at most one block; 13 characters + "none" fit a nibble
    assert 2 <= N.FB_HIST_COOP_RUN <= N.FB_HIST_BLOCK_CHARS


def test_symbols_are_bound_and_reject_a_null_context():
    lib = N.gpu_lib()
    bound = {n for n, _, _ in N.GPU_SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and hasattr(lib, name), name
    assert lib.fb_abi_version() == 4
    info = np.zeros(1, dtype=N.HIST_STORE_INFO_DTYPE)
    off = np.zeros(2, dtype=np.uint64)
    assert lib.fb_hist_store_enable(None, None) == N.FB_ERR_INVAL
    assert b"NULL" in lib.fb_last_error()
    assert lib.fb_hist_store_append_dev(None, None) == N.FB_ERR_INVAL
    assert lib.fb_hist_store_lengths_dev(None, None, 4, 1, N.ptr(off), None) == N.FB_ERR_INVAL
    assert lib.fb_hist_store_gather_dev(None, None, 4, 1, N.ptr(off), None, 0, None) == N.FB_ERR_INVAL
    assert lib.fb_hist_store_info_get(None, N.ptr(info)) == N.FB_ERR_INVAL
    assert lib.fb_format_zeek_hist_dev(None, None, 0, None, None, None, 0, None, None, None) == N.FB_ERR_INVAL
    assert not info.view(np.uint64).any()
