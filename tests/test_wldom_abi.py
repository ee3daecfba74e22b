"""The C ABI of the device-side domain matching (include/flodbadd_gpu.h: fb_set_whitelist_dom, fb_wl_name_matches_dev,
fb_wl_dom_info_get, FB_DEBUG_WL_NAME_HASH_MASK): symbols, struct sizes and constants on the CPU; on the GPU every
refusal of fb_set_whitelist_dom -- each leaving the installed list as it was -- and the mask knob."""
import os
import subprocess

import numpy as np
import pytest

import wldomspace as D
from flodbadd_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_and_constants_match_the_header(tmp_path):
    checks = [("fb_wl_stats", N.WL_STATS_DOM_DTYPE, ("flows", "changed", "dom_overflow")),
              ("fb_wl_dom_info", N.WL_DOM_INFO_DTYPE, N.WL_DOM_INFO_DTYPE.names)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s/include/flodbadd_gpu.h"' % ROOT, "int main(void) {"]
    want = []
    for st, dt, fields in checks:
        src.append('printf("%%zu\\n", sizeof(%s));' % st)
        want.append(dt.itemsize)
        for f in fields:
            src.append('printf("%%zu\\n", offsetof(%s, %s));' % (st, f))
            want.append(dt.fields[f][1])
    src.append('printf("%zu\\n", offsetof(fb_wl_stats, reserved));')  # the old name of the same word
    want.append(N.WL_STATS_DTYPE.fields["reserved"][1])
    for c, v in (("FB_WL_MAX_GENERAL", N.FB_WL_MAX_GENERAL), ("FB_WL_NAME_MATCHES", N.FB_WL_NAME_MATCHES),
                 ("FB_DEBUG_WL_NAME_HASH_MASK", N.FB_DEBUG_WL_NAME_HASH_MASK), ("FB_ABI_VERSION", N.FB_ABI_VERSION)):
        src.append('printf("%%u\\n", (unsigned)%s);' % c)
        want.append(v)
    src.append("return 0; }")
    c = tmp_path / "wld.c"
    c.write_text("\n".join(src) + "\n")
    subprocess.run(["gcc", "-o", str(tmp_path / "wld"), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "wld")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert (N.FB_WL_MAX_GENERAL, N.FB_WL_NAME_MATCHES, N.FB_DEBUG_WL_NAME_HASH_MASK, N.FB_ABI_VERSION) == (1024, 8, 8, 4)
    assert N.WL_STATS_DOM_DTYPE.fields["dom_overflow"][1] == N.WL_STATS_DTYPE.fields["reserved"][1] == 40


def test_symbols_are_exported_and_reject_a_null_context():
    lib = N.gpu_lib()
    for name in ("fb_set_whitelist_dom", "fb_wl_name_matches_dev", "fb_wl_dom_info_get"):
        assert hasattr(lib, name), name
    assert lib.fb_set_whitelist_dom(None, None, 0, None, None, None, 0, None, None, 0) == N.FB_ERR_INVAL
    assert lib.fb_wl_name_matches_dev(None, None, 0, None, None, None) == N.FB_ERR_INVAL
    assert lib.fb_wl_dom_info_get(None, None) == N.FB_ERR_INVAL


def _rows(n, domain=True):
    r = np.zeros(n, dtype=N.WL_ENDPOINT_DTYPE)
    r["flags"] = N.FB_WL_HAS_DOMAIN if domain else 0
    return r


@pytest.mark.gpu
def test_every_refusal_leaves_the_installed_list():
    from flodbadd_amd.capture import FlodbaddGpuCapture
    from flodbadd_amd.sessions import SessionFilter
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9, service_bitmap=bytes(8192),
                             track_dns=True)
    lib = N.gpu_lib()
    try:
        D.track_names(cap, ["a.example.com", "gx-z"])
        ids = {s: i for i, s in D.stored_names(cap).items()}
        good = ["*.example.com", "never.org"]
        D.install_patterns(cap, good)

        def installed_is_intact():
            info = cap.whitelist_domain_info()
            assert (info["suffix"], info["exact"], info["general"]) == (1, 1, 0)
            assert cap.whitelist_name_matches([ids["a.example.com"], ids["gx-z"]])[0][:, 0].tolist() == [1, 0]

        def call(rows, epp, pats, off=None, n_patterns=None):
            blob, o = D.pattern_arrays(pats)
            o = o if off is None else np.array(off, dtype=np.uint64)
            return lib.fb_set_whitelist_dom(cap.ctx, N.ptr(rows) if len(rows) else None, len(rows),
                                            N.ptr(np.array(epp, dtype=np.uint32)) if epp is not None else None,
                                            N.ptr(blob) if len(blob) else None, N.ptr(o),
                                            len(pats) if n_patterns is None else n_patterns, None, None, 0)

        installed_is_intact()
        assert call(_rows(2), [1, 3], ["a", "b"]) == N.FB_ERR_INVAL           # an id above n_patterns
        installed_is_intact()
        assert call(_rows(1, domain=False), [1], ["a"]) == N.FB_ERR_INVAL      # an id without FB_WL_HAS_DOMAIN
        installed_is_intact()
        gen = ["g%d*z" % j for j in range(N.FB_WL_MAX_GENERAL + 1)]
        assert call(_rows(0), None, gen) == N.FB_ERR_INVAL                     # 1025 general patterns
        installed_is_intact()
        assert call(_rows(0), None, ["ab"], off=[0, 1 << 32]) == N.FB_ERR_INVAL  # 2^32 bytes of patterns
        installed_is_intact()
        assert call(_rows(0), None, ["ab"], off=[0, 2], n_patterns=1 << 24) == N.FB_ERR_INVAL  # 2^24 patterns
        installed_is_intact()
        assert call(_rows(0), None, ["ab", "c"], off=[0, 2, 1]) == N.FB_ERR_INVAL  # offsets that descend
        assert call(_rows(0), None, ["ab"], off=[1, 2]) == N.FB_ERR_INVAL          # ... or do not start at 0
        installed_is_intact()
        bad = _rows(1)
        bad[0]["family"] = 7
        assert call(bad, [1], ["a"]) == N.FB_ERR_INVAL                         # what fb_set_whitelist refuses
        installed_is_intact()
        # 1024 general patterns are a list; id 0 on a domain endpoint and a NULL ep_pattern are allowed
        assert call(_rows(2), [0, 1024], gen[:-1]) == N.FB_OK
        assert cap.whitelist_domain_info()["general"] == N.FB_WL_MAX_GENERAL
        assert call(_rows(2), None, ["a"]) == N.FB_OK
    finally:
        cap.close()


@pytest.mark.gpu
def test_the_mask_knob_rebuilds_the_tables_and_forgets_the_rows():
    from flodbadd_amd.capture import FlodbaddGpuCapture
    from flodbadd_amd.sessions import SessionFilter
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=1 << 9, service_bitmap=bytes(8192),
                             track_dns=True)
    lib = N.gpu_lib()
    try:
        names = ["a.example.com", "b.example.org", "example.com"]
        pats = ["*.example.com", "example.com", "b.*", "b*g"]
        D.track_names(cap, names)
        ask = [{s: i for i, s in D.stored_names(cap).items()}[n] for n in names]
        N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_WL_NAME_HASH_MASK, 0x3))  # before any list: kept for the next
        D.install_patterns(cap, pats)
        want = [D.expected_row(n, pats)[0] for n in names]
        assert cap.whitelist_name_matches(ask)[0].tolist() == want
        for mask in (1 << 63, 0, 0xFFFF0000):
            assert cap.whitelist_domain_info()["names_done"] == 3
            N.check(lib.fb_debug_set(cap.ctx, N.FB_DEBUG_WL_NAME_HASH_MASK, mask))
            info = cap.whitelist_domain_info()
            assert info["names_done"] == 0 and (info["exact"], info["suffix"], info["prefix"], info["general"]) == (1, 1, 1, 1)
            assert cap.whitelist_name_matches(ask)[0].tolist() == want
        assert lib.fb_debug_set(cap.ctx, 5, 0) == N.FB_ERR_INVAL  # (5 is still no knob)
    finally:
        cap.close()
