"""The DNS tracker on the device (fb_dns_track_dev & co.) against DnsResolver.process over the same parsed
arrays: after EVERY call the pending queries, the resolutions and the name each response took are compared
(dnstrackgen.step).  Each test builds its own small context."""
import ipaddress
import random

import numpy as np
import pytest

import dnsgen as G
import dnstrackgen as T
from flodbadd_amd import _native as N
from flodbadd_amd.dns import DnsResolver, parse_dns

pytestmark = pytest.mark.gpu

S = 10**9


def test_hand_cases():
    cap, ref = T.new_capture()
    try:
        # query then response in one batch
        st = T.step(cap, ref, T.Batch().query(1, "a.example").response(1, ["192.0.2.1"]))
        assert (st["queries"], st["responses"], st["matched"], st["resolutions"], st["names_new"], st["addrs_new"]) == \
            (1, 1, 1, 1, 1, 1)
        # query in call k, response in call k + 1
        T.step(cap, ref, T.Batch().query(2, "b.example"))
        assert ref.pending == {2: "b.example"}
        T.step(cap, ref, T.Batch().response(2, ["192.0.2.2"]))
        assert ref.pending == {}
        # a response with no query
        st = T.step(cap, ref, T.Batch().response(3, ["192.0.2.3"]))
        assert st["matched"] == 0 and st["resolutions"] == 0
        # two queries on one id then one response: the second name wins
        T.step(cap, ref, T.Batch().query(4, "first.example").query(4, "second.example").response(4, ["192.0.2.4"]))
        assert ref.resolutions[ipaddress.ip_address("192.0.2.4")] == "second.example"
        # two responses in a row: the second gets nothing
        st = T.step(cap, ref, T.Batch().query(5, "c.example").response(5, ["192.0.2.5"]).response(5, ["192.0.2.55"]))
        assert st["matched"] == 1
        # a reverse or question-less query between a query and its response does not disturb pending
        T.step(cap, ref, T.Batch().query(6, "d.example").reverse(6).no_question(6).response(6, ["192.0.2.6"]))
        T.step(cap, ref, T.Batch().query(7, "e.example"))
        T.step(cap, ref, T.Batch().reverse(7).no_question(7))
        T.step(cap, ref, T.Batch().response(7, ["192.0.2.7"]))
        # a rejected message is skipped (query and response)
        T.step(cap, ref, T.Batch().query(8, "f.example").rejected(8, query=True).rejected(8, query=False, addrs=["192.0.2.80"])
               .response(8, ["192.0.2.8"]))
        # a response without answers still consumes pending
        st = T.step(cap, ref, T.Batch().query(9, "g.example").response(9, []).response(9, ["192.0.2.9"]))
        assert st["matched"] == 1 and st["resolutions"] == 0
        # one address resolved to two names: the later packet wins, within a call and across calls
        T.step(cap, ref, T.Batch().query(10, "old.example").query(11, "new.example").response(10, ["192.0.2.10"])
               .response(11, ["192.0.2.10"]))
        T.step(cap, ref, T.Batch().query(11, "new.example").query(10, "old.example").response(11, ["192.0.2.10"])
               .response(10, ["192.0.2.10"]))
        T.step(cap, ref, T.Batch().query(12, "newest.example").response(12, ["192.0.2.10"]))
        # v4 and v6, and a v4 and a v6 key whose first word is equal
        T.step(cap, ref, T.Batch().query(13, "v4.example").query(14, "v6.example").response(13, ["32.1.13.184"])
               .response(14, ["2001:db8::", "2001:db8::1"]))
        assert len({k.version for k in ref.resolutions}) == 2
        # 8 answers
        T.step(cap, ref, T.Batch().query(15, "eight.example").response(15, ["198.51.100.%d" % i for i in range(8)]))
        assert len(ref.resolutions) == cap.dns_track_info()["addrs"]
    finally:
        cap.close()


def test_twelve_answers_through_the_parse():
    """The parse keeps 8 of 12 answers; the tracker maps exactly those."""
    cap, ref = T.new_capture()
    try:
        wire = [G.query(6, "many.example"), G.response(6, "many.example", [("A", "10.0.%d.%d" % (i // 7, i)) for i in range(12)])]
        buf = np.frombuffer(b"".join(wire), dtype=np.uint8)
        recs = np.zeros(2, dtype=N.DNS_OUT_DTYPE)
        recs[0] = (0, 0, len(wire[0]), 17, 2, 0)
        recs[1] = (1, len(wire[0]), len(wire[1]), 17, 2, 0)
        parsed = parse_dns(buf, recs)
        assert int(parsed[0][1]["n_addrs"]) == 8 and int(parsed[0][1]["flags"]) & N.DNS_ADDRS_TRUNCATED
        st = T.step(cap, ref, parsed)
        assert st["resolutions"] == 8 and len(ref.resolutions) == 8
        # the capture's own path (records -> parse -> track, device to device) gives the same state
        cap2, _ = T.new_capture()
        try:
            cap2.track_dns_records(buf, recs)
            T.check_state(cap2, ref)
        finally:
            cap2.close()
    finally:
        cap.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 257, 4097])
def test_boundaries(n):
    cap, ref = T.new_capture()
    try:
        rnd = random.Random(n)
        T.step(cap, ref, T.Batch().query(7, "carried.example"))
        b = T.Batch()
        for i in range(n):
            tx = rnd.randrange(16)
            if rnd.random() < 0.5:
                b.query(tx, "n%d.example" % rnd.randrange(24))
            else:
                b.response(tx, ["203.0.%d.%d" % (rnd.randrange(2), rnd.randrange(40))])
        st = T.step(cap, ref, b)
        assert st["messages"] == n
    finally:
        cap.close()


def test_stats_n_dns_below_n():
    cap, ref = T.new_capture()
    try:
        b = T.Batch().query(1, "in.example").response(1, ["192.0.2.1"]).query(2, "in2.example").query(3, "out.example") \
            .response(2, ["192.0.2.2"])
        st = T.step(cap, ref, b, n_dns=3)
        assert st["messages"] == 3 and ref.pending == {2: "in2.example"}
    finally:
        cap.close()


def test_contention_one_transaction_id():
    cap, ref = T.new_capture()
    try:
        b = T.Batch()
        for i in range(4097):
            if i % 2 == 0:
                b.query(77, "alt%d.example" % (i % 10))
            else:
                b.response(77, ["198.18.0.%d" % (i % 5)])
        st = T.step(cap, ref, b)
        assert st["matched"] == 2048 and ref.pending == {77: "alt6.example"}
    finally:
        cap.close()


def test_contention_one_name():
    cap, ref = T.new_capture()
    try:
        b = T.Batch()
        for i in range(4097):
            b.query(i, "same.example", garbage=i & 0xFF)
        st = T.step(cap, ref, b)
        assert st["names_new"] == 1 and cap.dns_track_info()["names"] == 1 and len(ref.pending) == 4097
    finally:
        cap.close()


def test_contention_one_address():
    cap, ref = T.new_capture(dns_name_capacity=4096)
    try:
        b = T.Batch()
        for i in range(2048):
            b.query(i, "q%d.example" % i)
        for i in range(2048):
            b.response(i, ["198.18.7.7"])
        b.query(5, "last.example")
        st = T.step(cap, ref, b)
        assert st["addrs_new"] == 1 and cap.dns_track_info()["addrs"] == 1
        assert list(ref.resolutions.values()) == ["q2047.example"]
    finally:
        cap.close()


def test_name_edge_cases():
    cap, ref = T.new_capture()
    try:
        long_a, long_b = "x" * 254 + "a", "x" * 254 + "b"  # lengths 255, equal up to the last byte
        names = ["abcdefg1", "abcdefg2", "abcd", "abcde", "abcdef", "a", long_a, long_b, "Case.Example", "case.example"]
        b = T.Batch()
        for i, nm in enumerate(names):
            b.query(i, nm, garbage=0xEE)
        # the same bytes followed by different garbage past name_len: one id
        b.query(100, "garbage.example", garbage=0x00).query(101, "garbage.example", garbage=0xFF) \
            .query(102, "garbage.example", garbage=0x41)
        for i in range(len(names)):
            b.response(i, ["192.0.2.%d" % i])
        st = T.step(cap, ref, b)
        assert st["names_new"] == len(names) + 1
        ids, _ = cap.dns_pending_ids()
        assert int(ids[100]) != 0 and int(ids[100]) == int(ids[101]) == int(ids[102])
        # the same names again, other garbage: nothing new
        b2 = T.Batch()
        for i, nm in enumerate(names):
            b2.query(200 + i, nm, garbage=0x7F)
        st = T.step(cap, ref, b2)
        assert st["names_new"] == 0
        assert sorted(cap.dns_names(range(1, len(names) + 2)).values()) == sorted(names + ["garbage.example"])
        assert cap.dns_names([0, 9999]) == {9999: ""}  # an unknown id: length 0
    finally:
        cap.close()


def test_forced_tag_collisions():
    """hash_mask = 0x7: 64 names and 64 addresses over 8 tags -- every id still names its own string, the
    result equals the comparator's, and the insert loop needs more than two rounds."""
    cap, ref = T.new_capture(dns_hash_mask=0x7)
    try:
        b = T.Batch()
        for i in range(64):
            b.query(i, "collide-%02d.example" % i)
        for i in range(64):
            b.response(i, ["2001:db8::%x" % i if i % 2 else "198.51.100.%d" % i])
        st = T.step(cap, ref, b)
        assert st["rounds"] > 2 and st["names_new"] == 64 and st["addrs_new"] == 64
        names = cap.dns_names(range(1, 65))
        assert [names[i] for i in range(1, 65)] == ["collide-%02d.example" % i for i in range(64)]  # first-message order
        got = cap.dns_resolutions()
        assert got == ref.resolutions and len(got) == 64
        # a second call finds every name and address where the first left it
        st = T.step(cap, ref, b)
        assert st["names_new"] == 0 and st["addrs_new"] == 0
        assert (cap.dns_lookup(list(ref.resolutions)) != 0).all() and int(cap.dns_lookup(["203.0.113.1"])[0]) == 0
    finally:
        cap.close()


def test_randomised():
    cap, ref = T.new_capture()
    try:
        rnd = random.Random(20240611)
        names = ["host-%d.zone%d.example" % (i, i % 7) for i in range(200)]
        addrs = ["10.%d.%d.1" % (i // 200, i % 200) if i % 3 else "2001:db8:%x::1" % i for i in range(300)]
        for call in range(3):
            b = T.Batch()
            for i in range(20000):
                tx, r = rnd.randrange(64), rnd.random()
                if r < 0.04:
                    b.rejected(tx, query=rnd.random() < 0.5)
                elif r < 0.07:
                    b.reverse(tx)
                elif r < 0.10:
                    b.no_question(tx)
                elif r < 0.55:
                    b.query(tx, rnd.choice(names), garbage=rnd.randrange(256))
                else:
                    b.response(tx, rnd.sample(addrs, rnd.randrange(0, 5)))
            T.step(cap, ref, b)
        info = cap.dns_track_info()
        assert info["names"] <= 200 and info["addrs"] == len(ref.resolutions) and info["messages"] == 60000
        assert info["pending"] == len(ref.pending)
    finally:
        cap.close()


def test_growth_keeps_ids():
    cap, ref = T.new_capture(dns_name_capacity=64, dns_addr_capacity=64)
    try:
        seen = {}
        for call in range(4):
            b = T.Batch()
            for i in range(250):
                k = call * 250 + i
                b.query(k % 997, "grow-%04d.example" % k)
                b.response(k % 997, ["172.16.%d.%d" % (k // 250, k % 250), "2001:db8:1::%x" % k])
            T.step(cap, ref, b)
            names = cap.dns_names(range(1, cap.dns_track_info()["names"] + 1))
            cap._dns_names = {}  # read the strings from the device again after each (possibly grown) call
            fresh = cap.dns_names(range(1, len(names) + 1))
            assert fresh == names
            for i, s in seen.items():
                assert fresh[i] == s  # ids handed out before a growth still name the same strings
            seen = dict(fresh)
        info = cap.dns_track_info()
        assert info["names"] == 1000 and info["addrs"] == 2000 and info["name_capacity"] >= 1000 > 64
    finally:
        cap.close()


def test_expiry():
    cap, ref = T.new_capture()
    try:
        t = 1_700_000_000 * S
        b = T.Batch().query(1, "t0.example").query(2, "t20.example").query(3, "t40.example")
        T.step(cap, ref, b, ts=[t, t + 20 * S, t + 40 * S])
        T.step(cap, ref, T.Batch().query(4, "untimed.example"))  # stored without times: never expires
        assert cap.expire_dns(t + 45 * S) == 1
        ref.expire([1])
        T.check_state(cap, ref)
        _, times = cap.dns_pending_ids()
        assert int(times[2]) == t + 20 * S and int(times[4]) == N.FB_DNS_NO_TIME
        assert cap.expire_dns(t + 50 * S - 1) == 0 and cap.expire_dns(t + 50 * S) == 1  # age >= 30 s goes
        ref.expire([2])
        T.check_state(cap, ref)
        assert cap.expire_dns(t + 10**6 * S) == 1 and cap.dns_pending() == {4: "untimed.example"}
    finally:
        cap.close()


def test_enable_and_clear():
    from flodbadd_amd.capture import FlodbaddGpuCapture
    lib = N.gpu_lib()
    off = FlodbaddGpuCapture(0, flow_capacity=0)
    try:
        assert lib.fb_dns_track_dev(off.ctx, None, None, None, 0, None, None, None, None, None) == N.FB_ERR_INVAL
        assert lib.fb_dns_track_clear(off.ctx) == N.FB_ERR_INVAL
        assert lib.fb_dns_expire(off.ctx, 0, None) == N.FB_ERR_INVAL
        assert lib.fb_dns_lookup_dev(off.ctx, None, 0, None, None) == N.FB_ERR_INVAL
        bad = np.zeros(1, dtype=N.DNS_TRACK_CONFIG_DTYPE)
        bad[0]["reserved"] = 1
        assert lib.fb_dns_track_enable(off.ctx, N.ptr(bad)) == N.FB_ERR_INVAL
        bad[0]["reserved"], bad[0]["flags"] = 0, 1
        assert lib.fb_dns_track_enable(off.ctx, N.ptr(bad)) == N.FB_ERR_INVAL
        assert lib.fb_dns_track_enable(off.ctx, None) == N.FB_OK  # NULL: the defaults
        assert lib.fb_dns_track_enable(off.ctx, None) == N.FB_ERR_INVAL  # already enabled
    finally:
        off.close()
    cap, ref = T.new_capture()
    try:
        T.step(cap, ref, T.Batch().query(1, "a.example").response(1, ["192.0.2.1"]).query(2, "b.example"))
        d = N.DeviceBuffer(1024)
        assert lib.fb_dns_track_dev(cap.ctx, d.ptr, d.ptr.value + 2, d.ptr, 1, None, None, None, None, None) == N.FB_ERR_INVAL
        cap.clear_dns()
        info = cap.dns_track_info()
        assert (info["names"], info["addrs"], info["pending"], info["messages"]) == (0, 0, 0, 0)
        assert cap.dns_pending() == {} and cap.dns_resolutions() == {}
        ref = DnsResolver()
        T.step(cap, ref, T.Batch().response(2, ["192.0.2.2"]).query(3, "c.example").response(3, ["192.0.2.1"]))
        assert cap.dns_names([1]) == {1: "c.example"}
    finally:
        cap.close()
