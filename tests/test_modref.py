"""tests/modref.py -- the restatement of last_modified, the fetch timestamps and the set rules -- driven by
the reference's four incremental known-answer tests (src/capture.rs:2522-3167) and by the rules one by one."""
import pytest

import modref
from modref import A, B, MS, S, T0, ModRef, ModRefWorld


@pytest.mark.parametrize("getter", modref.SCENARIOS)
def test_reference_incremental_scenarios(getter):
    assert modref.incremental_scenario(ModRefWorld(), getter) == T0 + 50 * MS


def test_fetch_timestamps_move_only_on_a_full_fetch_with_a_now():
    m = ModRef()
    m.packet(A, T0)
    assert m.fetch_ts == dict.fromkeys(modref.GETTER_SET, 0)
    m.get("sessions")                                   # full, no now: stays
    m.get("sessions", T0 + S, incremental=True)         # incremental: stays
    assert m.fetch_ts["sessions"] == 0
    m.get("sessions", T0 + S)
    assert m.fetch_ts == {"sessions": T0 + S, "current": 0, "blacklisted": 0, "exceptions": 0}  # each getter its own
    assert m.get("sessions", incremental=True) == [] and m.get("current", incremental=True) == [A]
    m.reset_fetch_timestamps()
    assert m.get("sessions", incremental=True) == [A]


def test_the_comparison_is_strict():
    m = ModRef()
    m.packet(A, T0)
    m.packet(B, T0 + 1)
    assert m.select("all", T0 - 1) == sorted([A, B])
    assert m.select("all", T0) == [B]        # last_modified == since: skipped; since + 1 ns: returned
    assert m.select("all", T0 + 1) == []


def test_what_stamps():
    m = ModRef()
    m.packet(A, T0)
    m.packet(B, T0)
    assert m.blacklist_pass(lambda k: 1 if k == A else 0) == ([A], [A])
    assert (m.s[A].stamp, m.s[B].stamp) == (0, 0)             # pass time 0: no stamp
    m.set_pass_time(T0 + S)
    assert m.blacklist_pass(lambda k: 1 if k == A else 0) == ([], [])
    assert m.s[A].stamp == 0                                    # nothing changed: nothing stamped
    m.s[A].wl_state = 0
    assert m.blacklist_pass(lambda k: 1 if k == A else 0) == ([], [A])
    assert m.s[A].stamp == T0 + S and m.s[B].stamp == 0         # the fallback's mark stamps
    m.set_pass_time(T0 + 2 * S)
    assert m.whitelist_pass(lambda k: modref.WL_NONCONFORMING) == [A, B]
    assert m.s[B].stamp == T0 + 2 * S
    m.set_pass_time(T0 + 3 * S)
    assert m.anomaly_pass(lambda k: (1, 0)) == [A, B]
    m.set_pass_time(T0 + 4 * S)
    assert m.anomaly_pass(lambda k: (1, 0)) == [] and m.s[A].stamp == T0 + 3 * S
    m.age(T0 + 5 * S)
    assert m.s[A].stamp == T0 + 3 * S and m.s[A].status != 0    # aging never stamps


def test_last_modified_is_the_later_of_packet_and_stamp():
    m = ModRef()
    m.packet(A, T0)
    m.set_pass_time(T0 - S)
    m.whitelist_pass(lambda k: 2)
    assert m.s[A].stamp == T0 - S and m.last_modified(A) == T0   # an older stamp loses
    m.set_pass_time(T0 + S)
    m.whitelist_pass(lambda k: 1)
    assert m.last_modified(A) == T0 + S                          # a newer one wins
    m.packet(A, T0 + 2 * S)
    assert m.last_modified(A) == T0 + 2 * S
    u = ModRef(timed=False)
    u.packet(A)
    u.set_pass_time(7)
    u.whitelist_pass(lambda k: 2)
    assert u.last_modified(A) == 7                               # untimed: the stamp alone
    with pytest.raises(ValueError):
        u.select("all", 0)


def test_set_rules():
    m = ModRef()
    for k in (A, B):
        m.packet(k, T0)
    assert m.select("current") == sorted([A, B])                 # a zero status byte is current
    assert m.select("blacklisted") == m.select("exceptions") == m.select("anomalous") == []
    m.packet(A, T0 + 200 * S)
    m.age(T0 + 200 * S)
    assert m.select("current") == [A]                            # B: 200 s idle, past the 180-s span
    m.set_pass_time(T0 + 201 * S)
    m.blacklist_pass(lambda k: 4 if k == B else 0, mark=False)
    m.whitelist_pass(lambda k: 2 | 4 if k == A else 1)
    m.anomaly_pass(lambda k: (2, 1) if k == A else (1, 0))
    assert (m.select("blacklisted"), m.select("exceptions"), m.select("anomalous")) == ([B], [A], [A])
    assert m.select("all", keep=lambda k: k == B) == [B]
    assert m.s[A].stamp == T0 + 201 * S
    assert m.age(T0 + 200 * S + 86401 * S) == [A, B]             # both idle past the retention span: purged
    m.packet(A, T0 + 10 ** 6 * S)
    assert m.s[A].stamp == 0                                     # a purged session that returns starts afresh
