"""The session corpora of the endpoint learning tests (tests/test_learn_oracle.py on the CPU, tests/
test_gpu_learn.py on the device): lists of (protocol, src_ip, src_port, dst_ip, dst_port).  Source ports are
ones the service table does not name, so the table keeps every key as given (src/packets.rs:245-253)."""
import ipaddress

GROUP_SIZES = (1, 2, 63, 64, 65, 256, 257)


def group(size, dst="203.0.113.77", dport=443, proto="TCP", base=0):
    """`size` sessions of one fingerprint: sources 10.7.x.y, ports 61000 + ..."""
    return [(proto, "10.7.%d.%d" % ((base + i) >> 8, (base + i) & 255), 61000 + (base + i) % 300, dst, dport)
            for i in range(size)]


def one_field_apart():
    """Pairs of endpoints that differ in exactly one thing: each dst_ip word (IPv6), the port, the protocol, the
    family (an IPv4 address and an IPv6 address with the same word 0).  (The pair that differs in the name id
    alone needs the tracker's state: tests/test_gpu_learn.py builds it.)"""
    v6 = "2001:db8:1:2:3:4:5:6"
    w = int(ipaddress.ip_address(v6))
    out = [("TCP", "fd00::9", 61001, v6, 443)]
    for k in range(4):  # one bit of word k flipped
        out.append(("TCP", "fd00::9", 61002 + k, str(ipaddress.ip_address(w ^ (1 << (96 - 32 * k)))), 443))
    out += [("TCP", "10.8.0.1", 61010, "198.51.100.20", 443), ("TCP", "10.8.0.1", 61011, "198.51.100.20", 444),
            ("UDP", "10.8.0.1", 61012, "198.51.100.20", 443)]
    # 0x20010db8 = 32.1.13.184: the IPv4 address whose word 0 is the IPv6 address's
    out += [("TCP", "10.8.0.2", 61013, "32.1.13.184", 443), ("TCP", "fd00::a", 61014, "2001:db8::", 443)]
    return out


def representatives():
    """Groups whose members' order is decided late: IPv6 sources that differ only in the last word, IPv6 and
    IPv4 sources that differ only in the port; and groups of eight members spread over the table, so that the
    least session of some sits in a higher slot than another member."""
    out = []
    for k in (5, 3, 9, 1, 7):  # the last word alone orders them (1 is least)
        out.append(("TCP", "fd00::1:%x" % k, 61100, "2001:db8::50", 443))
    for p in (61207, 61203, 61209, 61201):  # the port alone
        out.append(("TCP", "fd00::2", p, "2001:db8::51", 443))
        out.append(("UDP", "10.9.0.1", p, "198.51.100.51", 53000))
    for k in (2, 1):  # words 0-1 equal, words 2-3 decide, the port disagrees with them
        out.append(("TCP", "fd00::%x:0:1" % k, 61300 - k, "2001:db8::52", 443))
    for g in range(8):
        for m in range(8):
            out.append(("TCP", "10.9.%d.%d" % (1 + (m * 5) % 8, 10 + g), 61400 + (m * 3) % 8, "198.51.100.%d" % (60 + g), 8443))
    return out


def distinct(n, v6_every=5):
    """n distinct endpoints, one session each (every v6_every-th over IPv6)."""
    out = []
    for i in range(n):
        if i % v6_every == 0:
            out.append(("TCP", "fd00::3", 61500 + i % 200, "2001:db8:2::%x" % (i + 1), 443))
        else:
            out.append(("UDP" if i % 3 == 0 else "TCP", "10.10.0.1", 61500 + i % 200, "192.0.2.%d" % (i % 250 + 1),
                        7000 + i // 250))
    return out


def mixed_local():
    """Local and global destinations, several sessions per endpoint (the selection tests)."""
    out = []
    for i in range(60):
        out.append(("TCP", "10.11.0.%d" % (i + 1), 61600 + i, "10.11.1.%d" % (i % 6 + 1), 8080))        # local
        out.append(("TCP", "10.11.0.%d" % (i + 1), 61700 + i, "198.51.100.%d" % (100 + i % 10), 443))   # global
    return out


def dns_for(corpus):
    """{ip: domain} for every third destination of a corpus, the literals Unknown / Resolving among them."""
    dsts = sorted({c[3] for c in corpus})
    names = {}
    for k, d in enumerate(dsts[::3]):
        names[d] = ("Unknown", "Resolving")[k % 2] if k % 7 == 3 else "host%d.example" % k
    return names


ALL = {"one_field_apart": one_field_apart, "representatives": representatives, "distinct_40": lambda: distinct(40),
       "distinct_300": lambda: distinct(300), "mixed_local": mixed_local}
ALL.update({"group_%d" % n: (lambda n=n: group(n)) for n in GROUP_SIZES})
