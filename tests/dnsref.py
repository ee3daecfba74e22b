"""A second restatement of the DNS divert parse (test helper, no tests), plain Python over `bytes`.

Written from the rules as DESIGN §3.6 and the header comment of flodbadd_amd/csrc/fb_dns.hip state
them (dns-parser 0.8.0's Packet::parse, parity unpinned: the crate is not in the reference mount),
not from oracle/oracle.c or the kernel, and shaped differently on purpose: rejections are
exceptions, a cursor walks the message by absolute offsets, a name's pointer rule is checked
against the list of every earlier target, and Display is built iteratively from the name's
segments (the labels between two jumps) instead of by recursion.

    parse_fields(msg, pkt_index)  -> (fields tuple in DNS_MSG_DTYPE order, name bytes, [(family, (w0..w3))])
    dns_parse(msg, pkt_index)     -> the numpy triple coracle.dns_parse returns

The rules that the discrimination tests bend are methods of DnsRef, so a mutant is a subclass;
mutants exist on the CPU only.
"""
import numpy as np

from flodbadd_amd import _native as N

(OK, HEADER_TOO_SHORT, UNEXPECTED_EOF, BAD_POINTER, UNKNOWN_LABEL_FORMAT, LABEL_NOT_ASCII, INVALID_QUERY_TYPE,
 INVALID_QUERY_CLASS, INVALID_TYPE, INVALID_CLASS, WRONG_RDATA_LENGTH, ADDITIONAL_OPT) = range(12)
RUNAWAY = 99  # never a real outcome: a mutant whose pointer rule admits a loop ends here

QTYPES = frozenset([1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 28, 33, 252, 253, 254, 255])
TYPES = frozenset([1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 28, 33, 41, 47])
QCLASSES = frozenset([1, 2, 3, 4, 255])
CLASSES = frozenset([1, 2, 3, 4])
A, NS, CNAME, SOA, PTR, MX, TXT, AAAA, SRV, OPT = 1, 2, 5, 6, 12, 15, 16, 28, 33, 41
ANSWER, AUTHORITY, ADDITIONAL = "answer", "authority", "additional"
MAX_NAME, MAX_ADDRS = N.FB_DNS_MAX_NAME, N.FB_DNS_MAX_ADDRS


class Reject(Exception):
    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


def _u16(msg, at):
    return msg[at] * 256 + msg[at + 1]


class DnsRef:
    # ---- the rules a mutant may bend -------------------------------------------------------
    def label_is_ascii(self, content):
        return all(c < 0x80 for c in content)

    def pointer_allowed(self, target, earlier):
        """Strictly before every earlier target of the same name (the first jump may go anywhere)."""
        return all(target < t for t in earlier)

    def is_reverse(self, full, stored):
        return full.endswith(b".in-addr.arpa") or full.endswith(b".ip6.arpa")

    def name_truncated(self, n):
        return n > MAX_NAME - 1

    def collects(self, section):
        return section == ANSWER

    def opt_ahead(self, msg, at):
        return at + 3 <= len(msg) and msg[at: at + 3] == b"\x00\x00\x29"

    # ---- names -----------------------------------------------------------------------------
    def walk_name(self, msg, start, limit):
        """Name::scan of msg[start:limit) with pointers into the whole message.  Returns
        (byte_len, segments): byte_len counts the bytes in place, up to and including the first
        pointer or the root byte; a segment is (labels between two jumps, ended by a pointer)."""
        if start >= limit:
            raise Reject(UNEXPECTED_EOF)
        at, stop, targets, in_place = start, limit, [], None
        segments, labels = [], []
        while True:
            if len(targets) > len(msg):
                raise Reject(RUNAWAY)
            b = msg[at]
            if b == 0:
                segments.append((labels, False))
                if in_place is None:
                    in_place = at + 1 - start
                return in_place, segments
            kind = b >> 6
            if kind == 3:
                if at + 2 > stop:
                    raise Reject(UNEXPECTED_EOF)
                target = _u16(msg, at) & 0x3FFF
                if target >= len(msg):
                    raise Reject(UNEXPECTED_EOF)
                if in_place is None:
                    in_place = at + 2 - start
                if not self.pointer_allowed(target, targets):
                    raise Reject(BAD_POINTER)
                targets.append(target)
                segments.append((labels, True))
                labels = []
                at, stop = target, len(msg)
            elif kind == 0:
                nxt = at + 1 + b
                if nxt > stop:
                    raise Reject(UNEXPECTED_EOF)
                content = msg[at + 1: nxt]
                if not self.label_is_ascii(content):
                    raise Reject(LABEL_NOT_ASCII)
                labels.append(content)
                if nxt >= stop:  # the byte that must follow a label
                    raise Reject(UNEXPECTED_EOF)
                at = nxt
            else:
                raise Reject(UNKNOWN_LABEL_FORMAT)

    @staticmethod
    def display(segments):
        """Labels joined by '.'; a pointer met after a label writes the '.' before it jumps."""
        out = bytearray()
        for labels, jumped in segments:
            out += b".".join(labels)
            if labels and jumped:
                out += b"."
        return bytes(out)

    # ---- records ---------------------------------------------------------------------------
    def check_rdata(self, msg, typ, lo, hi):
        n = hi - lo
        if typ == A or typ == AAAA:
            if n != (4 if typ == A else 16):
                raise Reject(WRONG_RDATA_LENGTH)
        elif typ in (NS, CNAME, PTR):
            self.walk_name(msg, lo, hi)
        elif typ == MX:
            if n < 3:
                raise Reject(WRONG_RDATA_LENGTH)
            self.walk_name(msg, lo + 2, hi)
        elif typ == SRV:
            if n < 7:
                raise Reject(WRONG_RDATA_LENGTH)
            self.walk_name(msg, lo + 6, hi)
        elif typ == SOA:
            first, _ = self.walk_name(msg, lo, hi)
            second, _ = self.walk_name(msg, lo + first, hi)
            if n - first - second < 20:
                raise Reject(WRONG_RDATA_LENGTH)
        elif typ == TXT:
            if n == 0:
                raise Reject(WRONG_RDATA_LENGTH)
            at = lo
            while at < hi:
                at += 1 + msg[at]
                if at > hi:
                    raise Reject(WRONG_RDATA_LENGTH)

    def record(self, msg, at, section, addrs, flags):
        """One resource record at `at`; returns the offset after it."""
        owner_len, _ = self.walk_name(msg, at, len(msg))
        at += owner_len
        if len(msg) - at < 10:
            raise Reject(UNEXPECTED_EOF)
        typ, cls, rdlen = _u16(msg, at), _u16(msg, at + 2) & 0x7FFF, _u16(msg, at + 8)
        if typ not in TYPES:
            raise Reject(INVALID_TYPE)
        if typ != OPT and cls not in CLASSES:
            raise Reject(INVALID_CLASS)
        lo = at + 10
        hi = lo + rdlen
        if hi > len(msg):
            raise Reject(UNEXPECTED_EOF)
        self.check_rdata(msg, typ, lo, hi)
        if typ in (A, AAAA) and self.collects(section):
            if len(addrs) < MAX_ADDRS:
                words = [int.from_bytes(msg[lo + k: lo + k + 4], "big") for k in range(0, rdlen, 4)]
                addrs.append((2 if typ == A else 10, tuple(words + [0] * (4 - len(words)))))
            else:
                flags.add(N.DNS_ADDRS_TRUNCATED)
        return hi

    def opt_record(self, msg, at):
        at += 1  # its root name
        if len(msg) - at < 10:
            raise Reject(UNEXPECTED_EOF)
        hi = at + 10 + _u16(msg, at + 8)
        if hi > len(msg):
            raise Reject(UNEXPECTED_EOF)
        return hi

    # ---- the message -----------------------------------------------------------------------
    def parse_fields(self, msg, pkt_index=0):
        msg = bytes(msg)
        if len(msg) < 12:
            return (pkt_index, 0, HEADER_TOO_SHORT, 0, 0, 0, 0, 0, 0), b"", []
        ident, qd, an, ns, ar = (_u16(msg, k) for k in (0, 4, 6, 8, 10))
        flags, addrs, first = set(), [], None
        if not msg[2] & 0x80:
            flags.add(N.DNS_QUERY)
        try:
            at = 12
            for q in range(qd):
                n, segments = self.walk_name(msg, at, len(msg))
                if first is None:
                    first = segments
                at += n
                if len(msg) - at < 4:
                    raise Reject(UNEXPECTED_EOF)
                if _u16(msg, at) not in QTYPES:
                    raise Reject(INVALID_QUERY_TYPE)
                if _u16(msg, at + 2) & 0x7FFF not in QCLASSES:
                    raise Reject(INVALID_QUERY_CLASS)
                at += 4
            for _ in range(an):
                at = self.record(msg, at, ANSWER, addrs, flags)
            for _ in range(ns):
                at = self.record(msg, at, AUTHORITY, addrs, flags)
            seen_opt = False
            for _ in range(ar):
                if self.opt_ahead(msg, at):
                    if seen_opt:
                        raise Reject(ADDITIONAL_OPT)
                    seen_opt = True
                    at = self.opt_record(msg, at)
                else:
                    at = self.record(msg, at, ADDITIONAL, addrs, flags)
        except Reject as e:
            return (pkt_index, ident, e.status, 0, qd, an, 0, 0, 0), b"", []
        name = b""
        if first is not None:
            full = self.display(first)
            name = full[: MAX_NAME - 1]
            flags.add(N.DNS_HAS_QUESTION)
            if self.is_reverse(full, name):
                flags.add(N.DNS_REVERSE)
            if self.name_truncated(len(full)):
                flags.add(N.DNS_NAME_TRUNCATED)
        return (pkt_index, ident, OK, sum(flags), qd, an, len(name), len(addrs), 0), name, addrs

    def dns_parse(self, msg, pkt_index=0):
        fields, name, addrs = self.parse_fields(msg, pkt_index)
        ips = np.zeros(len(addrs), dtype=N.FB_IP_DTYPE)
        for k, (fam, words) in enumerate(addrs):
            ips[k]["addr"], ips[k]["family"] = words, fam
        return np.array([fields], dtype=N.DNS_MSG_DTYPE)[0], name, ips


_REF = DnsRef()
parse_fields = _REF.parse_fields
dns_parse = _REF.dns_parse


# ---- the mutants of tests/test_dns_corpora.py (never applied to the kernel) ------------------
class SkipsFirstLabelByte(DnsRef):
    def label_is_ascii(self, content):
        return all(c < 0x80 for c in content[1:])


class SkipsLastLabelByte(DnsRef):
    def label_is_ascii(self, content):
        return all(c < 0x80 for c in content[:-1])


class PointerMayRepeatTarget(DnsRef):  # `>` for `>=`
    def pointer_allowed(self, target, earlier):
        return all(target <= t for t in earlier)


class SuffixIgnoresCase(DnsRef):
    def is_reverse(self, full, stored):
        return DnsRef.is_reverse(self, full.lower(), stored)


class SuffixOfStoredName(DnsRef):
    def is_reverse(self, full, stored):
        return DnsRef.is_reverse(self, stored, stored)


class TruncatesAt255(DnsRef):  # `>= 255` for `> 255`
    def name_truncated(self, n):
        return n >= MAX_NAME - 1


class CollectsAuthority(DnsRef):
    def collects(self, section):
        return section in (ANSWER, AUTHORITY)


class OptNeedsFourBytes(DnsRef):  # `at + 3 < len` for `at + 3 <= len`
    def opt_ahead(self, msg, at):
        return at + 3 < len(msg) and msg[at: at + 3] == b"\x00\x00\x29"
