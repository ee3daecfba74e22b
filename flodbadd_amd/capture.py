"""Host-side mirror of the reference's packet path surface, driving the C ABI.

`FlodbaddGpuCapture` stands where `FlodbaddCapture` (src/capture.rs:70-2030) feeds frames to
`parse_packet_pcap` + `process_parsed_packet` (src/capture.rs:1036-1061): it owns one fb_ctx
(one per capture interface, like the reference's one processor task per interface), exposes
the same knobs (`set_filter`/`get_filter`, capture.rs:185; own IPs, capture.rs:964-970;
`init_local_cache`-style IPv6 LAN prefixes, ip.rs:164-191), and turns batches of frames into
session records, DNS diversions and per-flow counters on the GPU.

There is no CPU path: every method calls libflodbadd_gpu.so, which requires a gfx950 device.
"""
import ctypes as C
import ipaddress

import numpy as np

from . import _native as N
from .sessions import (ZEEK_HEADER, Protocol, Session, SessionFilter, WhitelistState, flows_to_sessions, ip_to_words, is_lan_ip,
                       pack_histories, views_to_sessions, words_to_ip)
from .enrich import Blacklists
from .l7 import ProcessInterner, ProcessNameInterner
from .analyzer import SessionAnalyzer, anomaly_tag_of, default_service_codes, merge_criticality, path_cut
from .whitelists import Whitelists, dedup_endpoints, is_session_in_whitelist, no_match_reason


def lan_v6_table(prefixes):
    """[(ipv6 address, prefix_len)] -> fb_lan_v6 array (apply_mask_v6, src/ip.rs:44-51)."""
    t = np.zeros(len(prefixes), dtype=N.LAN_V6_DTYPE)
    for i, (ip, pfx) in enumerate(prefixes):
        net = ipaddress.IPv6Network("%s/%d" % (ipaddress.IPv6Address(ip), pfx), strict=False)
        t[i]["net"] = ip_to_words(net.network_address)[0]
        t[i]["prefix"] = pfx
    return t


def own_ip_table(ips):
    t = np.zeros(len(ips), dtype=N.FB_IP_DTYPE)
    for i, ip in enumerate(ips):
        w, fam = ip_to_words(ip)
        t[i]["addr"] = w
        t[i]["family"] = fam
    return t


class BatchResult:
    def __init__(self, records, dns, cls, stats):
        self.records = records  # PKT_OUT_DTYPE, packet order
        self.dns = dns          # DNS_OUT_DTYPE, packet order
        self.cls = cls          # uint8 per frame (fb_class)
        self.stats = stats      # dict of fb_batch_stats


def stats_dict(arr, fields=N.STATS_FIELDS):
    """A one-record counters array (fb_batch_stats, or the record `fields` names) -> {field: int}."""
    return {k: int(arr[0][k]) for k in fields if not k.startswith("reserved")}


class ZeekLog:
    """What FlodbaddGpuCapture.export_zeek downloads: the conn.log text (uint8), the n + 1 line offsets
    (line i is text[line_off[i]:line_off[i + 1]], '\\n' included) and the call's fb_zeek_stats."""

    def __init__(self, text, line_off, stats):
        self.text, self.line_off, self.stats = text, line_off, stats

    def __len__(self):
        return len(self.line_off) - 1

    def lines(self):
        """The lines as str, without their newlines, in the export's order (view order: Zeek logs are
        unordered, so nothing is sorted)."""
        return self.text.tobytes().decode("ascii").split("\n")[:-1] if len(self) else []

    def write(self, path, header=True):
        with open(path, "wb") as f:
            if header:
                f.write(ZEEK_HEADER.encode("ascii") + b"\n")
            f.write(self.text.tobytes())


class FlodbaddGpuCapture:
    def __init__(self, device=0, session_filter=SessionFilter.GlobalOnly, flow_capacity=1 << 20,
                 service_bitmap=None, lan_v6=(), own_ips=(), max_batch_packets=1 << 20, track_history=False,
                 grow=True, timed=False, track_dns=False, dns_name_capacity=0, dns_addr_capacity=0, dns_hash_mask=0,
                 history_on_device=False, history_block_capacity=0, history_max_blocks=0, processes_on_device=False,
                 domains_on_device=False):
        """timed: capture-time session state (FB_CFG_TIMED): every batch then comes with its frames'
        capture timestamps (`ts`, ns) and the sessions carry start / last / end times and the
        segment state with the reference's 5-s timeout (src/packets.rs:137-200).
        track_dns: the context keeps DnsPacketProcessor's state (fb_dns_track_enable): process_frames then
        parses and tracks its batch's DNS records on the device, update_sessions runs the domain pass, and the
        sessions carry src_domain / dst_domain.  dns_name_capacity / dns_addr_capacity: names and addresses
        before the first growth (0: the library's defaults); dns_hash_mask: fb_dns_track_config.hash_mask,
        a testing knob.
        history_on_device (with track_history): the history strings live in the context's device store
        (fb_hist_store_enable) instead of self.histories: every update is followed by one asynchronous append,
        the getters gather the strings of the flows they return, and export_zeek formats from the store with no
        history byte crossing the bus.  history_block_capacity / history_max_blocks: fb_hist_store_config (0:
        the library's defaults).
        processes_on_device: the whitelist check and the endpoint learning know the L7 pass's processes on the
        device (fb_set_l7_process_names): set_l7_sockets uploads the names of its processes,
        update_whitelist compiles the list with process ids and leaves only the flows a domain endpoint marks to
        the host, and create_custom_whitelists(on_device=True) / augment_custom_whitelists learn endpoints with
        their processes on the device.  A caller who passes process_names to those calls keeps the host path.
        domains_on_device (with track_dns): the whitelist check matches domain endpoints on the device
        (fb_set_whitelist_dom): update_whitelist compiles the list with its domain patterns
        instead of expanding the tracked resolutions into it -- so it installs the list once per list, not once
        per new resolution --, downloads no resolutions, and the pass decides and stamps the domain verdicts
        from the sessions' dst_domain (the domain plane).  Only the flows of a name that matched more than
        FB_WL_NAME_MATCHES patterns, or of a pattern the device has no id for, go through the host loop.  A
        caller who passes dns_resolutions keeps the host path."""
        if domains_on_device and not track_dns:
            raise ValueError("domains_on_device needs track_dns=True")
        lib = N.gpu_lib()
        self._keep = []
        cfg = N.FbConfig()
        cfg.abi_version = N.FB_ABI_VERSION
        cfg.filter = int(session_filter)
        if service_bitmap is not None:
            bm = np.ascontiguousarray(np.frombuffer(bytes(service_bitmap), dtype=np.uint8))
            if bm.size != 8192:
                raise ValueError("service bitmap must be 8192 bytes (one bit per port), got %d" % bm.size)
            self._keep.append(bm)
            cfg.service_bitmap = bm.ctypes.data
        lt = lan_v6_table(list(lan_v6))
        ot = own_ip_table(list(own_ips))
        self._keep += [lt, ot]
        cfg.lan_v6 = lt.ctypes.data if len(lt) else None
        cfg.n_lan_v6 = len(lt)
        cfg.own_ips = ot.ctypes.data if len(ot) else None
        cfg.n_own_ips = len(ot)
        cfg.flow_capacity = int(flow_capacity)
        cfg.max_batch_packets = int(max_batch_packets)
        cfg.flags = (0 if grow else N.FB_CFG_FIXED_TABLE) | (N.FB_CFG_TIMED if timed else 0)  # (the map is unbounded)
        ctx = lib.fb_create(int(device), C.byref(cfg))
        if not ctx:
            raise N.FbError(N.FB_ERR_NODEV, lib.fb_last_error().decode(errors="replace"))
        self.ctx = C.c_void_p(ctx)
        self.filter = SessionFilter(session_filter)
        self.device = device
        self.flow_capacity = flow_capacity
        self.timed = bool(timed)
        # history strings (src/packets.rs:187-198, 410-426) per table slot, appended batch by batch
        # from fb_flow_history_dev when track_history is set
        self.track_history = bool(track_history) and flow_capacity > 0
        self.histories = {}
        self.history_on_device = self.track_history and bool(history_on_device)
        if self.history_on_device:
            hc = np.zeros(1, dtype=N.HIST_STORE_CONFIG_DTYPE)
            hc[0]["block_capacity"], hc[0]["max_blocks"] = int(history_block_capacity), int(history_max_blocks)
            N.check(lib.fb_hist_store_enable(self.ctx, N.ptr(hc)))
        self._generation = 0  # table growths seen (slots move when the table grows)
        # whitelist conformance (src/capture.rs:101-106: no list active, conformance true, no exceptions)
        self._lan_v6 = list(lan_v6)
        self._asn_records = []
        self._whitelists = Whitelists()
        self._wl_name = ""
        self._wl_installed = None   # (CompiledWhitelist, dns_resolutions) the device holds, or None
        self._wl_inputs = (None, None)  # the last update's dns_resolutions / process_names
        self._wl_proc = None        # the process names that update decided its host-check flows with
        self._wl_host_ok = set()    # the Sessions the host resolved to Conforming (process names)
        self._wl_conformance = True
        # blacklist pass (src/blacklists.rs:456-731): the custom model, the name of every installed
        # list (bit l of a mask), whether a pass has run and whether one has marked whitelist bytes
        self._blacklists = Blacklists()
        self._bl_names = []
        self._bl_ran = False
        self._bl_marked = False
        # anomaly pass (src/analyzer.rs): the analyzer's host state, the model the device holds, and what the
        # last analyze_sessions did (None: no analysis yet; "model" / "warming_up" / "no_model")
        self.analyzer = SessionAnalyzer()
        self._an_model = None
        self._an_mode = None
        self._an_codes = False  # the device holds service codes (analyzer.default_service_codes, or a model's)
        # incremental queries (src/capture.rs:411-426): the time of each getter's last full fetch (0: the
        # reference's epoch)
        self._fetch_ts = dict.fromkeys(("sessions", "current", "blacklisted", "exceptions"), 0)
        # get_sessions_zeek's own fetch timestamp: a periodic exporter does not disturb get_sessions' increments
        self._zeek_fetch_ts = 0
        # DNS tracker (src/dns.rs:16-121): names are immutable per id, so the strings are fetched once
        # ({id: str}); the resolutions are exported again only when the tracker's `writes` has moved
        self.track_dns = bool(track_dns)
        self._dns_names = {}
        self._dns_res = (None, {})  # (writes, {ip: name id})
        self._dom_ran = False
        # L7 pass (src/l7.rs; fb_flow_l7): the processes handed to the device so far, whether a snapshot is
        # installed and whether a pass has run since the plane was last cleared
        self._l7_procs = ProcessInterner()
        self.processes_on_device = bool(processes_on_device)
        self._proc_names = ProcessNameInterner()  # shared by the whitelist compiler and the name table's upload
        self._wl_with_ids = False                 # the installed list was compiled with process ids
        self.domains_on_device = bool(domains_on_device)
        self._wl_dom = False                      # the installed list was compiled with domain patterns
        self.wl_installs = 0                      # lists update_whitelist has installed so far
        self._l7_installed = False
        self._l7_ran = False
        if self.track_dns:
            tc = np.zeros(1, dtype=N.DNS_TRACK_CONFIG_DTYPE)
            tc[0]["name_capacity"], tc[0]["addr_capacity"] = int(dns_name_capacity), int(dns_addr_capacity)
            tc[0]["hash_mask"] = int(dns_hash_mask)
            N.check(lib.fb_dns_track_enable(self.ctx, N.ptr(tc)))

    # ---- configuration -------------------------------------------------------------------
    def set_filter(self, flt):
        N.check(N.gpu_lib().fb_set_filter(self.ctx, int(flt)))
        self.filter = SessionFilter(flt)

    def get_filter(self):
        return self.filter

    def set_service_bitmap(self, bitmap):
        bm = np.ascontiguousarray(np.frombuffer(bytes(bitmap), dtype=np.uint8))
        if bm.size != 8192:
            raise ValueError("service bitmap must be 8192 bytes (one bit per port), got %d" % bm.size)
        N.check(N.gpu_lib().fb_set_service_bitmap(self.ctx, N.ptr(bm)))

    def set_lan_v6(self, prefixes):
        prefixes = list(prefixes)
        t = lan_v6_table(prefixes)
        N.check(N.gpu_lib().fb_set_lan_v6(self.ctx, N.ptr(t) if len(t) else None, len(t)))
        self._lan_v6 = prefixes

    def set_own_ips(self, ips):
        t = own_ip_table(list(ips))
        N.check(N.gpu_lib().fb_set_own_ips(self.ctx, N.ptr(t) if len(t) else None, len(t)))

    # ---- packet path -----------------------------------------------------------------------
    def _frame_times(self, ts, n):
        """Upload a batch's capture timestamps and hand them to the next update call (timed
        contexts); returns the device buffer (kept alive by the caller until the call is done)."""
        if not self.timed:
            if ts is not None:
                raise ValueError("capture timestamps need a timed capture (timed=True)")
            return None
        if ts is None:
            raise ValueError("a timed capture needs each batch's capture timestamps (ts)")
        ts = np.ascontiguousarray(ts, dtype=np.uint64)
        if ts.size < n:
            raise ValueError("%d timestamps for %d frames" % (ts.size, n))
        d = N.DeviceBuffer(max(ts.nbytes, 8))
        if ts.size:
            d.upload(ts)
        N.check(N.gpu_lib().fb_set_frame_times(self.ctx, d.ptr))
        return d

    def parse_classify(self, frames, offsets):
        """Host-memory batch: parse_packet_pcap + per-packet classification for every frame."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        n = offsets.size - 1
        out = np.zeros(max(n, 1), dtype=N.PKT_OUT_DTYPE)
        dns = np.zeros(max(n, 1), dtype=N.DNS_OUT_DTYPE)
        cls = np.zeros(max(n, 1), dtype=np.uint8)
        st = np.zeros(1, dtype=N.STATS_DTYPE)
        n_out, n_dns = C.c_uint32(0), C.c_uint32(0)
        N.check(N.gpu_lib().fb_parse_classify(self.ctx, N.ptr(frames), frames.nbytes, N.ptr(offsets), n,
                                              N.ptr(out), C.byref(n_out), N.ptr(dns), C.byref(n_dns),
                                              N.ptr(cls), N.ptr(st), None))
        return BatchResult(out[: n_out.value], dns[: n_dns.value], cls[:n], stats_dict(st))

    def process_parsed(self, packets, ts=None):
        """process_parsed_packet (src/packets.rs:202-537) for a batch of SessionPacketData (list)
        or PARSED_DTYPE records: canonical keys + filter on the GPU, then the session-table upsert
        when the capture has a flow table.  Returns a BatchResult (records, cls, stats)."""
        from .sessions import packets_to_parsed
        arr = packets if isinstance(packets, np.ndarray) else packets_to_parsed(list(packets))
        arr = np.ascontiguousarray(arr, dtype=N.PARSED_DTYPE)
        n = arr.size
        out = np.zeros(max(n, 1), dtype=N.PKT_OUT_DTYPE)
        cls = np.zeros(max(n, 1), dtype=np.uint8)
        st = np.zeros(1, dtype=N.STATS_DTYPE)
        n_out = C.c_uint32(0)
        d_ts = self._frame_times(ts, n) if self.flow_capacity else None  # (indexed by pkt_index)
        N.check(N.gpu_lib().fb_process_parsed(self.ctx, N.ptr(arr) if n else None, n, N.ptr(out), C.byref(n_out),
                                              N.ptr(cls), N.ptr(st), None))
        self._pull_history(n)
        return BatchResult(out[: n_out.value], np.zeros(0, dtype=N.DNS_OUT_DTYPE), cls[:n], stats_dict(st))

    def process_frames(self, frames, offsets, ts=None):
        """parse + classify + flow-table upsert (the whole process_parsed_packet per frame); ts: the
        frames' capture timestamps (ns) on a timed capture."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        n = offsets.size - 1
        lib = N.gpu_lib()
        d_fr = N.DeviceBuffer(max(frames.nbytes, 1)).upload(frames) if frames.nbytes else N.DeviceBuffer(1)
        d_off = N.DeviceBuffer(offsets.nbytes).upload(offsets)
        d_out = N.DeviceBuffer(max(n, 1) * N.PKT_OUT_DTYPE.itemsize)
        d_dns = N.DeviceBuffer(max(n, 1) * N.DNS_OUT_DTYPE.itemsize)
        d_cls = N.DeviceBuffer(max(n, 1))
        d_st = N.DeviceBuffer(N.STATS_DTYPE.itemsize)
        d_ts = self._frame_times(ts, n)  # noqa: F841 (alive until the call's results are read)
        N.check(lib.fb_process_dev(self.ctx, d_fr.ptr, frames.nbytes, d_off.ptr, n, d_out.ptr, d_dns.ptr,
                                   d_cls.ptr, d_st.ptr, None))
        st = d_st.download(np.zeros(1, dtype=N.STATS_DTYPE))
        sd = stats_dict(st)
        out = d_out.download(np.zeros(max(sd["n_session"], 1), dtype=N.PKT_OUT_DTYPE),
                             sd["n_session"] * N.PKT_OUT_DTYPE.itemsize)[: sd["n_session"]]
        dns = d_dns.download(np.zeros(max(sd["n_dns"], 1), dtype=N.DNS_OUT_DTYPE),
                             sd["n_dns"] * N.DNS_OUT_DTYPE.itemsize)[: sd["n_dns"]]
        cls = d_cls.download(np.zeros(max(n, 1), dtype=np.uint8), n)[:n]
        if sd["error"]:
            e = sd["error"]
            code = N.FB_ERR_TABLE_FULL if e & 4 else N.FB_ERR_INTERNAL
            raise N.FbError(code, "device error word %d" % e)
        self._pull_history(n)
        if self.track_dns and sd["n_dns"]:  # device to device: neither the names nor the answers come down
            self._track_dns_dev(d_fr, frames.nbytes, d_dns, sd["n_dns"], d_ts)
        return BatchResult(out, dns, cls, sd)

    # ---- DNS tracker (src/dns.rs:16-121; fb_dns_track_dev) ------------------------------------------
    def _need_dns(self):
        if not self.track_dns:
            raise ValueError("this capture does not track DNS (track_dns=True)")

    def _track_dns_dev(self, d_frames, frames_bytes, d_dns, n, d_ts=None, want_taken=False):
        """fb_dns_parse_dev + fb_dns_track_dev over n DNS side records in device memory."""
        lib = N.gpu_lib()
        d_msg = N.DeviceBuffer(n * N.DNS_MSG_DTYPE.itemsize)
        d_names = N.DeviceBuffer(n * N.FB_DNS_MAX_NAME)
        d_addrs = N.DeviceBuffer(n * N.FB_DNS_MAX_ADDRS * N.FB_IP_DTYPE.itemsize)
        N.check(lib.fb_dns_parse_dev(self.ctx, d_frames.ptr, frames_bytes, d_dns.ptr, n, None, d_msg.ptr, d_names.ptr,
                                     d_addrs.ptr, None))
        return self.track_dns_parsed_dev(d_msg, d_names, d_addrs, n, d_ts=d_ts, want_taken=want_taken)

    def track_dns_parsed_dev(self, d_msg, d_names, d_addrs, n, d_stats=None, d_ts=None, want_taken=False):
        """fb_dns_track_dev over DeviceBuffers as fb_dns_parse_dev wrote them: the call's counters
        (fb_dns_track_stats) and, with want_taken, the name id each response took."""
        self._need_dns()
        st = np.zeros(1, dtype=N.DNS_TRACK_STATS_DTYPE)
        d_taken = N.DeviceBuffer(max(n, 1) * 4) if want_taken else None
        N.check(N.gpu_lib().fb_dns_track_dev(self.ctx, d_msg.ptr, d_names.ptr, d_addrs.ptr, n,
                                             d_stats.ptr if d_stats is not None else None,
                                             d_ts.ptr if d_ts is not None else None,
                                             d_taken.ptr if want_taken else None, N.ptr(st), None))
        out = stats_dict(st, N.DNS_TRACK_STATS_FIELDS)
        if want_taken:
            out["taken"] = d_taken.download(np.zeros(max(n, 1), dtype=np.uint32))[:n]
        return out

    def track_dns_records(self, frames, dns_records, ts=None):
        """What process_frames does with its batch's DNS side records, for the callers of parse_classify:
        the records are parsed and tracked on the device.  ts: the frames' capture timestamps (ns), which
        the 30-s expiry of the pending queries runs on; without them the queries never expire."""
        self._need_dns()
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        dns_records = np.ascontiguousarray(dns_records, dtype=N.DNS_OUT_DTYPE)
        n = len(dns_records)
        if n == 0:
            return dict.fromkeys(N.DNS_TRACK_STATS_FIELDS, 0)
        d_fr = N.DeviceBuffer(max(frames.nbytes, 1))
        if frames.nbytes:
            d_fr.upload(frames)
        d_dns = N.DeviceBuffer(dns_records.nbytes).upload(dns_records)
        d_ts = None
        if ts is not None:
            ts = np.ascontiguousarray(ts, dtype=np.uint64)
            if ts.size <= int(dns_records["pkt_index"].max()):
                raise ValueError("%d timestamps, frame %d has a DNS record" % (ts.size, int(dns_records["pkt_index"].max())))
            d_ts = N.DeviceBuffer(ts.nbytes).upload(ts)
        return self._track_dns_dev(d_fr, frames.nbytes, d_dns, n, d_ts)

    def dns_track_info(self):
        """fb_dns_track_info_get: names, addrs, the two capacities, pending, messages, writes."""
        self._need_dns()
        t = np.zeros(1, dtype=N.DNS_TRACK_INFO_DTYPE)
        N.check(N.gpu_lib().fb_dns_track_info_get(self.ctx, N.ptr(t)))
        return stats_dict(t, N.DNS_TRACK_INFO_FIELDS)

    def dns_names(self, ids):
        """{id: str} for the given name ids (fb_dns_names_dev for the ids not fetched before; 0 is left out)."""
        want = sorted({int(i) for i in ids} - {0} - set(self._dns_names))
        if want:
            a = np.array(want, dtype=np.uint32)
            d_ids = N.DeviceBuffer(a.nbytes).upload(a)
            d_out, d_len = N.DeviceBuffer(len(a) * N.FB_DNS_MAX_NAME), N.DeviceBuffer(len(a) * 2)
            N.check(N.gpu_lib().fb_dns_names_dev(self.ctx, d_ids.ptr, len(a), d_out.ptr, d_len.ptr, None))
            raw = d_out.download(np.zeros((len(a), N.FB_DNS_MAX_NAME), dtype=np.uint8))
            ln = d_len.download(np.zeros(len(a), dtype=np.uint16))
            fetched = {i: bytes(r[: int(l)]).decode("ascii") for i, r, l in zip(want, raw, ln)}
            # (length 0 is also what an id the store does not hold yet gives: not kept)
            self._dns_names.update({i: s for i, s in fetched.items() if s})
        else:
            fetched = {}
        return {int(i): self._dns_names.get(int(i), fetched.get(int(i), "")) for i in ids if int(i)}

    def dns_resolution_ids(self):
        """{ip: name id} (fb_dns_export_resolutions_dev), exported again only when a resolution was written."""
        info = self.dns_track_info()
        if self._dns_res[0] != info["writes"]:
            cap = max(info["addrs"], 1)
            d_out, d_n = N.DeviceBuffer(cap * N.DNS_RESOLUTION_DTYPE.itemsize), N.DeviceBuffer(8)
            N.check(N.gpu_lib().fb_dns_export_resolutions_dev(self.ctx, d_out.ptr, cap, d_n.ptr, None))
            m = min(int(d_n.download(np.zeros(1, dtype=np.uint64))[0]), cap)
            recs = d_out.download(np.zeros(cap, dtype=N.DNS_RESOLUTION_DTYPE))[:m]
            self._dns_res = (info["writes"], {words_to_ip(r["ip"]["addr"], int(r["ip"]["family"])): int(r["name_id"])
                                              for r in recs})
        return self._dns_res[1]

    def dns_resolutions(self):
        """dns_resolutions (src/dns.rs:19): {ip: name}."""
        ids = self.dns_resolution_ids()
        names = self.dns_names(ids.values())
        return {ip: names[i] for ip, i in ids.items()}

    def dns_pending_ids(self):
        """(name id, query time) of every transaction id (fb_dns_export_pending_dev); 0: none pending."""
        self._need_dns()
        d_id, d_t = N.DeviceBuffer(N.FB_DNS_IDS * 4), N.DeviceBuffer(N.FB_DNS_IDS * 8)
        N.check(N.gpu_lib().fb_dns_export_pending_dev(self.ctx, d_id.ptr, d_t.ptr, None))
        return (d_id.download(np.zeros(N.FB_DNS_IDS, dtype=np.uint32)),
                d_t.download(np.zeros(N.FB_DNS_IDS, dtype=np.uint64)))

    def dns_pending(self):
        """pending_dns_queries (src/dns.rs:18): {transaction id: name}."""
        ids, _ = self.dns_pending_ids()
        tx = np.nonzero(ids)[0]
        names = self.dns_names(ids[tx])
        return {int(t): names[int(ids[t])] for t in tx}

    def expire_dns(self, now_ns):
        """The cleanup task of src/dns.rs:101-121 at now_ns on the capture clock: the pending queries of
        30 s and older are dropped; returns their number."""
        self._need_dns()
        n = C.c_uint64(0)
        N.check(N.gpu_lib().fb_dns_expire(self.ctx, int(now_ns), C.byref(n)))
        return n.value

    def dns_lookup(self, ips):
        """fb_dns_lookup_dev: the name id each address resolves to (0: none)."""
        self._need_dns()
        t = own_ip_table(list(ips))
        if not len(t):
            return np.zeros(0, dtype=np.uint32)
        d_ips, d_out = N.DeviceBuffer(t.nbytes).upload(t), N.DeviceBuffer(len(t) * 4)
        N.check(N.gpu_lib().fb_dns_lookup_dev(self.ctx, d_ips.ptr, len(t), d_out.ptr, None))
        return d_out.download(np.zeros(len(t), dtype=np.uint32))

    def clear_dns(self):
        """fb_dns_track_clear: the tracker's state and the sessions' domains are gone."""
        self._need_dns()
        N.check(N.gpu_lib().fb_dns_track_clear(self.ctx))
        self._dns_names = {}
        self._dns_res = (None, {})

    # ---- domain pass (src/capture.rs:1307-1411; fb_flow_domains) ----------------------------------
    def update_domains(self):
        """populate_domain_names over every current session from the tracked resolutions; returns the
        pass's counters (fb_dom_stats)."""
        self._need_dns()
        st = np.zeros(1, dtype=N.DOM_STATS_DTYPE)
        N.check(N.gpu_lib().fb_flow_domains(self.ctx, 0, N.ptr(st), None))
        self._dom_ran = True
        return stats_dict(st, N.DOM_STATS_FIELDS)

    def domain_ids(self):
        """fb_flow_domains_dev: the (src, dst) name ids of every table slot (index = fb_flow_rec.slot)."""
        return self._plane("fb_flow_domains_dev", N.FLOW_DOMAIN_DTYPE)

    def _domains(self):
        """views_to_sessions' `domains` (None while no domain pass has run)."""
        if not (self.track_dns and self._dom_ran):
            return None
        ids = self.domain_ids()
        pairs = np.stack([ids["src_name_id"], ids["dst_name_id"]], axis=1)
        return pairs, self.dns_names(np.unique(pairs))

    # ---- L7 pass (src/l7.rs:208-500, src/capture.rs:1414-1495; fb_flow_l7) --------------------------
    def set_l7_sockets(self, snapshot):
        """fb_set_l7_sockets: install an l7.SocketSnapshot -- what the reference's resolver reads from the OS
        once per cycle -- for the passes that follow.  Returns the number of sockets installed (those with a
        known process)."""
        socks = snapshot.compile(self._l7_procs)
        N.check(N.gpu_lib().fb_set_l7_sockets(self.ctx, N.ptr(socks) if len(socks) else None, len(socks)))
        if self.processes_on_device:  # the names of every process handed over so far (the interners only grow)
            m, v = self._proc_names.table(self._l7_procs.processes)
            N.check(N.gpu_lib().fb_set_l7_process_names(self.ctx, N.ptr(m), N.ptr(v), len(m)))
        self._l7_installed = True
        return len(socks)

    def update_l7(self, max_retries=N.FB_L7_DEFAULT_MAX_RETRIES):
        """One resolver cycle over every current session without a process (populate_l7 + resolve_l7_data);
        returns the pass's counters (fb_l7_stats)."""
        prm = np.zeros(1, dtype=N.L7_PARAMS_DTYPE)
        prm[0]["max_retries"] = int(max_retries)
        st = np.zeros(1, dtype=N.L7_STATS_DTYPE)
        N.check(N.gpu_lib().fb_flow_l7(self.ctx, N.ptr(prm), N.ptr(st), None))
        self._l7_ran = True
        return stats_dict(st, N.L7_STATS_FIELDS)

    def l7_records(self):
        """fb_flow_l7_dev: the L7 element (L7_REC_DTYPE) of every table slot (index = fb_flow_rec.slot)."""
        return self._plane("fb_flow_l7_dev", N.L7_REC_DTYPE)

    def l7_lookup(self, keys):
        """fb_l7_lookup_dev: the match of each key (records with fb_session_key's fields first, 40 bytes taken
        of each) against the installed snapshot, as L7_REC_DTYPE records."""
        keys = np.ascontiguousarray(keys)
        raw = np.ascontiguousarray(keys.view(np.uint8).reshape(len(keys), keys.dtype.itemsize)[:, :40])
        out = np.zeros(len(keys), dtype=N.L7_REC_DTYPE)
        d_k, d_o = N.DeviceBuffer(max(raw.nbytes, 8)), N.DeviceBuffer(max(out.nbytes, 8))
        if len(keys):
            d_k.upload(raw)
        N.check(N.gpu_lib().fb_l7_lookup_dev(self.ctx, d_k.ptr, len(keys), d_o.ptr, None))
        return d_o.download(out, out.nbytes) if len(keys) else out

    def clear_l7(self):
        """fb_l7_clear: the snapshot is dropped and every session is unresolved again."""
        N.check(N.gpu_lib().fb_l7_clear(self.ctx))
        self._l7_installed = False
        self._l7_ran = False

    def _l7(self):
        """views_to_sessions' `l7` (None while no L7 pass has run)."""
        if not self._l7_ran:
            return None
        return self.l7_records()["process_id"], self._l7_procs.processes

    def l7_process_names(self):
        """{Session: process name} of the sessions the L7 pass has resolved: what the whitelist calls take as
        process_names."""
        if not (self._l7_ran and self.flow_capacity):
            return {}
        flows, ids = self.export_flows(SessionFilter.All), self.l7_records()["process_id"]
        procs = self._l7_procs.processes
        return {Session.from_key(r): procs[int(ids[int(r["slot"])])].process_name
                for r in flows if int(ids[int(r["slot"])])}

    def _device_processes(self, process_names):
        """Does a whitelist call leave the processes to the device?  (processes_on_device, and the caller gave
        no process_names of their own.)"""
        return self.processes_on_device and process_names is None

    def _device_domains(self, dns_resolutions):
        """Does a whitelist call leave the domains to the device?  (domains_on_device, and the caller gave no
        dns_resolutions of their own.)"""
        return self.domains_on_device and dns_resolutions is None

    def _slot_domains(self, flows):
        """{Session: dst_domain} of the given fb_flow_rec records alone, from the domain plane."""
        if not (self._dom_ran and len(flows)):
            return {}
        ids = self.domain_ids()["dst_name_id"]
        names = self.dns_names(np.unique([int(ids[int(r["slot"])]) for r in flows]))
        return {Session.from_key(r): names[int(ids[int(r["slot"])])] for r in flows if int(ids[int(r["slot"])])}

    def _slot_process_names(self, flows):
        """{Session: process name} of the given fb_flow_rec records alone, from the L7 plane."""
        if not (self._l7_ran and len(flows)):
            return {}
        ids, procs = self.l7_records()["process_id"], self._l7_procs.processes
        return {Session.from_key(r): procs[int(ids[int(r["slot"])])].process_name
                for r in flows if int(ids[int(r["slot"])])}

    def _process_names(self, process_names):
        """The process names a whitelist call works with: the caller's when given, else the device's
        attribution once an L7 pass has run, else none."""
        if process_names is None and self._l7_ran:
            return self.l7_process_names()
        return process_names

    process = process_frames

    def process_frames_seg(self, frames, offsets, flow=True, ts=None):
        """The segmented streaming path (fb_process_seg_dev / fb_parse_classify_seg_dev): same
        classification and session-table update, records left in per-wavefront segments on the
        device; returned here densified (packet order) for comparison with process_frames."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        n = offsets.size - 1
        nseg = max((n + N.FB_SEG_FRAMES - 1) // N.FB_SEG_FRAMES, 1)
        lib = N.gpu_lib()
        d_fr = N.DeviceBuffer(max(frames.nbytes, 1)).upload(frames) if frames.nbytes else N.DeviceBuffer(1)
        d_off = N.DeviceBuffer(offsets.nbytes).upload(offsets)
        d_out = N.DeviceBuffer(nseg * N.SEG_BYTES)
        d_seg = N.DeviceBuffer(nseg * 4)
        d_cls = N.DeviceBuffer(max(n, 1))
        d_st = N.DeviceBuffer(N.STATS_DTYPE.itemsize)
        d_ts = self._frame_times(ts, n) if flow else None  # noqa: F841
        fn = lib.fb_process_seg_dev if flow else lib.fb_parse_classify_seg_dev
        N.check(fn(self.ctx, d_fr.ptr, frames.nbytes, d_off.ptr, n, d_out.ptr, d_seg.ptr, d_cls.ptr, d_st.ptr, None))
        sd = stats_dict(d_st.download(np.zeros(1, dtype=N.STATS_DTYPE)))
        if sd["error"]:
            e = sd["error"]
            raise N.FbError(N.FB_ERR_TABLE_FULL if e & 4 else N.FB_ERR_INTERNAL, "device error word %d" % e)
        if flow:
            self._pull_history(((n + N.FB_SEG_FRAMES - 1) // N.FB_SEG_FRAMES) * N.FB_SEG_FRAMES)
        seg = d_seg.download(np.zeros(nseg, dtype=np.uint32))
        raw = d_out.download(np.zeros(nseg * N.SEG_BYTES, dtype=np.uint8))
        out, dns = N.seg_unpack(raw, seg[: (n + N.FB_SEG_FRAMES - 1) // N.FB_SEG_FRAMES])
        cls = d_cls.download(np.zeros(max(n, 1), dtype=np.uint8), n)[:n]
        return BatchResult(out, dns, cls, sd)

    # ---- session table -----------------------------------------------------------------------
    def flow_history(self, n_slots):
        """fb_flow_history_dev: the last update's history characters grouped per flow, packet order
        inside each flow -> {table slot: str}.  n_slots = that update's record slots (its batch's
        n frames, dense; ceil(n/64)*64, segmented)."""
        m = max(int(n_slots), 1)
        d_h, d_s, d_n = N.DeviceBuffer(m), N.DeviceBuffer(4 * m), N.DeviceBuffer(4)
        N.check(N.gpu_lib().fb_flow_history_dev(self.ctx, d_h.ptr, d_s.ptr, d_n.ptr, None))
        k = int(d_n.download(np.zeros(1, dtype=np.uint32))[0])
        if k == 0:
            return {}
        chars = d_h.download(np.zeros(k, dtype=np.uint8), k)
        slots = d_s.download(np.zeros(k, dtype=np.uint32), 4 * k)
        cut = np.flatnonzero(np.diff(slots)) + 1
        starts, ends = np.r_[0, cut], np.r_[cut, k]
        return {int(slots[a]): chars[a:b].tobytes().decode("ascii") for a, b in zip(starts, ends)}

    def table_info(self):
        """fb_flow_table_info_get: capacity, partitions, growths, flows / fullest partition as the
        last completed update reported."""
        t = N.FlowTableInfo()
        N.check(N.gpu_lib().fb_flow_table_info_get(self.ctx, C.byref(t)))
        return dict(capacity=t.capacity, partitions=t.partitions, generation=t.generation, flows=t.flows,
                    max_partition=t.max_partition)

    def _follow_growth(self):
        """The table grew, or a purge re-packed it, since the histories were last keyed: move them to
        the new slots (fb_flow_slot_remap; only the last move's map is kept, and this runs after every
        batch and every purge)."""
        gen = self.table_info()["generation"]
        if gen == self._generation:
            return
        if gen != self._generation + 1:  # fb_flow_slot_remap keeps only the last growth's map
            raise N.FbError(N.FB_ERR_INTERNAL, "the table grew %d times since the histories were keyed"
                            % (gen - self._generation))
        self._generation = gen
        if not self.histories:
            return
        old_cap = max(self.histories) + 1
        m = np.zeros(max(old_cap, 1), dtype=np.uint32)
        n = C.c_uint64(0)
        N.check(N.gpu_lib().fb_flow_slot_remap(self.ctx, N.ptr(m), old_cap, C.byref(n)))
        # a purge (update_sessions_status) maps the flows it removed to 0xFFFFFFFF: their histories go
        # with them (a growth maps every occupied slot, so nothing is dropped then)
        self.histories = {int(m[k]): v for k, v in self.histories.items() if int(m[k]) != 0xFFFFFFFF}

    def _pull_history(self, n_slots):
        if not self.track_history:
            return
        if self.history_on_device:  # one asynchronous call: no wait, no download, nothing keyed on the host
            N.check(N.gpu_lib().fb_hist_store_append_dev(self.ctx, None))
            return
        self._follow_growth()
        for slot, run in self.flow_history(n_slots).items():
            self.histories[slot] = self.histories.get(slot, "") + run

    def history_store_info(self):
        """fb_hist_store_info_get: the device store's counters (history_on_device)."""
        info = np.zeros(1, dtype=N.HIST_STORE_INFO_DTYPE)
        N.check(N.gpu_lib().fb_hist_store_info_get(self.ctx, N.ptr(info)))
        return stats_dict(info, N.HIST_STORE_INFO_FIELDS)

    def _gather_histories(self, d_slots, stride, n):
        """The store's characters of n slots read on the device (d_slots / stride as fb_hist_store_lengths_dev
        takes them): lengths, one 8-byte read of the total, an exactly sized gather -> (d_chars, d_off, total)."""
        lib = N.gpu_lib()
        d_off = N.DeviceBuffer(8 * (n + 1))
        N.check(lib.fb_hist_store_lengths_dev(self.ctx, d_slots, stride, n, d_off.ptr, None))
        total = np.zeros(1, dtype=np.uint64)
        N.check(lib.fb_memcpy_d2h(N.ptr(total), C.c_void_p(d_off.ptr.value + 8 * n), 8, None))
        N.check(lib.fb_stream_sync(None))
        total = int(total[0])
        d_chars = N.DeviceBuffer(max(total, 1))
        N.check(lib.fb_hist_store_gather_dev(self.ctx, d_slots, stride, n, d_off.ptr, d_chars.ptr, total, None))
        return d_chars, d_off, total

    def flow_histories(self, slots=None):
        """The history strings the device store holds (history_on_device) -> {slot: str} for `slots` (an array
        of table slots; None: every slot of the table), flows without characters left out."""
        if not self.history_on_device:
            raise ValueError("flow_histories reads the device store (history_on_device=True)")
        if slots is None:
            n, d_slots, sl = int(self.table_info()["capacity"]), None, None
        else:
            sl = np.ascontiguousarray(slots, dtype=np.uint32)
            n = len(sl)
            if n == 0:
                return {}
            d_slots = N.DeviceBuffer(sl.nbytes).upload(sl)
        d_chars, d_off, total = self._gather_histories(d_slots.ptr if d_slots else None, 4, n)
        if total == 0:
            return {}
        off = d_off.download(np.zeros(n + 1, dtype=np.uint64)).astype(np.int64)
        text = d_chars.download(np.zeros(total, dtype=np.uint8), total).tobytes().decode("ascii")
        has = np.flatnonzero(off[1:] > off[:-1])
        return {int(i if sl is None else sl[i]): text[off[i]:off[i + 1]] for i in has}

    def flow_count(self):
        n = C.c_uint64(0)
        N.check(N.gpu_lib().fb_flow_count(self.ctx, C.byref(n), None))
        return n.value

    def export_flows(self, session_filter=SessionFilter.All):
        """fb_flow_export_sessions: every flow (All), or those passing the filter evaluated now."""
        cnt = self.flow_count()
        out = np.zeros(max(cnt, 1), dtype=N.FLOW_REC_DTYPE)
        n = C.c_uint64(0)
        N.check(N.gpu_lib().fb_flow_export_sessions(self.ctx, int(session_filter), N.ptr(out), cnt, C.byref(n), None))
        return out[: n.value]

    def export_times(self):
        """fb_flow_export_times: every flow's FLOW_TIME_DTYPE record (timed captures), with its slot."""
        cnt = self.flow_count()
        out = np.zeros(max(cnt, 1), dtype=N.FLOW_TIME_DTYPE)
        n = C.c_uint64(0)
        N.check(N.gpu_lib().fb_flow_export_times(self.ctx, N.ptr(out), cnt, C.byref(n), None))
        return out[: n.value]

    def status_bytes(self):
        """fb_flow_status_dev: the status byte of every table slot (index = fb_flow_rec.slot); all
        zero before the first update_sessions_status."""
        return self._plane("fb_flow_status_dev", np.uint8)

    def _plane(self, copy_fn, dtype):
        """One per-slot plane at whole table capacity (index = fb_flow_rec.slot) through its fb_flow_*_dev copy."""
        cap = int(self.table_info()["capacity"])
        out = np.zeros(max(cap, 1), dtype=dtype)
        if cap:
            d = N.DeviceBuffer(cap * out.itemsize)
            N.check(getattr(N.gpu_lib(), copy_fn)(self.ctx, d.ptr, cap, None))
            d.download(out, cap * out.itemsize)
        return out[:cap]

    def _compact_export(self, export_fn, dtypes, *lead, extra=()):
        """A compacting export -- export_fn(ctx, *lead, one output per dtype, cap, d_n, *extra, stream) -- with room
        for every flow: the count is read back and each output trimmed to it -> one array per dtype."""
        cap = max(self.flow_count(), 1)
        outs = [np.zeros(cap, dtype=t) for t in dtypes]
        bufs = [N.DeviceBuffer(o.nbytes) for o in outs]
        d_n = N.DeviceBuffer(8)
        N.check(getattr(N.gpu_lib(), export_fn)(self.ctx, *lead, *(b.ptr for b in bufs), cap, d_n.ptr, *extra, None))
        m = min(int(d_n.download(np.zeros(1, dtype=np.uint64))[0]), cap)
        return tuple(b.download(o)[:m] for b, o in zip(bufs, outs))

    # ---- incremental queries (src/capture.rs:411-426, 1578-1760) -------------------------------------
    def set_pass_time(self, now_ns):
        """fb_set_pass_time: the time -- on the capture timestamps' clock -- that the blacklist, whitelist and
        anomaly passes write into the sessions they change (SessionInfo.last_modified_ns); 0: no stamps."""
        N.check(N.gpu_lib().fb_set_pass_time(self.ctx, int(now_ns)))

    def reset_fetch_timestamps(self):
        """reset_fetch_timestamps (src/capture.rs:411-426): every getter's next incremental fetch is full."""
        self._fetch_ts = dict.fromkeys(self._fetch_ts, 0)
        self._zeek_fetch_ts = 0

    def modified_stamps(self):
        """fb_flow_modified_dev: the stamp of every table slot (index = fb_flow_rec.slot); all zero while no
        pass has run under a pass time."""
        return self._plane("fb_flow_modified_dev", np.uint64)

    @staticmethod
    def _view_query(view_set, since_ns, session_filter):
        q = np.zeros(1, dtype=N.VIEW_QUERY_DTYPE)
        q[0]["set"] = int(view_set)
        q[0]["filter"] = int(SessionFilter.All if session_filter is None else session_filter)
        if since_ns is not None:
            q[0]["flags"], q[0]["since_ns"] = N.FB_VIEW_MODIFIED_SINCE, int(since_ns)
        return q

    def export_view(self, view_set=N.FB_VIEW_ALL, since_ns=None, session_filter=None):
        """fb_flow_export_view: the FLOW_VIEW_DTYPE records of the flows of `view_set` (N.FB_VIEW_*) that pass
        session_filter evaluated now (None: every flow) and, with since_ns, whose last_modified_ns is later
        than it (timed captures)."""
        q = self._view_query(view_set, since_ns, session_filter)
        cnt = self.flow_count() if self.flow_capacity else 1
        out = np.zeros(max(cnt, 1), dtype=N.FLOW_VIEW_DTYPE)
        n = C.c_uint64(0)
        N.check(N.gpu_lib().fb_flow_export_view(self.ctx, N.ptr(q), N.ptr(out), cnt, C.byref(n), None))
        return out[: n.value]

    def learn_endpoints(self, view_set=N.FB_VIEW_ALL, since_ns=None, session_filter=None):
        """fb_flow_learn_endpoints_dev: the distinct endpoints -- (dst_ip, family, dst_port, protocol, dst name id)
        -- of the flows export_view would select with the same arguments, each with its least session as the
        representative, in ascending rep_slot order -> (LEARNED_ENDPOINT_DTYPE records, the call's counters)."""
        q = self._view_query(view_set, since_ns, session_filter)
        st = np.zeros(1, dtype=N.LEARN_STATS_DTYPE)
        recs, = self._compact_export("fb_flow_learn_endpoints_dev", [N.LEARNED_ENDPOINT_DTYPE], N.ptr(q),
                                     extra=(N.ptr(st),))
        return recs, stats_dict(st, N.LEARN_STATS_FIELDS)

    def _since(self, which, incremental):
        """What a getter call selects by: an incremental fetch, the flows modified since the getter's last full
        fetch with a now_ns (timed captures); a full fetch, every flow (None)."""
        if not incremental:
            return None
        if not self.timed:
            raise ValueError("incremental fetches need a timed capture (timed=True): last_modified has no clock")
        return self._fetch_ts[which]

    def _fetched(self, which, now_ns, incremental):
        """A full fetch with a now_ns moves the getter's fetch timestamp; nothing else does."""
        if now_ns is not None and not incremental:
            self._fetch_ts[which] = int(now_ns)

    def _view_sessions(self, view_set, since=None, session_filter=None, whitelist=True, blacklist=True, keep=None,
                       overlay_host_ok=False):
        """The SessionInfo list of every getter, from one view export: the flows of view_set that pass
        session_filter and changed since `since` (None: all of them), without the rows keep(views) drops, joined by
        views_to_sessions -- status and time fields on a timed capture only, the whitelist byte / blacklist mask
        decoded as asked -- then the host's whitelist verdicts and the anomaly tags merged in."""
        if not self.flow_capacity:  # no table (the view export refuses such a context): no sessions
            return []
        views = self.export_view(view_set, since, session_filter)
        if keep is not None and len(views):
            views = views[keep(views)]
        if self.history_on_device:  # the strings of the selected flows only, gathered from the store
            histories = self.flow_histories(views["rec"]["slot"])
        else:
            histories = self.histories if self.track_history else None
        out = views_to_sessions(views, histories, self._bl_names, timed=self.timed,
                                whitelist=whitelist, blacklist=blacklist, domains=self._domains(), l7=self._l7())
        for info in out if (overlay_host_ok and self._wl_host_ok) else ():  # the flows the pass left to the host
            if info.session in self._wl_host_ok and info.is_whitelisted is WhitelistState.NonConforming:
                info.is_whitelisted = WhitelistState.Conforming
        return self._merge_anomaly(out, views["rec"], views["an"])

    def update_sessions_status(self, now_ns, purge=True, activity_s=60, current_s=180, retention_s=86400):
        """update_sessions_status (src/capture.rs:1497-1551) at `now_ns` on the capture timestamps'
        clock (timed captures): every session's status and current_sessions membership recomputed, and
        with `purge` the sessions idle for longer than retention_s removed.  Returns the call's
        counters (fb_age_stats).  A purge that removed sessions moves others to new table slots; the
        history strings follow (fb_flow_slot_remap), those of removed sessions are dropped."""
        prm = np.zeros(1, dtype=N.AGE_PARAMS_DTYPE)
        prm[0]["activity_ns"] = int(round(activity_s * 1e9))
        prm[0]["current_ns"] = int(round(current_s * 1e9))
        prm[0]["retention_ns"] = int(round(retention_s * 1e9))
        st = np.zeros(1, dtype=N.AGE_STATS_DTYPE)
        N.check(N.gpu_lib().fb_flow_age(self.ctx, int(now_ns), N.ptr(prm), N.FB_AGE_PURGE if purge else 0, N.ptr(st),
                                        None))
        if self.track_history and not self.history_on_device:  # (the device store's plane follows by itself)
            self._follow_growth()
        return stats_dict(st, N.AGE_STATS_FIELDS)

    def get_sessions(self, now_ns=None, incremental=False):
        """get_sessions (src/capture.rs:1578-1612): the sessions that pass the CURRENT filter,
        is_local_session! evaluated at query time on the GPU (capture.rs:1603-1608), sorted by the
        derived Ord of Session (integer counters + derived f64s).  With now_ns (timed captures) the
        table is aged first, as the reference does on every query (capture.rs:1581).  incremental
        (capture.rs:1583-1621): only the sessions modified since this getter's last full fetch with a
        now_ns, from one view export; a full fetch with now_ns moves that timestamp, nothing else does."""
        since = self._since("sessions", incremental)
        if now_ns is not None:
            self.update_sessions_status(now_ns)
        self._fetched("sessions", now_ns, incremental)
        return self._view_sessions(N.FB_VIEW_ALL, since, self.filter, whitelist=bool(self._wl_name or self._bl_marked),
                                   blacklist=self._bl_ran, overlay_host_ok=True)

    def get_current_sessions(self, now_ns=None, incremental=False):
        """get_current_sessions (src/capture.rs:1624-1670): the members of current_sessions -- activity
        within the current span at the last aging, or inserted since (src/packets.rs:532) -- that pass
        the current filter.  With now_ns the table is aged first.  incremental: as get_sessions, with this
        getter's own fetch timestamp (capture.rs:1629-1666)."""
        if not self.timed:
            raise ValueError("current sessions need a timed capture (timed=True)")
        since = self._since("current", incremental)
        if now_ns is not None:
            self.update_sessions_status(now_ns)
        self._fetched("current", now_ns, incremental)
        return self._view_sessions(N.FB_VIEW_CURRENT, since, self.filter, whitelist=False, blacklist=self._bl_ran)

    # ---- Zeek conn.log export (format_sessions_zeek, src/sessions.rs:694-774) ---------------------------
    def export_zeek(self, view_set=N.FB_VIEW_ALL, since_ns=None, session_filter=None):
        """The conn.log lines of the flows export_view(view_set, since_ns, session_filter) selects, formatted on
        the device (fb_format_zeek_dev; timed captures): the view records stay in device memory, the history
        strings are uploaded when track_history is set (else every history field is empty), and only the text,
        its line offsets and the counters come back -> ZeekLog.  Lines are in view order.  The text buffer has
        room for every line (FB_ZEEK_FIXED_MAX each, plus the history bytes), so there is no retry."""
        lib = N.gpu_lib()
        q = self._view_query(view_set, since_ns, session_filter)
        cnt = self.flow_count() if self.flow_capacity else 0
        d_views, d_n = N.DeviceBuffer(max(cnt, 1) * N.FLOW_VIEW_DTYPE.itemsize), N.DeviceBuffer(8)
        N.check(lib.fb_flow_export_view_dev(self.ctx, N.ptr(q), d_views.ptr, cnt, d_n.ptr, None))
        n = min(int(d_n.download(np.zeros(1, dtype=np.uint64))[0]), cnt)
        d_hist = d_hoff = None
        n_slots = hist_bytes = 0
        if self.history_on_device and n:
            # the selected records' histories gathered from the store, indexed by record: no history byte
            # crosses the bus in either direction
            d_slot0 = C.c_void_p(d_views.ptr.value + N.FLOW_VIEW_DTYPE.fields["rec"][1] +
                                 N.FLOW_REC_DTYPE.fields["slot"][1])
            d_hist, d_hoff, hist_bytes = self._gather_histories(d_slot0, N.FLOW_VIEW_DTYPE.itemsize, n)
        elif self.track_history and not self.history_on_device:
            n_slots = int(self.table_info()["capacity"])
            chars, off = pack_histories(self.histories, n_slots)
            hist_bytes = len(chars)
            d_hist, d_hoff = N.DeviceBuffer(max(hist_bytes, 1)), N.DeviceBuffer(off.nbytes)
            if hist_bytes:
                d_hist.upload(chars)
            d_hoff.upload(off)
        text_cap = n * N.FB_ZEEK_FIXED_MAX + hist_bytes
        d_text, d_off, d_stats = N.DeviceBuffer(max(text_cap, 1)), N.DeviceBuffer(8 * (n + 1)), N.DeviceBuffer(64)
        if self.history_on_device and n:
            N.check(lib.fb_format_zeek_hist_dev(self.ctx, d_views.ptr, n, d_hist.ptr, d_hoff.ptr, d_text.ptr, text_cap,
                                                d_off.ptr, d_stats.ptr, None))
        else:
            N.check(lib.fb_format_zeek_dev(self.ctx, d_views.ptr, n, d_hist.ptr if d_hist else None,
                                           d_hoff.ptr if d_hoff else None, n_slots, d_text.ptr, text_cap, d_off.ptr,
                                           d_stats.ptr, None))
        st = stats_dict(d_stats.download(np.zeros(1, dtype=N.ZEEK_STATS_DTYPE)), N.ZEEK_STATS_FIELDS)
        if st["hist_mismatch"]:
            raise N.FbError(N.FB_ERR_INTERNAL, "%d flows whose history length differs from the table's hist_len"
                            % st["hist_mismatch"])
        if st["lines_written"] != n:
            raise N.FbError(N.FB_ERR_INTERNAL, "%d of %d lines fit the text buffer" % (st["lines_written"], n))
        line_off = d_off.download(np.zeros(n + 1, dtype=np.uint64))
        text = np.zeros(st["bytes"], dtype=np.uint8)
        if st["bytes"]:
            d_text.download(text, st["bytes"])
        return ZeekLog(text, line_off, st)

    def get_sessions_zeek(self, now_ns=None, incremental=False):
        """get_sessions as conn.log text: the flows that pass the current filter, the table aged first when
        now_ns is given, incremental (timed captures) the flows modified since this getter's last full fetch
        with a now_ns -> ZeekLog.  The getter has a fetch timestamp of its own, so a periodic exporter leaves
        get_sessions' incremental state alone; reset_fetch_timestamps resets it too."""
        if incremental and not self.timed:
            raise ValueError("incremental fetches need a timed capture (timed=True): last_modified has no clock")
        since = self._zeek_fetch_ts if incremental else None
        if now_ns is not None:
            self.update_sessions_status(now_ns)
            if not incremental:
                self._zeek_fetch_ts = int(now_ns)
        return self.export_zeek(N.FB_VIEW_ALL, since, self.filter)

    # ---- new-session enrichment (src/packets.rs:429-485) -------------------------------------
    def set_asn_tables(self, v4, v6, records=None):
        """ASN_RANGE_DTYPE tables (flodbadd_amd.enrich.asn_tables_from_tsv) -> fb_set_asn_tables.
        records: that function's third result, the (as_number, country, owner) of every
        fb_asn_range.record -- what the whitelist pass needs for an endpoint's as_owner / as_country."""
        v4 = np.ascontiguousarray(v4, dtype=N.ASN_RANGE_DTYPE)
        v6 = np.ascontiguousarray(v6, dtype=N.ASN_RANGE_DTYPE)
        N.check(N.gpu_lib().fb_set_asn_tables(self.ctx, N.ptr(v4) if len(v4) else None, len(v4),
                                              N.ptr(v6) if len(v6) else None, len(v6)))
        self._asn_records = list(records) if records is not None else []
        self._wl_installed = None  # the interned record ids belong to the installed list

    def set_blacklists(self, cidrs, names=None):
        """CIDR_DTYPE ranges (flodbadd_amd.enrich.blacklists_from_json) -> fb_set_blacklists.  names:
        that function's second result, the name of list l (the criticality tags need them; without
        them list l is called "l")."""
        cidrs = np.ascontiguousarray(cidrs, dtype=N.CIDR_DTYPE)
        N.check(N.gpu_lib().fb_set_blacklists(self.ctx, N.ptr(cidrs) if len(cidrs) else None, len(cidrs)))
        self._bl_names = list(names) if names is not None else [str(l) for l in range(N.FB_MAX_BLACKLISTS)]

    def ip_lookup(self, ips):
        """get_asn + is_ip_blacklisted for addresses (strings / ipaddress objects) ->
        (int32 ASN records, -1 = None; uint64 list masks)."""
        t = own_ip_table(list(ips))
        n = len(t)
        d_ip = N.DeviceBuffer(max(t.nbytes, 1))
        if n:
            d_ip.upload(t)
        d_a, d_l = N.DeviceBuffer(max(4 * n, 4)), N.DeviceBuffer(max(8 * n, 8))
        N.check(N.gpu_lib().fb_ip_lookup_dev(self.ctx, d_ip.ptr, n, d_a.ptr, d_l.ptr, None))
        return d_a.download(np.zeros(max(n, 1), dtype=np.int32))[:n], d_l.download(np.zeros(max(n, 1), dtype=np.uint64))[:n]

    def enrich(self, new_only=False):
        """fb_flow_enrich_dev -> FLOW_ENRICH_DTYPE records (slot-keyed; join with export_flows)."""
        return self._compact_export("fb_flow_enrich_dev", [N.FLOW_ENRICH_DTYPE], 1 if new_only else 0)[0]

    # ---- blacklist pass (src/blacklists.rs:404-437, 456-731; src/capture.rs:1680-1783, 1850-1871) ---
    def set_custom_blacklists(self, blacklist_json):
        """set_custom_blacklists (src/capture.rs:1772-1783): a BlacklistsJSON document (text) replaces
        the installed lists -- no local-range filtering for custom lists -- and the sessions are
        re-evaluated at once (update_sessions).  "" resets to no lists: there is no built-in database.
        Text that is not a BlacklistsJSON raises ValueError and the installed lists stay as they were."""
        model = Blacklists(blacklist_json)  # raises before anything is replaced
        self.set_blacklists(model.cidrs, model.names)
        self._blacklists = model
        return self.update_sessions(None, *self._wl_inputs)

    def get_blacklists(self):
        """get_blacklists (src/capture.rs:459): the custom model as BlacklistsJSON text."""
        return self._blacklists.to_json()

    def update_blacklist(self, mark_whitelist=True):
        """recompute_blacklist_for_sessions over every session (fb_flow_blacklist) and, with
        mark_whitelist, the fallback after it (src/capture.rs:1858-1871): a blacklisted session whose
        whitelist state is Unknown becomes NonConforming, "Session is blacklisted".  Returns the
        pass's counters (fb_bl_stats)."""
        st = np.zeros(1, dtype=N.BL_STATS_DTYPE)
        N.check(N.gpu_lib().fb_flow_blacklist(self.ctx, N.FB_BL_MARK_WHITELIST if mark_whitelist else 0, N.ptr(st),
                                              None))
        out = stats_dict(st, N.BL_STATS_FIELDS)
        self._bl_ran = True
        self._bl_marked = self._bl_marked or out["wl_marked"] > 0
        return out

    def blacklist_masks(self):
        """fb_flow_blacklist_dev: the blacklist mask of every table slot (index = fb_flow_rec.slot,
        bit l = list l); all zero before the first pass."""
        return self._plane("fb_flow_blacklist_dev", np.uint64)

    def export_blacklisted_flows(self):
        """fb_flow_export_blacklisted_dev: (the flows with a non-zero mask, their masks), slot order."""
        return self._compact_export("fb_flow_export_blacklisted_dev", [N.FLOW_REC_DTYPE, np.uint64])

    def get_blacklisted_sessions(self, now_ns=None, incremental=False):
        """get_blacklisted_sessions(false) (src/capture.rs:1680-1719): after an update, the sessions of
        the blacklisted list as SessionInfo, in the order new_blacklisted_sessions.sort() leaves the
        keys (src/blacklists.rs:693).  incremental: as get_sessions, with this getter's own fetch timestamp
        (capture.rs:1688-1715)."""
        since = self._since("blacklisted", incremental)
        self.update_sessions(now_ns, *self._wl_inputs)
        self._fetched("blacklisted", now_ns, incremental)
        return self._view_sessions(N.FB_VIEW_BLACKLISTED, since, whitelist=bool(self._wl_name or self._bl_marked))

    def get_blacklisted_status(self, now_ns=None):
        """get_blacklisted_status (src/capture.rs:1762-1770): after an update, some session is blacklisted."""
        return self.update_sessions(now_ns, *self._wl_inputs)["blacklist"]["blacklisted"] > 0

    def update_sessions(self, now_ns=None, dns_resolutions=None, process_names=None):
        """update_sessions_internal's per-session passes in the reference's order (src/capture.rs:
        1811-1882): the status (timed captures, when now_ns is given), the L7 pass when a socket snapshot is
        installed (set_l7_sockets; src/capture.rs:1815-1822), the domain pass when the capture
        tracks DNS (src/capture.rs:1824-1848), the blacklist pass with its whitelist fallback, then the
        whitelist pass when a list is active -- with the tracked resolutions when the caller hands it
        none.  Returns the calls' counters ({"status", "blacklist", "whitelist", "domains"}, and "l7" on a capture
        with a snapshot installed; None for a pass that did not run).  With now_ns the passes stamp the sessions
        they change with it (set_pass_time)."""
        if now_ns is not None:
            self.set_pass_time(now_ns)
        age = self.update_sessions_status(now_ns) if (self.timed and now_ns is not None) else None
        l7 = self.update_l7() if (self._l7_installed and self.flow_capacity) else None
        dom = self.update_domains() if (self.track_dns and self.flow_capacity) else None
        bl = self.update_blacklist(mark_whitelist=True)
        wl = self.update_whitelist(dns_resolutions, process_names)
        out = {"status": age, "blacklist": bl, "whitelist": wl, "domains": dom}
        if l7 is not None:  # (only a capture with a snapshot installed has the entry)
            out["l7"] = l7
        return out

    # ---- anomaly pass (src/analyzer.rs; fb_flow_anomaly) ------------------------------------------
    def set_anomaly_model(self, forest, stats, thresholds, service_codes=None):
        """Install a model on the device (fb_set_anomaly_model): an analyzer.Forest, feature_stats' result
        (mean, std, has_stats), the (suspicious, abnormal) SCORE thresholds -- turned into path cuts with
        path_cut -- and the service codes (default: analyzer.default_service_codes).  A forest the device
        rejects raises FbError and the installed model stays."""
        mean, std, has = stats
        prm = np.zeros(1, dtype=N.AN_PARAMS_DTYPE)
        prm[0]["mean"], prm[0]["std"], prm[0]["has_stats"] = mean, std, 1 if has else 0
        prm[0]["suspicious_cut"] = path_cut(thresholds[0], forest.sample_size, forest.n_trees)
        prm[0]["abnormal_cut"] = path_cut(thresholds[1], forest.sample_size, forest.n_trees)
        prm[0]["sample_size"] = forest.sample_size
        codes = np.ascontiguousarray(default_service_codes() if service_codes is None else service_codes, dtype=np.uint32)
        if codes.size != 65536:
            raise ValueError("service codes: one uint32 per port (65536), got %d" % codes.size)
        N.check(N.gpu_lib().fb_set_anomaly_model(self.ctx, N.ptr(forest.nodes), len(forest.nodes), N.ptr(forest.first),
                                                 forest.n_trees, N.ptr(prm), N.ptr(codes)))
        self._an_model = (forest, (list(mean), list(std), bool(has)), (float(thresholds[0]), float(thresholds[1])))
        self._an_codes = True

    def clear_anomaly_model(self):
        """fb_clear_anomaly_model: no model, every record back to zero."""
        N.check(N.gpu_lib().fb_clear_anomaly_model(self.ctx))
        self._an_model = None

    def anomaly_pass(self):
        """fb_flow_anomaly with the installed model -> the pass's counters (fb_an_stats)."""
        st = np.zeros(1, dtype=N.AN_STATS_DTYPE)
        N.check(N.gpu_lib().fb_flow_anomaly(self.ctx, 0, N.ptr(st), None))
        return stats_dict(st, N.AN_STATS_FIELDS)

    def anomaly_records(self):
        """fb_flow_anomaly_dev: the AN_REC_DTYPE record of every table slot (index = fb_flow_rec.slot); all
        zero before the first pass."""
        return self._plane("fb_flow_anomaly_dev", N.AN_REC_DTYPE)

    def export_features(self):
        """fb_flow_features_dev: (float64 [flows][10], their table slots) -- the training data."""
        if not self._an_codes:  # feature 7 reads the device's service codes: the defaults, unless a model brought its own
            N.check(N.gpu_lib().fb_set_service_codes(self.ctx, N.ptr(default_service_codes())))
            self._an_codes = True
        return self._compact_export("fb_flow_features_dev", [(np.float64, (N.FB_AN_FEATURES,)), np.uint32])

    def export_anomalous_flows(self, min_level=N.FB_AN_SUSPICIOUS):
        """fb_flow_export_anomalous_dev: (the flows at min_level or above, their records)."""
        return self._compact_export("fb_flow_export_anomalous_dev", [N.FLOW_REC_DTYPE, N.AN_REC_DTYPE], int(min_level))

    def analyze_sessions(self, now_ns=None):
        """SessionAnalyzer::analyze_sessions (src/analyzer.rs:1200-1570) over every session -- the consumer's
        call, not part of update_sessions.  Every flow's vector joins the analyzer's recent_data (Session
        order); during the warm-up (30 s of the caller's clock from the first call) the model is trained and
        sessions without a tag read "anomaly:normal/warming_up"; after it the model is trained if there is
        none ("anomaly:normal/no_model" while fewer than two distinct vectors exist), installed, and one
        device pass scores every flow.  Returns the pass's counters, or None when no pass ran.  With now_ns
        the pass stamps the sessions whose tag it changes with it (set_pass_time)."""
        if now_ns is not None:
            self.set_pass_time(now_ns)
        a = self.analyzer
        feats, slots = self.export_features()
        flows = self.export_flows()
        by_slot = {int(s): k for k, s in enumerate(slots)}
        order = sorted(range(len(flows)), key=lambda k: Session.from_key(flows[k]).sort_key())
        a.add_session_data(feats[by_slot[int(flows[k]["slot"])]] for k in order)
        warming = a.warming_up(now_ns)
        if warming or a.forest is None:
            a.train()
            self._an_model = None
        if warming:
            self._an_mode = "warming_up"
            return None
        if a.forest is None:
            self._an_mode = "no_model"
            return None
        want = (a.forest, a.stats, (a.suspicious_threshold, a.abnormal_threshold))
        if self._an_model is None or self._an_model[0] is not want[0] or self._an_model[1:] != want[1:]:
            self.set_anomaly_model(*want)
        self._an_mode = "model"
        return self.anomaly_pass()

    def _merge_anomaly(self, infos, flows, recs):
        """The anomaly: tag of the last analysis merged into each SessionInfo's criticality; before any
        analysis nothing changes.  A flow no pass has seen (inserted since) keeps what it has.  flows: the
        fb_flow_rec records the infos were made from; recs: their AN_REC_DTYPE records, recs[k] that of flows[k]."""
        if self._an_mode is None or not infos:
            return infos
        if self._an_mode == "model":
            rec_of = {Session.from_key(r): rec for r, rec in zip(flows, recs)}
            for i in infos:
                rec = rec_of[i.session]
                if rec["level"]:
                    i.criticality = merge_criticality(i.criticality, *anomaly_tag_of(rec))
        elif self._an_mode == "warming_up":
            for i in infos:
                if not i.criticality:
                    i.criticality = "anomaly:normal/warming_up"   # src/analyzer.rs:1288-1292
        else:
            for i in infos:
                if "blacklist:" not in i.criticality:
                    i.criticality = "anomaly:normal/no_model"     # src/analyzer.rs:1547-1551
        return infos

    def get_anomalous_sessions(self, now_ns=None):
        """get_anomalous_sessions: the suspicious and abnormal sessions of the last analysis as SessionInfo,
        in Session order, each as get_sessions reports it."""
        if self._an_mode != "model":
            return []
        return self._view_sessions(N.FB_VIEW_ANOMALOUS, whitelist=bool(self._wl_name or self._bl_marked),
                                   blacklist=self._bl_ran)

    def get_anomalous_status(self):
        """get_anomalous_status: some session of the last analysis is suspicious or abnormal."""
        if self._an_mode != "model":
            return False
        return len(self.export_anomalous_flows(N.FB_AN_SUSPICIOUS)[0]) > 0

    # ---- whitelist conformance (src/whitelists.rs:810-1023, src/capture.rs:131-183, 463-531) ---
    def set_custom_whitelists(self, whitelist_json):
        """set_custom_whitelists (src/capture.rs:463-509): a WhitelistsJSON document (str or dict)
        becomes the model and "custom_whitelist" the active list; an empty one clears the model (and
        the name, if it was the custom list).  The states are reset and one pass runs; returns its
        counters (None without an active list)."""
        if not whitelist_json:
            self._whitelists = Whitelists()
            if self._wl_name == "custom_whitelist":
                self._wl_name = ""
        else:
            try:
                self._whitelists = Whitelists(whitelist_json)
                self._wl_name = "custom_whitelist"
            except (ValueError, TypeError, KeyError):
                self._wl_name = ""  # "Error setting custom whitelists" (capture.rs:501-506)
        self.reset_whitelist()
        return self.update_whitelist()

    def set_whitelist(self, name):
        """set_whitelist (src/capture.rs:151-179).  There are no built-in lists: a name other than ""
        must be a list of the model set_custom_whitelists loaded."""
        if name and name not in self._whitelists.whitelists:
            raise ValueError("Invalid whitelist name: %s" % name)
        self._wl_name = name
        self.reset_whitelist()
        return self.update_whitelist()

    def get_whitelist_name(self):
        return self._wl_name

    def reset_whitelist(self):
        """reset_whitelist (src/capture.rs:131-149): conformance true, no exceptions, every session
        Unknown (fb_clear_whitelist; the next update installs the list again)."""
        N.check(N.gpu_lib().fb_clear_whitelist(self.ctx))
        self._bl_marked = False  # (the blacklist fallback's bytes are gone with the others)
        self._wl_installed = None
        self._wl_host_ok = set()
        self._wl_conformance = True

    def whitelist_bytes(self):
        """fb_flow_whitelist_dev: the whitelist state byte of every table slot (index = fb_flow_rec.slot)."""
        return self._plane("fb_flow_whitelist_dev", np.uint8)

    def export_whitelist_flows(self, state_mask):
        """fb_flow_export_whitelist_dev: the flows whose state byte has a bit of state_mask, slot order."""
        return self._compact_export("fb_flow_export_whitelist_dev", [N.FLOW_REC_DTYPE], int(state_mask))[0]

    def install_whitelist(self, compiled):
        """fb_set_whitelist with a CompiledWhitelist (or bare WL_ENDPOINT_DTYPE rows); fb_set_whitelist_dom with
        one compiled with domain_patterns."""
        rows = np.ascontiguousarray(getattr(compiled, "rows", compiled), dtype=N.WL_ENDPOINT_DTYPE)
        own = np.ascontiguousarray(getattr(compiled, "rec_owner_id", np.zeros(0)), dtype=np.uint32)
        cty = np.ascontiguousarray(getattr(compiled, "rec_country_id", np.zeros(0)), dtype=np.uint32)
        if getattr(compiled, "ep_pattern", None) is not None:
            epp = np.ascontiguousarray(compiled.ep_pattern, dtype=np.uint32)
            blob = np.ascontiguousarray(compiled.pattern_bytes, dtype=np.uint8)
            off = np.ascontiguousarray(compiled.pattern_off, dtype=np.uint64)
            if len(epp) != len(rows):
                raise ValueError("ep_pattern has %d entries for %d rows" % (len(epp), len(rows)))
            N.check(N.gpu_lib().fb_set_whitelist_dom(
                self.ctx, N.ptr(rows) if len(rows) else None, len(rows), N.ptr(epp) if len(epp) else None,
                N.ptr(blob) if len(blob) else None, N.ptr(off), len(off) - 1, N.ptr(own) if len(own) else None,
                N.ptr(cty) if len(own) else None, len(own)))
            return
        N.check(N.gpu_lib().fb_set_whitelist(self.ctx, N.ptr(rows) if len(rows) else None, len(rows),
                                             N.ptr(own) if len(own) else None, N.ptr(cty) if len(own) else None,
                                             len(own)))

    def whitelist_pass(self):
        """fb_flow_whitelist: one pass over the table -> the call's counters (fb_wl_stats)."""
        st = np.zeros(1, dtype=N.WL_STATS_DTYPE)
        N.check(N.gpu_lib().fb_flow_whitelist(self.ctx, 0, N.ptr(st), None))
        return stats_dict(st, N.WL_STATS_FIELDS)

    def whitelist_name_matches(self, ids):
        """fb_wl_name_matches_dev: (rows, flags) of the given DNS name ids -- rows[i] the ids (1-based, ascending,
        zero-padded) of the installed domain patterns name ids[i] matches, at most FB_WL_NAME_MATCHES; flags[i]
        bit 0: it matches more.  Brings the device's match state up to date first."""
        a = np.ascontiguousarray(ids, dtype=np.uint32)
        n = len(a)
        d_ids = N.DeviceBuffer(max(a.nbytes, 4)).upload(a)
        d_rows, d_flags = N.DeviceBuffer(max(n, 1) * N.FB_WL_NAME_MATCHES * 4), N.DeviceBuffer(max(n, 1))
        N.check(N.gpu_lib().fb_wl_name_matches_dev(self.ctx, d_ids.ptr, n, d_rows.ptr, d_flags.ptr, None))
        return (d_rows.download(np.zeros((n, N.FB_WL_NAME_MATCHES), dtype=np.uint32)) if n else
                np.zeros((0, N.FB_WL_NAME_MATCHES), dtype=np.uint32),
                d_flags.download(np.zeros(n, dtype=np.uint8)) if n else np.zeros(0, dtype=np.uint8))

    def whitelist_domain_info(self):
        """fb_wl_dom_info_get: the installed patterns per kind ({"exact", "suffix", "prefix", "general",
        "never"}), and names_done / names_matched / names_overflowed of the names matched so far."""
        t = np.zeros(1, dtype=N.WL_DOM_INFO_DTYPE)
        N.check(N.gpu_lib().fb_wl_dom_info_get(self.ctx, N.ptr(t)))
        out = {k: int(v) for k, v in zip(N.WL_DOM_KINDS, t[0]["patterns"])}
        out.update({f: int(t[0][f]) for f in ("names_done", "names_matched", "names_overflowed")})
        return out

    def _dst_asn(self, ips):
        """SessionInfo.dst_asn of destination addresses (src/packets.rs:468-485): Db::lookup on the GPU
        unless it is a LAN address -> [(as_number, country, owner) or None]."""
        rec = self.ip_lookup(ips)[0] if ips else []
        return [None if (int(k) < 0 or int(k) >= len(self._asn_records) or is_lan_ip(ip, self._lan_v6))
                else self._asn_records[int(k)] for ip, k in zip(ips, rec)]

    def update_whitelist(self, dns_resolutions=None, process_names=None):
        """recompute_whitelist_for_sessions (src/whitelists.rs:810-1023) for every session: nothing
        happens without an active list (whitelists.rs:840-845); otherwise the active list -- with the
        domains of dns_resolutions {ip: domain} expanded to addresses -- is installed if it is not yet
        and the table is evaluated in one pass.  process_names {Session: process name}: the flows the
        pass marks for a host check are then decided by the full endpoint_matches with their domain
        and process.  A capture that tracks DNS uses its own resolutions when dns_resolutions is None, and one
        whose L7 pass has run the device's process attribution when process_names is None.
        processes_on_device (and process_names None): the list is compiled with process ids, the pass decides
        the process endpoints itself -- and stamps what it changes --, no {Session: name} dictionary is
        downloaded, and only the flows a domain endpoint marks go through the host loop, with the processes
        of just those flows.
        domains_on_device (and dns_resolutions None): the list is compiled with its domain patterns and no
        resolutions -- a new resolution changes nothing installed --, the pass decides the domain endpoints from
        the domain plane, and the host loop sees only the flows of an overflowed name or of a pattern without an
        id, with the dst_domain of just those flows.
        Returns the pass's counters, or None."""
        self._wl_inputs = (dns_resolutions, process_names)
        self._wl_proc = None
        if not self._wl_name:
            return None
        dom_dev = self._device_domains(dns_resolutions)
        if dns_resolutions is None and self.track_dns and not dom_dev:  # the capture's own passive resolutions
            dns_resolutions = {str(ip): name for ip, name in self.dns_resolutions().items()}
        want = dict(dns_resolutions or {})
        on_dev = self._device_processes(process_names)
        if (self._wl_installed is None or self._wl_installed[1] != want or self._wl_with_ids != on_dev
                or self._wl_dom != dom_dev):
            comp = self._whitelists.compile(self._wl_name, self._asn_records, None if dom_dev else want,
                                            process_ids=self._proc_names if on_dev else None, domain_patterns=dom_dev)
            self.install_whitelist(comp)
            self._wl_installed = (comp, want)
            self._wl_with_ids = on_dev
            self._wl_dom = dom_dev
            self.wl_installs += 1
        comp = self._wl_installed[0]
        stats = self.whitelist_pass()
        self._wl_host_ok = set()
        marked = None
        if stats["host_check"] and on_dev:  # domain keys only: the processes of just those flows
            marked = self.export_whitelist_flows(N.FB_WL_HOST_CHECK)
            process_names = self._slot_process_names(marked)
            host_loop = bool(process_names)
        else:
            if stats["host_check"]:
                process_names = self._wl_proc = self._process_names(process_names)
            host_loop = bool(process_names) and bool(stats["host_check"])
        domain_of = None
        if dom_dev and stats["host_check"]:  # what the rows could not decide: the domains of just those flows
            if marked is None:
                marked = self.export_whitelist_flows(N.FB_WL_HOST_CHECK)
            domain_of = self._slot_domains(marked)
            process_names = process_names or {}
            host_loop = True
        if host_loop:
            if marked is None:
                marked = self.export_whitelist_flows(N.FB_WL_HOST_CHECK)
            marked = [Session.from_key(r) for r in marked]
            for s, asn in zip(marked, self._dst_asn([s.dst_ip for s in marked])):
                a = asn or (None, None, None)
                dom = domain_of.get(s) if domain_of is not None else want.get(str(s.dst_ip))
                if is_session_in_whitelist(comp.endpoints, comp.name, dom, str(s.dst_ip), s.dst_port,
                                           s.protocol.name, a[0], a[1], a[2], process_names.get(s))[0]:
                    self._wl_host_ok.add(s)
        exc = self.export_whitelist_flows(N.FB_WL_NONCONFORMING)
        self._wl_conformance = not any(Session.from_key(r) not in self._wl_host_ok for r in exc)
        return stats

    def get_whitelist_conformance(self):
        """get_whitelist_conformance (src/capture.rs:1672-1678): after an update, no exception exists."""
        self.update_whitelist(*self._wl_inputs)
        return self._wl_conformance

    def get_whitelist_exceptions(self, now_ns=None, incremental=False):
        """get_whitelist_exceptions(false) (src/capture.rs:1721-1760): the NonConforming sessions as
        SessionInfo, sorted by Session as new_exceptions.sort() leaves the keys (whitelists.rs:951),
        each with the reference's whitelist_reason.  With now_ns the pass stamps the sessions it changes
        with it; incremental: as get_sessions, with this getter's own fetch timestamp (capture.rs:1729-1756).
        The host's verdict for a host-check flow (process names) applies to full and incremental fetches alike
        and stamps nothing."""
        since = self._since("exceptions", incremental)
        if now_ns is not None:
            self.set_pass_time(now_ns)
        self.update_whitelist(*self._wl_inputs)
        self._fetched("exceptions", now_ns, incremental)
        if not self._wl_name:  # no list is active: no exceptions, whatever the blacklist fallback marked
            return []
        host_ok = self._wl_host_ok  # (the sessions the host resolved to Conforming are no exceptions)
        keep = (lambda v: np.array([Session.from_key(r) not in host_ok for r in v["rec"]], dtype=bool)) if host_ok else None
        out = self._view_sessions(N.FB_VIEW_WL_EXCEPTIONS, since, whitelist=False, blacklist=False, keep=keep)
        proc = self._wl_proc or self._wl_inputs[1] or {}
        if self._wl_with_ids:  # the processes the device decided with: the returned sessions' own l7
            proc = {i.session: i.l7.process_name for i in out if i.l7 is not None}
        comp, dns = self._wl_installed  # (the resolutions the installed list was compiled with)
        for info, asn in zip(out, self._dst_asn([i.session.dst_ip for i in out])):
            s, a = info.session, asn or (None, None, None)
            # (an exception is a session no endpoint matched: the reason needs no second scan of the list)
            info.is_whitelisted = WhitelistState.NonConforming
            dom = info.dst_domain if self._wl_dom else dns.get(str(s.dst_ip))  # (the domain the device decided with)
            info.whitelist_reason = no_match_reason(comp.endpoints, comp.name, dom, str(s.dst_ip),
                                                    s.dst_port, s.protocol.name, a[0], a[1], a[2], proc.get(s))
        return out

    def _learned(self, view_set, dns_resolutions=None, processes=False):
        """The custom_whitelist model learned on the device from the flows of view_set (learn_endpoints,
        Whitelists.from_learned).  A capture that tracks DNS brings the flows' domains forward first
        (update_domains: dst_domain as the reference's sessions carry it); dns_resolutions {ip: domain}, when
        given, stands for dst_domain instead, as on the host path.  processes (processes_on_device): the records
        carry the flows' process name ids, and the endpoints come in the order of their representative sessions
        -- the order new_from_sessions meets them in a sorted session list, so the document is the host path's."""
        if self.track_dns and dns_resolutions is None:
            self.update_domains()
        recs, _ = self.learn_endpoints(view_set)
        names = self.dns_names(recs["dst_name_id"]) if (self.track_dns and dns_resolutions is None) else {}
        if processes:
            def rep_key(r):  # the representative session's place in Session's derived Ord
                fam = int(r["family"])
                return Session(Protocol(int(r["protocol"])), words_to_ip(r["rep_src_ip"], fam), int(r["rep_src_port"]),
                               words_to_ip(r["dst_ip"], fam), int(r["dst_port"])).sort_key()
            recs = recs[sorted(range(len(recs)), key=lambda k: rep_key(recs[k]))]
        w = Whitelists.from_learned(recs, names, self._proc_names.names if processes else None)
        if dns_resolutions is not None:
            info = w.whitelists["custom_whitelist"]
            for ep in info.endpoints:
                dom = dns_resolutions.get(ep.ip)
                ep.domain = None if dom in ("Unknown", "Resolving") else dom
            info.endpoints = dedup_endpoints(info.endpoints)  # (ids told apart what one dictionary entry names)
        return w

    def create_custom_whitelists(self, dns_resolutions=None, process_names=None, on_device=False):
        """create_custom_whitelists (src/capture.rs:511-531): the WhitelistsJSON text of a list learned
        from every session of the table.  on_device: the distinct endpoints and their representative
        sessions are found by one pass on the device (learn_endpoints) instead of a download of every flow;
        the endpoints are then in table-slot order of their representatives, and the domains those the capture
        tracked itself (track_dns) unless dns_resolutions is given.  With processes_on_device (and no
        process_names from the caller) the device's fingerprint holds the process and the document is the host
        path's, endpoint for endpoint.  Otherwise it holds none: with a non-empty process_names -- the caller's,
        or the L7 pass's attribution when the caller gives none -- the host path runs, whatever on_device says."""
        if on_device and self._device_processes(process_names):
            return self._learned(N.FB_VIEW_ALL, dns_resolutions, processes=True).to_json()
        process_names = self._process_names(process_names)
        if on_device and not process_names:
            return self._learned(N.FB_VIEW_ALL, dns_resolutions).to_json()
        sessions = flows_to_sessions(self.export_flows(SessionFilter.All))
        return Whitelists.new_from_sessions(sessions, dns_resolutions, process_names).to_json()

    def augment_custom_whitelists(self, now_ns=None, dns_resolutions=None, process_names=None):
        """augment_custom_whitelists (src/capture.rs:533-612): the current model's custom_whitelist (none: no
        endpoints, no extends) with the endpoints learned from the current whitelist exceptions appended,
        de-duplicated by fingerprint -- existing endpoints win --, as compact WhitelistsJSON text: one list named
        custom_whitelist, the `extends` preserved, today's date, no signature.  With now_ns the sessions are
        brought forward first (update_sessions), else the whitelist pass runs with the inputs given here or,
        without any, the stored ones (as get_whitelist_exceptions).  The exceptions' endpoints are learned on
        the device over FB_VIEW_WL_EXCEPTIONS; with process names -- which the device does not hold, and which
        can make the host accept a session the pass marked -- on the host from get_whitelist_exceptions().
        Without an active list there are no exceptions: the current custom list comes back re-dated."""
        if dns_resolutions is None and process_names is None:
            dns_resolutions, process_names = self._wl_inputs
        if now_ns is not None:
            self.update_sessions(now_ns, dns_resolutions, process_names)
        else:
            self.update_whitelist(dns_resolutions, process_names)
        on_dev = self._device_processes(process_names)
        if not on_dev:
            process_names = self._process_names(process_names)
        cur = self._whitelists.whitelists.get("custom_whitelist")
        endpoints, extends = (list(cur.endpoints), cur.extends) if cur else ([], None)
        if not self._wl_name:
            learned = []
        elif on_dev and not self._wl_host_ok:  # (a session the host accepted is no exception: then its list decides)
            learned = self._learned(N.FB_VIEW_WL_EXCEPTIONS, dns_resolutions, processes=True)
        elif on_dev:
            dns = dns_resolutions
            if dns is None and self.track_dns:
                dns = {str(ip): name for ip, name in self.dns_resolutions().items()}
            exc = self.get_whitelist_exceptions()
            learned = Whitelists.new_from_sessions(exc, dns, {i.session: i.l7.process_name for i in exc if i.l7 is not None})
        elif process_names:
            dns = dns_resolutions
            if dns is None and self.track_dns:
                dns = {str(ip): name for ip, name in self.dns_resolutions().items()}
            learned = Whitelists.new_from_sessions(self.get_whitelist_exceptions(), dns, process_names)
        else:
            learned = self._learned(N.FB_VIEW_WL_EXCEPTIONS, dns_resolutions)
        if learned:
            learned = learned.whitelists["custom_whitelist"].endpoints
        return Whitelists().as_custom(dedup_endpoints(endpoints + learned), extends).to_json(compact=True)

    @staticmethod
    def merge_custom_whitelists(json_a, json_b):
        """merge_custom_whitelists (src/capture.rs:614-625): Whitelists.merge_custom_whitelists."""
        return Whitelists.merge_custom_whitelists(json_a, json_b)

    def clear_all_sessions(self):
        """src/capture.rs:396 (`stop()` clears the table, capture.rs:383)."""
        N.check(N.gpu_lib().fb_flow_clear(self.ctx, None))
        N.check(N.gpu_lib().fb_stream_sync(None))
        if not self.history_on_device:  # (fb_flow_clear emptied the device store)
            self.histories = {}
        self._wl_host_ok = set()
        self._bl_marked = False
        self._dom_ran = False

    def close(self):
        if getattr(self, "ctx", None):
            N.gpu_lib().fb_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IngestRing:
    """fb_ring_* (include/flodbadd_gpu.h): the capture reader's batch ring in front of a
    FlodbaddGpuCapture's context -- replaces the reader -> Vec<u8> -> mpsc(1000) -> processor
    path (src/capture.rs:1016, 1082-1142).  Frames are appended into pinned batches, each full
    batch is copied in, parsed, classified and upserted into the context's session table on the
    GPU while the next one fills; the producer waits (never drops) when every batch is in flight."""

    def __init__(self, capture, slots=4, max_packets=1 << 20, max_bytes=64 << 20, flow=True):
        self.lib = N.gpu_lib()
        cfg = N.FbRingConfig(slots, max_packets, max_bytes, 0 if flow else N.FB_RING_NO_FLOW, 0)
        r = self.lib.fb_ring_create(capture.ctx, C.byref(cfg))
        if not r:
            raise N.FbError(N.FB_ERR_INVAL, self.lib.fb_last_error().decode(errors="replace"))
        self.r = C.c_void_p(r)
        self.capture = capture  # the context must outlive the ring

    def push(self, frame):
        f = np.frombuffer(bytes(frame), dtype=np.uint8)
        N.check(self.lib.fb_ring_push(self.r, N.ptr(f) if f.size else None, f.size))

    def push_block(self, frames, offsets):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        N.check(self.lib.fb_ring_push_block(self.r, N.ptr(frames), N.ptr(offsets), offsets.size - 1))

    def sync(self):
        N.check(self.lib.fb_ring_sync(self.r))

    def stats(self):
        """(PACKET_STATS totals over the completed batches, batches completed, frames pushed)."""
        tot = np.zeros(1, dtype=N.STATS_DTYPE)
        nb, nf = C.c_uint64(), C.c_uint64()
        N.check(self.lib.fb_ring_stats(self.r, N.ptr(tot), C.byref(nb), C.byref(nf)))
        return stats_dict(tot), nb.value, nf.value

    def poll_dns(self, max_records=1 << 16, max_bytes=1 << 24):
        """DNS side records of completed batches: [(packet_seq, protocol, family, payload bytes)]
        -- what the reference hands to process_dns_packet (src/capture.rs:1051-1057)."""
        out = np.zeros(max_records, dtype=N.RING_DNS_DTYPE)
        buf = np.zeros(max_bytes, dtype=np.uint8)
        n, nb = C.c_uint32(), C.c_uint64()
        N.check(self.lib.fb_ring_poll_dns(self.r, N.ptr(out), max_records, N.ptr(buf), max_bytes, C.byref(n),
                                          C.byref(nb)))
        return [(int(d["packet_seq"]), int(d["protocol"]), int(d["family"]),
                 buf[int(d["payload_offset"]): int(d["payload_offset"]) + int(d["payload_length"])].tobytes())
                for d in out[: n.value]]

    def close(self):
        if getattr(self, "r", None):
            self.lib.fb_ring_destroy(self.r)
            self.r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
