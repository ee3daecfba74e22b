"""The device history store measured against the host-dict path it replaces.

Three captures see the same C4-style batches (synth config 4, --frames frames each, --batches of them, capture
times 1 s apart, timed contexts): history off (the floor), track_history with the host dict (the path of the
parent commit, unchanged on this branch: fb_flow_history_dev, a device wait, two D2H copies and a Python loop per
batch), and history_on_device (one asynchronous fb_hist_store_append_dev per batch).

  batch    wall clock of process_frames_seg + a stream sync per batch, per mode; the first --warm batches are
           left out, the figure is the median of the rest, the spread their min .. max.
  zeek     wall clock of export_zeek() with history on the table the batches built: host blob (pack_histories +
           upload) against the store (lengths, gather, fb_format_zeek_hist_dev), everything selected and the
           ~1 % modified most recently; median of --reps after one warm-up, min .. max beside it.
  kernels  device events on the null stream: fb_hist_store_append_dev alone after an update (history launcher +
           append + commit; one sample per batch on a fourth capture) beside fb_flow_history_dev alone on the
           same batches; lengths + gather over the whole table; fb_flow_age with a purge of the flows the last
           --keep batches did not touch, with and without the store's free sweep (one sample each: a purge is
           not repeatable).  bytes: what each moves at least, and the fraction of --hbm-gbs that implies.

--lib PATH loads another build of the library (one made with -DFB_HIST_COOP_RUN=N) and --only kernels runs
just the last section: the FB_HIST_COOP_RUN A/B.

Usage: python tools/experiments/hist_store_bench.py [--frames 1048576] [--batches 7] [--warm 2] [--reps 5]
       [--zipf 1.1] [--only batch,zeek,kernels] [--lib PATH] [--out profiles/hist_store_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

S = 10 ** 9
T0 = 1_700_000_000 * S


def spread(xs, nd=4):
    return dict(median=round(statistics.median(xs), nd), min=round(min(xs), nd), max=round(max(xs), nd), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keep", type=int, default=2)
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--zipf", type=float, default=0.0, help="Zipf(s) flow popularity instead of uniform (e.g. 1.1)")
    ap.add_argument("--only", default="batch,zeek,kernels")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    only = set(a.only.split(","))

    from flodbadd_amd import _native as N
    if a.lib:
        N.GPU_LIB_PATH = os.path.abspath(a.lib)
    from flodbadd_amd import synth
    from flodbadd_amd.capture import FlodbaddGpuCapture
    from flodbadd_amd.sessions import SessionFilter

    lib, n = N.gpu_lib(), a.frames
    zipf = dict(zipf=1, zipf_s=a.zipf) if a.zipf else {}   # (hot flows: runs of thousands of characters)
    batches = [synth.generate(4, n, first=k * n, **zipf) for k in range(a.batches)]
    times = [T0 + k * S + np.arange(n, dtype=np.uint64) * 50 for k in range(a.batches)]
    res = dict(what=__doc__.split("\n\n")[1].replace("\n", " "), frames_per_batch=n, batches=a.batches, warm=a.warm,
               lib=a.lib or "default", coop_run_default=N.FB_HIST_COOP_RUN, zipf=a.zipf)

    def make(mode):
        return FlodbaddGpuCapture(0, session_filter=SessionFilter.All, flow_capacity=a.capacity, max_batch_packets=n,
                                  timed=True, track_history=mode != "off", history_on_device=mode == "device")

    caps = {}
    if only & {"batch", "zeek"}:
        res["batch_s"] = {}
        for mode in ("off", "host_dict", "device_store"):
            cap = caps[mode] = make({"host_dict": "host", "device_store": "device"}.get(mode, "off"))
            per = []
            for (fr, of), ts in zip(batches, times):
                t = time.perf_counter()
                cap.process_frames_seg(fr, of, ts=ts)
                N.check(lib.fb_stream_sync(None))
                per.append(time.perf_counter() - t)
            res["batch_s"][mode] = dict(spread(per[a.warm:]), all=[round(x, 4) for x in per])
            print(mode, res["batch_s"][mode], flush=True)
        res["flows"] = caps["off"].flow_count()
        res["store_info"] = caps["device_store"].history_store_info()
        caps.pop("off").close()

    if "zeek" in only:
        host, dev = caps["host_dict"], caps["device_store"]
        la = np.sort(dev.export_view()["time"]["last_activity_ns"])
        since = int(la[int(0.99 * len(la))])
        res["zeek_s"] = {}
        for name, cap in (("host_blob", host), ("device_store", dev)):
            for sel, kw in (("all", {}), ("1pct", dict(since_ns=since))):
                log = cap.export_zeek(**kw)                     # warm-up
                per = []
                for _ in range(a.reps):
                    t = time.perf_counter()
                    log = cap.export_zeek(**kw)
                    per.append(time.perf_counter() - t)
                res["zeek_s"]["%s.%s" % (name, sel)] = dict(spread(per), lines=len(log), text_bytes=int(len(log.text)))
                print(name, sel, res["zeek_s"]["%s.%s" % (name, sel)], flush=True)
        for sel in ("all", "1pct"):
            x, y = res["zeek_s"]["host_blob." + sel], res["zeek_s"]["device_store." + sel]
            assert (x["lines"], x["text_bytes"]) == (y["lines"], y["text_bytes"]), (x, y)
    for c in caps.values():
        c.close()

    if "kernels" in only:
        e0, e1 = N.Event(), N.Event()

        def timed_us(fn):
            N.check(lib.fb_stream_sync(None))
            e0.record(None)
            fn()
            e1.record(None)
            return e0.elapsed_ms(e1) * 1000.0

        dev, plain = make("device"), make("off")
        dev.track_history = False                              # (the append is issued here, under the events)
        nslots = (n + 63) // 64 * 64
        d_h, d_s, d_n = N.DeviceBuffer(nslots), N.DeviceBuffer(4 * nslots), N.DeviceBuffer(4)
        app, hist, chars = [], [], []
        for (fr, of), ts in zip(batches, times):
            dev.process_frames_seg(fr, of, ts=ts)
            app.append(timed_us(lambda: N.check(lib.fb_hist_store_append_dev(dev.ctx, None))))
            plain.process_frames_seg(fr, of, ts=ts)
            hist.append(timed_us(lambda: N.check(lib.fb_flow_history_dev(plain.ctx, d_h.ptr, d_s.ptr, d_n.ptr, None))))
            chars.append(int(d_n.download(np.zeros(1, dtype=np.uint32))[0]))
        dev.track_history = True
        info = dev.history_store_info()
        assert info["missed_updates"] == 0 and info["chars"] == sum(chars), info
        k = res["kernels_us"] = dict(append=dict(spread(app[a.warm:], 1), all=[round(x, 1) for x in app]),
                                     flow_history_dev=dict(spread(hist[a.warm:], 1), all=[round(x, 1) for x in hist]),
                                     chars_per_batch=chars)
        cap_slots = int(dev.table_info()["capacity"])
        d_off, d_chars = N.DeviceBuffer(8 * (cap_slots + 1)), N.DeviceBuffer(max(info["chars"], 1))

        def read_all():
            N.check(lib.fb_hist_store_lengths_dev(dev.ctx, None, 0, cap_slots, d_off.ptr, None))
            N.check(lib.fb_hist_store_gather_dev(dev.ctx, None, 0, cap_slots, d_off.ptr, d_chars.ptr, info["chars"], None))

        read_all()
        k["lengths_gather_all"] = spread([timed_us(read_all) for _ in range(a.reps)], 1)
        # bytes each moves at least: the append reads a character and a slot word per character, reads and writes a
        # 16-B element per flow it touches (bounded by the flows) and writes half a byte per character; the
        # gather reads every element and started block and writes a byte per character
        c_med = statistics.median(chars[a.warm:])
        b_app = c_med * 5.5
        b_read = cap_slots * (16 + 16) + info["blocks_in_use"] * 64 + info["chars"]
        k["bytes"] = dict(append_min=int(b_app), lengths_gather=int(b_read))
        k["hbm_fraction"] = dict(append=round(b_app / (k["append"]["median"] * 1e-6) / (a.hbm_gbs * 1e9), 4),
                                 lengths_gather=round(b_read / (k["lengths_gather_all"]["median"] * 1e-6) / (a.hbm_gbs * 1e9), 4))
        # the purge: the flows the last --keep batches did not touch
        prm = np.zeros(1, dtype=N.AGE_PARAMS_DTYPE)
        prm[0]["activity_ns"], prm[0]["current_ns"], prm[0]["retention_ns"] = 60 * S, 180 * S, a.keep * S
        now = T0 + a.batches * S
        purge = {}
        for name, cap in (("with_store", dev), ("without_store", plain)):
            st = np.zeros(1, dtype=N.AGE_STATS_DTYPE)
            t = time.perf_counter()
            N.check(lib.fb_flow_age(cap.ctx, now, N.ptr(prm), N.FB_AGE_PURGE, N.ptr(st), None))
            purge[name] = dict(wall_us=round((time.perf_counter() - t) * 1e6, 1), purged=int(st[0]["purged"]),
                               remaining=int(st[0]["remaining"]))
        k["purge"] = purge
        k["store_after_purge"] = dev.history_store_info()
        dev.close()
        plain.close()

    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
