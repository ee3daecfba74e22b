"""The anomaly pass (fb_flow_anomaly) timed on the C4 table: flow_capacity 2^21, two 10,485,760-frame C4
batches (the flows the bench's C4 stream leaves behind; an untimed table, so features 1 and 4 are 0),
with the reference's forest size: 25 trees grown on 128 of 300 vectors to depth 6.  The 300 training
vectors are every (flows / 300)-th flow in slot order.  Under device events on the null stream, medians
after warm-ups:

  first      fb_flow_anomaly over a zeroed plane: every flow's 16-B record is written (before each
             repetition fb_clear_anomaly_model zeroes the plane and the model is installed again -- not timed)
  steady     the same call again: nothing changes, nothing is written
  features   fb_flow_features_dev: the sweep with the feature arithmetic alone, 84 B written per flow
  score      fb_if_score_dev over the exported vectors: the walk alone (80 B read, 8 B written per vector)
  blacklist  the parent's fb_flow_blacklist (steady, 1,000 nets) on the same table, for scale
  host       analyzer.Forest.path_sums (numpy, one thread) over the same vectors -- the CPU figure

fb_flow_anomaly and fb_flow_blacklist are synchronous calls (counter memset, kernel, read-back, stream sync)
and the events bracket all of it.  No tracing is active.  The device's path sums are compared with the host
scorer's bit for bit before anything is timed.  Bytes per the model of DESIGN.md §3.12.
Usage: python tools/experiments/anomaly_sweep.py [--frames N] [--capacity C] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from flodbadd_amd import _native as N  # noqa: E402
from flodbadd_amd import analyzer as A  # noqa: E402
from flodbadd_amd import synth  # noqa: E402
from flodbadd_amd.capture import FlodbaddGpuCapture  # noqa: E402
from flodbadd_amd.sessions import SessionFilter  # noqa: E402
from blacklist_sweep import nets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10 * (1 << 20))
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-vectors", type=int, default=0, help="vectors the host scorer is timed on (0: all)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib, n = N.gpu_lib(), a.frames
    cap = FlodbaddGpuCapture(0, session_filter=SessionFilter.GlobalOnly, flow_capacity=a.capacity, max_batch_packets=n,
                             grow=False)
    N.check(lib.fb_set_session_records(cap.ctx, 0))
    nseg = (n + 63) // 64
    d_out, d_seg, d_st = N.DeviceBuffer(nseg * N.SEG_BYTES), N.DeviceBuffer(nseg * 4), N.DeviceBuffer(128)
    for k in range(2):
        fr, of = synth.generate(4, n, first=k * n)
        d_fr, d_of = N.DeviceBuffer(fr.nbytes).upload(fr), N.DeviceBuffer(of.nbytes).upload(of)
        N.check(lib.fb_process_seg_dev(cap.ctx, d_fr.ptr, fr.nbytes, d_of.ptr, n, d_out.ptr, d_seg.ptr, None, d_st.ptr, None))
        N.check(lib.fb_stream_sync(None))
        st = d_st.download(np.zeros(1, dtype=N.STATS_DTYPE))
        if int(st[0]["error"]):
            raise RuntimeError("update error word %d" % int(st[0]["error"]))
        del fr, of, d_fr, d_of
    del d_out, d_seg
    info = cap.table_info()
    cap_slots = int(info["capacity"])
    feats, slots = cap.export_features()
    order = np.argsort(slots)
    feats, slots = np.ascontiguousarray(feats[order]), slots[order]   # (the export's block order varies)
    flows = len(slots)
    res = dict(frames_per_batch=n, capacity=cap_slots, flows=flows, partitions=int(info["partitions"]))

    data = feats[:: max(1, flows // A.MAX_SAMPLES)][:A.MAX_SAMPLES]
    forest = A.train_forest(data, seed=1)
    stats = A.feature_stats(data)
    thr = A.compute_dynamic_thresholds(forest.score(data))
    sizes = np.diff(forest.first.astype(np.int64))
    res["forest"] = dict(trees=forest.n_trees, sample_size=forest.sample_size, nodes=int(len(forest.nodes)),
                         max_tree_nodes=int(sizes.max()), bytes=int(forest.nodes.nbytes), thresholds=thr,
                         unique_training_vectors=len(A.dedup_rows(data)))
    cap.set_anomaly_model(forest, stats, thr)

    # the device against the host scorer, every flow
    t0 = time.perf_counter()
    nh = flows if a.host_vectors <= 0 else min(a.host_vectors, flows)
    host = forest.path_sums(feats[:nh])
    res["host"] = dict(vectors=nh, seconds=time.perf_counter() - t0)
    res["host"]["us_per_1e6_vectors"] = res["host"]["seconds"] / nh * 1e12
    first_stats = cap.anomaly_pass()
    recs = cap.anomaly_records()
    dev = recs["path_sum"][slots[:nh]]
    res["equal_path_sums"] = bool(dev.tobytes() == host.tobytes())
    if not res["equal_path_sums"]:
        raise RuntimeError("device and host path sums differ in %d of %d flows" % (int((dev.view(np.uint64) != host.view(np.uint64)).sum()), nh))
    res["levels"] = first_stats

    e0, e1 = N.Event(), N.Event()

    def timed(fn):
        e0.record(None)
        r = fn()
        e1.record(None)
        return e0.elapsed_ms(e1) * 1000.0, r

    def med(fn, warm, reps, before=None):
        t = []
        for i in range(warm + reps):
            if before:
                before()
            us = timed(fn)[0]
            if i >= warm:
                t.append(us)
        t.sort()
        return dict(median_us=statistics.median(t), min_us=t[0], max_us=t[-1], reps=reps)

    def zero_plane():
        cap.clear_anomaly_model()
        cap.set_anomaly_model(forest, stats, thr)

    res["first"] = med(cap.anomaly_pass, 3, a.reps, before=zero_plane)
    res["steady"] = med(cap.anomaly_pass, 3, a.reps)
    res["steady"]["last"] = cap.anomaly_pass()

    d_f, d_s, d_n = N.DeviceBuffer(flows * 80), N.DeviceBuffer(flows * 4), N.DeviceBuffer(8)
    res["features"] = med(lambda: N.check(lib.fb_flow_features_dev(cap.ctx, d_f.ptr, d_s.ptr, flows, d_n.ptr, None)), 3, a.reps)
    d_x, d_p = N.DeviceBuffer(feats.nbytes).upload(feats), N.DeviceBuffer(flows * 8)
    res["score"] = med(lambda: N.check(lib.fb_if_score_dev(cap.ctx, d_x.ptr, flows, d_p.ptr, None)), 3, a.reps)
    got = d_p.download(np.zeros(flows))
    res["equal_score_dev"] = bool(got[:nh].tobytes() == host.tobytes())

    bl = nets(np.sort(cap.export_flows(), order="slot"), 1000, np.random.default_rng(5))
    cap.set_blacklists(bl)
    cap.update_blacklist(mark_whitelist=False)
    res["blacklist"] = med(lambda: cap.update_blacklist(mark_whitelist=False), 3, a.reps)

    # per slot its 128-B table line; per flow the 16-B record read, and written where it
    # changed; per step of 256 slots with a flow in it the whole forest staged from L2
    steps = int(len(np.unique(slots // 256)))
    scan = cap_slots * 128 + flows * 16
    res["model_bytes"] = dict(first=scan + flows * 16, steady=scan, features=cap_slots * 128 + flows * 84,
                              score=flows * 88, forest_staging=steps * int(forest.nodes.nbytes), steps=steps)
    for k in ("first", "steady", "features", "score"):
        res[k]["model_GBps"] = res["model_bytes"][k] / res[k]["median_us"] / 1e3
    res["steady"]["staging_GBps"] = res["model_bytes"]["forest_staging"] / res["steady"]["median_us"] / 1e3
    res["steady"]["ns_per_flow"] = res["steady"]["median_us"] * 1e3 / flows
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    cap.close()


if __name__ == "__main__":
    main()
