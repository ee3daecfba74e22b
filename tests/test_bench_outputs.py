"""bench.py's plain run and --dump-outputs: the plain result line carries the headline fields and
nothing that takes a run of its own, --steps sets the timed steps, and the arrays written for the
last timed step are the oracle's records for the same synthetic batch, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
N_FRAMES = 5003  # not a multiple of the 64-frame segment, more than one workgroup


def _bench(args, timeout=120):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_columns_and_sample_are_fixed():
    sys.path.insert(0, ROOT)
    import bench
    from flodbadd_amd import _native as N
    a = np.zeros(1000, dtype=N.DNS_OUT_DTYPE)
    a["pkt_index"] = np.arange(1000)
    a["protocol"] = 17
    full = bench._dump_array(a, 1 << 20)
    assert full.dtype == np.float64 and full.shape == (1000, 5)  # the reserved field is left out
    assert np.array_equal(full[:, 0], np.arange(1000)) and np.all(full[:, 3] == 17)
    cut = bench._dump_array(a, 100 * 5 * 8)
    assert cut.shape == (100, 5) and np.all(np.diff(cut[:, 0]) > 0)  # a sample, rows kept in order
    assert np.array_equal(cut, bench._dump_array(a, 100 * 5 * 8))  # the same sample every time
    assert sum(bench.DUMP_CAPS.values()) + (1 << 20) < 64 * 10 ** 6


@pytest.mark.gpu
def test_full_run_keeps_the_other_measurements():
    """--full brings back what the plain run leaves out, and the --no-* options still select among it."""
    r = _bench(["--gpus", "1", "--steps", "4", "--warmup", "2", "--packets", str(N_FRAMES), "--rotate", "4", "--full",
                "--no-c4", "--no-host", "--no-cpu-baseline", "--no-queue", "--no-imix"])
    assert sorted(r["extra"]) == ["mode_dense", "single_batch_launch"]
    assert r["extra"]["mode_dense"]["value"] > 0 and r["extra"]["single_batch_launch"]["ms_per_step"] > 0
    assert r["roofline"]["stream_copy_GBs"] > 0 and r["cpu_baseline"] is None
    assert r["steps"] == 4 and r["ms_per_step"] > 0


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    from flodbadd_amd import synth
    from oracle import coracle
    sys.path.insert(0, ROOT)
    import bench
    common = ["--gpus", "1", "--warmup", "2", "--config", "3", "--packets", str(N_FRAMES), "--rotate", "4"]
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    r1 = _bench(common + ["--steps", "3", "--dump-outputs", d1])
    r2 = _bench(common + ["--steps", "6", "--dump-outputs", d2])
    for r, k in ((r1, 3), (r2, 6)):
        assert r["steps"] == k and r["unit"] == "Mpackets/s" and r["higher_is_better"] is True and r["dtype"] == "u8"
        assert r["ms_per_step"] > 0 and r["value"] > 0
        # value and ms_per_step describe the same timed region (rounded to 2 and 4 decimals in the line)
        ms = r["ms_per_step"]
        assert N_FRAMES / (ms + 5e-5) / 1e3 - 0.01 <= r["value"] <= N_FRAMES / max(ms - 5e-5, 1e-9) / 1e3 + 0.01
        assert "extra" not in r and r["cpu_baseline"] is None and r["roofline"]["stream_copy_GBs"] is None
    names = sorted(os.listdir(d1))
    assert names == ["dns_records.npy", "segment_counts.npy", "session_records.npy", "stats.npy"]
    assert sorted(os.listdir(d2)) == names
    got = {n[:-4]: np.load(os.path.join(d1, n)) for n in names}
    for n in names:  # every batch is the same synthetic frames: any step's outputs are these
        assert got[n[:-4]].dtype == np.float64
        assert np.array_equal(got[n[:-4]], np.load(os.path.join(d2, n))), n
    frames, offs = synth.generate(3, N_FRAMES)
    e_out, e_dns, _, e_st = coracle.parse_classify(coracle.make_cfg(1), frames, offs)
    assert len(e_out) > 0 and len(e_dns) > 0
    assert np.array_equal(got["session_records"], bench._columns_f64(e_out))
    assert np.array_equal(got["dns_records"], bench._columns_f64(e_dns))
    assert got["segment_counts"].shape == ((N_FRAMES + 63) // 64, 2)
    assert got["segment_counts"].sum(axis=0).tolist() == [len(e_out), len(e_dns)]
    for j, f in enumerate(k for k in e_st.dtype.names if not k.startswith("reserved")):
        if f not in ("new_sessions", "updated_sessions"):  # the parse alone keeps no table
            assert got["stats"][0, j] == float(e_st[0][f]), f
