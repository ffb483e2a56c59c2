"""bench.py as a command: a plain run's result line and --dump-outputs (an 8x8 grid, so the runs take moments).
The dumped arrays are the timed path's own results: they equal the oracle's run of the same scenario, and
two runs with the same arguments write the same bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nsref
import p2p

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--grid", "8", *args],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1  # (one JSON result line)
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_outputs(tmp_path):
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    out = run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", d1)
    run_bench("--steps", "2", "--warmup", "0", "--dump-outputs", d2)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "events/s" and out["higher_is_better"] is True
    assert out["dtype"] == "int64" and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(out["config"]["events_per_step"] / (out["ms_per_step"] / 1e3), rel=1e-9)
    # nothing that takes runs of its own in a plain line
    assert not {"roofline", "cpu_baseline", "speedup_vs_cpu", "secondary"} & set(out)

    sc = p2p.grid(8, 8)
    s = sc.c_struct()
    st = p2p.P2PStats()
    devc = np.zeros(s.n_devices, p2p.DEV_COUNTERS_DTYPE)
    appc = np.zeros(s.n_apps, p2p.APP_COUNTERS_DTYPE)
    nsref.p2p_run(s, st, devc, appc)
    assert out["config"]["events_per_step"] == st.dispatched
    files = sorted(os.listdir(d1))
    want = ["stats.npy"] + [f"dev.{f}.npy" for f in devc.dtype.names if not f.startswith("pad")] + \
        [f"app.{f}.npy" for f in appc.dtype.names]
    assert files == sorted(want) == sorted(os.listdir(d2))
    got = {f: np.load(os.path.join(d1, f)) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    names = [f for f, _ in st._fields_]
    stats = got["stats.npy"]
    i = names.index("digest")
    assert (int(stats[i]) << 32) | int(stats[i + 1]) == st.digest
    assert len(stats) == len(names) + 1  # (the digest's two halves: the fields after it are one further on)
    assert stats[names.index("dispatched")] == st.dispatched and stats[names.index("final_ts") + 1] == st.final_ts
    for f in devc.dtype.names:
        if not f.startswith("pad"):
            assert np.array_equal(got[f"dev.{f}.npy"], devc[f]), f
    for f in appc.dtype.names:
        assert np.array_equal(got[f"app.{f}.npy"], appc[f]), f
    assert got["app.rx_packets.npy"].sum() > 0
    for f in files:  # the same arguments' inputs are the same: so are the outputs, whatever --steps is
        assert np.array_equal(got[f], np.load(os.path.join(d2, f))), f
