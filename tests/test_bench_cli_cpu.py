"""bench.py's command line and --dump-outputs writer (no GPU): a plain run is the default, --full is the switch
for everything that takes runs of its own, and the dumped arrays are float64, exact and reproducible."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_plain_run_is_the_default_and_full_is_a_switch():
    a = bench.parser().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)
    a = bench.parser().parse_args(["--full", "--dump-outputs", "out", "--no-secondary"])
    assert a.full and a.dump_outputs == "out" and a.no_secondary and not a.no_cpu_baseline


def test_stats_vector_is_exact():
    import p2p
    st = p2p.P2PStats()
    st.dispatched, st.digest, st.final_ts, st.windows = 2_471_295, 0xFEDCBA9876543211, 2_100_000_000, 91_113
    v = bench.stats_vector(st)
    names = [f for f, _ in st._fields_]
    assert v.dtype == np.float64 and len(v) == len(names) + 1
    i = names.index("digest")
    assert (int(v[i]) << 32) | int(v[i + 1]) == 0xFEDCBA9876543211  # (high and low halves)
    assert v[names.index("dispatched")] == 2_471_295 and v[names.index("windows") + 1] == 91_113
    with pytest.raises(ValueError):
        bench.stats_vector([("final_ts", (1 << 53) + 1)])


def test_dump_outputs_fields_sample_and_limit(tmp_path):
    rec = np.dtype([("ts", "<u8"), ("uid", "<u4"), ("pad_", "<u4"), ("rx_dbm", "<f8")])
    n = bench.DUMP_ROWS + 1000
    big = np.zeros(n, rec)
    big["ts"] = np.arange(n, dtype=np.uint64) * 1000 + 7
    big["uid"] = np.arange(n) % 65_521
    big["rx_dbm"] = -60.0 - np.arange(n) * 1e-7
    small = np.arange(5, dtype=np.uint32)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(d1, {"rx": big, "count": small})
    bench.dump_outputs(d2, {"rx": big.copy(), "count": small})
    assert sorted(os.listdir(d1)) == ["count.npy", "rx.rx_dbm.npy", "rx.ts.npy", "rx.uid.npy"]
    got = {f: np.load(os.path.join(d1, f)) for f in os.listdir(d1)}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["count.npy"], small)
    # the same sorted sample of rows for every field, the same in every run
    rows = ((got["rx.ts.npy"] - 7) / 1000).astype(np.int64)
    assert len(rows) == bench.DUMP_ROWS and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["rx.uid.npy"], big["uid"][rows])
    assert np.array_equal(got["rx.rx_dbm.npy"], big["rx_dbm"][rows])
    for f, a in got.items():
        assert np.array_equal(a, np.load(os.path.join(d2, f)))
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_LIMIT
    with pytest.raises(ValueError):  # a 64-bit value float64 cannot hold is an error, not a rounding
        bench.dump_outputs(str(tmp_path / "c"), {"x": np.array([1 << 60], np.uint64)})
    with pytest.raises(ValueError):  # the 64 MB limit
        bench.dump_outputs(str(tmp_path / "d"), {f"c{i}": np.zeros(bench.DUMP_ROWS) for i in range(17)})
