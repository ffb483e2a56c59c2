"""The notification stream's reference (tests/wifi_note_model.py) pinned against the oracle on the CPU, and the
C-ABI of the notification calls (exports, record layout).  tests/test_gpu_wifi_notes.py compares the device's
stream with this model."""
import ctypes
import os
import re

import numpy as np
import pytest

import nsref
import wifi
from wifi_loop_harness import run_oracle, scenario
from wifi_note_model import model_notes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("nsgpu_wifil_notify", "nsgpu_wifil_read_notes", "nsgpu_sim_wifi_set_note_handler",
               "nsgpu_sim_wifi_notify")
KINDS = (("sync", wifi.NOTE_SYNC), ("drop_rx", wifi.NOTE_DROP_RX), ("drop_tx", wifi.NOTE_DROP_TX),
         ("drop_ed", wifi.NOTE_DROP_ED))


def dense_scenario(stop_ns=150_000_000):
    return scenario(n_side=6, spacing=60.0, seed=3, period=12_000_000, stop_ns=stop_ns, size=600)


def burst():
    """A 10x10 grid 30 m apart: the 80 phys with p % 5 != 0 SendPacket at 1 us, the 20 others at 2 ms (1000-B
    frames at 1 Mb/s, 8.2 ms each) — every phy takes 79-80 Receives inside one epoch, the 20 that sync are
    cancelled by their own SendPacket."""
    x, y, z = wifi.grid(10, 30.0)
    ph = wifi.LoopPhys(x, y, z, tx_cap=256, rxq_cap=256, ni_cap=512)
    sends = [(1_000, p) for p in range(100) if p % 5] + [(2_000_000, p) for p in range(100) if p % 5 == 0]
    return dict(phys=ph, sends=sends, size=1000, mode=wifi.DSSS_1M, preamble=wifi.PREAMBLE_LONG, dbm=17.0206,
                stop_ns=30_000_000)


def burst_oracle(b, log_cap=1 << 16):
    ts = np.array([t for t, _p in b["sends"]], np.uint64)
    phy = np.array([p for _t, p in b["sends"]], np.uint32)
    size = np.full(len(ts), b["size"], np.uint32)
    return nsref.wifil_replay(b["phys"].c_struct(), ts, phy, size, b["mode"], b["preamble"], b["dbm"], b["stop_ns"],
                              b["phys"].n_phy, wifi.WIFIL_END_DTYPE, wifi.PHY_COUNTERS_DTYPE, log_cap=log_cap)


def pin(sc, stop_ns, log, ends, ophys, tot, state_fields):
    ph = sc["phys"]
    n = ph.n_phy
    notes, models = model_notes(ph, tot["txs"], log, ends, range(n), sc["size"], sc["mode"], sc["preamble"], sc["dbm"])
    key = notes["ts"].astype(object) * (1 << 32) + notes["uid"]
    assert all(key[i] < key[i + 1] for i in range(len(key) - 1))
    for name, kind in KINDS:
        got = np.bincount(notes["phy"][notes["kind"] == kind], minlength=n)
        assert np.array_equal(got, ophys[name]), name
    assert np.array_equal(np.bincount(notes["phy"], minlength=n), ophys["rx"])
    assert np.array_equal(np.bincount(notes["phy"][notes["cca_duration"] != 0], minlength=n), ophys["cca_switches"])
    assert (notes["rx_duration"][notes["kind"] != wifi.NOTE_SYNC] == 0).all()
    # the syncs and the EndReceives: one to one on (phy, tx, end time); a sync without a record ends past the Stop
    sy = notes[notes["kind"] == wifi.NOTE_SYNC]
    skey = sorted((int(s["phy"]), int(s["tx"]), int(s["ts"]) + int(s["rx_duration"])) for s in sy)
    ekey = sorted((int(e["phy"]), int(e["tx"]), int(e["ts"])) for e in ends)
    assert len(set(skey)) == len(skey) and len(set(ekey)) == len(ekey)
    assert set(ekey) <= set(skey)
    assert all(k[2] >= stop_ns for k in set(skey) - set(ekey))
    if state_fields:
        for j in range(n):
            m = models[j]
            assert (m.end_rx, m.end_cca, int(m.rxing)) == (int(ophys["end_rx"][j]), int(ophys["end_cca_busy"][j]),
                                                           int(ophys["rxing"][j])), j
    return notes


def test_model_equals_oracle_grid_4x4():
    sc = scenario()
    log, ends, ophys, tot = run_oracle(sc)
    notes = pin(sc, sc["stop_ns"], log, ends, ophys, tot, True)
    sums = {name: int(np.count_nonzero(notes["kind"] == kind)) for name, kind in KINDS}
    sums["cca"] = int(np.count_nonzero(notes["cca_duration"]))
    assert sums == dict(sync=760, drop_rx=530, drop_tx=120, drop_ed=990, cca=1100)
    assert set(np.unique(notes["state"])) == {wifi.IDLE, wifi.RX, wifi.TX, wifi.CCA_BUSY}


def test_model_equals_oracle_grid_6x6_dense():
    sc = dense_scenario()
    log, ends, ophys, tot = run_oracle(sc)
    notes = pin(sc, sc["stop_ns"], log, ends, ophys, tot, True)
    assert all((notes["kind"] == kind).any() for _name, kind in KINDS)


def test_model_equals_oracle_burst_replay():
    b = burst()
    log, ends, ophys, tot = burst_oracle(b)
    notes = pin(b, b["stop_ns"], log, ends, ophys, tot, False)  # (the replay returns the counters only)
    assert (np.bincount(notes["phy"], minlength=100) == 99).all()
    assert int(np.count_nonzero(notes["kind"] == wifi.NOTE_SYNC)) == 20
    assert len(ends) == 20 and ((ends["flags"] & wifi.END_CANCELLED) != 0).all()
    assert int(np.count_nonzero(notes["cca_duration"])) == 9870
    first = notes[notes["ts"] < 2_000_000]  # the first wave's Receives: one epoch of the device run
    assert set(np.bincount(first["phy"], minlength=100)) == {79, 80}


# ---------------------------------------------------------------- the C-ABI
def test_library_exports_the_notification_calls():
    import nsgpu
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "nsgpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nsgpu_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW_SYMBOLS) <= declared, set(NEW_SYMBOLS) - declared
    assert re.search(r"typedef\s+void\s*\(\*nsgpu_wifi_note_fn\)", hdr)
    assert set(NEW_SYMBOLS) <= set(nsgpu.SIGNATURES)
    if not os.path.exists(nsgpu.LIB_PATH):
        pytest.skip("libnsgpu.so not built (run __graft_entry__.build())")
    so = ctypes.CDLL(nsgpu.LIB_PATH)
    missing = [s for s in NEW_SYMBOLS if not hasattr(so, s)]
    assert not missing, missing


def test_note_dtype_is_the_c_record():
    """WIFIL_NOTE_DTYPE against nsgpu_wifil_note as include/nsgpu_types.h declares it: the same fields at the same
    offsets (the C layout computed by ctypes from the header's text), the same size."""
    txt = open(os.path.join(REPO, "include", "nsgpu_types.h")).read()
    body = re.search(r"typedef struct nsgpu_wifil_note \{(.*?)\} nsgpu_wifil_note;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            t, names = decl.split(None, 1)
            fields += [(nm.strip(), ctype[t]) for nm in names.split(",")]

    class Note(ctypes.Structure):
        _fields_ = fields

    dt = wifi.WIFIL_NOTE_DTYPE
    assert dt.itemsize == ctypes.sizeof(Note) == 48
    assert list(dt.names) == [f for f, _t in fields]
    for f, t in fields:
        assert dt.fields[f][1] == getattr(Note, f).offset and dt.fields[f][0].itemsize == ctypes.sizeof(t), f
    kinds = dict(re.findall(r"(NSGPU_WIFIL_NOTE_[A-Z_]+) = (\d+)", txt))
    assert [int(kinds["NSGPU_WIFIL_NOTE_" + k]) for k in ("SYNC", "DROP_RX", "DROP_TX", "DROP_ED")] == \
        [wifi.NOTE_SYNC, wifi.NOTE_DROP_RX, wifi.NOTE_DROP_TX, wifi.NOTE_DROP_ED]
