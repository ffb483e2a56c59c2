"""The comparison of a device run of the closed-loop Wi-Fi PHY with a run of its plain-Python model
(tests/wifi_switch_model.py and the models over it), shared by tests/test_gpu_wifi_switch.py, tests/test_gpu_lossx.py
and tests/test_gpu_wifi_fuzz.py; tests/test_wifi_fuzz_cpu.py runs it on the CPU, model against mutated model.

Exactly equal: the pop log (ts, uid, context), the dispatch count and next uid, the per-phy counters and state fields,
the end records' integer fields, every switch call's outcome, get_channel's records, GetState / GetDelayUntilIdle at
every probe.  snr / per / rx_w: tests/test_gpu_wifi_per.py's compare_record (1e-9 relative; the K_DEVICE bound on per)
against the model's 60-digit reference values.  equal_fuzz adds what the fuzz cases have on top: every attempt (held or
sent, with the state it met), every hand-back, the notes, the mobility models' final reads and, for a run without a
log, the host digest.

A failure names the run (`what`), the first differing pop-log entry and — through `describe`, a function of the phy —
what lives on the phy concerned."""
import re

import numpy as np

import test_wifi_switch_cpu as sc
import wifi
import wifi_switch_model as wsm
from p2p_pyref import digest_term
from test_gpu_wifi_per import compare_record

PHY_FIELDS = wsm.COUNTERS + ("end_tx", "end_rx", "end_cca_busy", "rxing", "ni_len")
M64 = (1 << 64) - 1


def error_code(e):
    return int(re.match(r"nsgpu error (\d+)", str(e)).group(1))


def finish(g):
    g["lp"].close()
    g["sim"].close()


def first_log_difference(got, want, describe=None):
    """The first pop-log entry at which two logs — (ts, uid, ctx) arrays — differ, as text; None: equal."""
    n = min(len(got[0]), len(want[0]))
    diff = np.zeros(n, bool)
    for a, b in zip(got, want):
        diff |= np.asarray(a[:n]) != np.asarray(b[:n])
    if not diff.any() and len(got[0]) == len(want[0]):
        return None
    i = int(np.flatnonzero(diff)[0]) if diff.any() else n
    entry = lambda log: tuple(int(a[i]) for a in log) if i < len(log[0]) else None
    g, w = entry(got), entry(want)
    ctx = (w or g)[2]
    where = describe(ctx) if describe and ctx != wsm.NO_CONTEXT else "no phy's context"
    return f"pop log differs first at entry {i}: got (ts, uid, ctx) {g}, the model has {w}; {where}"


def digest_of(m):
    """The host digest of a run with the model's pop log: nsgpu_dispatch_digest_term summed over it
    (tests/test_wifi_fuzz_cpu.py holds this to the oracle's own digest)."""
    d = 0
    for rank, (ts, uid, _ctx) in enumerate(m.log):
        d = (d + digest_term(rank, ts, uid)) & M64
    return d


def equal_model(g, m, what="", describe=None):
    """g: a device run (dict: log — or None for a run without one —, dispatched, next_uid, phys, ends, switches,
    probes, channels).  Returns the worst per ratio."""
    mlog = m.log_arrays()
    where = first_log_difference(g["log"], mlog, describe) if g["log"] is not None else "no pop log"
    tell = lambda j: describe(int(j)) if describe else f"phy {int(j)}"
    assert (g["dispatched"], g["next_uid"]) == (len(mlog[0]), m.uid), (what, g["dispatched"], len(mlog[0]), g["next_uid"],
                                                                     m.uid, where)
    if g["log"] is not None:
        for a, b, f in zip(g["log"], mlog, ("ts", "uid", "ctx")):
            assert np.array_equal(a, b), (what, f, np.flatnonzero(a != b)[:5], where)
    mc_ = m.counters()
    for f in PHY_FIELDS:
        bad = np.flatnonzero(g["phys"][f] != mc_[f])[:8]
        assert np.array_equal(g["phys"][f], mc_[f]), (what, f, bad, tell(bad[0]))
    gends, mends = g["ends"], m.end_records()
    assert len(gends) == len(mends), (what, len(gends), len(mends))
    for f in sc.END_FIELDS:
        bad = np.flatnonzero(gends[f] != mends[f])[:1]
        assert np.array_equal(gends[f], mends[f]), (what, f, int(bad[0]), tell(mends["phy"][bad[0]]))
    worst = -1.0
    for e, r in zip(gends, m.end_refs):
        if r is None:
            assert int(e["flags"]) & wifi.END_CANCELLED and e["snr"] == 0.0 and e["per"] == 0.0 and e["rx_w"] == 0.0, \
                (what, tell(e["phy"]))
            continue
        snr, per, chunks, rx_w = r
        label = (what, int(e["phy"]), int(e["tx"])) + ((describe(int(e["phy"])),) if describe else ())
        worst = max(worst, compare_record(e, snr, per, chunks, rx_w, label))
    retried = set(m.retries)
    assert g["switches"] == [s for s in m.switches if (s[0], s[1]) not in retried], what
    assert g["probes"] == m.probes, (what, first_list_difference(g["probes"], m.probes, 2, tell))
    assert g["channels"] == m.channel_records(), what
    print(f"{what}: {len(mlog[0])} events, {len(gends)} ends, worst per ratio {worst:.2f}")
    return worst


def first_list_difference(got, want, phy_at, tell):
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return i, a, b, tell(b[phy_at])
    return min(len(got), len(want)), len(got), len(want)


def equal_fuzz(g, m, what="", describe=None, notes=None, finals=None):
    """equal_model, then: the attempts, the hand-backs (each seen by the handler at its record's now and uid: the
    driver asserts that where it records them), with notes (the model's note_records () of a run in which the same
    phys notify) the notes field by field, with finals ({phy: the model's read at the stop time}) the mobility models'
    final reads bit for bit, and for a run without a log the host digest."""
    tell = lambda j: describe(int(j)) if describe else f"phy {int(j)}"
    worst = equal_model(g, m, what, describe)
    assert g["attempts"] == m.attempts, (what, "attempts", first_list_difference(g["attempts"], m.attempts, 2, tell))
    assert g["handbacks"] == m.handbacks, (what, "hand-backs", first_list_difference(g["handbacks"], m.handbacks, 2, tell))
    if notes is not None:
        assert len(g["notes"]) == len(notes), (what, "notes", len(g["notes"]), len(notes))
        for f in wifi.WIFIL_NOTE_DTYPE.names:
            bad = np.flatnonzero(g["notes"][f] != notes[f])[:1]
            assert np.array_equal(g["notes"][f], notes[f]), (what, "note", f, int(bad[0]), tell(notes["phy"][bad[0]]))
    if finals is not None:
        assert set(g["finals"]) == set(finals), what
        for j, want in finals.items():
            assert g["finals"][j] == want, (what, "final read", g["finals"][j], want, tell(j))
    if g["log"] is None:
        assert g["digest"] == digest_of(m), (what, "host digest")
    return worst


def as_device(m, finals=None):
    """A model run in the form of a device run: what equal_model / equal_fuzz take as g."""
    retried = set(m.retries)
    return dict(log=m.log_arrays(), dispatched=len(m.log), next_uid=m.uid, ends=m.end_records(), phys=m.counters(),
                notes=m.note_records(), probes=list(m.probes), channels=m.channel_records(),
                switches=[s for s in m.switches if (s[0], s[1]) not in retried], attempts=list(m.attempts),
                handbacks=list(m.handbacks), finals=finals, digest=digest_of(m))
