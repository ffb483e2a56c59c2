"""The scenarios of tests/test_gpu_lossx.py (the device under an extended loss chain) and tests/test_lossx_model_cpu.py
(the same scenarios on tests/lossx_model.py alone: margins to the thresholds, branches taken).

A case: dict (phys, closures, stop, lossx, mob).  closures: (ts, [actions]) in setup order; actions are
wifi_switch_model's ("send", phy, size) / ("switch", phy, nch, delay_ns) plus ("probe", phy) — GetState alone — and
("loss", spec), spec = (links, entries) or None (the config's chain).  lossx: the chain installed before the first
closure (or None).  mob: () -> {phy: mobility_ref.CvModel} (a fresh set per run), or None.
Frames are 200 B at DsssRate1Mbps (1 792 000 ns) sent at 16.0206 dBm; RxGain 1 dB, ED threshold -96 dBm, CCA -99 dBm:
a frame syncs up to a loss of 113.02 dB and raises CCA up to 116.02 dB."""
import numpy as np

import loss_ref as lr
import mobility_ref
import test_wifi_switch_cpu as sc
import wifi

DBL_MAX = 1.7976931348623157e308
SIZE = sc.SIZE
MS = 1_000_000
TRG = (lr.TWO_RAY_GROUND, 0.125, 1.0, 0.5, 1.5)
THREE = (lr.THREE_LOG, 1.0, 200.0, 500.0, 1.9, 3.8, 3.8, 46.6777)


def send(t_ms, phy):
    return (int(round(t_ms * MS)), [("send", int(phy), SIZE)])


def probe(t_ms, *phys):
    return (int(round(t_ms * MS)), [("probe", int(p)) for p in phys])


def case(phys, closures, stop_ms, lossx=None, mob=None):
    return dict(phys=phys, closures=closures, stop=int(stop_ms * MS), lossx=lossx, mob=mob)


# ---------------------------------------------------------------- hidden terminal (wifi-hidden-terminal.cc's shape)
A, B, C = 0, 1, 2
HIDDEN = [(A, B, 60.0), (B, A, 60.0), (B, C, 65.0), (C, B, 65.0)]


def hidden_terminal_case(mid_run=False):
    """A - B - C with MatrixPropagationLossModel, DefaultLoss DBL_MAX: A and C reach B and not each other.  A and C
    send overlapping frames; at 3.9 ms A's has ended and C's is still on the air.  mid_run: a closure then sets
    A <-> C to 70 dB (later frames are heard), and a last closure sends from B, drops B -> A and moves C -> A to 80 dB,
    then sends from C: B's frame keeps the chain of its own SendPacket."""
    ph = sc.phys_of([0.0, 50.0, 100.0], np.zeros(3), np.zeros(3), [1, 1, 1])
    m = (lr.MATRIX, DBL_MAX)
    cl = [send(2.0, A), send(2.5, C), probe(3.9, A, B, C)]
    if mid_run:
        heard = HIDDEN + [(A, C, 70.0), (C, A, 70.0)]
        last = [e for e in heard if e[:2] not in ((B, A), (C, A))] + [(C, A, 80.0)]
        cl += [(10 * MS, [("loss", ([m], heard))]), send(12.0, A), probe(12.5, B, C),
               (20 * MS, [("send", B, SIZE), ("loss", ([m], last)), ("send", C, SIZE)]), probe(20.9, A, B, C)]
    return case(ph, cl, 30, lossx=([m], HIDDEN))


# ---------------------------------------------------------------- 16 phys, ThreeLogDistance
def three_log_case():
    """A line of 16 phys whose pairs fall in all four branches (under 1 m, 1 - 200 m, 200 - 500 m, beyond) and on both
    sides of the ED and CCA ranges (787 m, 945 m); nine sends, three pairs of them overlapping."""
    x = np.array([0.0, 0.6, 40.0, 120.0, 190.0, 230.0, 300.0, 380.0, 470.0, 520.0, 600.0, 700.0, 760.0, 830.0, 930.0, 1100.0])
    ph = sc.phys_of(x, np.zeros(16), np.zeros(16), np.ones(16))
    sends = [(2.0, 0), (2.8, 12), (6.0, 8), (9.0, 15), (9.9, 5), (13.0, 1), (16.0, 9), (16.5, 3), (20.0, 12)]
    return case(ph, [send(t, p) for t, p in sends] + [probe(21.0, 0, 7, 15)], 30, lossx=([THREE], ()))


# ---------------------------------------------------------------- 16 phys, TwoRayGround, one of them rising
def two_ray_case():
    """16 phys on a line out to 2.6 km at mixed heights: pairs under MinDistance's far side on both sides of their
    crossover distance.  Phy 6 (600 m from phy 0) rises at 100 m/s: at phy 0's first send (2 ms, z = 0.2 m) the
    pair's crossover is 256 m — two-ray — and at its second (42 ms, z = 4.2 m) 859 m — Friis."""
    x = np.array([0.0, 100.0, 200.0, 300.0, 400.0, 500.0, 600.0, 700.0, 800.0, 1000.0, 1200.0, 1400.0, 1700.0, 2000.0,
                  2300.0, 2600.0])
    z = np.array([0.0, 1.0, 4.0, 10.0, 0.0, 0.0, 0.0, 4.0, 1.0, 0.0, 10.0, 4.0, 0.0, 1.0, 10.0, 4.0])
    ph = sc.phys_of(x, np.zeros(16), z, np.ones(16))
    sends = [(2.0, 0), (2.9, 9), (6.0, 3), (10.0, 12), (14.0, 6), (18.0, 15), (22.0, 1), (42.0, 0), (46.0, 9)]
    mob = lambda: {6: mobility_ref.CvModel((600.0, 0.0, 0.0), (0.0, 0.0, 100.0), paused=False, last_update=0)}
    return case(ph, [send(t, p) for t, p in sends] + [probe(47.0, 0, 6, 15)], 55, lossx=([TRG], ()), mob=mob)


# ---------------------------------------------------------------- 324 phys, Matrix
def big_matrix_case(seed=5):
    """18 x 18 phys (two 256-thread blocks of k_wl_rx, the second partial).  Sender 100's row has 65 entries — among
    them receivers 255, 256 and 323 — sender 7's none; 255, 256 and 323 send too, each with a short row that names
    the others and phys of both blocks.  Losses 50 - 125 dB, on both sides of the thresholds; DefaultLoss 200 dB."""
    rng = np.random.default_rng(seed)
    i = np.arange(324)
    ph = sc.phys_of((i % 18) * 60.0, (i // 18) * 60.0, np.zeros(324), np.ones(324))
    e = []
    row100 = sorted(set(rng.choice(np.setdiff1d(i, [100, 255, 256, 323]), 62, replace=False).tolist()) | {255, 256, 323})
    assert len(row100) == 65
    for b in row100:
        e.append((100, b, float(np.round(rng.uniform(50.0, 125.0), 3))))
    for a in (255, 256, 323):
        for b in (0, 100, 254, 255, 256, 257, 322, 323):
            if b != a:
                e.append((a, b, float(np.round(rng.uniform(50.0, 125.0), 3))))
    order = rng.permutation(len(e))  # (any order; a duplicate of (100, 255) whose later value stays)
    e = [e[q] for q in order] + [(100, 255, 71.25)]
    sends = [(2.0, 100), (6.0, 7), (10.0, 255), (10.7, 256), (14.0, 323), (18.0, 100)]
    return case(ph, [send(t, p) for t, p in sends] + [probe(19.0, 255, 256, 323)], 26, lossx=([(lr.MATRIX, 200.0)], e))


# ---------------------------------------------------------------- Matrix and a channel switch
def matrix_switch_case(seed=6):
    """Six phys on channels 1 / 1 / 6 / 1 / 6 / 11 with a Matrix entry for most ordered pairs.  Phy 2 switches to
    channel 1 at 5 ms: its place in the channel's receiver loop changes, its Matrix rows and columns (keyed by phy) do
    not — phy 0's second frame reaches it with the (0, 2) entry, and its own frame leaves with row 2."""
    rng = np.random.default_rng(seed)
    ph = sc.phys_of(np.array(sc.LINE_X), np.array(sc.LINE_Y), np.zeros(6), sc.LINE_CH)
    e = [(a, b, float(np.round(rng.uniform(55.0, 120.0), 3))) for a in range(6) for b in range(6)
         if a != b and (a, b) not in ((1, 3), (3, 2))]
    cl = [send(2.0, 0), (5 * MS, [("switch", 2, 1, sc.DELAY)]), send(8.0, 0), send(12.0, 2), send(14.0, 4), send(16.0, 3),
          probe(17.0, 0, 1, 2, 3)]
    return case(ph, cl, 24, lossx=([(lr.MATRIX, 130.0)], e))


# ---------------------------------------------------------------- back to the config's chain, and on to another
def revert_case(seed=7):
    """The 4 x 4 grid (60 m pitch) under a Matrix chain installed before the first send; at 10 ms set_loss (None) —
    the config's LogDistance chain again — and at 20 ms Matrix followed by TwoRayGround (a chain of two links)."""
    rng = np.random.default_rng(seed)
    x, y, z = wifi.grid(4, 60.0)
    ph = sc.phys_of(x, y, z, np.ones(16))
    e = [(a, b, float(np.round(rng.uniform(50.0, 120.0), 3))) for a in range(16) for b in range(16) if a != b and (a + b) % 3]
    e2 = [(a, b, float(np.round(rng.uniform(0.0, 30.0), 3))) for a in range(16) for b in range(16) if a != b and (a * b) % 2]
    cl = [send(2.0, 0), send(2.7, 15), send(6.0, 5), (10 * MS, [("loss", None)]), send(12.0, 0), send(12.6, 10),
          send(16.0, 5), (20 * MS, [("loss", ([(lr.MATRIX, 5.0), TRG], e2))]), send(22.0, 0), send(22.9, 15), send(26.0, 5),
          probe(27.0, 0, 5, 15)]
    return case(ph, cl, 34, lossx=([(lr.MATRIX, 140.0)], e))


def old_kinds_case():
    """sc.grid_switch_case — switches, every branch of StartReceivePacket — with its own config chain installed as an
    extended chain (kinds 1 - 4 alone): the wrapped model must then be the unwrapped one, and the device under
    set_loss the device without it."""
    c = sc.grid_switch_case()
    links = [tuple(link) for link in c["phys"].loss]
    return dict(phys=c["phys"], closures=c["closures"], stop=c["stop"], lossx=(links, ()), mob=None)


CASES = dict(hidden=hidden_terminal_case, hidden_mid_run=lambda: hidden_terminal_case(True), three_log=three_log_case,
             two_ray=two_ray_case, big_matrix=big_matrix_case, matrix_switch=matrix_switch_case, revert=revert_case,
             old_kinds=old_kinds_case)
