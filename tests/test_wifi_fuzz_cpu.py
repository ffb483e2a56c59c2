"""The seeded cross-feature Wi-Fi scenarios (tests/wifi_fuzz_cases.py) and their model (tests/wifi_fuzz_model.py)
without a GPU.

1. The model is a reference, so it is pinned first: with no new action it is tests/lossx_model.py exactly; its
   hand-back, with the harness's MAC stand-in restated over it, equals the C++ oracle's closed-loop run
   (nsref.wifil_run) on the scenarios of test_gpu_wifi_loop's hand-back test; frames of five (mode, preamble) pairs
   overlapping at one receiver equal the oracle's per-send replay; and the host digest of a run is
   nsgpu_dispatch_digest_term summed over the pop log (what tests/test_gpu_wifi_fuzz.py expects of a run without a log).
2. Every committed case is accepted — no reception within 1e-6 of a threshold, no draw within 1e-6 of its per, every
   engine capacity kept, no per that follows the last bits of earlier powers (m_firstPower's residue, below), not
   vacuous — and the set as a whole reaches each interaction it is there for in at least two cases.
3. The comparison the device test makes can fail: run model against mutated model it names the case and the phy.

Seeds examined: grid 0 - 11, dense 0 - 5, blocks 0 - 2, the first of each family, all accepted: none rejected for a
threshold, a draw or a capacity.  The residue condition was added after the device's per left compare_record's bound on
grid 11 (ratio 161, everything discrete equal) under unpadded ThreeLogDistance / TwoRayGround chains; with it grid 5 and
all six dense seeds were rejected, so the generators were changed (wifi_fuzz_cases.PAD_DB, DENSE_PAD_DB) and no seed
was picked: the same first seeds are all accepted now."""
import numpy as np
import pytest

import lossx_cases
import lossx_model
import nsref
import test_wifi_switch_cpu as sc
import wifi
import wifi_fuzz_cases as FZ
import wifi_fuzz_model as fm
import wifi_loop_harness as harness
import wifi_model_compare as cmp
import wifi_switch_model as wsm
import wifi_per_ref as per_ref
from test_wifi_per_cpu import K_DEVICE
from wifi_per_ref import mode_tuple

NSEND, LPE_CAP = 8, 8  # csrc/nsgpu_wifil_dev.h
_runs = {}


def run(family, seed):
    """(case, the model's run, the erase=False control), computed once."""
    if (family, seed) not in _runs:
        case = FZ.build(family, seed)
        _runs[(family, seed)] = (case, fm.run(case), fm.run(case, erase=False))
    return _runs[(family, seed)]


# ---------------------------------------------------------------- 1: the model against what it wraps and the oracle
def test_no_new_action_is_the_lossx_model():
    c = lossx_cases.old_kinds_case()
    args = (c["phys"], sc.MODE, sc.PREAMBLE, sc.DBM)
    a = lossx_model.Model(*args, notify=range(16), lossx=c["lossx"]).run(c["closures"], c["stop"])
    b = fm.Model(*args, notify=range(16), lossx=c["lossx"]).run(c["closures"], c["stop"])
    assert a.log == b.log and a.uid == b.uid and a.probes == b.probes and a.switches == b.switches
    assert a.ends == b.ends and a.notes == b.notes and len(a.ends) > 20  # (floats and all: the same doubles)
    assert np.array_equal(a.counters(), b.counters()) and a.channel_records() == b.channel_records()
    assert not b.attempts and not b.handbacks and not b.draws


class MacModel(fm.Model):
    """wifi_loop_harness.run_gpu's MAC stand-in (nsref.h: nsref_wifil_mac) over the model: ("mac", i, reply) is
    attempt i — SendPacket if phy i is IDLE, and Schedule (period, attempt i); otherwise Schedule (backoff[i],
    attempt i); a reply does neither Schedule — and the hand-back's draw is 0.5."""

    def __init__(self, s):
        super().__init__(s["phys"], s["mode"], s["preamble"], s["dbm"], listen=range(s["phys"].n_phy))
        self.s, self.sends, self.busy = s, 0, 0

    def act(self, a):
        if a[0] != "mac":
            return super().act(a)
        i, reply, s = a[1], a[2], self.s
        if self.phy[i].state(self.now) != wsm.IDLE:
            self.busy += 1
            if not reply:
                self.call_later(int(s["backoff"][i]), [a])
            return
        self.send_packet(i, s["size"])
        self.sends += 1
        if not reply:
            self.call_later(s["period"], [a])

    def mac(self, j, end_index, per):
        if 0.5 > per:
            self.call_later(self.s["reply_delay"], [("mac", j, True)])


@pytest.mark.parametrize("reply_delay", [10_000, 0])
@pytest.mark.parametrize("dense", [False, True])
def test_hand_back_equals_the_oracle(reply_delay, dense):
    if dense:
        s = harness.scenario(n_side=6, spacing=60.0, seed=3, period=12_000_000, stop_ns=80_000_000, size=600)
    else:
        s = harness.scenario(stop_ns=120_000_000)
    s["reply_delay"] = reply_delay
    o = harness.run_oracle(s)
    m = MacModel(s).run([(int(t), [("mac", i, False)]) for i, t in enumerate(s["first"])], s["stop_ns"])
    sc.equal_oracle(m, o)
    otot = o[3]
    assert (m.sends, m.busy, cmp.digest_of(m)) == (otot["sends"], otot["busy"], otot["digest"])
    live = sum(1 for r in m.end_refs if r is not None)
    assert len(m.handbacks) == live > 20
    replies = [e for e, k in zip(m.log, m.log_kinds) if k == "closure" and e[2] != wsm.NO_CONTEXT]
    assert len(replies) > 10  # (a reply's closure runs in its EndReceive's context, the initial ones in none)


MIXED = [(mode_tuple("DsssRate1Mbps"), wifi.PREAMBLE_LONG), (mode_tuple("DsssRate11Mbps"), wifi.PREAMBLE_SHORT),
         (mode_tuple("OfdmRate6Mbps"), wifi.PREAMBLE_LONG), (mode_tuple("OfdmRate54Mbps"), wifi.PREAMBLE_LONG),
         (mode_tuple("OfdmRate6MbpsBW10MHz"), wifi.PREAMBLE_LONG), (mode_tuple("DsssRate5_5Mbps"), wifi.PREAMBLE_LONG)]


def test_mixed_modes_equal_the_oracles_per_send_replay():
    """Seven phys around a receiver; it locks on a 1500 B DsssRate1Mbps frame and five frames of five other (mode,
    preamble) pairs overlap it, the second sender repeating later so that a frame of another kind is locked on too."""
    x = np.array([0.0, 20.0, -35.0, 50.0, -60.0, 45.0, -25.0])
    y = np.array([0.0, 10.0, 20.0, -30.0, -15.0, 40.0, -45.0])
    ph = sc.phys_of(x, y, np.zeros(7), np.ones(7))
    sends = [(2_000_000, 1, 1500, MIXED[0]), (3_000_000, 2, 400, MIXED[1]), (4_100_000, 3, 1500, MIXED[2]),
             (5_300_000, 4, 800, MIXED[3]), (6_000_123, 5, 200, MIXED[4]), (7_700_000, 6, 800, MIXED[5]),
             (20_000_000, 2, 800, MIXED[2]), (20_400_000, 3, 100, MIXED[1]), (20_900_000, 4, 100, MIXED[4])]
    m = fm.Model(ph, *FZ.FRAME).run([(t, [("attempt", p, size, fr[0], fr[1], sc.DBM)]) for t, p, size, fr in sends],
                                   30_000_000)
    o = nsref.wifil_replay(ph.c_struct(), [s[0] for s in sends], [s[1] for s in sends], [s[2] for s in sends], sc.MODE,
                           sc.PREAMBLE, sc.DBM, 30_000_000, 7, wifi.WIFIL_END_DTYPE, wifi.PHY_COUNTERS_DTYPE,
                           modes=[s[3][0] for s in sends], preambles=[s[3][1] for s in sends])
    sc.equal_oracle(m, o)
    assert cmp.digest_of(m) == o[3]["digest"]
    at0 = [mix for e, mix in zip(m.ends, m.end_mix) if e[2] == 0 and mix is not None]
    assert max(mix[2] for mix in at0) >= 6 and max(mix[0] for mix in at0) >= 9, at0
    assert all(a[3] for a in m.attempts) and len(m.ends) >= 15


# ---------------------------------------------------------------- 2: acceptance
def test_the_case_list():
    fams = [f for f, _s in FZ.FUZZ_CASES]
    assert (fams.count("grid"), fams.count("dense"), fams.count("blocks")) == (12, 6, 3)
    assert len(set(FZ.FUZZ_CASES)) == len(FZ.FUZZ_CASES)


def test_generators_are_deterministic():
    for fam in FZ.FAMILIES:
        a, b = FZ.build(fam, 1), FZ.build(fam, 1)
        assert a["closures"] == b["closures"] and a["specs"] == b["specs"] and a["reply"] == b["reply"]
        assert np.array_equal(a["phys"].x, b["phys"].x) and np.array_equal(a["phys"].channel, b["phys"].channel)
        assert (a["listen"], a["notify"], a["stop"], a["lossx"]) == (b["listen"], b["notify"], b["stop"], b["lossx"])
        assert FZ.build(fam, 2)["closures"] != a["closures"]


@pytest.mark.parametrize("family,seed", FZ.FUZZ_CASES)
def test_case_is_accepted_and_not_vacuous(family, seed):
    case, m, _control = run(family, seed)
    ph = case["phys"]
    closest = lossx_model.clear_of_thresholds(m, 1e-6)
    margin = min(abs(u - float(per)) for _e, _j, _k, u, per in m.draws)
    assert margin >= 1e-6, margin
    # per must not follow the last bits of earlier powers: m_firstPower is at most n additions of powers up to P_max off
    # (2^-53 P_max each) where the device's powers differ from the host's in their last bit; that much more noise
    # may move the reference per by 0.9 of compare_record's bound at most (the device's arithmetic alone takes 0.5 of
    # that bound's 128 units: tests/test_gpu_wifi_per.py)
    worst_residue = 0.0
    for i, (r, inp) in enumerate(zip(m.end_refs, m.end_inputs)):
        if r is None:
            continue
        snr, per, chunks, rx_w = r
        window, _rxing, k = inp
        floor = rx_w / snr  # (the noise floor and m_firstPower at the frame's start)
        rel = 2.0 * len(window) * 2.0 ** -53 * max(e[2] for e in window) / floor
        moved = abs(fm.per_under_more_noise(m, i, rel) - per)
        share = float(moved / per_ref.psr_bound(chunks, 1 - per, K_DEVICE))
        worst_residue = max(worst_residue, share)
        assert share <= 0.9, (family, seed, i, share, float(per), snr, rel)
    assert m.max_pending_ends <= LPE_CAP and m.max_ni <= ph.ni_cap and m.max_pending_rx <= ph.rxq_cap
    assert len(m.txs) <= ph.tx_cap and len(m.log) < 20_000  # (a GPU test of a few seconds)
    live = sum(1 for r in m.end_refs if r is not None)
    sent = sum(1 for a in m.attempts if a[5] and a[3])
    held = sum(1 for a in m.attempts if a[5] and not a[3])
    assert live >= 30 and sent >= 1 and held >= 1, (live, sent, held)
    # every phy notifying changes the notes alone (what the device's `notes` pipeline is compared with)
    noted = fm.run(case, notify=range(ph.n_phy))
    assert noted.log == m.log and noted.ends == m.ends and noted.probes == m.probes and noted.attempts == m.attempts
    assert len(noted.notes) == int(m.counters()["rx"].sum()) >= len(m.notes)
    assert set(fm.final_reads(noted, case["stop"])) == set(case["specs"])  # (every model can be read at the stop time)
    print(f"{family} {seed}: {ph.n_phy} phys, {len(m.log)} events, {live} live ends, {len(m.draws)} draws (closest to its "
          f"per {margin:.2g}), replies {sent} sent {held} held, closest reception to a threshold {closest:.2g}, pending "
          f"ends {m.max_pending_ends}, Receives {m.max_pending_rx}, ni {m.max_ni}; m_firstPower's residue may move a per by "
          f"{worst_residue:.2g} of its bound")


@pytest.mark.parametrize("family,seed", [c for c in FZ.FUZZ_CASES if c[0] == "grid"])
def test_grid_cases_are_what_the_family_says(family, seed):
    case, m, _control = run(family, seed)
    acts = [a for _t, al in case["closures"] for a in al]
    frames = {(a[3], a[4]) for a in acts if a[0] == "attempt"}
    assert 16 <= case["phys"].n_phy <= 25 and len(set(case["phys"].channel)) in (2, 3)
    assert len(frames) >= 8 and {a[5] for a in acts if a[0] == "attempt"} == set(FZ.POWERS)
    delays = [a[3] for a in acts if a[0] == "switch"]
    assert 0 in delays and max(delays) >= 3 * FZ.MS and len(delays) >= 4
    assert sum(a[0] in fm.COURSE for a in acts) >= 3 and 1 <= sum(a[0] == "loss" for a in acts)
    assert {s[0] for s in case["specs"].values()} == {"cv", "wp", "acc"} and len(case["specs"]) < case["phys"].n_phy
    assert abs(len(case["listen"]) - case["phys"].n_phy / 2) <= 1
    assert {case["reply"][j][0] for j in case["listen"]} == {0, 10_000}


# ---------------------------------------------------------------- 2: reach
def frame_dur(m, k):
    return FZ.dur(m.tx_sizes[k], *m.tx_frames[k][:2])


def reach(case, m, control):
    """What one case contributes: {item: bool}."""
    f = {}
    ends, listen = m.ends, set(case["listen"])
    cancelled = {(e[2], e[5]) for e in ends if e[6] & wifi.END_CANCELLED}
    handed = set(m.handbacks)
    f["switch_of_listened_phy_in_rx"] = any(
        cause == "switch" and j in listen and (j, tx) in cancelled for _t, _u, j, cause, tx in m.cancels) and \
        all((e[0], e[1], e[2]) not in handed for e in ends if e[6] & wifi.END_CANCELLED) and \
        all(m.ndraw[j] == sum(1 for e in ends if e[2] == j and not e[6] & wifi.END_CANCELLED) for j in listen)
    replies = [a for a in m.attempts if a[5]]
    f["reply_held_switching"] = any(not a[3] and a[4] == wsm.SWITCHING for a in replies)
    f["reply_held_tx"] = any(not a[3] and a[4] == wsm.TX for a in replies)
    sends_cancel = {(t, u, j) for t, u, j, cause, _tx in m.cancels if cause == "send"}
    f["reply_sent_in_rx_cancels_a_lock"] = any(a[3] and a[4] == wsm.RX and a[:3] in sends_cancel for a in replies)
    f["reply_sent_in_cca_busy"] = any(a[3] and a[4] == wsm.CCA_BUSY for a in replies)
    # a reply with delay 0: its closure in the nanosecond of its EndReceive, Receive events of that nanosecond between
    at = {}
    for i, (e, k) in enumerate(zip(m.log, m.log_kinds)):
        at.setdefault(e[0], []).append((i, k, e))
    hb = {(t, j): u for t, u, j in m.handbacks}
    f["reply_delay_0_among_receives"] = any(
        case["reply"][a[2]][0] == 0 and (a[0], a[2]) in hb and
        any(k == "rx" and hb[(a[0], a[2])] < e[1] < a[1] for _i, k, e in at[a[0]]) for a in replies)
    between = [(t, u) for t, u, _a in m.actions]
    f["postponed_switch_retried_after_a_loss_or_course_call"] = any(
        out == wsm.POSTPONED and any(t < ta < t + d for ta, _u in between) and
        any(e[0] == t + d and k == "retry" for e, k in zip(m.log, m.log_kinds))
        for t, _u, _j, out, _st, d in m.switches)
    f["drop_switching_note_with_cca"] = any(n[4] == wsm.NOTE_DROP_SWITCHING and n[8] > 0 and n[2] in case["notify"]
                                           for n in m.notes)
    received = {k for k, _j, _w, _t in m.rx_powers}
    f["loss_action_with_frames_on_the_air"] = any(
        a[0] == "loss" and any(x[0] < t < x[0] + frame_dur(m, k) and k in received for k, x in enumerate(m.txs))
        for t, _u, a in m.actions)
    # a mover alone on a channel while others send, heard again after it came back
    j = case.get("loner")
    f["loner"] = None
    if j is not None:
        done = [s for s in m.switches if s[2] == j and s[3] == wsm.DONE]
        out = [s[0] for s in done]
        if len(out) >= 2:
            t_out, t_back = out[0], out[-1]
            others = sum(1 for x in m.txs if t_out < x[0] < t_back and x[2] != j)
            heard = any(not e[6] & wifi.END_CANCELLED and m.txs[e[5]][2] == j and m.txs[e[5]][0] > t_back for e in ends)
            if others >= 3 and heard:
                f["loner"] = case["specs"][j][0]
    # a collision of a Matrix-hidden pair's OFDM frames at a common receiver
    pw = {(k, r): w for k, r, w, _t in m.rx_powers}
    hidden = set()
    for sp in [case["lossx"]] + [a[1] for _t, _u, a in m.actions if a[0] == "loss"]:
        if sp is not None:
            hidden |= {(a, b) for a, b, db in sp[1] if db == FZ.HIDE_DB}
    f["hidden_pair_ofdm_collision"] = False
    for ka, xa in enumerate(m.txs):
        for kb, xb in enumerate(m.txs):
            if (xa[2], xb[2]) in hidden and xa[0] < xb[0] < xa[0] + frame_dur(m, ka) and FZ.is_ofdm(m.tx_frames[ka][0]) \
                    and FZ.is_ofdm(m.tx_frames[kb][0]) and pw.get((ka, xb[2]), 1.0) < m.cca_w:
                f["hidden_pair_ofdm_collision"] |= any(pw.get((ka, c), 0.0) > m.ed_w and pw.get((kb, c), 0.0) > m.cca_w
                                                       for c in range(len(m.phy)))
    f["chunk_walk_over_mixed_interferers"] = any(mix is not None and mix[0] >= 3 and mix[1] >= 2 for mix in m.end_mix)
    csnr = {(e[0], e[1], e[2]): e[3] for e in control.ends if not e[6] & wifi.END_CANCELLED}
    f["snr_differs_without_erase"] = any(
        not e[6] & wifi.END_CANCELLED and (e[0], e[1], e[2]) in csnr and m.phy[e[2]].switches > 0 and
        abs(csnr[(e[0], e[1], e[2])] - e[3]) > 1e-3 * e[3] for e in ends)  # (more than a residue of additions undone)
    f["more_than_nsend_attempts_and_another_call"] = any(
        sum(a[0] == "attempt" for a in al) > NSEND and any(a[0] != "attempt" for a in al) for _t, al in case["closures"])
    f["more_than_nsend_without_mobility"] = f["more_than_nsend_attempts_and_another_call"] and not case["specs"]
    if case["family"] == "blocks":
        for j in (255, 256):
            f[f"blocks_{j}"] = any(x[2] == j for x in m.txs) and \
                any(e[2] == j and not e[6] & wifi.END_CANCELLED for e in ends) and \
                any(a[1] == j and a[0] in fm.COURSE for _t, _u, a in m.actions) and \
                any(s[2] == j and s[3] == wsm.DONE for s in m.switches) and j in case["specs"]
    return f


ITEMS = ["switch_of_listened_phy_in_rx", "reply_held_switching", "reply_held_tx", "reply_sent_in_rx_cancels_a_lock",
         "reply_delay_0_among_receives", "postponed_switch_retried_after_a_loss_or_course_call",
         "drop_switching_note_with_cca", "loss_action_with_frames_on_the_air", "hidden_pair_ofdm_collision",
         "chunk_walk_over_mixed_interferers", "snr_differs_without_erase", "more_than_nsend_attempts_and_another_call",
         "more_than_nsend_without_mobility", "blocks_255", "blocks_256"]


@pytest.mark.parametrize("item", ITEMS)
def test_at_least_two_cases_reach(item):
    got = [c for c in FZ.FUZZ_CASES if reach(*run(*c)).get(item)]
    print(item, got)
    assert len(got) >= 2, (item, got)


@pytest.mark.parametrize("kind", ["cv", "wp", "acc"])
def test_a_mover_of_each_kind_leaves_for_a_channel_of_its_own_and_is_heard_again(kind):
    got = [c for c in FZ.FUZZ_CASES if reach(*run(*c))["loner"] == kind]
    assert len(got) >= 2, (kind, got)
    for c in got:  # alone there it keeps its last update whatever the others send: its model at the moment before it
        case, m, _control = run(*c)  # returns is its model of just after it left (or after its last course call there)
        j = case["loner"]
        mine = [(t, a) for t, al in case["closures"] for a in al if a[1:2] == (j,)]
        t_out = [t for t, a in mine if a[0] == "switch" and a[2] == 13][0]
        t_back = [t for t, a in mine if a[0] == "switch" and a[2] != 13 and t > t_out][0]
        t_out = [s[0] for s in m.switches if s[2] == j and s[3] == wsm.DONE and s[0] >= t_out][0]  # (or its retry's)
        since = max([t_out] + [t for t, a in mine if a[0] in fm.COURSE and t_out < t < t_back])
        state = lambda mm: {k: v for k, v in vars(mm).items() if k != "hits"}
        assert state(fm.run(case, stop=t_back - 1).mob[j]) == state(fm.run(case, stop=since + 1).mob[j])
        assert sum(1 for x in m.txs if since < x[0] < t_back and x[2] != j) >= 3 and t_back - since > 5 * FZ.MS


# ---------------------------------------------------------------- 3: the comparison can fail
MUTANT_CASE = ("grid", 0)


def mutant_message(**kw):
    family, seed = MUTANT_CASE
    case, m, _control = run(family, seed)
    bad = fm.run(case, **kw)
    label = "%s seed %d, mutant" % (family, seed)
    same = fm.run(case)
    cmp.equal_fuzz(cmp.as_device(same), m, label, lambda j: FZ.describe_phy(case, j), notes=m.note_records())
    with pytest.raises(AssertionError) as ei:
        cmp.equal_fuzz(cmp.as_device(bad), m, label, lambda j: FZ.describe_phy(case, j), notes=m.note_records())
    msg = str(ei.value)
    assert "grid seed 0" in msg and "phy " in msg and "channels [" in msg, msg
    return msg, bad, m


def test_comparison_catches_a_model_without_erase_events():
    msg, bad, m = mutant_message(erase=False)
    print(msg[:400])


def test_comparison_catches_one_flipped_draw():
    _case, m, _control = run(*MUTANT_CASE)
    msg, bad, _m = mutant_message(flip={len(m.draws) // 2})
    assert "pop log differs first at entry" in msg and bad.log != m.log, msg


def test_comparison_catches_one_frames_mode_changed_after_the_fact():
    """The frame keeps its duration and its place in every list; only CalculateSnrPer takes it for another mode.  Of
    the frames tried the first whose change leaves the pop log alone is used: per alone must give it away."""
    case, m, _control = run(*MUTANT_CASE)
    other = {True: (mode_tuple("DsssRate1Mbps"), wifi.PREAMBLE_LONG), False: (mode_tuple("OfdmRate54Mbps"), wifi.PREAMBLE_LONG)}
    for k in range(len(m.txs)):
        kw = dict(remode={k: other[FZ.is_ofdm(m.tx_frames[k][0])]})
        bad = fm.run(case, **kw)
        if bad.log == m.log and [r and r[1] for r in bad.end_refs] != [r and r[1] for r in m.end_refs]:
            msg, bad, _m = mutant_message(**kw)
            assert "pop log" not in msg and bad.log == m.log, msg
            return
    raise AssertionError("no frame's mode can change without the pop log changing")
