"""Measurement: what one nsgpu_wifil_set_channel call costs at 10,000 phys (the bench's 100x100 closed-loop grid, phys
on channels 1 / 6 / 11), and what the SWITCHING instantiation of the epoch kernel costs an epoch.

(a) argv[1] calls (default 200) on an idle engine, each on another phy at its own `now` (so every one is a DONE
    switch: the batch flush, k_wl_rechan over 10,000 phys, k_wl_switch and the host's receiver counts), timed over
    the whole loop with the stream drained at the end: us per call.  One more loop with every call followed by
    nsgpu_wifil_get_channel (a device trip) for comparison.
(b) the closed loop with the C MAC stand-in (bench.WifiLoop.run_native), Stop argv[2] s (default 0.03): us per epoch
    before any switch (k_wl_stepw<false, false>) and after one phy far from everyone has switched at ts 1
    (k_wl_stepw<false, true> from then on; a corner phy moved to an unused channel number changes no one's
    receptions but its own)."""
import os
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ns-3-dev-dnemu_amd")]
import numpy as np  # noqa: E402
import bench  # noqa: E402
import nsgpu  # noqa: E402
import wifi  # noqa: E402

nsgpu.check(nsgpu.lib().nsgpu_set_device(0))
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
stop = float(sys.argv[2]) if len(sys.argv) > 2 else 0.03
w = bench.WifiLoop(types.SimpleNamespace(wifi_side=100, wifi_loop_stop=stop, wifi_mac="native"), None)
ph = w.sc["phys"]
n = ph.n_phy

# (a) the call
ph3 = wifi.LoopPhys(ph.x, ph.y, ph.z, channel=np.array([(1, 6, 11)[j % 3] for j in range(n)], np.uint32))
lp = wifi.LoopPhy(ph3)
pick = [int(p) for p in np.random.default_rng(7).choice(n, calls, replace=False)]
nxt = {1: 6, 6: 11, 11: 1}
lp.set_channel(1, pick[0], nxt[int(ph3.channel[pick[0]])], 250_000)  # (the first call allocates its count word)
lp.pending()
for label, read in (("set_channel", False), ("set_channel + get_channel", True)):
    t0 = time.perf_counter()
    for k, p in enumerate(pick[1:], 2):
        out = lp.set_channel(1_000 * k, p, nxt[int(ph3.channel[p])], 250_000)
        assert out[0] == wifi.SWITCH_DONE, out
        if read:
            lp.get_channel(p)
    lp.pending()  # (drains the stream)
    dt = time.perf_counter() - t0
    print(f"{label:>26}: {dt / (calls - 1) * 1e6:8.1f} us a call over {calls - 1} calls at {n} phys", flush=True)
    lp.close()
    lp = wifi.LoopPhy(ph3)
    lp.set_channel(1, pick[0], nxt[int(ph3.channel[pick[0]])], 250_000)
    lp.pending()
lp.close()

# (b) the epoch kernel's instantiations
for label, switched in (("warm-up", False), ("no switch", False), ("one phy switched", True), ("no switch again", False)):
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(ph)
    sim.attach_wifi(lp)
    if switched:
        assert lp.set_channel(1, n - 1, 14, 250_000)[0] == wifi.SWITCH_DONE
    disp, digest, info = w.run_native(w.sc, sim, lp)
    print(f"{label:>26}: {info['us_per_epoch']:8.1f} us/epoch over {info['epochs']} epochs, {info['sends']} sends, "
          f"{disp} dispatches, digest {digest:#x}", flush=True)
