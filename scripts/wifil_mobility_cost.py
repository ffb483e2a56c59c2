"""Measurement: what constant-velocity mobility (nsgpu_wifil_set_mobility) costs the closed-loop PHY an epoch.  The
bench's 100x100 closed loop with the C MAC stand-in (bench.WifiLoop.run_native), Stop argv[1] s (default 0.03), in
one process: no mobile phy, 64 mobile phys, every phy mobile, and none again — us per epoch (wall time of
Simulator::Run over the nsgpu_wifil_advance calls).  A mobile phy moves at up to 30 m/s; while any phy has a model
every SendPacket launches k_wl_move ahead of its k_wl_rx (one more launch a send, whatever the number of models).
The first and the last run (no model) must give the same digest."""
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ns-3-dev-dnemu_amd")]
import numpy as np  # noqa: E402
import bench  # noqa: E402
import nsgpu  # noqa: E402
import wifi  # noqa: E402

nsgpu.check(nsgpu.lib().nsgpu_set_device(0))
stop = float(sys.argv[1]) if len(sys.argv) > 1 else 0.03
w = bench.WifiLoop(types.SimpleNamespace(wifi_side=100, wifi_loop_stop=stop, wifi_mac="native"), None)
ph = w.sc["phys"]
n = ph.n_phy
some = sorted(int(p) for p in np.random.default_rng(64).choice(n, 64, replace=False))
vel = np.random.default_rng(65).uniform(-30.0, 30.0, (n, 3)) * (1.0, 1.0, 0.0)
digests = {}
for label, mobile in (("warm-up", []), ("none", []), ("64 phys", some), ("all phys", range(n)), ("none again", [])):
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(ph)
    sim.attach_wifi(lp)
    for p in mobile:
        lp.set_mobility(p, (ph.x[p], ph.y[p], ph.z[p]), vel[p])
    disp, digest, info = w.run_native(w.sc, sim, lp)
    digests[label] = digest
    print(f"{label:>10}: {info['us_per_epoch']:8.1f} us/epoch over {info['epochs']} epochs, {info['sends']} sends, "
          f"{disp} dispatches, digest {digest:#x}", flush=True)
same = digests["none"] == digests["none again"]
print("digest of the first and the last run (no model):", "the same" if same else "DIFFERENT", flush=True)
sys.exit(0 if same else 1)
