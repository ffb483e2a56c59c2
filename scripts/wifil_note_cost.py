"""Measurement: what the closed-loop PHY's notification path (nsgpu_wifil_notify) costs an epoch.  The bench's
100x100 closed loop with the C MAC stand-in (bench.WifiLoop.run_native), Stop argv[1] s (default 0.03), in one
process: no phy notifying, 64 phys, every phy, and no phy again — us per epoch (wall time of Simulator::Run over
the nsgpu_wifil_advance calls) and the notes left with the PHY (no handler: the record path and the host's
per-epoch copy and sort, not a callback's cost)."""
import ctypes as C
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
n = w.sc["phys"].n_phy
some = sorted(int(p) for p in np.random.default_rng(64).choice(n, 64, replace=False))
for label, opted in (("warm-up", []), ("none", []), ("64 phys", some), ("all phys", range(n)), ("none again", [])):
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(w.sc["phys"])
    sim.attach_wifi(lp)
    for p in opted:
        lp.notify(p)
    left = C.c_uint64()

    def counted_close(lp=lp, close=lp.close, left=left):  # (run_native closes the PHY: count what it holds first)
        if lp.h:
            nsgpu.check(nsgpu.lib().nsgpu_wifil_read_notes(lp.h, None, 0, C.byref(left)))
        close()

    lp.close = counted_close
    disp, digest, info = w.run_native(w.sc, sim, lp)
    print(f"{label:>10}: {info['us_per_epoch']:8.1f} us/epoch over {info['epochs']} epochs, {disp} dispatches, "
          f"digest {digest:#x}, {left.value} notes", flush=True)
