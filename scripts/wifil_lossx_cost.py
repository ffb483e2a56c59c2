"""Measurement: what the closed-loop PHY's extended loss chain (nsgpu_wifil_set_loss) costs at 10,000 phys (the bench's
100x100 closed-loop grid).

(a) the closed loop with the C MAC stand-in (bench.WifiLoop.run_native), Stop argv[1] s (default 0.03): us per epoch
    with the config's chain (k_wl_rx<false> / k_wl_send<false>), with the same chain installed through set_loss — the
    same powers through k_wl_rx<true> / k_wl_send<true>, which isolates the LX path: the digest must not change — and
    with a Matrix link of each phy's 8 grid neighbours at the config chain's loss for their distance, DefaultLoss
    200 dB (another workload: everyone farther is inaudible; the table walk is what is looked at).
(b) argv[2] set_loss calls (default 50) with that table (~79,000 entries) on an idle engine, timed over the whole loop
    with the stream drained at the end: us per call — the host's sort and de-duplication, the copy into the pinned
    block and the upload."""
import math
import os
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ns-3-dev-dnemu_amd")]
import bench  # noqa: E402
import nsgpu  # noqa: E402
import wifi  # noqa: E402

nsgpu.check(nsgpu.lib().nsgpu_set_device(0))
stop = float(sys.argv[1]) if len(sys.argv) > 1 else 0.03
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
side = 100
w = bench.WifiLoop(types.SimpleNamespace(wifi_side=side, wifi_loop_stop=stop, wifi_mac="native"), None)
ph = w.sc["phys"]
n = ph.n_phy
pitch = float(ph.x[1] - ph.x[0])
(kind, exponent, d0, l0), = ph.loss
assert kind == nsgpu.LOSS_LOG_DISTANCE
entries = []
for j in range(n):
    r, c = divmod(j, side)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if (dr or dc) and 0 <= r + dr < side and 0 <= c + dc < side:
                d = pitch * math.hypot(dr, dc)
                entries.append((j, (r + dr) * side + c + dc, l0 + 10 * exponent * math.log10(d / d0)))
same = nsgpu.lossx(*ph.loss)
matrix = nsgpu.lossx((nsgpu.LOSSX_MATRIX, 200.0), entries=entries)

# (a) the epoch under the three chains
for label, lx in (("warm-up", None), ("config chain", None), ("same chain, set_loss", same),
                  (f"Matrix, {len(entries) / n:.1f} a phy", matrix), ("config chain again", None)):
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(ph)
    sim.attach_wifi(lp)
    if lx is not None:
        lp.set_loss(lx)
    disp, digest, info = w.run_native(w.sc, sim, lp)
    print(f"{label:>24}: {info['us_per_epoch']:8.1f} us/epoch over {info['epochs']} epochs, {info['sends']} sends, "
          f"{disp} dispatches, digest {digest:#x}", flush=True)

# (b) the call
lp = wifi.LoopPhy(ph)
lp.set_loss(matrix)  # (the first call allocates the blocks)
lp.pending()
t0 = time.perf_counter()
for _ in range(calls):
    lp.set_loss(matrix)
lp.pending()  # (drains the stream)
dt = time.perf_counter() - t0
print(f"{'set_loss':>24}: {dt / calls * 1e6:8.1f} us a call over {calls} calls, {len(entries)} entries at {n} phys", flush=True)
lp.close()
