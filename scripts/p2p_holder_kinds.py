"""Diagnostic: k2_handle's 64 holder blocks at sampled windows of the default grid (lib/libnsgpu_prof.so): each
block's end time beside what its lanes ran (Receives, gen-0 TransmitCompletes, local records, Sends, other kinds,
the busiest lane's events).  The question it answers: are the blocks that end last the ones that ran a Send?
With --marks also where a lane's local record took its time (handle_node2's HN_T marks, the block's slowest lane):
from its parent's slot_done to local_record's return, lq_push's, the record's pop, its own slot_done and the loop's
next top, in us (shader-clock cycles scaled by the block's stamped duration over the holder's cycles); a fused
record has the first and the fourth only (the fourth: from local_record's return).
Usage: python scripts/p2p_holder_kinds.py [n] [first] [step] [count] [--table] [--marks]
Each sample re-runs the engine with the stamps aimed at window w (nsgpu_p2p_phase_read(-w))."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("NSGPU_LIB", os.path.join(REPO, "ns-3-dev-dnemu_amd", "lib", "libnsgpu_prof.so"))
sys.path[:0] = [os.path.join(REPO, "ns-3-dev-dnemu_amd")]
import numpy as np  # noqa: E402
import nsgpu  # noqa: E402
import p2p  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
table = "--table" in sys.argv
marks = "--marks" in sys.argv
MARK_NAMES = ("local_record", "lq_push", "to the pop", "the event", "next top")
n = int(args[0]) if len(args) > 0 else 128
first = int(args[1]) if len(args) > 1 else 300
step = int(args[2]) if len(args) > 2 else 100
count = int(args[3]) if len(args) > 3 else 10
nsgpu.check(nsgpu.lib().nsgpu_set_device(0))
eng = p2p.Engine(p2p.grid(n, n))
st, _, _, _ = eng.run()
W = int(st.windows)
print(f"grid {n} x {n}: {st.dispatched} events, {W} windows, wide {eng.wide()}", flush=True)
BLK, GT, NHB, NK = 2048, 8192, 64, 16
buf = np.zeros(64 + 3 * BLK * 2 + GT * 8 + NHB * NK // 2, np.uint64)
rows = []
for w in list(range(first, W, step))[:count]:
    nsgpu.check(nsgpu.lib().nsgpu_p2p_phase_read(buf.ctypes.data, 64, -w))
    eng.run()
    nsgpu.check(nsgpu.lib().nsgpu_p2p_phase_read(buf.ctypes.data, buf.size, 0))
    b = buf[64:64 + 3 * BLK * 2].reshape(3, BLK, 2).astype(np.int64)[1]
    kinds = buf[64 + 3 * BLK * 2 + GT * 8:].view(np.uint32).reshape(NHB, NK).astype(np.int64)
    ok = b[:, 1] > 0
    if not ok[:NHB].all():
        print(f"w {w}: no stamps")
        continue
    t0 = b[ok, 0].min()
    end = (b[:NHB, 1] - t0) * 0.01
    dur = (b[:NHB, 1] - b[:NHB, 0]) * 0.01
    span = (b[ok, 1].max() - t0) * 0.01
    send = kinds[:, 3] + kinds[:, 4] > 0
    order = np.argsort(-end)
    last8 = order[:8]
    print(f"w {w:5d}: kernel span {span:5.2f} us; holders end p50 {np.median(end):5.2f} max {end.max():5.2f}; "
          f"blocks with a Send/other {send.sum():2d}: end mean {end[send].mean() if send.any() else 0:5.2f} vs "
          f"{end[~send].mean() if (~send).any() else 0:5.2f} without; of the 8 last blocks {send[last8].sum()} had one; "
          f"corr(end, busiest lane's events) {np.corrcoef(end, kinds[:, 5])[0, 1]:+.2f}", flush=True)
    if table:
        print("   blk   end    dur  recv  txc  local send other  busiest holders")
        for i in order:
            k = kinds[i]
            print(f"   {i:3d} {end[i]:5.2f} {dur[i]:6.2f} {k[0]:5d} {k[1]:4d} {k[2]:6d} {k[3]:4d} {k[4]:5d} {k[5]:8d} {k[6]:7d}")
    if marks:
        full = (kinds[:, 6] >= 60) & (kinds[:, 2] >= kinds[:, 6] - 2) & (kinds[:, 13] > 0)  # every lane ran a pair
        if full.any():
            us = dur[full, None] * kinds[full, 8:13] / kinds[full, 13:14]
            print(f"   {full.sum()} blocks whose lanes each made a local record: holder {dur[full].mean():5.2f} us = "
                  f"{kinds[full, 13].mean():.0f} cycles; " +
                  ", ".join(f"{n} {u:.2f} us ({c:.0f} cy)" for n, u, c in zip(MARK_NAMES, us.mean(0), kinds[full, 8:13].mean(0))),
                  flush=True)
    rows.append((end, dur, kinds.copy(), send))
if rows:
    end = np.concatenate([r[0] for r in rows])
    dur = np.concatenate([r[1] for r in rows])
    kinds = np.concatenate([r[2] for r in rows])
    send = np.concatenate([r[3] for r in rows])
    print(f"all {len(rows)} windows: holder block dur mean {dur.mean():.2f} us; with a Send/other "
          f"{dur[send].mean() if send.any() else 0:.2f} (n={send.sum()}), without {dur[~send].mean():.2f} (n={(~send).sum()}); "
          f"events a block {kinds[:, :5].sum(1).mean():.1f}, busiest lane {kinds[:, 5].mean():.2f}; "
          f"corr(dur, busiest lane) {np.corrcoef(dur, kinds[:, 5])[0, 1]:+.2f}, corr(dur, sends) "
          f"{np.corrcoef(dur, kinds[:, 3])[0, 1]:+.2f}, corr(dur, events) {np.corrcoef(dur, kinds[:, :5].sum(1))[0, 1]:+.2f}")
