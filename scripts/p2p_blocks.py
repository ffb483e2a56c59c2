"""Diagnostic: per-block start / end times of the three window kernels in one sampled window
(lib/libnsgpu_prof.so, NSGPU_LIB): which roles finish last, how late blocks start.  On a wide engine the third kernel
is k2_rank<true>: its roles (bookkeeping, accounting, lists, tiles), df_sdef's marks and, from a build with
-DNSGPU_TILE_MARKS, the tile marks.

Usage: python scripts/p2p_blocks.py [grid side] [NSDEF] [NLIST]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("NSGPU_LIB", os.path.join(REPO, "ns-3-dev-dnemu_amd", "lib", "libnsgpu_prof.so"))
sys.path[:0] = [os.path.join(REPO, "ns-3-dev-dnemu_amd")]
import numpy as np  # noqa: E402
import nsgpu  # noqa: E402
import p2p  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
# k2_rank<true>'s blocks after the bookkeeping one: accounting (NSDEF), lists (NLIST), then the tiles (nsgpu_p2p_win.h;
# a build without list blocks: 0)
nsdef = int(sys.argv[2]) if len(sys.argv) > 2 else 4
nlist = int(sys.argv[3]) if len(sys.argv) > 3 else 4
eng = p2p.Engine(p2p.grid(n, n))
eng.set_eager(True)
eng.run()
BLK = 2048
buf = np.zeros(64 + 3 * BLK * 2, np.uint64)
nsgpu.check(nsgpu.lib().nsgpu_p2p_phase_read(buf.ctypes.data, buf.size, 1))
blk = buf[64:].reshape(3, BLK, 2).astype(np.int64)
nslot = (4096 + 4096) // 256 if eng.wide() else 16  # (wide: gen-0 slots + the local records' dense list)
roles = {0: [("slot", 0, 16), ("lslot", 16, nslot), ("pool", nslot, 256)],
         1: [("holder", 0, 64), ("rank", 64, 1088), ("hub", 1088, 1120), ("maint", 1120, 1248)],
         2: [("scan", 0, 1)]}
if eng.wide():  # (the deferred pipeline: the third kernel is k2_rank<true>, its blocks record in k2_scan's slot)
    roles[2] = [("book", 0, 1), ("account", 1, 1 + nsdef), ("list", 1 + nsdef, 1 + nsdef + nlist),
                ("tiles", 1 + nsdef + nlist, 256)]
for k, name in enumerate(("k2_pa", "k2_handle", "k2_rank" if eng.wide() else "k2_scan")):
    b = blk[k]
    ok = b[:, 1] > 0
    t0 = b[ok, 0].min()
    print(f"{name}: blocks {ok.sum()}, span {(b[ok, 1].max() - t0) * 0.01:.2f} us (s_memrealtime, 10 ns)")
    for rn, lo, hi in roles[k]:
        r = b[lo:hi][ok[lo:hi]]
        if len(r) == 0:
            continue
        st, en = (r[:, 0] - t0) * 0.01, (r[:, 1] - t0) * 0.01
        print(f"  {rn:7s} n={len(r):5d} start {st.min():6.2f}..{st.max():6.2f}  end p50 {np.median(en):6.2f} "
              f"max {en.max():6.2f}  dur p50 {np.median(en - st):6.2f} max {(en - st).max():6.2f} us")
ph = buf[:64]
marks = {32: "snapshot issued", 34: "bound/publish (waits snapshot)", 36: "digest/log/classify (waits slot data)",
         38: "block_alloc2 (atomics+barriers)", 40: "writes (node-table atomics)", 42: "loop exit", 44: "publish_min+digest"}
print("k2_pa slot blocks, mean per block (sampled window):")
for i, nm in marks.items():
    c = max(int(ph[i + 1]), 1)
    print(f"  {nm:40s} {ph[i] * 0.01 / c:6.2f} us  (n={int(ph[i + 1])})")
print(f"k2_pa inputs (sampled window): pool end {int(buf[46])}, last window gen-0 {int(buf[47])}, local {int(buf[48])}; "
      f"pool entries taken {int(buf[49])}, pool chunks swept {int(buf[50])}")
print("k2_pa pool blocks, mean per block (sampled window):")
for i, nm in ((52, "run control + barrier"), (54, "pool sweep"), (62, "publish_min + digest")):
    c = max(int(buf[i + 1]), 1)
    print(f"  {nm:40s} {buf[i] * 0.01 / c:6.2f} us  (n={int(buf[i + 1])})")
if eng.wide():
    print("k2_rank accounting blocks (df_sdef), mean per block (sampled window; a hub block's marks share 22..27):")
    for i, nm in ((22, "records arrive"), (24, "block scan"), (26, "LDS arrays, prefixes"), (28, "resolve, log, digest"),
                  (30, "clears (and the stores' drain)")):
        c = max(int(buf[i + 1]), 1)
        print(f"  {nm:40s} {buf[i] * 0.01 / c:6.2f} us  (n={int(buf[i + 1])})")
    print("k2_rank tile blocks (a build with NSGPU_TILE_MARKS), mean per block and mark (sampled window):")
    for i, nm in ((4, "control, prefix -> first tile"), (6, "tile operands -> barrier"), (10, "compare loop"),
                  (12, "rank atomic -> barrier")):
        c = max(int(buf[i + 1]), 1)
        print(f"  {nm:40s} {buf[i] * 0.01 / c:6.2f} us  (n={int(buf[i + 1])})")
