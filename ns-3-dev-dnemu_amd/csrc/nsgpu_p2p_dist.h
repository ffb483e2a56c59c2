// nsgpu_p2p_dist.h — the partitioned p2p run's device code (included by nsgpu_p2p.hip after the window pipeline,
// nsgpu_p2p_win.h: the same translation unit, so that the window kernels and these compile together).
#pragma once
#include "nsgpu_p2p_dev.h"

namespace nsgpu {

// ================================ partitioned run (multi-GPU) ================================
// DistributedSimulatorImpl (src/mpi/model/distributed-simulator-impl.cc:146-326) gives every rank
// the nodes of its system id and grants it min over ranks of (next ts) + lookahead after an
// MPI_Allgather of LbtsMessage (:276-313); remote packets travel as {rx ns, node, dev, serialized
// packet} (mpi-interface.cc:414-506).  Here every rank runs the single-GPU engine's window kernels
// over its own nodes, and three fixed-size collectives per window (RCCL, captured into the window
// graph with the kernels) make the partitioned run reproduce the SEQUENTIAL pop order — uids
// included, which DistributedSimulatorImpl itself does not (its uids are per rank):
//   k2_pa<true>  as single-GPU (in-place pool), plus the remote events of the last X2;
//   X0           allgather of every rank's window size and hub flag (16 B, straight from Ctl);
//   k2_handle    holders and hub blocks (no rank tiles), writing this rank's X1 summary and entries —
//                unless some rank's window does not fit: then nothing runs and the window becomes a
//                partitioned sorted run (every rank sorts its candidates once; chunks cut at the smallest
//                of the ranks' fitting keys, nsgpu_p2p_win.h);
//   X1           allgather of the summaries;
//   k_gtile      per own event, over the merged windows: # smaller keys (global dispatch rank) and the
//                child / inline-child sums below it and below its same-ts group (uid prefixes);
//   k_dfin2      own events' dispatch info, remote children -> X2 with their final uids, the pool
//                bookkeeping, and the run bookkeeping from the merged summaries: the LBTS (the next
//                window's bound), `done`, a compaction every rank makes;
//   X2           all-to-all of remote events.

// ---- partitioned sorted runs: the host step that starts one (nsgpu_p2p_win.h, "partitioned sorted runs") ----
// The window that did not fit (C.W candidates in the window records, relative to its tmin) is sorted by key into
// rn_* (k_rs_*), after its node-table entries are cleared (k_drun_clear: the chunks claim them again); k_drun_start
// keeps the window's bound and sends this rank's fitting key (its WCAP-th entry's key; ~0 when all fit) and size,
// and after their all-gather k_drun_first moves the first chunk in.  The candidates that came from the pool stay
// there until their chunk runs (its maintenance tombstones them); the others live in the run only.
__global__ __launch_bounds__(256) void k_drun_clear(const P2PDev M) {
  const Ctl &C = *M.C;
  const uint64_t W = C.W;
  const uint64_t nt = W < (uint64_t)WCAP ? W : (uint64_t)WCAP;  // (k2_write claims slots below WCAP only)
  for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < nt; s += (uint64_t)gridDim.x * 256) {
    const uint32_t c = lp_of(M, M.wctx[s], M.wkind[s], M.wa[s]);
    if (c < M.n_nodes) M.node_tab[(uint64_t)c * NTAB] = 0;
  }
}
__global__ void k_drun_start(const P2PDev M, uint64_t n) {
  Ctl &C = *M.C;
  if (M.wide) n = C.drcut < n ? C.drcut : n;  // (k_drun_trim: the run is the window's narrow part)
  const WinBound b = window_bound(C.rt ? C.red[0] : C.red[1]);  // (the bound k2_pa formed the window with)
  C.drb_tmin = b.tmin;
  C.drb_span = b.span;
  C.drb_bound = b.bound;
  C.drb_stop = b.stop_packed;
  C.drb_nbound = b.nbound;
  C.drb_lim = b.lim;
  C.dr0 = C.dr1 = 0;
  C.drW = n;
  C.W = 0;
  C.nhub = 0;
  C.overflow = 0;
  C.drlo = ~0ull;
  C.drtrim = 0;
  C.dtrim = 0;
  {  // the pending set outside the run, as the overflowing window's k2_pa reduced it (the run's entries: k_drun_red)
    const Red r = x1hdr(M.x1_send, 0)->red;
    C.drn_tmin = r.tmin;
    C.drn_wend = r.wend;
    C.drn_stopts = r.stopts;
    C.drn_stopuid = r.stopuid;
    C.drn_wendw = r.wendw;
  }
  M.xk_send[0] = n > (uint64_t)WCAP ? M.rn_key[WCAP - 1] : ~0ull;  // (this rank's fitting key)
  M.xk_send[1] = n ? M.rn_key[0] : ~0ull;                           // (its head key)
}
// During the run the pool is not swept: the pending set's reduction at its start (k_drun_start) and the run's
// entries' (all of them: conservative, some are dispatched before the run ends) are folded into every chunk's; the
// chunks' children fold in as they are parked.  So the first window after the run is bounded safely.
__global__ __launch_bounds__(256) void k_drun_red(const P2PDev M, uint64_t n) {
  Ctl &C = *M.C;
  const uint64_t tmin = C.drb_tmin;
  uint64_t tmn = ~0ull, wnd = ~0ull, wndw = ~0ull;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t ts = tmin + (M.rn_key[i] >> 32);
    const uint32_t kd = (M.rn_kind[i] & 0xffu) % K_NKINDS;
    const uint64_t x = ts + (uint64_t)M.lookahead[kd], xw = ts + (uint64_t)M.lookw[kd];
    tmn = ts < tmn ? ts : tmn;
    wnd = x < wnd ? x : wnd;
    wndw = xw < wndw ? xw : wndw;
  }
  tmn = wave_min64(tmn);
  wnd = wave_min64(wnd);
  wndw = wave_min64(wndw);
  if ((threadIdx.x & 63) == 0) {
    if (tmn != ~0ull) atomicMin((unsigned long long *)&C.drn_tmin, (unsigned long long)tmn);
    if (wnd != ~0ull) atomicMin((unsigned long long *)&C.drn_wend, (unsigned long long)wnd);
    if (M.wide && wndw != ~0ull) atomicMin((unsigned long long *)&C.drn_wendw, (unsigned long long)wndw);
  }
}
// A widened window some rank cannot hold (wide partitioned engines): the run must be a narrow window (every child
// of a run event sorts after every run event), so the sorted candidates past the window's narrow bound leave it —
// those from the pool stay there, the others (children, remote events) are parked in the fresh buffer, which the
// next handled window's maintenance moves into the pool; k_drun_red folds every candidate into the reduction.
__global__ __launch_bounds__(1024) void k_drun_trim(const P2PDev M, uint64_t n) {
  Ctl &C = *M.C;
  const uint64_t nb = C.nbound, tmin = C.tmin;
  __shared__ uint64_t s_cut;
  if (threadIdx.x == 0) {  // the first candidate past the narrow bound (rn_key is sorted)
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (M.rn_key[mid] <= nb) lo = mid + 1;
      else hi = mid;
    }
    s_cut = lo;
  }
  __syncthreads();
  const uint64_t cut = s_cut;
  for (uint64_t i = cut + threadIdx.x; i < n; i += 1024) {
    if (M.rn_src[i] != NOSRC) continue;  // (still in the pool)
    const uint64_t fi = atomicAdd((unsigned long long *)&C.nF, 1ull);
    if (fi >= M.fcap) {
      atomicOr(M.error, 1u);
      continue;
    }
    const uint64_t k = M.rn_key[i];
    M.f_ts[fi] = tmin + (k >> 32);
    M.f_uid[fi] = (uint32_t)k;
    M.f_ctx[fi] = M.rn_ctx[i];
    M.f_kind[fi] = M.rn_kind[i];
    M.f_a[fi] = M.rn_a[i];
    M.f_pkt[fi] = M.rn_pkt[i];
  }
  if (threadIdx.x == 0) C.drcut = cut;
}
// The next chunk's cut key from the ranks' smallest fitting key fk and smallest head key hk (every rank computes
// the same): a chunk that continues the same-ts group the last one cut (gp: the last chunk's key) takes more of
// that group, and when the rest of the group fits, exactly the rest — and the run ends after it (its queued
// DoForwardUp leaves at that ts are pending: they sort before every later run entry); otherwise the chunk backs
// off to the start of the group its fitting key would cut, unless that group alone fills it.
struct DrunCut {
  uint64_t g, lo;
  uint32_t trim;
};
__device__ __forceinline__ DrunCut drun_cut(uint64_t fk, uint64_t hk, uint64_t gp) {
  const uint64_t T0 = hk >> 32, gend = (T0 << 32) | 0xffffffffull;
  if (gp != ~0ull && (uint32_t)gp != 0xffffffffu && (gp >> 32) == T0)  // (a real key's uid is below 0xffffffff)
    return fk >= gend ? DrunCut{gend, T0, 1u} : DrunCut{fk, T0, 0u};
  if (fk != ~0ull && (fk >> 32) > T0) return DrunCut{((fk >> 32) << 32) - 1, ~0ull, 0u};
  return DrunCut{fk, ~0ull, 0u};
}
__global__ __launch_bounds__(TB) void k_drun_first(const P2PDev M) {
  Ctl &C = *M.C;
  uint64_t fk = ~0ull, hk = ~0ull;
  for (uint32_t q = 0; q < M.nranks; q++) {
    fk = M.xk_recv[2 * q] < fk ? M.xk_recv[2 * q] : fk;
    hk = M.xk_recv[2 * q + 1] < hk ? M.xk_recv[2 * q + 1] : hk;
  }
  const uint64_t g = drun_cut(fk, hk, ~0ull).g;
  drun_chunk<TB>(M, C, (uint64_t)blockIdx.x * TB + threadIdx.x, 0, C.drW, g);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const WinBound b = drun_bound(C, g);
    publish_bound(C, b);
    C.split_lo = ~0ull;  // (leaves at a cut group's ts are queued: pending events of that ts sort before them)
    C.split_hi = drun_cuts_group(g, C.drb_bound) ? (g >> 32) : b.span;
    C.hrel = C.split_hi;
    C.hcap = 0;
    C.drun = 1;
    C.drg = g;
    C.prep = 1;  // (the next k2_pa finds the window formed: it appended the last window already)
    C.mode = MODE_NORMAL;
  }
}

constexpr int GT_CT = 1;  // column tiles of one k_gtile work item (more: fewer atomics, but the compares bound it)
constexpr int GJ = 64;    // columns of one k_gtile tile (smaller tiles, more waves a SIMD to interleave: 256 -> 64
                          // columns took a wide window's k_gtile from 25 to 17 us)
static_assert(GJ <= 64, "k_gtile's packed column counts (7-bit count field)");
constexpr int GTB = 8192;  // blocks of k_gtile (grid-stride over tiles: a wide window's ~5,600 tiles in one round)
// The partitioned window's dispatch order, in three steps (r06; before, k_gtile compared every row with every
// rank's records, so its work grew with the ranks: 12.6 / 19.6 / 40.6 / 52.8 us a window at 1 / 2 / 4 / 8
// loopback partitions, profiles/r06/gtile_scale/):
//   k_gtile (before the X1 exchange): this rank's records among themselves, all pairs in tiles;
//   k_gsort (more than one rank): each record into the rank's X1 at its rank there (SEnt: its order key and the
//     exclusive prefixes of the children / inline children before it, a sentinel with the totals after them);
//   k_gsearch (after the exchange): a record's place among another rank's records is a binary search of that
//     rank's sorted list (records of different ranks never tie), its counts and prefixes read at that place.
// Rows: this rank's window records — its W gen-0 slots, then (WIDE) its L local records in X1Loc order; columns:
// this rank's, in column tiles of GJ (its gen-0 tiles, then its local tiles).  Per row, over the rank's window: the
// records before it (its rank), those of a smaller ts, those of ts <= its own (its same-ts group's end), and the
// children / inline children of the records before it and before its group (uid and dispatch prefixes).  A gen-0
// record precedes a local one of equal ts; two local records compare by their order words, a tie by the ancestor
// uid, then (same ancestor: same node, this rank) by their exact chains.
template <bool WIDE>
__global__ __launch_bounds__(HB, 6) void k_gtile(const P2PDev M) {  // (6 waves a SIMD: 73 VGPRs; 8 spilled)
  Ctl &C = *M.C;
  // the run control and every rank's window size in one trip (the sizes loaded before the test: a load after a
  // branch on C.hdl waited for it)
  const uint32_t hdl = C.hdl, W = C.pW;
  const X1Hdr *hs = x1hdr(M.x1_send, 0);  // (this rank's summary: the tiles rank its records among themselves)
  const uint32_t L0 = WIDE ? hs->L : 0u, tq0 = hs->tinl;
#ifdef NSGPU_PHASE_PROF
  const uint64_t gt_t0 = __builtin_amdgcn_s_memrealtime();
  const bool gt_rec = C.windows == g_blk_win && blockIdx.x < (uint32_t)GT_BLK_MAX;
  uint64_t gt_t[4] = {0, 0, 0, 0}, gt_kind = 0;
#define GT_MARK(k)                                                       \
  do {                                                                   \
    if (gt_rec && !gt_t[k]) gt_t[k] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define GT_MARK(k) (void)0
#endif
  if (!hdl) return;  // (k2_handle ran nothing: a cut, a pause, the end)
  // a column tile in LDS: its rel ts (the common test), child counts, and the fine key an equal ts needs — a
  // gen-0 record's uid; a local record's order words' low part and second word (ties: ancestor uid, record)
  // a column's child counts packed for the row's before-sum (tpb: 1 | children << 7 | inline children << 29 — over
  // one tile of GJ <= 64 columns the three fields stay within 7, 22 and 22 bits) and its inline children alone
  // (read four columns at a time as 16-B vectors)
  __shared__ __align__(16) uint32_t tts[GJ], tni[GJ], tfa[GJ];
  __shared__ __align__(16) uint64_t tpb[GJ], tfb[GJ];  // (tfb: a gen-0 column's whole key, a local one's w2)
  __shared__ uint32_t tu[WIDE ? GJ : 1], tr[WIDE ? GJ : 1];
  const uint32_t L = L0;
  const uint32_t ng = (W + GJ - 1) / GJ;  // (column tiles: the gen-0 records', then the local records')
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // (for k_dfin2: its record blocks then read no X1 header, and its
    C.gt_tinl = tq0;                          //  block 0, the only reader left, resets this rank's header; more
    C.gt_lown = L;                            //  ranks: k_gsearch sums every rank's inline children)
  }
  GT_MARK(0);
  const uint32_t njt = ng + (L + GJ - 1) / GJ, NR = W + L;
  // a work item: one row tile against GT_CT consecutive column tiles, summed in registers (one pair of atomics per
  // row and item: the accumulators' atomics, not the compares, bound the kernel)
  const uint32_t nseg = (njt + GT_CT - 1) / GT_CT;
  const uint32_t nrt = (NR + HB - 1) / HB;
  const uint64_t T = (uint64_t)nrt * nseg;
  for (uint64_t t = blockIdx.x; t < T; t += gridDim.x) {  // (uniform over the block)
   // the local rows' tiles first (the last row tiles): their loads and compares take about twice a gen-0
   // tile's, and the blocks dispatched first start first
   const uint32_t ti = nrt - 1u - (uint32_t)(t / nseg), sg = (uint32_t)(t % nseg);
   const uint32_t i = ti * HB + threadIdx.x;
   const bool lrow = WIDE && i >= W;
   uint32_t tx = 0, fax = 0, xu = 0, xrec = 0;
   uint64_t fbx = 0;
   if (i < NR) {
     if (lrow) {
       const X1Loc e = x1loc(M)[i - W];
       tx = (uint32_t)(e.w1 >> 32), fax = (uint32_t)e.w1, fbx = e.w2, xu = e.anc, xrec = e.rec;
     } else {
       const uint64_t key = M.wkey[i];
       tx = (uint32_t)(key >> 32), fax = (uint32_t)key;
     }
   }
   uint32_t gr = 0, cp = 0, ip = 0, ipf = 0, lp = 0;
   const uint32_t tj1 = (sg + 1) * GT_CT < njt ? (sg + 1) * GT_CT : njt;
   for (uint32_t tj = sg * GT_CT; tj < tj1; tj++) {
    const bool ltile = WIDE && tj >= ng;  // a tile of the local records
    const uint32_t j0 = (ltile ? tj - ng : tj) * GJ, nq = ltile ? L : W;
    const uint32_t n = nq - j0 < (uint32_t)GJ ? nq - j0 : (uint32_t)GJ;
    if (ltile) {
      const X1Loc *E = x1loc(M) + j0;
      for (uint32_t k = threadIdx.x; k < (uint32_t)GJ; k += HB) {  // (padding: a ts after every row's)
        const bool in = k < n;
        const uint64_t w1 = in ? E[k].w1 : ~0ull;
        tts[k] = (uint32_t)(w1 >> 32);
        tfa[k] = (uint32_t)w1;
        tfb[k] = in ? E[k].w2 : ~0ull;
        const uint32_t c = in ? E[k].cnt : 0u;
        tpb[k] = 1ull | (uint64_t)(c & 0xffffu) << 7 | (uint64_t)(c >> 16) << 29;
        tni[k] = c >> 16;
        tu[k] = in ? E[k].anc : 0u;
        tr[k] = in ? E[k].rec : 0u;
      }
    } else {
      const X1Ent *E = x1ent(M) + j0;
      for (uint32_t k = threadIdx.x; k < (uint32_t)GJ; k += HB) {
        const uint64_t key = k < n ? E[k].key : ~0ull;
        tts[k] = (uint32_t)(key >> 32);
        tfa[k] = (uint32_t)key;
        tfb[k] = key;
        const uint32_t c = k < n ? E[k].cnt : 0u;
        tpb[k] = 1ull | (uint64_t)(c & 0xffffu) << 7 | (uint64_t)(c >> 16) << 29;
        tni[k] = c >> 16;
      }
    }
    __syncthreads();
    GT_MARK(1);
#ifdef NSGPU_PHASE_PROF
    gt_kind |= (ltile ? 1u : 0u) | (__any(lrow) ? 2u : 0u) | (__any(i < NR) ? 8u : 0u);
#endif
    if (i < NR) {
      // per column: earlier ts -> before (and in ipf); equal ts -> the fine key: gen-0 x gen-0 by uid, a gen-0
      // record before a local one, local x local by the order words (their ties after the loop)
      // (the compares bound the kernel: one 64-bit add of the packed counts a column instead of three selects)
      uint64_t ab = 0;
      // columns y0..y0+3: rel ts, inline children, packed counts (and, FA / FB, the fine key's parts)
      struct Col4 {
        uint32_t ts[4], ni[4], fa[4];
        uint64_t pb[4], fb[4];
      };
      auto col4 = [&](uint32_t y0, bool FA, bool FB) {
        Col4 c;
        const uint4 a = *(const uint4 *)&tts[y0], b = *(const uint4 *)&tni[y0];
        const ulonglong2 p0 = *(const ulonglong2 *)&tpb[y0], p1 = *(const ulonglong2 *)&tpb[y0 + 2];
        c.ts[0] = a.x, c.ts[1] = a.y, c.ts[2] = a.z, c.ts[3] = a.w;
        c.ni[0] = b.x, c.ni[1] = b.y, c.ni[2] = b.z, c.ni[3] = b.w;
        c.pb[0] = p0.x, c.pb[1] = p0.y, c.pb[2] = p1.x, c.pb[3] = p1.y;
#pragma unroll
        for (int k = 0; k < 4; k++) {  // (opaque: else the selects below become a masked load each, and a wait)
          asm("" : "+v"(c.pb[k]));
          asm("" : "+v"(c.ni[k]));
        }
        if (FA) {
          const uint4 f = *(const uint4 *)&tfa[y0];
          c.fa[0] = f.x, c.fa[1] = f.y, c.fa[2] = f.z, c.fa[3] = f.w;
        }
        if (FB) {
          const ulonglong2 f0 = *(const ulonglong2 *)&tfb[y0], f1 = *(const ulonglong2 *)&tfb[y0 + 2];
          c.fb[0] = f0.x, c.fb[1] = f0.y, c.fb[2] = f1.x, c.fb[3] = f1.y;
        }
        return c;
      };
      auto acc = [&](const Col4 &c, int k, bool bef, bool lt, bool le) {
        ab += bef ? c.pb[k] : 0ull;
        lp += le;
        ipf += lt ? c.ni[k] : 0u;
      };
      if (!ltile && !lrow) {  // (the whole keys in one 64-bit compare)
        const uint64_t kx = (uint64_t)tx << 32 | fax;
#pragma unroll 2
        for (uint32_t y0 = 0; y0 < (uint32_t)GJ; y0 += 4) {
          const Col4 c = col4(y0, false, true);
#pragma unroll
          for (int k = 0; k < 4; k++) acc(c, k, c.fb[k] < kx, c.ts[k] < tx, c.ts[k] <= tx);
        }
      } else if (!lrow) {  // gen-0 row, local columns: before iff an earlier ts
#pragma unroll 4
        for (uint32_t y0 = 0; y0 < (uint32_t)GJ; y0 += 4) {
          const Col4 c = col4(y0, false, false);
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const bool lt = c.ts[k] < tx;
            acc(c, k, lt, lt, c.ts[k] <= tx);
          }
        }
      } else if (!ltile) {  // local row, gen-0 columns: before iff ts <= the row's
#pragma unroll 4
        for (uint32_t y0 = 0; y0 < (uint32_t)GJ; y0 += 4) {
          const Col4 c = col4(y0, false, false);
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const bool le = c.ts[k] <= tx;
            acc(c, k, le, c.ts[k] < tx, le);
          }
        }
      } else {  // local x local
        const int self = (i - W >= j0 && i - W < j0 + n) ? (int)(i - W - j0) : -1;
        bool tie = false;
#pragma unroll 2
        for (uint32_t y0 = 0; y0 < (uint32_t)GJ; y0 += 4) {
          const Col4 c = col4(y0, true, true);
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const bool lt = c.ts[k] < tx, eq = c.ts[k] == tx;
            const bool ea = eq & (c.fa[k] == fax);
            tie |= ea & (c.fb[k] == fbx) & ((int)(y0 + k) != self);
            acc(c, k, lt | (eq & (c.fa[k] < fax)) | (ea & (c.fb[k] < fbx)), lt, lt | eq);
          }
        }
#ifdef NSGPU_PHASE_PROF
        gt_kind |= __any(tie) ? 4u : 0u;
#endif
        if (tie) {  // (rare: equal words — a clamped ancestor uid, or one ancestor's chains)
          for (uint32_t y = 0; y < n; y++) {
            if (tts[y] != tx || tfa[y] != fax || tfb[y] != fbx || (int)y == self) continue;
            const bool lt = tu[y] != xu ? tu[y] < xu : lk_before(M.lkey[tr[y] - LBASE], M.lkey[xrec - LBASE]);
            if (lt) ab += tpb[y];
          }
        }
      }
      gr += (uint32_t)(ab & 0x7fu);
      cp += (uint32_t)((ab >> 7) & 0x3fffffu);
      ip += (uint32_t)((ab >> 29) & 0x3fffffu);
    }
    GT_MARK(2);
    __syncthreads();
   }
   if (i < NR) {
     // two packed 64-bit accumulators instead of five words: (rank, group end, inline prefix: each at
     // most MAXR x NACC < 2^21) and (child prefix < 2^32, the group's inline prefix)
     unsigned long long *A = reinterpret_cast<unsigned long long *>(M.gacc);
     const uint32_t row = lrow ? (uint32_t)WCAP + (i - W) : i;
     const uint64_t w0 = (uint64_t)gr | ((uint64_t)lp << 21) | ((uint64_t)ip << 42);
     const uint64_t w1 = (uint64_t)cp | ((uint64_t)ipf << 32);
     if (w0) atomicAdd(&A[row], (unsigned long long)w0);
     if (w1) atomicAdd(&A[NACC + row], (unsigned long long)w1);
   }
  }
#ifdef NSGPU_PHASE_PROF
  __builtin_amdgcn_s_waitcnt(0);
  if (gt_rec && threadIdx.x == 0) {
    g_gt[blockIdx.x][0] = gt_t0;
    for (int k = 0; k < 3; k++) g_gt[blockIdx.x][1 + k] = gt_t[k];
    g_gt[blockIdx.x][4] = __builtin_amdgcn_s_memrealtime();
    uint32_t xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
    g_gt[blockIdx.x][5] = xcc;
    g_gt[blockIdx.x][6] = gt_kind;
  }
#endif
#undef GT_MARK
}

// k_gsort: this rank's records into its X1 list at their ranks among themselves (k_gtile's accumulators hold only
// this rank's contributions until k_gsearch), with the prefixes before each and the totals after the last.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_gsort(const P2PDev M) {
  const Ctl &C = *M.C;
  const uint32_t hdl = C.hdl, W = C.pW;
  const uint32_t L = WIDE ? x1hdr(M.x1_send, 0)->L : 0u;
  if (!hdl) return;
  const uint32_t NR = W + L, i = blockIdx.x * 256 + threadIdx.x;
  SEnt *S = x1srt(M.x1_send, 0);
  if (NR == 0) {
    if (i == 0) S[0] = SEnt{~0ull, ~0ull, ~0u, 1u, 0u, 0u};
    return;
  }
  if (i >= NR) return;
  const uint64_t *A = reinterpret_cast<const uint64_t *>(M.gacc);
  const bool lrow = WIDE && i >= W;
  const uint32_t row = lrow ? (uint32_t)WCAP + (i - W) : i;
  const uint64_t w0 = A[row], w1 = A[NACC + row];
  SEnt e;
  uint32_t cnt;
  if (lrow) {
    const X1Loc x = x1loc(M)[i - W];
    e = SEnt{x.w1, x.w2, x.anc, 1u, 0u, 0u};
    cnt = x.cnt;
  } else {
    const X1Ent x = x1ent(M)[i];
    e = SEnt{x.key, 0ull, 0u, 0u, 0u, 0u};
    cnt = x.cnt;
  }
  const uint32_t gr = (uint32_t)(w0 & 0x1fffffu);
  e.cp = (uint32_t)w1;
  e.ip = (uint32_t)(w0 >> 42);
  if (gr < NR) S[gr] = e;
  else atomicOr(M.error, 64u);  // (ranks among the rank's own records are a permutation)
  if (gr == NR - 1) S[NR] = SEnt{~0ull, ~0ull, ~0u, 1u, e.cp + (cnt & 0xffffu), e.ip + (cnt >> 16)};
}

// Record e of another rank before this rank's record x, in the merged dispatch order: earlier rel ts, then a gen-0
// record before a local one, then (gen-0) the uid, (local) the order words and the ancestor uid.
__device__ __forceinline__ bool sent_before(uint64_t ek0, uint32_t eL, uint64_t eb, uint32_t ec, uint64_t xk0, uint32_t xL,
                                            uint64_t xb, uint32_t xc) {
  if ((ek0 >> 32) != (xk0 >> 32)) return (ek0 >> 32) < (xk0 >> 32);
  if (eL != xL) return eL < xL;
  if ((uint32_t)ek0 != (uint32_t)xk0) return (uint32_t)ek0 < (uint32_t)xk0;
  if (eb != xb) return eb < xb;
  return ec < xc;
}
constexpr int GS_T = 256;             // k_gsearch: rows a block (one peer rank per blockIdx.y)
constexpr int GS_STEP = 32;           // every GS_STEP-th record of the peer's list sampled into LDS
constexpr int GS_NS = NACC / GS_STEP + 1;
// k_gsearch: this rank's records against each other rank's sorted list — three searches a (row, peer): the
// records before the row, those of a smaller ts, those of ts <= its own — first over the list's samples in LDS,
// then within GS_STEP entries in the list (five trips); the counts and the prefixes found there are added to the
// row's accumulators (k_gtile's packing).  Block (0, 0) also sums every rank's inline children for k_dfin2.
template <bool WIDE>
__global__ __launch_bounds__(GS_T) void k_gsearch(const P2PDev M) {
  Ctl &C = *M.C;
  const uint32_t hdl = C.hdl, W = C.pW;
  const uint32_t L = WIDE ? x1hdr(M.x1_send, 0)->L : 0u;
  const uint32_t q = blockIdx.y < M.rank ? blockIdx.y : blockIdx.y + 1u;  // (the peer)
  const X1Hdr *hq = x1hdr(M.x1_recv, q);
  const uint32_t nq = hq->W + (WIDE ? hq->L : 0u);
  const uint32_t tq = threadIdx.x < M.nranks ? x1hdr(M.x1_recv, threadIdx.x)->tinl : 0u;
  if (!hdl) return;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) {  // (wave 0: one lane per rank)
    const uint32_t tg = wave_sum32(tq);
    if (threadIdx.x == 0) C.gt_tinl = tg;
  }
  const uint32_t NR = W + L, i = blockIdx.x * GS_T + threadIdx.x;
  if (blockIdx.x * GS_T >= NR) return;  // (block-uniform)
  const SEnt *S = x1srt(M.x1_recv, q);
  __shared__ uint64_t s_k0[GS_NS], s_b[GS_NS];
  __shared__ uint32_t s_c[GS_NS], s_L[GS_NS];
  const uint32_t ns = (nq + GS_STEP - 1) / GS_STEP;
  for (uint32_t k = threadIdx.x; k < ns; k += GS_T) {
    const SEnt e = S[k * GS_STEP];
    s_k0[k] = e.k0, s_b[k] = e.b, s_c[k] = e.c, s_L[k] = e.L;
  }
  __syncthreads();
  if (i >= NR) return;
  const bool lrow = WIDE && i >= W;
  uint64_t xk0, xb = 0;
  uint32_t xc = 0, xL = 0;
  if (lrow) {
    const X1Loc x = x1loc(M)[i - W];
    xk0 = x.w1, xb = x.w2, xc = x.anc, xL = 1u;
  } else {
    xk0 = x1ent(M)[i].key;
  }
  const uint32_t xts = (uint32_t)(xk0 >> 32);
  // the samples: how many satisfy each predicate (a prefix of them: the list is sorted)
  uint32_t lo[3] = {0, 0, 0}, cn[3] = {ns, ns, ns};
  while (cn[0] | cn[1] | cn[2]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (!cn[k]) continue;
      const uint32_t h = cn[k] >> 1, m = lo[k] + h;
      const uint32_t ets = (uint32_t)(s_k0[m] >> 32);
      const bool p = k == 0 ? sent_before(s_k0[m], s_L[m], s_b[m], s_c[m], xk0, xL, xb, xc) : k == 1 ? ets < xts : ets <= xts;
      if (p) lo[k] = m + 1, cn[k] -= h + 1;
      else cn[k] = h;
    }
  }
  // within the list: entries ((c - 1) * STEP, min (c * STEP, nq)) after the last satisfying sample c - 1
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint32_t c = lo[k];
    if (c == 0) {
      cn[k] = 0;
    } else {
      lo[k] = (c - 1) * GS_STEP + 1;
      const uint32_t hi = c * GS_STEP < nq ? c * GS_STEP : nq;
      cn[k] = hi > lo[k] ? hi - lo[k] : 0u;
    }
  }
  while (cn[0] | cn[1] | cn[2]) {  // (the three searches' loads in flight together)
    uint32_t m[3];
    uint64_t ek0[3];
#pragma unroll
    for (int k = 0; k < 3; k++) m[k] = lo[k] + (cn[k] >> 1);
    const SEnt e0 = S[m[0]];
    ek0[0] = e0.k0;
    ek0[1] = S[m[1]].k0;
    ek0[2] = S[m[2]].k0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (!cn[k]) continue;
      const uint32_t h = cn[k] >> 1, ets = (uint32_t)(ek0[k] >> 32);
      const bool p = k == 0 ? sent_before(e0.k0, e0.L, e0.b, e0.c, xk0, xL, xb, xc) : k == 1 ? ets < xts : ets <= xts;
      if (p) lo[k] = m[k] + 1, cn[k] -= h + 1;
      else cn[k] = h;
    }
  }
  const uint32_t p = lo[0], plt = lo[1], ple = lo[2];  // (<= nq: entry nq is the sentinel)
  const SEnt ep = S[p];
  const uint32_t ipf = S[plt].ip;
  if (p < nq && ep.k0 == xk0 && ep.L == xL && ep.b == xb && ep.c == xc) atomicOr(M.error, 64u);  // (a tie: impossible)
  unsigned long long *A = reinterpret_cast<unsigned long long *>(M.gacc);
  const uint32_t row = lrow ? (uint32_t)WCAP + (i - W) : i;
  const uint64_t w0 = (uint64_t)p | ((uint64_t)ple << 21) | ((uint64_t)ep.ip << 42);
  const uint64_t w1 = (uint64_t)ep.cp | ((uint64_t)ipf << 32);
  if (w0) atomicAdd(&A[row], (unsigned long long)w0);
  if (w1) atomicAdd(&A[NACC + row], (unsigned long long)w1);
}

// Block 0 also does the pool bookkeeping (k2_scan's) and, last, the run bookkeeping; the other blocks
// read only fields block 0 leaves alone (pW, puid0, hdl, done < 2).  WIDE: threads WCAP.. take this rank's local
// records (X1Loc order): a local record's uid is its parent's child prefix + its child index.
constexpr int DF2_FB = 2;  // k_dfin2's blocks before the record blocks (the books, the free-stack move)
template <bool WIDE>
__global__ __launch_bounds__(HB) void k_dfin2(const P2PDev M) {
  Ctl &C = *M.C;
  BLK_T0();
#ifdef NSGPU_PHASE_PROF
  const uint64_t c_win = C.windows;  // (diagnostic: block stamps in g_blk[2], the partitioned path runs no k2_scan)
#endif
  const uint32_t hdl = C.hdl, W = C.pW;  // (tested after the loads below: a load after a branch on it waited for it)
  const uint32_t tinl_g = C.gt_tinl, Lown = WIDE ? C.gt_lown : 0u;  // (k_gtile's, from the X1 headers)
  // block 0: every rank's X1 header at once, one lane per rank (HB = one wave)
  const uint32_t lq = threadIdx.x;
  const X1Hdr *lh = x1hdr(M.x1_recv, lq < M.nranks ? lq : 0u);
  const bool lv = lq < M.nranks;
  const uint32_t l_q = (WIDE && lv && blockIdx.x == 0) ? lh->L : 0u;  // (the ranks' local records)
  // (block 0: the rest of the summaries and the run control, for the run bookkeeping, in the same trip)
  struct Bk {
    uint64_t nF, nfree, npush, pK0, ptmin, windows, P_end, live, inline_lim, max_windows, max_window, drg, dr1;
    uint64_t bound, span_t;
    uint32_t nhub, puid0, rt, drtrim, drun;
  } bk{};
  if (blockIdx.x <= 1)  // (block 1: the free-stack move and the hubs' tables, beside block 0's bookkeeping)
    bk = Bk{C.nF, C.nfree, C.npush, C.pK0, C.ptmin, C.windows, C.P_end, C.live, C.inline_lim, C.max_windows,
            C.max_window, C.drg, C.dr1, WIDE ? C.bound : 0, WIDE ? C.span_t : 0, C.nhub, C.puid0, C.rt, C.drtrim,
            C.drun};
  uint32_t hW = 0, htc = 0, hneedc = 0, hsuid = 0;
  uint64_t hlk = 0, htmin = ~0ull, hwend = ~0ull, hwendw = ~0ull, hsts = ~0ull, hrkey = ~0ull, hrrem = 0,
           hrhead = ~0ull;
  if (blockIdx.x == 0 && lv) {
    hW = lh->W;
    htc = lh->tc;
    hneedc = lh->needc;
    hlk = lh->lastkey;
    htmin = lh->red.tmin;
    hwend = lh->red.wend;
    hwendw = lh->red.wendw;
    hsts = lh->red.stopts;
    hsuid = lh->red.stopuid;
    hrkey = lh->rkey;
    hrrem = lh->rrem;
    hrhead = lh->rhead;
  }
  // the record's accumulators, record and first children, all loaded before anything waits — with the headers,
  // before the arrival's wait (WIDE: thread WCAP + k takes local record k of this rank, its record index from
  // the X1Loc list: one more trip; its parent's child prefix needs the parent's accumulator, one more)
  // (block 0 keeps the books, block 1 moves the free stack: the records are the next blocks' — block 0 was the
  //  kernel's tail with the books after its own records, block 1 with the stack move after its records)
  const bool rec_block = blockIdx.x >= (uint32_t)DF2_FB;
  const uint32_t ti = (rec_block ? blockIdx.x - (uint32_t)DF2_FB : 0u) * HB + threadIdx.x;
  const bool loc = WIDE && ti >= (uint32_t)WCAP;
  uint64_t *A = reinterpret_cast<uint64_t *>(M.gacc);
  uint64_t w0, w1, wk;
  uint32_t s = ti, wc, ncr, ckw[PFC], cctx[PFC], wpar = 0;
  {  // (speculative: every thread loads, whether or not its record exists — the indices stay in range)
    uint64_t lw1 = 0;
    if (loc) {
      const X1Loc e = x1loc(M)[ti - WCAP];
      s = e.rec < (uint32_t)WTOT ? e.rec : (uint32_t)WTOT - 1u;
      lw1 = e.w1;
      wpar = e.par;
    }
    w0 = A[ti];
    w1 = A[NACC + ti];
    wk = loc ? lw1 : M.wkey[s];
    wc = M.wctx[s];
    ncr = M.nchild[s];
#pragma unroll
    for (int j = 0; j < PFC; j++) {  // (a child index past maxc loads the slot's last one: in range, ignored)
      const uint32_t sl = s * M.maxc + min((uint32_t)j, M.maxc - 1u);
      ckw[j] = M.ch_kind[sl];
      cctx[j] = M.ch_ctx[sl];
    }
  }
  if (!hdl) return;  // (k2_handle ran nothing: a cut, a pause, the end)
  // X1 is all-gathered in place (x1_send is this rank's slot of x1_recv): block 0, the kernel's only reader of the
  // headers (k_gtile's reads ended with its launch), resets this rank's for the next window once its loads have
  // returned (one wave: the wave's wait covers every lane)
  if (blockIdx.x == 0) {
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __builtin_amdgcn_s_waitcnt(0);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    X1Hdr *hs = x1hdr(M.x1_send, 0);
    hs->W = hs->tc = hs->tinl = hs->needc = 0;
    hs->L = 0;
    hs->lastkey = 0;
    hs->red.tmin = hs->red.wend = hs->red.stopts = hs->red.wendw = ~0ull;
    hs->red.stopuid = 0;
    hs->rkey = ~0ull;
    hs->rrem = 0;
  }
  const bool vs = rec_block && (loc ? ti - (uint32_t)WCAP < Lown : ti < W);
  if (vs) {
    if (!WIDE) {  // (wide: k2_handle zeroes them — a local record reads its parent's below)
      A[ti] = 0;
      A[NACC + ti] = 0;
    }
    const uint32_t gr = (uint32_t)(w0 & 0x1fffffu), lp = (uint32_t)((w0 >> 21) & 0x1fffffu),
                   ip = (uint32_t)(w0 >> 42), cp = (uint32_t)w1, ipf = (uint32_t)(w1 >> 32);
    // as k2_scan: (dispatch rank rel. K0, rank of the first inline child, child prefix, inline prefix)
    M.sinfo[s] = make_uint4(gr + (tinl_g ? ipf : 0), lp + ip, cp, ip);
    if (loc) {  // uid = the parent's child prefix + the child index (DefaultSimulatorImpl::Schedule order)
      const uint32_t prow = wpar & 0xffffffu;  // (k_xlcompact: the parent's row, gen-0 slot or WCAP + compact index)
      const uint32_t pcp = (uint32_t)A[NACC + (prow < (uint32_t)NACC ? prow : 0u)];
      M.pwkey[s] = ((wk >> 32) << 32) | (uint32_t)(C.puid0 + pcp + (wpar >> 24));
      M.lrec[ti - WCAP] = s;
    } else {
      M.pwkey[s] = wk;
    }
    M.pwctx[s] = wc;
    const uint32_t uid0 = C.puid0;
    // the record's children on other ranks' nodes -> X2 (one rank: none).  Their kinds eight at a time (one
    // dependent load a child past the first PFC held a record with many children ~10 us: the kernel's tail)
    constexpr int KB = 8;
    static_assert(PFC <= KB, "the preloaded kinds fit the first batch");
    for (uint32_t j0 = 0; M.nranks > 1 && j0 < ncr; j0 += KB) {
      uint32_t kwv[KB];
#pragma unroll
      for (int q = 0; q < KB; q++) {
        const uint32_t j = j0 + q;
        kwv[q] = (j0 == 0 && q < PFC) ? ckw[q < PFC ? q : 0] : j < ncr ? M.ch_kind[s * M.maxc + j] : 0u;
      }
#pragma unroll
      for (int q = 0; q < KB; q++) {
        const uint32_t j = j0 + q, kw = kwv[q];
        if (j >= ncr || (kw & 0xffu) == K_FWD_UP) continue;
        if (!(kw & REMOTEBIT)) continue;  // (a Receive on another rank's node: the device step marked it)
        const uint32_t sl = s * M.maxc + j;
        const uint32_t ctx = (j0 == 0 && q < PFC) ? cctx[q < PFC ? q : 0] : M.ch_ctx[sl];
        const uint32_t qr = M.owner[ctx];
        const uint32_t pos = atomicAdd(&x2hdr(M, M.x2_send, qr)->n, 1u);
        if (pos < M.capx)
          x2rec(M, M.x2_send, qr)[pos] = Ev{M.ch_ts[sl], uid0 + cp + j, ctx, kw, M.ch_a[sl], M.ch_pkt[sl]};
        else
          atomicOr(M.error, 16u);
      }
    }
  }
  // ---- pool bookkeeping (k2_scan's): the free stack loses the slots the fresh children took and gains
  // the window's; its pushed part is moved down over the popped hole; the hubs' slot tables are cleared
  const uint64_t nF = bk.nF, nfree = bk.nfree, npush = bk.npush;
  const uint64_t consumed = nF < nfree ? nF : nfree;
  const uint64_t mv = consumed < npush ? consumed : npush;
  const uint32_t nh = bk.nhub < (uint32_t)MAXHUB ? bk.nhub : (uint32_t)MAXHUB;
  if (blockIdx.x == 1) {  // the free-stack move and the hubs' slot tables (the two ranges are disjoint: eight
    constexpr int SB = 8;  // loads in flight a lane, then the stores)
    for (uint64_t i0 = threadIdx.x; i0 < mv; i0 += (uint64_t)HB * SB) {
      uint32_t v[SB];
#pragma unroll
      for (int k = 0; k < SB; k++) {
        const uint64_t i = i0 + (uint64_t)k * HB;
        v[k] = i < mv ? M.fstack[nfree + npush - mv + i] : 0u;
      }
#pragma unroll
      for (int k = 0; k < SB; k++) {
        const uint64_t i = i0 + (uint64_t)k * HB;
        if (i < mv) M.fstack[nfree - consumed + i] = v[k];
      }
    }
    for (uint32_t h = threadIdx.x; h < nh; h += HB) M.node_tab[(uint64_t)M.hub_list[h] * NTAB] = 0;
  }
  if (blockIdx.x != 0) {
    BLK_REC(2, c_win);
    return;
  }
  // the ranks' summaries, reduced across the lanes (rank q's in lane q)
  const uint32_t Wg = wave_sum32(hW), tcg = wave_sum32(htc), Lg = WIDE ? wave_sum32(l_q) : 0u;
  const uint32_t needc = __ballot(hneedc != 0) ? 1u : 0u;
  // a partitioned sorted run: entries left on some rank -> the next chunk (drun_cut), unless the chunk just
  // run ended the run (it ended a cut same-ts group)
  const bool drun_more = __ballot(hrrem != 0) != 0;
  const uint64_t drfk = wave_min64(hrrem != 0 ? hrkey : ~0ull), drhk = wave_min64(hrrem != 0 ? hrhead : ~0ull);
  const uint64_t lk = wave_max64(hW ? hlk : 0ull);
  Red rg{~0ull, ~0ull, ~0ull, 0, 0, ~0ull};
  rg.tmin = wave_min64(htmin);
  rg.wend = wave_min64(hwend);
  if (WIDE) rg.wendw = wave_min64(hwendw);
  // wide windows: the adaptive span keeps every rank's window inside its capacity (WCAP gen-0, NMAX records;
  // marks at 7/8 and 3/4 of both — the single engine's are span_next's, nsgpu_p2p_span.h: its capacities differ,
  // XLCAP and X1 are sized otherwise — from the largest rank's counts so that every rank forms the same bound)
  const uint64_t mxW = WIDE ? wave_max64(hW) : 0, mxN = WIDE ? wave_max64((uint64_t)hW + l_q) : 0;
  {  // the pending Stop: the smallest stopts, the first rank holding it
    rg.stopts = wave_min64(hsts);
    const uint64_t m = __ballot(lv && hsts == rg.stopts && rg.stopts != ~0ull);
    const int first = m ? __ffsll((unsigned long long)m) - 1 : 0;
    rg.stopuid = __shfl(hsuid, first);
  }
  if (threadIdx.x != 0) return;  // (the reductions above took the whole wave)
  C.K = bk.pK0 + Wg + Lg + tinl_g;
  if (WIDE) {
    C.plt = Lown;  // (the next k2_pa appends them from lrec)
    if (!bk.drun) {  // (a run's chunks are narrow)
      const uint64_t span = bk.bound >> 32;
      if (mxN > (uint64_t)(7 * NMAX / 8) || mxW > (uint64_t)(7 * WCAP / 8)) C.span_t = span - span / 4;
      else if (mxN < (uint64_t)(3 * NMAX / 4) && mxW < (uint64_t)(3 * WCAP / 4) && bk.span_t < (1ull << 40))
        C.span_t = bk.span_t + bk.span_t / 8 + 1;
    }
  }
  C.uid = bk.puid0 + tcg;
  if (Wg) C.last_ts = bk.ptmin + (lk >> 32);
  const uint32_t rt = bk.rt;
  C.red[rt] = rg;  // bounds the next window (k2_pa reads red[rt ^ 1] after the flip)
  C.rt = rt ^ 1;
  const uint64_t windows = bk.windows + 1;
  C.windows = windows;
  if (Wg + Lg > bk.max_window) C.max_window = Wg + Lg;
  const uint64_t P_end = bk.P_end + (nF > nfree ? nF - nfree : 0);
  C.nfree = nfree - consumed + npush;
  C.P_end = P_end;
  C.live = bk.live - npush + nF;
  C.npush = 0;
  C.nF = 0;
  C.nhub = 0;
  C.W = 0;
  C.overflow = 0;
  C.prep = 0;
  {
    const bool go = drun_more && !bk.drtrim;
    const DrunCut dc = go ? drun_cut(drfk, drhk, bk.drg) : DrunCut{~0ull, ~0ull, 0u};
    C.drun = go ? 1u : 0u;
    C.dr0 = bk.dr1;  // (the chunk just run ended there; k2_pa reads dr0 at its start)
    C.drg = dc.g;
    C.drlo = dc.lo;
    C.drtrim = dc.trim;
    C.dtrim = drun_more && bk.drtrim ? 1u : 0u;  // (the next k2_pa returns the run's entries left to pending)
  }
  // the window that held Simulator::Stop ends the run (every rank knows it from the bound), as does an
  // empty pending set on every rank (a run's entries from the fresh buffer are pending outside the pool)
  bool done = bk.inline_lim != ~0ull || (rg.tmin == ~0ull && !drun_more);
  if (P_end > M.pool_cap) {
    atomicOr(M.error, 1u);
    done = true;
  }
  if (windows >= bk.max_windows && !done) {
    atomicOr(M.error, 4u);
    done = true;
  }
  if ((uint64_t)bk.puid0 + tcg > UID_MAX_NEXT) {  // (every rank: tcg is the merged window's)
    atomicOr(M.error, 2048u);
    done = true;
  }
  if (done) C.done = 1;
  else if (needc && !drun_more) C.mode = MODE_COMPACT;  // (every rank: the pipelines stay in step; a run's
                                                         //  pool entries keep their slots until it ends)
  BLK_REC(2, c_win);
}

// Loopback transport (nsgpu_p2p_group_*: every partition on one device): one block per copy.
struct CopyDesc {
  const uint8_t *src;
  uint8_t *dst;
  uint64_t bytes;  // multiple of 16
};
__global__ __launch_bounds__(256) void k_copies(const CopyDesc *__restrict__ d) {
  const CopyDesc c = d[blockIdx.x];
  const uint4 *src = (const uint4 *)c.src;
  uint4 *dst = (uint4 *)c.dst;
  for (uint64_t i = threadIdx.x; i < c.bytes / 16; i += 256) dst[i] = src[i];
}


}  // namespace nsgpu
