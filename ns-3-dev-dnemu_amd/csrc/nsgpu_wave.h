// nsgpu_wave.h — the wave-wide cross-lane helpers the engines' kernels share (nsgpu_p2p_dev.h, nsgpu_wifil_dev.h):
// DPP moves, wave sum / min / max reductions, inclusive scans and the previous-lane moves.  Every one of them needs
// every lane of the wave active.  (nsgpu_hold.hip's moves carry an identity operand and nsgpu_p2p_win.h's cmap_dpp a
// bound-control flag: different functions, kept where they are.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nsgpu {

// Wave reductions (every lane of the wave active; the result in every lane): within each row of 16 lanes by DPP
// moves — quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror: each step pairs a lane with one of the other
// half of its group, so after four steps every lane holds its row's value — then the four rows' values read into
// scalars (v_readlane).  (The __shfl_xor butterflies were 6 dependent ds_bpermute rounds, LDS-latency each: the
// holders' five counter sums alone cost config 4 ~0.5 us a window.)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ uint64_t dpp64(uint64_t v) {
  return ((uint64_t)dpp32<CTRL>((uint32_t)(v >> 32)) << 32) | dpp32<CTRL>((uint32_t)v);
}
__device__ __forceinline__ uint32_t rl32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ uint64_t rl64(uint64_t v, int l) { return ((uint64_t)rl32((uint32_t)(v >> 32), l) << 32) | rl32((uint32_t)v, l); }
constexpr int DPP_X1 = 0xB1, DPP_X2 = 0x4E, DPP_HMIRROR = 0x141, DPP_MIRROR = 0x140;
__device__ __forceinline__ uint64_t wave_min64(uint64_t v) {
  uint64_t w;
  w = dpp64<DPP_X1>(v), v = w < v ? w : v;
  w = dpp64<DPP_X2>(v), v = w < v ? w : v;
  w = dpp64<DPP_HMIRROR>(v), v = w < v ? w : v;
  w = dpp64<DPP_MIRROR>(v), v = w < v ? w : v;
  const uint64_t a = rl64(v, 0), b = rl64(v, 16), c = rl64(v, 32), d = rl64(v, 48);
  const uint64_t x = a < b ? a : b, y = c < d ? c : d;
  return x < y ? x : y;
}
__device__ __forceinline__ uint64_t wave_max64(uint64_t v) {
  uint64_t w;
  w = dpp64<DPP_X1>(v), v = w > v ? w : v;
  w = dpp64<DPP_X2>(v), v = w > v ? w : v;
  w = dpp64<DPP_HMIRROR>(v), v = w > v ? w : v;
  w = dpp64<DPP_MIRROR>(v), v = w > v ? w : v;
  const uint64_t a = rl64(v, 0), b = rl64(v, 16), c = rl64(v, 32), d = rl64(v, 48);
  const uint64_t x = a > b ? a : b, y = c > d ? c : d;
  return x > y ? x : y;
}
__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
  v = max(v, dpp32<DPP_X1>(v));
  v = max(v, dpp32<DPP_X2>(v));
  v = max(v, dpp32<DPP_HMIRROR>(v));
  v = max(v, dpp32<DPP_MIRROR>(v));
  return max(max(rl32(v, 0), rl32(v, 16)), max(rl32(v, 32), rl32(v, 48)));
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
  v += dpp32<DPP_X1>(v);
  v += dpp32<DPP_X2>(v);
  v += dpp32<DPP_HMIRROR>(v);
  v += dpp32<DPP_MIRROR>(v);
  return rl32(v, 0) + rl32(v, 16) + rl32(v, 32) + rl32(v, 48);
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
  v += dpp64<DPP_X1>(v);
  v += dpp64<DPP_X2>(v);
  v += dpp64<DPP_HMIRROR>(v);
  v += dpp64<DPP_MIRROR>(v);
  return rl64(v, 0) + rl64(v, 16) + rl64(v, 32) + rl64(v, 48);
}
// Inclusive wave scans by DPP (every lane active): row_shr 1 / 2 / 4 / 8 within each row of 16 (a lane without a
// source adds 0), then row_bcast:15 (rows 1 and 3 add the previous row's last lane) and row_bcast:31 (rows 2 and 3
// add lane 31) — six DPP steps instead of six ds_bpermute rounds.
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ uint32_t dppm32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false);
}
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ uint64_t dppm64(uint64_t v) {
  return ((uint64_t)dppm32<CTRL, ROWS>((uint32_t)(v >> 32)) << 32) | dppm32<CTRL, ROWS>((uint32_t)v);
}
__device__ __forceinline__ uint32_t wave_incscan32(uint32_t v) {
  v += dppm32<0x111>(v);
  v += dppm32<0x112>(v);
  v += dppm32<0x114>(v);
  v += dppm32<0x118>(v);
  v += dppm32<0x142, 0xa>(v);
  v += dppm32<0x143, 0xc>(v);
  return v;
}
__device__ __forceinline__ uint64_t wave_incscan64(uint64_t v) {
  v += dppm64<0x111>(v);
  v += dppm64<0x112>(v);
  v += dppm64<0x114>(v);
  v += dppm64<0x118>(v);
  v += dppm64<0x142, 0xa>(v);
  v += dppm64<0x143, 0xc>(v);
  return v;
}
__device__ __forceinline__ uint32_t wave_exscan32(uint32_t v, int lane) {
  (void)lane;
  return wave_incscan32(v) - v;
}
// The previous lane's value (wave_shr:1; lane 0 gets 0).
__device__ __forceinline__ uint32_t prev_lane32(uint32_t v) { return dppm32<0x138>(v); }
__device__ __forceinline__ uint64_t prev_lane64(uint64_t v) {
  return ((uint64_t)prev_lane32((uint32_t)(v >> 32)) << 32) | prev_lane32((uint32_t)v);
}

}  // namespace nsgpu
