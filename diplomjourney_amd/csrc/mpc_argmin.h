// mpc_argmin.h — the lexicographic (cost, index) arg-min primitives (gfx950).
//
//   cost_key, cost_key_nonneg, key_cost   a cost as a totally ordered 64-bit key
//   rec_less                              (key, index) order: lowest cost, then lowest index
//   argmin_dpp_level, wave_argmin, wave_min_u32, wave_argmin32
//                                         the minimum over a wave by DPP moves
//   kBlock, kWaves, Rec, block_argmin     the block's minimum (LDS) and its 16-B record
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace mpc {

// Total order on costs for the arg-min: non-finite costs (NaN, +inf) map to
// the largest key and never win; -0 is folded into +0.
__device__ __forceinline__ uint64_t cost_key(double c) {
  if (!(c < __builtin_inf())) return ~0ull;
  c = c + 0.0;
  const uint64_t u = static_cast<uint64_t>(__double_as_longlong(c));
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// cost_key for a criterion value, which is never negative (a sum of
// 10000 * sqrt(.) and squares: +0 at least, or NaN / +inf): the same key
// without the sign fold — 2 VALU per candidate instead of ~6.
__device__ __forceinline__ uint64_t cost_key_nonneg(double c) {
  const uint64_t u = static_cast<uint64_t>(__double_as_longlong(c));
  return c < __builtin_inf() ? (u | 0x8000000000000000ull) : ~0ull;
}

__device__ __forceinline__ double key_cost(uint64_t k) {
  if (k == ~0ull) return __builtin_inf();
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double(static_cast<long long>(u));
}

// Lexicographic (key, index) order: lowest cost, then lowest index — the
// first strict minimum of the reference's ascending scan (:351).
__device__ __forceinline__ bool rec_less(uint64_t ka, int64_t ia, uint64_t kb, int64_t ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// One level of the wave reduction: every lane combines its (key, index) with
// the lane the DPP pattern CTRL names.  DPP moves run on the VALU: a level is
// a few cycles instead of an LDS round trip per 32-bit half (ds_bpermute).
// Lanes of rows outside RM receive an undefined value (no copy of the old
// one): the reduction below reads only lane 63, whose inputs are all defined.
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ void argmin_dpp_level(uint64_t& k, int64_t& i) {
  auto mv = [](uint64_t x) {
    const int lo = __builtin_amdgcn_mov_dpp(static_cast<int>(x), CTRL, RM, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(static_cast<int>(x >> 32), CTRL, RM, 0xf, true);
    return (static_cast<uint64_t>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo);
  };
  const uint64_t ok = mv(k);
  const int64_t oi = static_cast<int64_t>(mv(static_cast<uint64_t>(i)));
  const bool lt = rec_less(ok, oi, k, i);
  k = lt ? ok : k;
  i = lt ? oi : i;
}

// Lexicographic (key, index) minimum over the 64 lanes of a wave (all lanes
// active), returned in every lane.  quad_perm [1,0,3,2] and [2,3,0,1], then
// row_half_mirror and row_mirror leave each row of 16 lanes holding its
// minimum in every lane; row_bcast:15 (into rows 1, 3: lane 31 then holds
// rows 0-1, lane 63 rows 2-3) and row_bcast:31 (lane 31 into row 3) fold the
// rows into lane 63, which is broadcast.  The minimum of a total order does
// not depend on the combination order: the same result as any other
// reduction tree.
__device__ __forceinline__ void wave_argmin(uint64_t& k, int64_t& i) {
  argmin_dpp_level<0xB1>(k, i);
  argmin_dpp_level<0x4E>(k, i);
  argmin_dpp_level<0x141>(k, i);
  argmin_dpp_level<0x140>(k, i);
  argmin_dpp_level<0x142, 0xA>(k, i);
  argmin_dpp_level<0x143, 0xC>(k, i);
  auto lane63 = [](uint64_t x) {
    const uint32_t lo = __builtin_amdgcn_readlane(static_cast<int>(x), 63);
    const uint32_t hi = __builtin_amdgcn_readlane(static_cast<int>(x >> 32), 63);
    return (static_cast<uint64_t>(hi) << 32) | lo;
  };
  k = lane63(k);
  i = static_cast<int64_t>(lane63(static_cast<uint64_t>(i)));
}

// Minimum of a 32-bit value over the 64 lanes of a wave (all lanes active),
// returned in every lane: the DPP pattern of wave_argmin with v_min_u32
// (lanes a pattern does not feed get the identity 0xffffffff).
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
  auto lvl = [](uint32_t v, auto ctrl, auto rm) {
    constexpr int C = decltype(ctrl)::value, M = decltype(rm)::value;
    const uint32_t o = static_cast<uint32_t>(
        __builtin_amdgcn_update_dpp(-1, static_cast<int>(v), C, M, 0xf, false));
    return v < o ? v : o;
  };
  using std::integral_constant;
  x = lvl(x, integral_constant<int, 0xB1>{}, integral_constant<int, 0xf>{});
  x = lvl(x, integral_constant<int, 0x4E>{}, integral_constant<int, 0xf>{});
  x = lvl(x, integral_constant<int, 0x141>{}, integral_constant<int, 0xf>{});
  x = lvl(x, integral_constant<int, 0x140>{}, integral_constant<int, 0xf>{});
  x = lvl(x, integral_constant<int, 0x142>{}, integral_constant<int, 0xA>{});
  x = lvl(x, integral_constant<int, 0x143>{}, integral_constant<int, 0xC>{});
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(x), 63));
}

// wave_argmin for 31-bit indices (a lane without a candidate holds the
// sentinel (~0, INT64_MAX)): three 32-bit minima — the key's high word, its
// low word among the lanes holding that high word, the index among the lanes
// holding the whole key — give the same lexicographic minimum with ~40 VALU
// instead of ~70 (two 64-bit compares and four selects per level).
__device__ __forceinline__ void wave_argmin32(uint64_t& k, int64_t& i) {
  const uint32_t hi = static_cast<uint32_t>(k >> 32), lo = static_cast<uint32_t>(k);
  const uint32_t ix = k == ~0ull ? 0xffffffffu : static_cast<uint32_t>(i);
  const uint32_t m1 = wave_min_u32(hi);
  const uint32_t m2 = wave_min_u32(hi == m1 ? lo : 0xffffffffu);
  const uint32_t m3 = wave_min_u32(hi == m1 && lo == m2 ? ix : 0xffffffffu);
  k = (static_cast<uint64_t>(m1) << 32) | m2;
  i = k == ~0ull ? INT64_MAX : static_cast<int64_t>(m3);
}

constexpr int kBlock = 256;  // 4 waves of 64
constexpr int kWaves = kBlock / 64;

struct Rec {
  uint64_t key;
  int64_t idx;
};

// Block-level arg-min: wave shuffle, then the kWaves wave records via LDS.
// The block winner ends up in thread 0.
// IDX31: every index is below 2^31 (wave_argmin32).
template <bool IDX31 = false>
__device__ __forceinline__ void block_argmin(uint64_t& k, int64_t& i) {
  __shared__ uint64_t s_key[kWaves];
  __shared__ int64_t s_idx[kWaves];
  if constexpr (IDX31)
    wave_argmin32(k, i);
  else
    wave_argmin(k, i);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_key[wave] = k;
    s_idx[wave] = i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w)
      if (rec_less(s_key[w], s_idx[w], k, i)) {
        k = s_key[w];
        i = s_idx[w];
      }
  }
}

}  // namespace mpc
