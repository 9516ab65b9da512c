// mpc_kernels.h — the kernels of the one-shot entries: rollout + arg-min,
// their obstacle variants, the batched robots and the selection (gfx950).
//
//   k_rollout_argmin   one lane per CPL adjacent candidates (mpc_lanes.h);
//                      lane -> wave (DPP) -> block (LDS) lexicographic
//                      (cost, index) arg-min (mpc_argmin.h); one 16-B record
//                      per block.  k_rollout_argmin_stream: the aligned path.
//   k_rollout_argmin_obs / _stream_obs   the same with keep-out circles
//                      (kernarg_obs); blocked_slots, store_wave_blocked,
//                      add_block_blocked: the blocked-count epilogue, also of
//                      the episode kernels (mpc_chain.h, mpc_episode_obs.h).
//   k_rollout_argmin_keepout / _stream_keepout   the same with keep-out circles
//                      and polygons (kernarg_keepout, mpc_keepout.h).
//   k_stream_probe     the streaming kernel's memory side alone.
//   k_rollout_argmin_batched / k_finalize_batched   robot-segmented variant.
//   select_index, k_select_winner   lexicographic min over gathered per-rank results.
// (k_finalize, which completes the one-shot entries, is in mpc_finalize.h; the
// sampler in mpc_sampler.h.)
//
// Template modes: INTEG, ROT, STATES as in mpc_lanes.h; KDEV (problem
// constants read from device memory: the device-resident episode).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_argmin.h"
#include "mpc_device.h"
#include "mpc_keepout.h"
#include "mpc_lanes.h"
#include "mpc_winner.h"

namespace mpc {

// The waves' blocked-candidate counts of the obstacle variants, one-shot and
// episode (LDS only in the kernels that call this).
__device__ __forceinline__ uint32_t* blocked_slots() {
  __shared__ uint32_t s_blocked[kWaves];
  return s_blocked;
}

// The blocked-count epilogue, in two halves around block_argmin (whose barrier
// orders the stores before thread 0's reads): every wave stores its uniform
// count; thread 0 adds the block's sum to n_blocked (nullable), one atomic.
__device__ __forceinline__ void store_wave_blocked(uint32_t wave_blocked) {
  if ((threadIdx.x & 63) == 0) blocked_slots()[threadIdx.x >> 6] = wave_blocked;
}
__device__ __forceinline__ void add_block_blocked(unsigned long long* __restrict__ n_blocked) {
  if (threadIdx.x == 0 && n_blocked) {
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += blocked_slots()[w];
    if (total) atomicAdd(n_blocked, static_cast<unsigned long long>(total));
  }
}

// Obs::kOn: a blocked candidate takes the key of a non-finite cost (~0: never
// wins), so the block records and everything downstream of them are those of
// the kernels without obstacles; n_blocked (nullable) gets the number of
// blocked candidates — a ballot popcount per wave and candidate slot, then
// store_wave_blocked / add_block_blocked.
template <int CPL, int INTEG, int ROT, bool STATES, bool KDEV, class Obs = NoObs>
__device__ __forceinline__ void rollout_argmin_body(
    const Consts& Karg, const Consts* __restrict__ Kdev, const double* __restrict__ v,
    const double* __restrict__ b, int64_t n_cand, int n_steps, Rec* __restrict__ part,
    double* __restrict__ states, const Obs& obs = Obs{},
    unsigned long long* __restrict__ n_blocked = nullptr) {
  const Consts K = KDEV ? *Kdev : Karg;
  const int64_t n_tiles = (n_cand + kBlock * CPL - 1) / (kBlock * CPL);
  uint64_t best_k = ~0ull;
  int64_t best_i = INT64_MAX;
  [[maybe_unused]] uint32_t wave_blocked = 0;   // (wave-uniform)
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t c0 = tile * (kBlock * CPL) + threadIdx.x * CPL;
    if (c0 < n_cand) {  // CPL > 1 requires n_cand % CPL == 0: the whole group is valid
      double cst[CPL];
      [[maybe_unused]] bool blocked[CPL];
      rollout_lane<CPL, INTEG, ROT, STATES, Obs>(K, v, b, n_cand, c0, n_steps, cst, states,
                                                 n_cand, obs, blocked);
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        uint64_t kk = cost_key_nonneg(cst[j]);
        if constexpr (Obs::kOn) {
          kk = blocked[j] ? ~0ull : kk;
          wave_blocked += __builtin_popcountll(__builtin_amdgcn_ballot_w64(blocked[j]));
        }
        if (kk < best_k) {  // ascending index per lane: strict < keeps the first
          best_k = kk;
          best_i = c0 + j;
        }
      }
    }
  }
  if constexpr (Obs::kOn) store_wave_blocked(wave_blocked);
  block_argmin<CPL == kCplWide>(best_k, best_i);   // (wide path: rows < 2^28 candidates)
  if (threadIdx.x == 0) part[blockIdx.x] = Rec{best_k, best_i};
  if constexpr (Obs::kOn) add_block_blocked(n_blocked);
}

// Scalar (CPL = 1), CoordinateTree-states and register-ring paths.
template <int CPL, int INTEG, int ROT, bool STATES, bool KDEV>
__global__ __launch_bounds__(kBlock, 1) void k_rollout_argmin(
    Consts Karg, const Consts* __restrict__ Kdev, const double* __restrict__ v,
    const double* __restrict__ b, int64_t n_cand, int n_steps, Rec* __restrict__ part,
    double* __restrict__ states) {
  rollout_argmin_body<CPL, INTEG, ROT, STATES, KDEV>(Karg, Kdev, v, b, n_cand, n_steps, part,
                                                      states);
}

// The streaming kernel of the aligned path (CPL = 2, LDS-DMA ring).  With the
// irregular-candidate recompute free of the device library's large-argument
// trig (mpc_trig.h reduce_pio2_large), its registers fit kStreamWaves waves
// per SIMD (5: <= 96 VGPRs; 6 spills).
constexpr int kStreamWaves = 5;
template <int INTEG, int ROT, bool KDEV>
__global__ __launch_bounds__(kBlock, kStreamWaves) void k_rollout_argmin_stream(
    Consts Karg, const Consts* __restrict__ Kdev, const double* __restrict__ v,
    const double* __restrict__ b, int64_t n_cand, int n_steps, Rec* __restrict__ part) {
  rollout_argmin_body<kCplWide, INTEG, ROT, false, KDEV>(Karg, Kdev, v, b, n_cand, n_steps,
                                                          part, nullptr);
}

// The obstacle variants (mpc_rollout_partials_obstacles): the same bodies with
// the CircleObs<NOBS> hook.  The circle tables are the kernels' FIRST argument
// `O`, i.e. offset 0 of the kernel-argument segment, and are read through the
// segment pointer (constant address space, scalar loads; see CircleObs for why
// not through the by-value parameter).
// kObsStreamWaves: the launch bound of the streaming variant.
template <int NOBS>
__device__ __forceinline__ CircleObs<NOBS> kernarg_obs() {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto* a = (const __attribute__((address_space(4))) ObstacleArgs*)
      __builtin_amdgcn_kernarg_segment_ptr();
  return CircleObs<NOBS>{&a->loop, &a->world};
#else
  return CircleObs<NOBS>{nullptr, nullptr};   // (the host pass only parses the kernels)
#endif
}

template <int CPL, int INTEG, int ROT, bool STATES, int NOBS>
__global__ __launch_bounds__(kBlock, 1) void k_rollout_argmin_obs(
    ObstacleArgs O, Consts Karg, const double* __restrict__ v, const double* __restrict__ b,
    int64_t n_cand, int n_steps, Rec* __restrict__ part, double* __restrict__ states,
    unsigned long long* __restrict__ n_blocked) {
  rollout_argmin_body<CPL, INTEG, ROT, STATES, false>(Karg, nullptr, v, b, n_cand, n_steps, part,
                                                       states, kernarg_obs<NOBS>(), n_blocked);
}

constexpr int kObsStreamWaves = 5;
template <int INTEG, int ROT, int NOBS>
__global__ __launch_bounds__(kBlock, kObsStreamWaves) void k_rollout_argmin_stream_obs(
    ObstacleArgs O, Consts Karg, const double* __restrict__ v, const double* __restrict__ b,
    int64_t n_cand, int n_steps, Rec* __restrict__ part,
    unsigned long long* __restrict__ n_blocked) {
  rollout_argmin_body<kCplWide, INTEG, ROT, false, false>(Karg, nullptr, v, b, n_cand, n_steps,
                                                           part, nullptr, kernarg_obs<NOBS>(),
                                                           n_blocked);
}

// The keep-out variants (mpc_rollout_partials_keepout): the twins of the two
// kernels above with the KeepoutObs<NOBS> hook (mpc_keepout.h) — the same
// bodies, grids, launch bounds and blocked-count epilogue.  The circle and
// polygon tables and the polygon count are the FIRST argument `O`, read
// through the segment pointer as above.
template <int NOBS>
__device__ __forceinline__ KeepoutObs<NOBS> kernarg_keepout() {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto* a = (const __attribute__((address_space(4))) KeepoutArgs*)
      __builtin_amdgcn_kernarg_segment_ptr();
  return KeepoutObs<NOBS>{&a->loop, &a->world, &a->ploop, &a->pworld, a->n_polygons};
#else
  return KeepoutObs<NOBS>{nullptr, nullptr, nullptr, nullptr, 0};   // (host pass: parse only)
#endif
}

template <int CPL, int INTEG, int ROT, bool STATES, int NOBS>
__global__ __launch_bounds__(kBlock, 1) void k_rollout_argmin_keepout(
    KeepoutArgs O, Consts Karg, const double* __restrict__ v, const double* __restrict__ b,
    int64_t n_cand, int n_steps, Rec* __restrict__ part, double* __restrict__ states,
    unsigned long long* __restrict__ n_blocked) {
  rollout_argmin_body<CPL, INTEG, ROT, STATES, false>(Karg, nullptr, v, b, n_cand, n_steps, part,
                                                       states, kernarg_keepout<NOBS>(), n_blocked);
}

template <int INTEG, int ROT, int NOBS>
__global__ __launch_bounds__(kBlock, kObsStreamWaves) void k_rollout_argmin_stream_keepout(
    KeepoutArgs O, Consts Karg, const double* __restrict__ v, const double* __restrict__ b,
    int64_t n_cand, int n_steps, Rec* __restrict__ part,
    unsigned long long* __restrict__ n_blocked) {
  rollout_argmin_body<kCplWide, INTEG, ROT, false, false>(Karg, nullptr, v, b, n_cand, n_steps,
                                                           part, nullptr, kernarg_keepout<NOBS>(),
                                                           n_blocked);
}

// Measurement probe (mpc_stream_probe): the streaming kernel's memory side
// alone — the same grid, tiles, lanes and LDS-DMA control ring (kRing slots,
// kRing-1 steps in flight, `nt`), each landed slot read back from LDS and
// folded into one word per lane, no rollout arithmetic.  Its duration is the
// read-only stream ceiling of the rollout's own access pattern at the
// launch's size (launch ramp and tail included), the denominator the
// streaming kernels' time is compared with.
// TILED: the same over MPC_LAYOUT_TILED controls (a tile's rows at tile base +
// s * 1024 doubles, the lane's offset within its tile).
template <bool TILED>
__global__ __launch_bounds__(kBlock, kStreamWaves) void k_stream_probe(
    const double* __restrict__ v, const double* __restrict__ b, int64_t n_cand, int n_steps,
    uint64_t* __restrict__ sink) {
  constexpr int R = kRing;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t ring0 = __builtin_amdgcn_readfirstlane(lds_addr(&g_ring[wv][0][0][0]));
  constexpr uint32_t kSlot = 2 * 64 * sizeof(double2);
  auto dst = [&](int slot) { return ring0 + slot * kSlot; };
  const int64_t n_tiles = (n_cand + kBlock * 2 - 1) / (kBlock * 2);
  uint64_t acc = 0;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t c0 = tile * (kBlock * 2) + threadIdx.x * 2;
    if (c0 >= n_cand) continue;   // n_cand even (host check): the pair is valid
    const int64_t ld = TILED ? 2 * MPC_TILE : n_cand;   // row pitch
    const double* tv = TILED ? v + tile * ld * n_steps : v;
    const double* tb = TILED ? b + tile * ld * n_steps : b;
    const uint32_t voff = static_cast<uint32_t>(TILED ? c0 - tile * MPC_TILE : c0) * 8u;
#pragma unroll
    for (int u = 0; u < R - 1; ++u)
      if (u < n_steps) glds_pair(tv + u * ld, tb + u * ld, voff, dst(u), dst(u) + kSlot / 2);
    double2 v2 = make_double2(0.0, 0.0), b2 = v2;
#pragma unroll 1
    for (int s = 0; s < n_steps; s += R) {
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int st = s + u;
        if (st < n_steps) {
          if (st + R - 1 < n_steps) {
            const int sr = st + R - 1, slot = (u + R - 1) % R;
            glds_refill(tv + sr * ld, tb + sr * ld, voff, dst(slot), dst(slot) + kSlot / 2, v2,
                        b2);
            wait_vm<2 * (R - 1)>();
          } else {
            wait_vm<0>();
          }
          v2 = g_ring[wv][u][0][lane];
          b2 = g_ring[wv][u][1][lane];
          acc ^= static_cast<uint64_t>(__double_as_longlong(v2.x)) ^
                 static_cast<uint64_t>(__double_as_longlong(b2.y));
        }
      }
    }
  }
  if (acc == 0x5eedull) sink[blockIdx.x * kBlock + threadIdx.x] = acc;   // keeps the reads live
}

// --------------------------- batched robots --------------------------------
// The wide variant runs the streaming kernel's lane (LDS-DMA ring): the same
// 5 waves per SIMD (4 at the default bound: 120 VGPRs).
template <int CPL, int INTEG, int ROT>
__global__ __launch_bounds__(kBlock, CPL == kCplWide ? kStreamWaves : 1) void
k_rollout_argmin_batched(
    const mpc_problem_t* __restrict__ probs, const double* __restrict__ v,
    const double* __restrict__ b, int64_t cand, int n_steps, int64_t ld, Rec* __restrict__ part) {
  const int r = blockIdx.y;
  const Consts K = uniform_consts(consts_from_problem(probs[r]));
  uint64_t best_k = ~0ull;
  int64_t best_i = INT64_MAX;
  const int64_t tiles = (cand + kBlock * CPL - 1) / (kBlock * CPL);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t cl = tile * (kBlock * CPL) + threadIdx.x * CPL;  // local index
    if (cl < cand) {
      double cst[CPL];
      rollout_lane<CPL, INTEG, ROT, false>(K, v, b, ld, r * cand + cl, n_steps, cst, nullptr, 0);
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const uint64_t kk = cost_key_nonneg(cst[j]);
        if (kk < best_k) {
          best_k = kk;
          best_i = cl + j;
        }
      }
    }
  }
  block_argmin(best_k, best_i);
  if (threadIdx.x == 0)
    part[static_cast<int64_t>(r) * gridDim.x + blockIdx.x] = Rec{best_k, best_i};
}

template <int INTEG, int ROT>
__global__ __launch_bounds__(kBlock) void k_finalize_batched(
    const Rec* __restrict__ part, int n_part, const mpc_problem_t* __restrict__ probs,
    const double* __restrict__ incumbents, const double* __restrict__ v,
    const double* __restrict__ b, int64_t cand, int n_steps, int64_t ld,
    mpc_result_t* __restrict__ out) {
  const int r = blockIdx.x;
  uint64_t k = ~0ull;
  int64_t i = INT64_MAX;
  for (int p = threadIdx.x; p < n_part; p += kBlock) {
    const Rec q = part[static_cast<int64_t>(r) * n_part + p];
    if (rec_less(q.key, q.idx, k, i)) {
      k = q.key;
      i = q.idx;
    }
  }
  block_argmin(k, i);
  const Consts K = consts_from_problem(probs[r]);
  const double inc = incumbents ? incumbents[r] : __builtin_inf();
  __shared__ EmitLds lds;
  emit_winner<INTEG, ROT>(K, v, b, ld, n_steps, k, r * cand + i, i, inc, &out[r], &lds);
}

// --------------------------- exchange ----------------------------------------
// Lexicographic (cost, global index) min over n gathered per-rank results.
__device__ int select_index(const mpc_result_t* __restrict__ res, int n, uint64_t& bk) {
  int best = 0;
  int64_t bi = INT64_MAX;
  bk = ~0ull;
  for (int r = 0; r < n; ++r) {
    const uint64_t k = res[r].index < 0 ? ~0ull : cost_key(res[r].cost);
    const int64_t i = res[r].index < 0 ? INT64_MAX : res[r].index;
    if (r == 0 || rec_less(k, i, bk, bi)) {
      best = r;
      bk = k;
      bi = i;
    }
  }
  return best;
}

#ifndef MPC_TEMPLATES_ONLY   // (a unit that is not mpc_rollout.hip: mpc_episodes_obs_launch.h)
__global__ void k_select_winner(const mpc_result_t* __restrict__ res, int n, double incumbent,
                                mpc_result_t* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint64_t bk;
  const int best = select_index(res, n, bk);
  *out = res[best];
  out->found = (bk != ~0ull && out->cost < incumbent) ? 1 : 0;
}
#endif

}  // namespace mpc
