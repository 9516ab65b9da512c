// mpc_fulltree_obs.h — keep-out circles in the full tree
// (mpc_fulltree_argmin_obstacles, mpc_fulltree_argmin_batched_obstacles,
// mpc_fulltree_episodes_run_obstacles; gfx950).
//
//   k_ft_reach               one wave: the control table's largest |v * h|, then
//                            per circle the squared reach radius (ft_reach_r2)
//   k_ft_leaves_obs, k_ft_leaves_batched_obs, k_ftl_leaves_obs
//                            k_ft_leaves, k_ft_leaves_batched and k_ftl_leaves with
//                            the FtCircleObs hook of ft_leaves_body (mpc_fulltree.h)
//   launch_ft_*_obs          their launches (defined in mpc_episodes_obs.hip, the
//                            unit of the circle kernels: mpc_episodes_obs_launch.h)
//
// The world table is the kernels' FIRST argument `W` and is read through the
// segment pointer (kernarg_world, mpc_episode_obs.h: scalar loads).  The
// controls of the last layer are wave-uniform, so a leaf's circle test has
// scalar circle operands.  The plain kernels, k_ft_controls, k_ftl_prepare and
// the finalize / update kernels run unchanged around these.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_episode_obs.h"
#include "mpc_ftepisodes.h"
#include "mpc_fulltree.h"

namespace mpc {

// reach2[i], i < n_obs, from the control table of the call (after k_ft_controls
// / k_ftl_prepare on the stream).  One wave.
__global__ __launch_bounds__(64) void k_ft_reach(Obstacles W, const FtCtl* __restrict__ ctl,
                                                 int64_t s1, int n_obs,
                                                 double* __restrict__ reach2) {
  const ObsTable t = kernarg_world();
  double m = 0.0;
  for (int64_t k = threadIdx.x; k < s1; k += 64) m = fmax(m, fabs(ctl[k].vh));   // (NaN: ignored)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
  const int i = threadIdx.x;
  if (i < n_obs) reach2[i] = ft_reach_r2(t->c[i].cx, t->c[i].cy, t->c[i].r2, m);
}

template <int INTEG, bool ROT>
__global__ __launch_bounds__(kBlock, kFtWaves) void k_ft_leaves_obs(
    Obstacles W, Consts K, double atan_t, const FtCtl* __restrict__ ctl,
    const uint32_t* __restrict__ no_rot, const double* __restrict__ reach2, int n_obs,
    int64_t s1, int64_t u_lo, int64_t u_hi, Rec* __restrict__ part,
    int64_t* __restrict__ n_blocked) {
  uint64_t best_k = ~0ull;
  int64_t best_i = INT64_MAX;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWaves +
                       __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWaves;
  const FtCrit F = ft_crit(K, atan_t);
  FtCircleObs obs{kernarg_world(), reach2, n_obs};
  if (ROT && *no_rot == 0u)
    ft_leaves_body<INTEG, true>(K, F, ctl, s1, u_lo, u_hi, best_k, best_i, wave, n_waves, &obs);
  else
    ft_leaves_body<INTEG, false>(K, F, ctl, s1, u_lo, u_hi, best_k, best_i, wave, n_waves, &obs);
  ft_store_blocked(obs.blocked);
  block_argmin(best_k, best_i);
  if (threadIdx.x == 0) part[blockIdx.x] = Rec{best_k, best_i};
  ft_add_blocked(n_blocked);
}

// blockIdx.y = robot; n_blocked: [robots] (nullable).
template <int INTEG, bool ROT>
__global__ __launch_bounds__(kBlock, kFtWaves) void k_ft_leaves_batched_obs(
    Obstacles W, const FtRobot* __restrict__ robots, const FtCtl* __restrict__ ctl,
    const uint32_t* __restrict__ no_rot, const double* __restrict__ reach2, int n_obs,
    int64_t s1, Rec* __restrict__ part, int64_t* __restrict__ n_blocked) {
  const int r = blockIdx.y;
  const Consts K = robots[r].K;
  const double atan_t = robots[r].atan_t;
  const int64_t n_items = ft_units(s1);
  uint64_t best_k = ~0ull;
  int64_t best_i = INT64_MAX;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWaves +
                       __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWaves;
  const FtCrit F = ft_crit(K, atan_t);
  FtCircleObs obs{kernarg_world(), reach2, n_obs};
  if (ROT && *no_rot == 0u)
    ft_leaves_body<INTEG, true>(K, F, ctl, s1, 0, n_items, best_k, best_i, wave, n_waves, &obs);
  else
    ft_leaves_body<INTEG, false>(K, F, ctl, s1, 0, n_items, best_k, best_i, wave, n_waves, &obs);
  ft_store_blocked(obs.blocked);
  block_argmin(best_k, best_i);
  if (threadIdx.x == 0) part[static_cast<int64_t>(r) * gridDim.x + blockIdx.x] =
      Rec{best_k, best_i};
  ft_add_blocked(n_blocked ? n_blocked + r : nullptr);
}

// n_blocked: [robots of the batch] (nullable); a live robot's blocks add to its own.
template <int INTEG, bool ROT>
__global__ __launch_bounds__(kBlock, kFtWaves) void k_ftl_leaves_obs(
    Obstacles W, const FtLockstep* __restrict__ ls, const FtCtl* __restrict__ ctl,
    const int32_t* __restrict__ live, const FtRobot* __restrict__ robots,
    const double* __restrict__ reach2, int n_obs, int64_t s1, Rec* __restrict__ part,
    int64_t* __restrict__ n_blocked) {
  const int n_live = ls->n_live, bpr = ls->bpr;
  const int j = static_cast<int>(blockIdx.x) / (bpr > 0 ? bpr : 1);
  if (n_live == 0 || j >= n_live) return;   // (uniform)
  const int share = static_cast<int>(blockIdx.x) - j * bpr;
  const int r = live[j];
  const Consts K = uniform_consts(robots[r].K);
  const FtCrit F = ft_crit(K, robots[r].atan_t);
  uint64_t best_k = ~0ull;
  int64_t best_i = INT64_MAX;
  const int64_t wave = static_cast<int64_t>(share) * kWaves +
                       __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_waves = static_cast<int64_t>(bpr) * kWaves;
  FtCircleObs obs{kernarg_world(), reach2, n_obs};
  if (ROT && ls->no_rot == 0)
    ft_leaves_body<INTEG, true>(K, F, ctl, s1, 0, ft_units(s1), best_k, best_i, wave, n_waves,
                                &obs);
  else
    ft_leaves_body<INTEG, false>(K, F, ctl, s1, 0, ft_units(s1), best_k, best_i, wave, n_waves,
                                 &obs);
  ft_store_blocked(obs.blocked);
  block_argmin(best_k, best_i);
  if (threadIdx.x == 0) part[blockIdx.x] = Rec{best_k, best_i};
  ft_add_blocked(n_blocked ? n_blocked + r : nullptr);
}

}  // namespace mpc
