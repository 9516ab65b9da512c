// mpc_generated.h — the episode's own controls: sampled from the step's grids
// into HBM, or generated inside the rollout (gfx950).
//
//   episode_grids      this step's grids (:239-256, slow-down :312-316), one wave
//   k_episode_sample   every block derives the grids and samples its
//                      candidates; block 0 publishes the grids.  (t += dt
//                      (:302), the step's problem constants and seed are
//                      prepared by reset / the previous advance.)
//   generated_lane, k_rollout_generated   sampler and streaming rollout in one kernel
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpc_argmin.h"
#include "mpc_device.h"
#include "mpc_episode.h"
#include "mpc_sampler.h"

namespace mpc {

// Grids (:239-256) with the reference's expressions and the slow-down
// override (:312-316), computed by one wave: lane i evaluates grid point i,
// a ballot compacts the accepted points in order.  Writes s_v[nv], s_b[nb].
__device__ inline void episode_grids(const mpc_episode_config_t& c, const EpisodeHead& S,
                                     double* s_v, double* s_b, int& nv_out, int& nb_out) {
  const int lane = threadIdx.x & 63;
  const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const int n_v = 1 + 2 * static_cast<int>(c.ratio_v);
  int nv = 0;
  double vmin = __builtin_inf();
  for (int base = 0; base < n_v; base += 64) {
    const int i = base + lane;
    const double cand = S.v + c.delta_v * (static_cast<double>(i) - c.ratio_v);
    const bool ok = i < n_v && !(cand < 0.0) && cand < c.v_max;
    const uint64_t m = __ballot(ok);
    const int pos = nv + __popcll(m & below);
    if (ok && pos < kEpMaxGrid) s_v[pos] = cand;
    if (S.steps_for_slowing > 0) {   // (uniform) min(V) only for the slow-down
      double mn = ok ? cand : __builtin_inf();
      for (int off = 32; off > 0; off >>= 1) mn = fmin(mn, __shfl_xor(mn, off, 64));
      vmin = fmin(vmin, mn);
    }
    nv += __popcll(m);
  }
  nv = nv < kEpMaxGrid ? nv : kEpMaxGrid;
  if (S.steps_for_slowing > 0 && nv > 0) {
    const double vel = vmin > c.v_min ? vmin : c.v_min;
    for (int i = lane; i < nv; i += 64) s_v[i] = vel;
  }
  const int n_b = 1 + 2 * static_cast<int>(c.ratio_beta);
  int nb = 0;
  for (int base = 0; base < n_b; base += 64) {
    const int i = base + lane;
    const double cand = S.beta + c.delta_beta * (static_cast<double>(i) - c.ratio_beta);
    const bool ok = i < n_b && fabs(cand) <= c.beta_bound;
    const uint64_t m = __ballot(ok);
    const int pos = nb + __popcll(m & below);
    if (ok && pos < kEpMaxGrid) s_b[pos] = cand;
    nb += __popcll(m);
  }
  nv_out = nv;
  nb_out = nb < kEpMaxGrid ? nb : kEpMaxGrid;
}

#ifndef MPC_TEMPLATES_ONLY   // (a unit that is not mpc_rollout.hip: mpc_episodes_obs_launch.h)
__global__ __launch_bounds__(kBlock) void k_episode_sample(
    mpc_episode_config_t c, EpisodeState* __restrict__ S, int64_t n_cand, int n_steps,
    int64_t base, double* __restrict__ v, double* __restrict__ b, int pairs) {
  __shared__ double s_v[kEpMaxGrid], s_b[kEpMaxGrid];
  __shared__ double2 s_grid[kSampleLdsEntries];
  __shared__ int s_nv, s_nb;
  if (threadIdx.x < 64) {
    int nv, nb;
    episode_grids(c, S->h, s_v, s_b, nv, nb);
    if (threadIdx.x == 0) {
      s_nv = nv;
      s_nb = nb;
    }
  }
  __syncthreads();
  const int nv = s_nv, nb = s_nb;
  const uint64_t seed = S->h.seed;
  const uint32_t n_grid = static_cast<uint32_t>(nv) * static_cast<uint32_t>(nb);
  const bool staged = n_grid <= static_cast<uint32_t>(kSampleLdsEntries);
  if (staged)
    for (uint32_t k = threadIdx.x; k < n_grid; k += kBlock)
      s_grid[k] = make_double2(s_v[k / nb], s_b[k % nb]);
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    S->h.nv = nv;
    S->h.nb = nb;
    for (int i = 0; i < nv; ++i) S->grid_v[i] = s_v[i];
    for (int i = 0; i < nb; ++i) S->grid_b[i] = s_b[i];
  }
  if (n_grid == 0 && !c.enumerate) return;
  if (!staged) {
    // more than kSampleLdsEntries of the 64 x 64 entries (grids far wider than
    // the reference's): direct lookups in s_v / s_b, one division per element,
    // as k_sample_controls does for such a grid
    for (int64_t cc = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x; cc < n_cand;
         cc += static_cast<int64_t>(gridDim.x) * kBlock) {
      const uint64_t g = static_cast<uint64_t>(base + cc);
      for (int st = 0; st < n_steps; ++st) {
        const bool pad = c.enumerate && g >= n_grid;
        const uint32_t k = pad ? 0u : grid_entry(seed, st, g, n_grid, 1);
        v[ctl_off<false>(st, cc, n_cand)] = pad ? __builtin_nan("") : s_v[k / nb];
        b[ctl_off<false>(st, cc, n_cand)] = pad ? 0.0 : s_b[k % nb];
      }
    }
    return;
  }
  sample_items(s_grid, n_grid, n_cand, n_steps, seed, base, c.enumerate ? 2 : 1, v, b, n_cand,
               pairs);
}
#endif

// ---------------------------------------------------------------------------
// Generated controls (inputs "generated", mpc_episode_generate_step): the
// sampler of k_episode_sample and the rollout of k_rollout_argmin_stream in
// ONE kernel — every block builds the step's grid (episode_grids) in LDS and
// each lane draws its candidates' (v, beta) per step from it with the same
// splitmix64 -> multiply-shift map (grid_entry, constant prefix included),
// so the controls never touch HBM.  Per lane two candidates, the same
// operations in the same order as the streaming kernel's lane
// (rollout_lane_glds_k), so results equal the sampled path's bit for bit.
// Each block also writes its best candidate's controls to part_v / part_b
// [block][MPC_MAX_STEPS] for the selection's winner re-roll (k_finalize_gen).
template <int INTEG, int ROT, bool PL2>
__device__ __forceinline__ void generated_lane(const Consts& K, const double2* s_grid,
                                               uint32_t n_grid, uint64_t seed, uint64_t g0,
                                               int n_steps, double (&cst)[2]) {
  double x[2], y[2], ph[2], sn[2], cs[2];
  bool bad[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    step_start<ROT>(K, x[j], y[j], ph[j], sn[j], cs[j]);
    bad[j] = false;
  }
  trig::Leads lead = trig::const_leads();
#pragma unroll 1
  for (int st = 0; st < n_steps; ++st) {
    const double2 e0 = s_grid[grid_entry(seed, st, g0, n_grid, 1)];
    const double2 e1 = s_grid[grid_entry(seed, st, g0 + 1, n_grid, 1)];
    double ph0 = ROT ? 0.0 : ph[0], ph1 = ROT ? 0.0 : ph[1];
    step_core<INTEG, ROT, PL2>(x[0], y[0], ph0, sn[0], cs[0], e0.x, e0.y, K, bad[0], &lead);
    step_core<INTEG, ROT, PL2>(x[1], y[1], ph1, sn[1], cs[1], e1.x, e1.y, K, bad[1], &lead);
    if (!ROT) {
      ph[0] = ph0;
      ph[1] = ph1;
    }
  }
  if constexpr (ROT == kRotCum) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (!bad[j]) cum_pose<PL2>(K, x[j], y[j], x[j], y[j]);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (bad[j]) {
      x[j] = K.x;
      y[j] = K.y;
      ph[j] = K.phi;
      for (int sr = 0; sr < n_steps; ++sr) {
        const double2 e = s_grid[grid_entry(seed, sr, g0 + j, n_grid, 1)];
        step_safe<INTEG>(x[j], y[j], ph[j], e.x, e.y, K);
      }
    }
    cst[j] = cost(x[j], y[j], K);
  }
}

constexpr int kGenWaves = 4;   // launch bound of the generated-controls rollout (5 spills)
// PL2 (wheelbase a power of two) is a template parameter picked by the host
// from cfg, as in the chained step (one rollout variant per kernel).
template <int INTEG, int ROT, bool PL2>
__global__ __launch_bounds__(kBlock, kGenWaves) void k_rollout_generated(
    mpc_episode_config_t c, EpisodeState* __restrict__ S, int64_t n_cand, int n_steps,
    int64_t base, Rec* __restrict__ part, double* __restrict__ part_v,
    double* __restrict__ part_b) {
  extern __shared__ double2 s_gen_grid[];   // the expanded grid (dynamic: nv x nb entries)
  __shared__ double s_v[kEpMaxGrid], s_b[kEpMaxGrid];
  __shared__ int s_nv, s_nb;
  if (threadIdx.x < 64) {
    int nv, nb;
    episode_grids(c, S->h, s_v, s_b, nv, nb);
    if (threadIdx.x == 0) {
      s_nv = nv;
      s_nb = nb;
    }
  }
  __syncthreads();
  const int nv = s_nv, nb = s_nb;
  const uint32_t n_grid = static_cast<uint32_t>(nv) * static_cast<uint32_t>(nb);
  for (uint32_t k = threadIdx.x; k < n_grid; k += kBlock)
    s_gen_grid[k] = make_double2(s_v[k / nb], s_b[k % nb]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // as k_episode_sample: the step's grid
    // a state reset with another wheelbase form than cfg's: flag it (chain error 2)
    if ((S->h.K.L_pow2 != 0) != PL2) S->chain_error = 2u;
    S->h.nv = nv;
    S->h.nb = nb;
    for (int i = 0; i < nv; ++i) S->grid_v[i] = s_v[i];
    for (int i = 0; i < nb; ++i) S->grid_b[i] = s_b[i];
  }
  __syncthreads();
  const uint64_t seed = S->h.seed;
  const Consts K = S->h.K;
  const int64_t n_tiles = (n_cand + kBlock * 2 - 1) / (kBlock * 2);
  uint64_t best_k = ~0ull;
  int64_t best_i = INT64_MAX;
  if (n_grid > 0) {
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const int64_t c0 = tile * (kBlock * 2) + threadIdx.x * 2;
      if (c0 < n_cand) {   // n_cand even (host check): the pair is valid
        double cst[2];
        const uint64_t g0 = static_cast<uint64_t>(base + c0);
        generated_lane<INTEG, ROT, PL2>(K, s_gen_grid, n_grid, seed, g0, n_steps, cst);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint64_t kk = cost_key_nonneg(cst[j]);
          if (kk < best_k) {   // ascending index per lane: strict < keeps the first
            best_k = kk;
            best_i = c0 + j;
          }
        }
      }
    }
  }
  block_argmin(best_k, best_i);
  if (threadIdx.x == 0) part[blockIdx.x] = Rec{best_k, best_i};
  // the block's best candidate's controls, one step per lane
  __shared__ int64_t s_best;
  if (threadIdx.x == 0) s_best = best_k == ~0ull ? -1 : best_i;
  __syncthreads();
  const int64_t bi = s_best;
  if (bi >= 0 && threadIdx.x < n_steps) {
    const double2 e =
        s_gen_grid[grid_entry(seed, threadIdx.x, static_cast<uint64_t>(base + bi), n_grid, 1)];
    part_v[blockIdx.x * MPC_MAX_STEPS + threadIdx.x] = e.x;
    part_b[blockIdx.x * MPC_MAX_STEPS + threadIdx.x] = e.y;
  }
}

}  // namespace mpc
