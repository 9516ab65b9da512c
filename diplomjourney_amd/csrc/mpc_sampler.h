// mpc_sampler.h — synthetic control sequences (gfx950).
//
//   splitmix64, grid_entry   (seed, step, candidate) -> an entry of the |V| x |B| grid
//   sample_items             one thread per candidate pair, the grid staged in LDS
//   k_sample_controls        mpc_sample_controls / mpc_sample_controls_tiled
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpc_argmin.h"
#include "mpc_lanes.h"

namespace mpc {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// --------------------------- sampler -----------------------------------------
// Grid entry of one (step, candidate): candidate g < n_grid of the constant
// prefix is the reference's enumeration k = g; otherwise the top 32 bits of
// splitmix64(seed ^ s<<40 ^ g) are mapped onto [0, n_grid) by multiply-shift
// (Lemire's fastrange: no integer division on the VALU).
__device__ __forceinline__ uint32_t grid_entry(uint64_t seed, int s, uint64_t g, uint32_t n_grid,
                                               int cprefix) {
  if (cprefix && g < n_grid) return static_cast<uint32_t>(g);
  const uint64_t h = splitmix64(seed ^ (static_cast<uint64_t>(s) << 40) ^ g);
  return static_cast<uint32_t>(((h >> 32) * static_cast<uint64_t>(n_grid)) >> 32);
}

constexpr int kSampleLdsEntries = 2048;  // expanded (v, beta) grid staged in LDS

// One thread per candidate pair (16-B stores), looping over the steps.  The
// grid |V| x |B| (<= 451 entries for the reference's acceleration limits) is
// expanded once per block into LDS, so the per-element lookup is one
// ds_read_b128 instead of a division by |B| and two loads.
// cprefix 2 (the episode's enumeration mode): candidates past the grid are
// padding — NaN controls, a NaN cost, never chosen.
// tiled: v / b are the MPC_LAYOUT_TILED buffer's base and base + 512, ld its
// n_steps (ctl_off).
__device__ void sample_items(const double2* s_grid, uint32_t n_grid, int64_t n_cand, int n_steps,
                             uint64_t seed, int64_t base, int cprefix, double* __restrict__ v,
                             double* __restrict__ b, int64_t ld, int pairs, int tiled = 0) {
  const int cpt = pairs ? 2 : 1;
  const int64_t n_items = n_cand / cpt;
  for (int64_t it = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x; it < n_items;
       it += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t c = it * cpt;
    const uint64_t g = static_cast<uint64_t>(base + c);
    const double2 pad = make_double2(__builtin_nan(""), 0.0);
    for (int st = 0; st < n_steps; ++st) {
      const double2 e0 =
          (cprefix == 2 && g >= n_grid) ? pad : s_grid[grid_entry(seed, st, g, n_grid, cprefix)];
      if (pairs) {
        const double2 e1 = (cprefix == 2 && g + 1 >= n_grid)
                               ? pad
                               : s_grid[grid_entry(seed, st, g + 1, n_grid, cprefix)];
        const int64_t o = tiled ? ctl_off<true>(st, c, ld) : ctl_off<false>(st, c, ld);
        *reinterpret_cast<double2*>(v + o) = make_double2(e0.x, e1.x);
        *reinterpret_cast<double2*>(b + o) = make_double2(e0.y, e1.y);
      } else {   // one candidate per item: the same layout choice as the pairs
        const int64_t o = tiled ? ctl_off<true>(st, c, ld) : ctl_off<false>(st, c, ld);
        v[o] = e0.x;
        b[o] = e0.y;
      }
    }
  }
}

#ifndef MPC_TEMPLATES_ONLY   // (a unit that is not mpc_rollout.hip: mpc_episodes_obs_launch.h)
__global__ __launch_bounds__(kBlock) void k_sample_controls(
    const double* __restrict__ vg, int nv, const double* __restrict__ bg, int nb, int64_t n_cand,
    int n_steps, uint64_t seed, int64_t base, int cprefix, double* __restrict__ v,
    double* __restrict__ b, int64_t ld, int pairs, int tiled) {
  __shared__ double2 s_grid[kSampleLdsEntries];
  const uint32_t n_grid = static_cast<uint32_t>(nv) * static_cast<uint32_t>(nb);
  if (n_grid > kSampleLdsEntries) {
    // large grids: direct lookups (one division per element)
    const int cpt = pairs ? 2 : 1;
    for (int64_t it = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x; it < n_cand / cpt;
         it += static_cast<int64_t>(gridDim.x) * kBlock) {
      const int64_t c = it * cpt;
      for (int st = 0; st < n_steps; ++st)
        for (int j = 0; j < cpt; ++j) {
          const uint32_t k = grid_entry(seed, st, base + c + j, n_grid, cprefix);
          const int64_t o = tiled ? ctl_off<true>(st, c + j, ld) : ctl_off<false>(st, c + j, ld);
          v[o] = vg[k / nb];
          b[o] = bg[k % nb];
        }
    }
    return;
  }
  for (uint32_t k = threadIdx.x; k < n_grid; k += kBlock)
    s_grid[k] = make_double2(vg[k / nb], bg[k % nb]);
  __syncthreads();
  sample_items(s_grid, n_grid, n_cand, n_steps, seed, base, cprefix, v, b, ld, pairs, tiled);
}
#endif

}  // namespace mpc
