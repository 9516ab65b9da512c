// mpc_fulltree.h — full-tree MPC of run_math_model.py / math_model.py
// (SURVEY §8f 3): S1^3 leaves per MPC step, generated from the leaf index.
//
// predictive_control (run_math_model.py:133-228) fills leaf j = k0*S1^2 +
// k1*S1 + k2 with the controls u_k0, u_k1, u_k2 (u_k = (V[k / |B|],
// B[k % |B|]), loop order :158-160) applied in turn to the initial state, and
// scans the heading-term criterion (:82-86) with strict < against a running
// incumbent (:193-196).
//
//   k_ft_controls   per control k: v, dphi = Q((v/L) tan(beta)) (the same for
//                   all three layers: one quad window per call), the rotation
//                   factors of dphi, v*h; a launch-wide flag when some
//                   |dphi| > kRotMax (the rotation form is then not used)
//   k_ft_leaves     work units = (group of 64 consecutive (k0, k1) pairs, k2);
//                   a shard owns a contiguous unit range, each wave an equal
//                   contiguous share of it, one pair per lane: each lane derives
//                   its pair's layer-0 and layer-1 states once per group, then
//                   runs its k2 with the control WAVE-UNIFORM (scalar loads, no
//                   per-leaf vector memory traffic); lexicographic (cost, j)
//                   arg-min per lane -> wave -> block record
//   k_ft_finalize   record reduction, the winner's three layers re-derived
//                   with the same functions
#pragma once

#include "mpc_argmin.h"
#include "mpc_ftdevice.h"   // FtCtl, FtState, FtCrit, ft_crit, cost_fulltree, ft_apply
#include "mpc_lanes.h"

namespace mpc {

template <int INTEG>
__global__ __launch_bounds__(kBlock) void k_ft_controls(Consts K, const double* __restrict__ V,
                                                        const double* __restrict__ B, int nb,
                                                        int64_t s1, FtCtl* __restrict__ ctl,
                                                        uint32_t* __restrict__ no_rot) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (k >= s1) return;
  // (tests/replica_harness.cpp repeats this derivation, from `FtCtl u` to the
  // store, on the host: factored into a function, this kernel's code changed)
  FtCtl u;
  u.v = V[k / nb];
  u.beta = B[k % nb];
  u.vh = u.v * K.h;
  const double w = K.L_pow2 ? u.v * K.inv_L : u.v / K.L;
  u.dphi = heading_incr<INTEG>(w, trig::tan_fast(u.beta), K);
  if (fabs(u.dphi) <= trig::kRotMax) {
    trig::rotation_sc(u.dphi, u.sd, u.cd);
  } else {
    u.sd = u.cd = 0.0;
    atomicOr(no_rot, 1u);
  }
  ctl[k] = u;
}

constexpr int kFtWaves = 7;    // launch bound (waves per SIMD): <= 72 VGPRs, no scratch

// Work units: u = g * S1 + k2 — group g of 64 consecutive (k0, k1) pairs (one
// per lane), control k2 of the last layer.  A launch (or shard, or robot) owns
// the contiguous range [u_lo, u_hi); wave `wave` of `n_waves` takes an equal
// contiguous share of it (+-1 unit).  Round 4 dealt whole (group, 256-k2
// chunk) items round-robin: at S1 = 451 that was one item per wave with the
// 256- and 195-k2 chunks landing on alternate SIMDs and 6 or 7 waves per
// SIMD — the launch waited on its most loaded SIMDs.
__host__ __device__ __forceinline__ int64_t ft_units(int64_t s1) {
  return ((s1 * s1 + 63) / 64) * s1;
}

// The leaf (k0, k1, k2) of lane-pair mm and control k2 from the layer-1 state.
template <int INTEG, bool ROT>
__device__ __forceinline__ double ft_leaf(const FtState& l1, const FtCtl& u, const Consts& K,
                                          const FtCrit& F) {
  const FtState lf = ft_apply<INTEG, ROT>(l1, u, K);
  return cost_fulltree(lf.x, lf.y, lf.ph, F);
}

// Keep-out circles in the leaf loop (mpc_fulltree_argmin_obstacles; the style
// of NoObs / CircleObs, mpc_device.h).  FtNoObs: the kernels without circles
// (no obstacle statement is instantiated: their code is unchanged).
// FtCircleObs: a leaf is blocked if any of its three layer states lies strictly
// inside a circle (ft_inside, mpc_ftdevice.h).
//   t        the world table, kernel argument 0 (scalar loads)
//   reach2   per circle, the squared radius inflated by one last-layer step
//            (ft_reach_r2, written by k_ft_reach): a layer-1 state at that
//            squared distance or beyond has no leaf inside the circle
//   n        circles in use
//   blocked  the wave's count of blocked leaves (wave-uniform)
struct FtNoObs {
  static constexpr bool kOn = false;
};
struct FtCircleObs {
  static constexpr bool kOn = true;
  ObsTable t;
  const double* __restrict__ reach2;
  int n;
  int64_t blocked = 0;

  // (x, y) strictly inside any of the n circles
  __device__ __forceinline__ bool inside_any(double x, double y) const {
    bool in = false;
    for (int i = 0; i < n; ++i) in |= ft_inside(x, y, t->c[i].cx, t->c[i].cy, t->c[i].r2);
    return in;
  }
};

// The waves' blocked-leaf counts (LDS only in the kernels that call this), in
// two halves around block_argmin, whose barrier orders the stores before
// thread 0's reads: one 64-bit atomic per block with a non-zero sum.
__device__ __forceinline__ int64_t* ft_blocked_slots() {
  __shared__ int64_t s_blocked[kWaves];
  return s_blocked;
}
__device__ __forceinline__ void ft_store_blocked(int64_t wave_blocked) {
  if ((threadIdx.x & 63) == 0) ft_blocked_slots()[threadIdx.x >> 6] = wave_blocked;
}
__device__ __forceinline__ void ft_add_blocked(int64_t* __restrict__ n_blocked) {
  if (threadIdx.x == 0 && n_blocked) {
    int64_t total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += ft_blocked_slots()[w];
    if (total)
      atomicAdd(reinterpret_cast<unsigned long long*>(n_blocked),
                static_cast<unsigned long long>(total));
  }
}

// wave / n_waves: this wave's rank among the waves that share [u_lo, u_hi)
// (the launch's waves; a block's own in the device-resident episodes).
// Each lane keeps the first strict minimum of its leaves — which ascend in
// leaf index (units ascend: (k0, k1) with g, k2 within a group) — in three
// steps, so that the per-leaf bookkeeping is 1.5 VALU instead of 3:
//   * per 4 consecutive k2 (a quad): the quad minimum (3 fmin); if it is
//     strictly below the lane's best, the quad's first k2 (one compare, one
//     32-bit select) — the first quad reaching a value keeps it, as the scan
//     would;
//   * per piece (the wave's run of k2 within one group): the group of the best
//     quad, if the piece improved it;
//   * once per wave: the winning quad re-evaluated (the same operations, so the
//     same bits) to find its first leaf at the minimum.
// Costs are compared as doubles: the criterion is >= 0, where the double order
// is the cost keys' (+-0 equal, +inf and NaN never below a best; fmin ignores
// a NaN), so the key is formed once per lane.
// Obs::kOn (FtCircleObs), per piece:
//   * layers 0 and 1 are tested once per lane, where l0 and l1 are formed; a
//     lane whose pair is blocked counts its k2_hi - k2_lo leaves and gets a NaN
//     l1.x — NaN leaves, which never win and are inside nothing, so the k2 loop
//     needs no mask for it; a piece whose real lanes are all blocked is skipped;
//   * reach culling: each lane tests its l1 against every circle inflated by
//     one last-layer step (reach2); a ballot per circle gives the wave-uniform
//     list of the circles that some lane can reach.  An empty list runs the
//     plain k2 loops below; otherwise the hooked loops test the listed circles
//     only, a blocked leaf's cost becoming +inf before the quad minimum;
//   * the winning quad's re-evaluation applies the same mask (all circles).
template <int INTEG, bool ROT, class Obs = FtNoObs>
__device__ __forceinline__ void ft_leaves_body(const Consts& K, const FtCrit& F,
                                               const FtCtl* __restrict__ ctl, int64_t s1,
                                               int64_t u_lo, int64_t u_hi,
                                               uint64_t& best_k, int64_t& best_i, int64_t wave,
                                               int64_t n_waves, Obs* obs = nullptr) {
  const int lane = threadIdx.x & 63;
  const int64_t n_pairs = s1 * s1;
  const int64_t total = u_hi - u_lo, share = total / n_waves, rem = total % n_waves;
  int64_t u = u_lo + wave * share + (wave < rem ? wave : rem);
  const int64_t u_end = u + share + (wave < rem ? 1 : 0);
  const FtState s0{K.x, K.y, K.phi, K.s0, K.c0};
  double best_c = key_cost(best_k);   // (+inf: none yet)
  int64_t best_mm = -1;               // the pair of the lane's best quad (-1: best_i stands)
  int32_t best_q = 0;                 // ... and its first k2
  while (u < u_end) {   // wave-uniform
    const int64_t g = u / s1;
    const int64_t k2_lo = u - g * s1;
    const int64_t k2_hi = (s1 - k2_lo < u_end - u) ? s1 : k2_lo + (u_end - u);
    u += k2_hi - k2_lo;
    const int64_t m = g * 64 + lane;           // this lane's (k0, k1) pair
    const int64_t mm = m < n_pairs ? m : n_pairs - 1;
    const int64_t k0 = mm / s1, k1 = mm - k0 * s1;
    const FtState l0 = ft_apply<INTEG, ROT>(s0, ctl[k0], K);
    FtState l1 = ft_apply<INTEG, ROT>(l0, ctl[k1], K);
    int32_t q = -1;   // the piece's best quad (first k2; -1: none)
    int64_t k2 = k2_lo;
    if constexpr (Obs::kOn) {
      const bool real = m < n_pairs;   // (a clamped lane counts nothing)
      bool pair_blocked = false;
      uint32_t list = 0;               // the circles some lane's l1 can reach (wave-uniform)
      for (int i = 0; i < obs->n; ++i) {
        const double cx = obs->t->c[i].cx, cy = obs->t->c[i].cy, r2 = obs->t->c[i].r2;
        const double dx = l1.x - cx, dy = l1.y - cy;
        const double d2 = fma(dy, dy, dx * dx);   // (ft_inside's own operations)
        pair_blocked |= ft_inside(l0.x, l0.y, cx, cy, r2) | (d2 < r2);
        // (!(>=): a NaN l1 stays on the list — its leaves are NaN either way)
        if (__ballot(!(d2 >= obs->reach2[i])) != 0) list |= 1u << i;
      }
      obs->blocked += __popcll(__ballot(real && pair_blocked)) * (k2_hi - k2_lo);
      if (__ballot(real && !pair_blocked) == 0) continue;   // (wave-uniform; u has advanced)
      if (pair_blocked) l1.x = __builtin_nan("");
      if (list != 0) {   // the plain loops' twins, with the listed circles
        for (; k2 < k2_hi;) {
          const int nq = k2 + 4 <= k2_hi ? 4 : 1;   // (a quad, or a quad of one)
          double c[4], x[4], y[4];
          bool in[4] = {false, false, false, false};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const FtState lf = ft_apply<INTEG, ROT>(l1, ctl[j < nq ? k2 + j : k2], K);
            c[j] = cost_fulltree(lf.x, lf.y, lf.ph, F);
            x[j] = lf.x;
            y[j] = lf.y;
          }
          for (uint32_t rest = list; rest != 0; rest &= rest - 1) {
            const int i = __builtin_ctz(rest);
            const double cx = obs->t->c[i].cx, cy = obs->t->c[i].cy, r2 = obs->t->c[i].r2;
#pragma unroll
            for (int j = 0; j < 4; ++j) in[j] |= ft_inside(x[j], y[j], cx, cy, r2);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < nq) obs->blocked += __popcll(__ballot(real && in[j]));
            c[j] = in[j] ? __builtin_inf() : c[j];
          }
          const double cm = fmin(fmin(c[0], c[1]), fmin(c[2], c[3]));
          if (cm < best_c) q = static_cast<int32_t>(k2);
          best_c = fmin(best_c, cm);
          k2 += nq;
        }
      }
    }
    for (; k2 + 4 <= k2_hi; k2 += 4) {   // wave-uniform controls
      const double c0 = ft_leaf<INTEG, ROT>(l1, ctl[k2], K, F);
      const double c1 = ft_leaf<INTEG, ROT>(l1, ctl[k2 + 1], K, F);
      const double c2 = ft_leaf<INTEG, ROT>(l1, ctl[k2 + 2], K, F);
      const double c3 = ft_leaf<INTEG, ROT>(l1, ctl[k2 + 3], K, F);
      const double cm = fmin(fmin(c0, c1), fmin(c2, c3));
      if (cm < best_c) q = static_cast<int32_t>(k2);
      best_c = fmin(best_c, cm);
    }
    for (; k2 < k2_hi; ++k2) {   // the piece's last < 4 leaves: quads of one
      const double c = ft_leaf<INTEG, ROT>(l1, ctl[k2], K, F);
      if (c < best_c) q = static_cast<int32_t>(k2);
      best_c = fmin(best_c, c);
    }
    if (q >= 0) {
      best_mm = mm;
      best_q = q;
    }
  }
  if (__ballot(best_mm >= 0) != 0) {   // the winning quad's first leaf at best_c
    if (best_mm >= 0) {
      const int64_t k0 = best_mm / s1, k1 = best_mm - k0 * s1;
      const FtState l0 = ft_apply<INTEG, ROT>(s0, ctl[k0], K);
      const FtState l1 = ft_apply<INTEG, ROT>(l0, ctl[k1], K);
      // (a quad of one — a piece's last leaves — matches at j = 0: the scan
      // never reaches past its quad)
      int32_t hit = -1;
      for (int32_t j = 0; j < 4 && hit < 0 && best_q + j < s1; ++j) {
        if constexpr (Obs::kOn) {   // (a blocked leaf may share best_c's bits)
          const FtState lf = ft_apply<INTEG, ROT>(l1, ctl[best_q + j], K);
          if (cost_fulltree(lf.x, lf.y, lf.ph, F) == best_c && !obs->inside_any(lf.x, lf.y))
            hit = best_q + j;
        } else {
          if (ft_leaf<INTEG, ROT>(l1, ctl[best_q + j], K, F) == best_c) hit = best_q + j;
        }
      }
      best_i = best_mm * s1 + (hit >= 0 ? hit : best_q);   // (hit >= 0: same bits)
    }
  }
  best_k = cost_key_nonneg(best_c);   // (+inf: ~0, no finite leaf)
}

template <int INTEG, bool ROT>
__global__ __launch_bounds__(kBlock, kFtWaves) void k_ft_leaves(Consts K, double atan_t,
                                                      const FtCtl* __restrict__ ctl,
                                                      const uint32_t* __restrict__ no_rot,
                                                      int64_t s1, int64_t u_lo,
                                                      int64_t u_hi, Rec* __restrict__ part) {
  uint64_t best_k = ~0ull;
  int64_t best_i = INT64_MAX;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWaves +
                       __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kWaves;
  const FtCrit F = ft_crit(K, atan_t);
  if (ROT && *no_rot == 0u)
    ft_leaves_body<INTEG, true>(K, F, ctl, s1, u_lo, u_hi, best_k, best_i, wave, n_waves);
  else
    ft_leaves_body<INTEG, false>(K, F, ctl, s1, u_lo, u_hi, best_k, best_i, wave, n_waves);
  block_argmin(best_k, best_i);
  if (threadIdx.x == 0) part[blockIdx.x] = Rec{best_k, best_i};
}

template <int INTEG, bool ROT>
__global__ __launch_bounds__(kFinBlock) void k_ft_finalize(
    const Rec* __restrict__ part, int n_part, Consts K, const FtCtl* __restrict__ ctl,
    const uint32_t* __restrict__ no_rot, int64_t s1, double incumbent,
    mpc_fulltree_result_t* __restrict__ out) {
  __shared__ uint64_t s_key[kFinBlock / 64];
  __shared__ int64_t s_idx[kFinBlock / 64];
  uint64_t k = ~0ull;
  int64_t i = INT64_MAX;
  for (int p = threadIdx.x; p < n_part; p += kFinBlock)
    if (rec_less(part[p].key, part[p].idx, k, i)) {
      k = part[p].key;
      i = part[p].idx;
    }
  wave_argmin(k, i);
  if ((threadIdx.x & 63) == 0) {
    s_key[threadIdx.x >> 6] = k;
    s_idx[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < kFinBlock / 64; ++w)
    if (rec_less(s_key[w], s_idx[w], k, i)) {
      k = s_key[w];
      i = s_idx[w];
    }
  out->s1 = static_cast<int32_t>(s1);
  if (k == ~0ull) {
    out->cost = __builtin_inf();
    out->leaf = -1;
    out->found = 0;
    return;
  }
  const double c = key_cost(k);
  out->cost = c;
  out->leaf = i;
  out->found = c < incumbent ? 1 : 0;
  const int64_t kk[3] = {i / (s1 * s1), (i / s1) % s1, i % s1};
  const bool rot = ROT && *no_rot == 0u;
  FtState st{K.x, K.y, K.phi, K.s0, K.c0};
  for (int l = 0; l < 3; ++l) {
    const FtCtl u = ctl[kk[l]];
    st = rot ? ft_apply<INTEG, true>(st, u, K) : ft_apply<INTEG, false>(st, u, K);
    out->k[l] = kk[l];
    out->v[l] = u.v;
    out->beta[l] = u.beta;
    out->traj[l][0] = st.x;
    out->traj[l][1] = st.y;
    out->traj[l][2] = st.ph;
  }
}

// ---------------------------------------------------------------------------
// Robot-batched full tree (the run_math_model.py:231-280 episodes run side by
// side, one robot per episode, in lockstep: every robot's MPC step k uses the
// same quad window, so the per-control table is shared).  blockIdx.y = robot.

struct FtRobot {
  Consts K;
  double atan_t;
};

#ifndef MPC_TEMPLATES_ONLY   // (a unit that is not mpc_rollout.hip: mpc_episodes_obs_launch.h)
__global__ void k_ft_robots(const mpc_fulltree_problem_t* __restrict__ probs, int n,
                            double L, double t_a, double t_b, FtRobot* __restrict__ robots) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  mpc_problem_t q;
  q.x = probs[r].x;
  q.y = probs[r].y;
  q.phi = probs[r].phi;
  q.x_t = probs[r].x_t;
  q.y_t = probs[r].y_t;
  q.x_0 = probs[r].x_0;
  q.y_0 = probs[r].y_0;
  q.L = L;
  q.t_a = t_a;
  q.t_b = t_b;
  robots[r].K = consts_from_problem(q);
  robots[r].atan_t = probs[r].atan_target;
}
#endif

template <int INTEG, bool ROT>
__global__ __launch_bounds__(kBlock, kFtWaves) void k_ft_leaves_batched(
    const FtRobot* __restrict__ robots, const FtCtl* __restrict__ ctl,
    const uint32_t* __restrict__ no_rot, int64_t s1, Rec* __restrict__ part) {
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
  if (ROT && *no_rot == 0u)
    ft_leaves_body<INTEG, true>(K, F, ctl, s1, 0, n_items, best_k, best_i, wave, n_waves);
  else
    ft_leaves_body<INTEG, false>(K, F, ctl, s1, 0, n_items, best_k, best_i, wave, n_waves);
  block_argmin(best_k, best_i);
  if (threadIdx.x == 0) part[static_cast<int64_t>(r) * gridDim.x + blockIdx.x] =
      Rec{best_k, best_i};
}

template <int INTEG, bool ROT>
__global__ __launch_bounds__(kBlock) void k_ft_finalize_batched(
    const Rec* __restrict__ part, int n_part, const FtRobot* __restrict__ robots,
    const FtCtl* __restrict__ ctl, const uint32_t* __restrict__ no_rot, int64_t s1,
    const double* __restrict__ incumbents, mpc_fulltree_result_t* __restrict__ outs) {
  const int r = blockIdx.x;
  uint64_t k = ~0ull;
  int64_t i = INT64_MAX;
  for (int p = threadIdx.x; p < n_part; p += kBlock) {
    const Rec rec = part[static_cast<int64_t>(r) * n_part + p];
    if (rec_less(rec.key, rec.idx, k, i)) {
      k = rec.key;
      i = rec.idx;
    }
  }
  block_argmin(k, i);
  if (threadIdx.x != 0) return;
  mpc_fulltree_result_t* out = outs + r;
  const Consts& K = robots[r].K;
  out->s1 = static_cast<int32_t>(s1);
  if (k == ~0ull) {
    out->cost = __builtin_inf();
    out->leaf = -1;
    out->found = 0;
    return;
  }
  const double c = key_cost(k);
  out->cost = c;
  out->leaf = i;
  out->found = c < (incumbents ? incumbents[r] : __builtin_inf()) ? 1 : 0;
  const int64_t kk[3] = {i / (s1 * s1), (i / s1) % s1, i % s1};
  const bool rot = ROT && *no_rot == 0u;
  FtState st{K.x, K.y, K.phi, K.s0, K.c0};
  for (int l = 0; l < 3; ++l) {
    const FtCtl u = ctl[kk[l]];
    st = rot ? ft_apply<INTEG, true>(st, u, K) : ft_apply<INTEG, false>(st, u, K);
    out->k[l] = kk[l];
    out->v[l] = u.v;
    out->beta[l] = u.beta;
    out->traj[l][0] = st.x;
    out->traj[l][1] = st.y;
    out->traj[l][2] = st.ph;
  }
}

}  // namespace mpc
