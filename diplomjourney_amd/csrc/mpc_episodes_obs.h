// mpc_episodes_obs.h — keep-out circles in the batched robots' device-resident
// episodes (mpc_episodes_run_obstacles; gfx950).
//
//   k_episodes_run_obs<INTEG, ROT, NOBS>   k_episodes_run (mpc_episodes.h) with
//                            one circle table for all robots of the launch
//
// The semantics are mpc_rollout_partials_obstacles' (include/mpc_rollout.h):
// world-frame circles, the strictly-inside test on the step-end states 1..N of
// every candidate, a blocked candidate never wins, an all-blocked step is the
// step without a finite cost (index -1, found 0, a stale step).
// The world-frame modes (qk21, rect, +rot) test the kernel-argument table
// (CircleObs).  rect+cum accumulates sums that know no pose: its table is
// formed in the frame of the sums (FrameObs, mpc_episode_obs.h) ONCE PER MPC
// STEP of each robot, from that step's constants — the robot moves between
// the steps of one launch.
// (Apart from the header mpc_episodes.h, which tests/replica_harness.cpp
// parses on the host: FrameObs pulls in the chained kernels.)
#pragma once

#include <type_traits>

#include "mpc_episode_obs.h"
#include "mpc_episodes.h"

namespace mpc {

// const_pair_cost_l (mpc_episodes.h) with the obstacle hook of the rollout
// lanes (mpc_device.h: NoObs, the default, instantiates no obstacle statement
// and is that function; CircleObs / FrameObs test circles).  Two `blocked`
// flags sit next to `bad`; ONE loop<2> call after each step of the pair reads
// the table once for both candidates (the unrolled horizon and the generic
// one alike); a flagged candidate's recompute resets its flag and tests every
// step_safe state against the world table.  blocked_out[2] (Obs::kOn only).
// (A copy: the existing kernel and what it calls keep their text, so that its
// code stays what was measured — tools/kernel_digest.py, DESIGN.md §5.  A
// change to either belongs in both.)
template <int INTEG, int ROT, bool PL2, int NS = 0, class Obs = NoObs>
__device__ __forceinline__ void const_pair_cost_obs_l(const Consts& K, const double (&v)[2],
                                                      const double (&b)[2], int n_steps,
                                                      double (&cst)[2], const Obs& obs = Obs{},
                                                      bool* blocked_out = nullptr) {
  if constexpr (NS > 0) n_steps = NS;
  double x[2], y[2], ph[2], s[2], c[2];
  bool bad[2];
  [[maybe_unused]] bool blocked[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    step_start<ROT>(K, x[j], y[j], ph[j], s[j], c[j]);
    bad[j] = false;
    if constexpr (Obs::kOn) blocked[j] = false;
  }
  auto one_step = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      step_core<INTEG, ROT, PL2>(x[j], y[j], ph[j], s[j], c[j], v[j], b[j], K, bad[j]);
    if constexpr (Obs::kOn) obs.template loop<2>(x, y, blocked);
  };
  if constexpr (NS > 0) {
#pragma unroll
    for (int st = 0; st < NS; ++st) one_step();
  } else {
    for (int st = 0; st < n_steps; ++st) one_step();
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if constexpr (ROT == kRotCum) {
      if (!bad[j]) cum_pose<PL2>(K, x[j], y[j], x[j], y[j]);
    }
    if (bad[j]) {
      x[j] = K.x;
      y[j] = K.y;
      ph[j] = K.phi;
      if constexpr (Obs::kOn) blocked[j] = false;   // the recompute's states replace the loop's
      for (int st = 0; st < n_steps; ++st) {
        step_safe<INTEG>(x[j], y[j], ph[j], v[j], b[j], K);
        if constexpr (Obs::kOn) obs.world(x[j], y[j], blocked[j]);
      }
    }
    cst[j] = cost(x[j], y[j], K);
    if constexpr (Obs::kOn) blocked_out[j] = blocked[j];
  }
}

template <int INTEG, int ROT, int NS = 0, class Obs = NoObs>
__device__ __forceinline__ void const_pair_cost_obs(const Consts& K, const double (&v)[2],
                                                    const double (&b)[2], int n_steps,
                                                    double (&cst)[2], const Obs& obs = Obs{},
                                                    bool* blocked_out = nullptr) {
  if (K.L_pow2)
    const_pair_cost_obs_l<INTEG, ROT, true, NS, Obs>(K, v, b, n_steps, cst, obs, blocked_out);
  else
    const_pair_cost_obs_l<INTEG, ROT, false, NS, Obs>(K, v, b, n_steps, cst, obs, blocked_out);
}

// The launch's sum of the lanes' counts, valid in thread 0 (every thread of
// the block calls it).
__device__ __forceinline__ int64_t block_sum_i64(int64_t n) {
  __shared__ int64_t s_part[kWaves];
  uint64_t sum = static_cast<uint64_t>(n);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {   // (two 32-bit halves: no carry between lanes' words)
    const uint32_t lo = __shfl_xor(static_cast<int>(static_cast<uint32_t>(sum)), off, 64);
    const uint32_t hi = __shfl_xor(static_cast<int>(static_cast<uint32_t>(sum >> 32)), off, 64);
    sum += (static_cast<uint64_t>(hi) << 32) | lo;
  }
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = static_cast<int64_t>(sum);
  __syncthreads();
  int64_t all = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kWaves; ++w) all += s_part[w];
  return all;
}

// k_episodes_run with circles.  W: the world table, kernel argument 0 (read
// through kernarg_world(): scalar loads).  n_blocked (optional): [n] per robot
// the candidates blocked in the steps this launch ran for it (0 if none ran),
// written beside progress[r] by thread 0 — a lane-private add per pair, one
// block reduction at the end of the launch, no atomic.
// (The loop is a copy of k_episodes_run's, mpc_episodes.h — the winner's
// re-derivation, the update and the log are its statements unchanged; routing
// both kernels through one templated body is not done, since a function layer
// alone has moved the existing kernels' code before: DESIGN.md §5.  A change
// to either loop belongs in both.)
template <int INTEG, int ROT, int NOBS>
__global__ __launch_bounds__(kBlock, 2) void k_episodes_run_obs(
    Obstacles W, const mpc_episode_config_t* __restrict__ cfgs, RobotState* __restrict__ robots,
    int n_steps, int max_calls, mpc_episode_log_t* __restrict__ log, int cap,
    mpc_episodes_progress_t* __restrict__ progress, int64_t* __restrict__ n_blocked) {
  using Obs = std::conditional_t<ROT == kRotCum, FrameObs<NOBS>, CircleObs<NOBS>>;
  const int r = blockIdx.x;
  const mpc_episode_config_t& c = cfgs[r];
  RobotState* __restrict__ R = &robots[r];
  __shared__ uint64_t s_head[kStoredWords];   // head + stale trajectory
  __shared__ double s_v[kEpMaxGrid], s_b[kEpMaxGrid];
  __shared__ int s_nv, s_nb, s_stop, s_calls;
  __shared__ uint64_t s_bk;
  __shared__ int64_t s_bi;
  __shared__ mpc_episode_log_t s_log;
  __shared__ mpc_result_t s_out;
  __shared__ EmitLds lds;
  for (int q = threadIdx.x; q < kStoredWords; q += kBlock)
    s_head[q] = reinterpret_cast<const uint64_t*>(R)[q];
  if (threadIdx.x == 0) {
    s_stop = R->stop;
    s_calls = R->calls;
  }
  Obs obs = [] {   // (FrameObs: its world table; the frame table per step)
    if constexpr (ROT == kRotCum)
      return FrameObs<NOBS>{kernarg_world()};
    else
      return CircleObs<NOBS>{kernarg_world(), kernarg_world()};
  }();
  int64_t cands = 0;   // (thread 0)
  int64_t n_blk = 0;   // this lane's blocked candidates
  for (int call = 0; call < max_calls; ++call) {
    __syncthreads();
    if (s_stop) break;   // uniform
    const EpisodeHead* Hs = reinterpret_cast<const EpisodeHead*>(s_head);
    if (threadIdx.x < 64) {
      int nv, nb;
      episode_grids(c, *Hs, s_v, s_b, nv, nb);
      if (threadIdx.x == 0) {
        s_nv = nv;
        s_nb = nb;
      }
    }
    __syncthreads();
    const Consts K = uniform_consts(Hs->K);
    // the circles in the frame of THIS step's sums (uniform: the whole block is
    // here; the table's last readers passed the barriers above)
    if constexpr (ROT == kRotCum) obs.form(K, K.L_pow2 != 0);
    const double incumbent = Hs->incumbent;
    const int nv = s_nv, nb = s_nb, n_grid = nv * nb;
    uint64_t best_k = ~0ull;
    int64_t best_i = INT64_MAX;
    for (int k0 = threadIdx.x; k0 < n_grid; k0 += 2 * kBlock) {
      const int k1 = k0 + kBlock;
      const bool has1 = k1 < n_grid;
      const int kq = has1 ? k1 : k0;   // (a valid stand-in: neither wins nor is counted)
      const double vv[2] = {s_v[k0 / nb], s_v[kq / nb]};
      const double bb[2] = {s_b[k0 % nb], s_b[kq % nb]};
      double cst[2];
      bool blk[2];
      if (n_steps == 3)   // uniform: the reference's horizon, unrolled
        const_pair_cost_obs<INTEG, ROT, 3, Obs>(K, vv, bb, n_steps, cst, obs, blk);
      else
        const_pair_cost_obs<INTEG, ROT, 0, Obs>(K, vv, bb, n_steps, cst, obs, blk);
      blk[1] = has1 && blk[1];
      n_blk += static_cast<int>(blk[0]) + static_cast<int>(blk[1]);
      uint64_t kk = blk[0] ? ~0ull : cost_key_nonneg(cst[0]);
      if (kk < best_k) {
        best_k = kk;
        best_i = k0;
      }
      kk = blk[1] ? ~0ull : cost_key_nonneg(cst[1]);
      if (has1 && kk < best_k) {
        best_k = kk;
        best_i = k1;
      }
    }
    block_argmin<true>(best_k, best_i);
    if (threadIdx.x == 0) {
      s_bk = best_k;
      s_bi = best_i;
      cands += n_grid;
    }
    __syncthreads();
    const uint64_t bk = s_bk;
    const int64_t bi = s_bi;
    __shared__ Winner s_win;
    Winner& win = s_win;
    if constexpr (ROT != kRotCum) {
      if (threadIdx.x < 64) {
        if (threadIdx.x == 0) {
          win.n_steps = n_steps;
          win.cost = bk == ~0ull ? __builtin_inf() : key_cost(bk);
          win.index = bk == ~0ull ? -1 : bi;
          win.found = bk != ~0ull && key_cost(bk) < incumbent ? 1 : 0;
        }
        if (bk != ~0ull) {
          const double wv = s_v[bi / nb], wb = s_b[bi % nb];
          if (threadIdx.x == 0) {
            win.v = wv;
            win.beta = wb;
          }
          if constexpr (ROT == 0) {
            if (K.L_pow2)
              wave_winner_states_l<INTEG, true>(K, wv, wb, n_steps, win);
            else
              wave_winner_states_l<INTEG, false>(K, wv, wb, n_steps, win);
          } else if (threadIdx.x == 0) {
            if (K.L_pow2)
              const_winner_states_l<INTEG, ROT, true>(K, wv, wb, n_steps, win);
            else
              const_winner_states_l<INTEG, ROT, false>(K, wv, wb, n_steps, win);
          }
        }
      }
    } else {
      if (bk != ~0ull && threadIdx.x < n_steps) {
        lds.pv[threadIdx.x] = s_v[bi / nb];
        lds.pb[threadIdx.x] = s_b[bi % nb];
      }
      emit_winner<INTEG, ROT>(K, lds.pv, lds.pb, 1, n_steps, bk, bi, bi, incumbent, &s_out,
                              &lds, &win, lds.pv, lds.pb, false);
    }
    if (threadIdx.x == 0) {   // (emit_winner, if it ran, ended with a barrier)
      EpisodeHead H;
      __builtin_memcpy(&H, s_head, sizeof(EpisodeHead));
      episode_advance<false>(c, H, *reinterpret_cast<StaleTraj*>(&s_head[kHeadWords]), win,
                             s_log);
      __builtin_memcpy(s_head, &H, sizeof(EpisodeHead));
      if (s_log.status & kEpEnded) s_stop = s_log.status;
      s_calls += 1;
    }
    __syncthreads();
    if (log && cap > 0 && threadIdx.x < kLogWords)
      reinterpret_cast<uint64_t*>(&log[static_cast<int64_t>(r) * cap + s_log.step % cap])
          [threadIdx.x] = reinterpret_cast<const uint64_t*>(&s_log)[threadIdx.x];
  }
  __syncthreads();
  for (int q = threadIdx.x; q < kStoredWords; q += kBlock)
    reinterpret_cast<uint64_t*>(R)[q] = s_head[q];
  int64_t blocked_all = 0;
  if (n_blocked) blocked_all = block_sum_i64(n_blk);   // (uniform: a kernel argument)
  if (threadIdx.x == 0) {
    R->stop = s_stop;
    R->calls = s_calls;
    R->candidates += cands;
    if (progress) {
      progress[r].calls = s_calls;
      progress[r].stop = s_stop;
      progress[r].candidates = R->candidates;
    }
    if (n_blocked) n_blocked[r] = blocked_all;
  }
}

}  // namespace mpc
