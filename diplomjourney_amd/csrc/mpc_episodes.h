// mpc_episodes.h — R robots' MPC episodes, device-resident and batched.
//
// run_math_model.py:231-280 runs one episode per robot (random start and
// target, MPC steps until on target or stuck); its MPC step, at config.py's
// resolution, is math_model_tree.py's tree expansion (SURVEY Fact 2).  Here
// every robot is one block that runs its episode's MPC steps back to back in
// ONE launch — no host round trip per step and no lockstep:
//
//   per MPC step of robot r (block r):
//     grid        episode_grids: vector_of_velocities / vector_of_beta_angles
//                 around the robot's (v, beta) (:239-256), slow-down (:312-316)
//     candidates  the reference's enumeration k = a*|B| + b of the step's
//                 |V|*|B| constant sequences (:308-350), two per lane, from
//                 the grid in LDS (never in HBM)
//     rollout     the N-step recurrence of rollout_candidate_l (the kernels'
//                 arithmetic, bitwise), the criterion (:82-87)
//     arg-min     lowest index among the minima, strict < against the robot's
//                 incumbent (:351)
//     winner      re-rolled from its controls (emit_winner: the layer states)
//     update      episode_advance without restart: finishing logic m
//                 (:392-414), the stuck detector of cfg.stop_rule, operator
//                 events (math_mpc, :564-569; off for run_math_model),
//                 arrival (:542 / run_math_model.py:261), the step limit
//     log         one mpc_episode_log_t per step in the robot's ring
//
// Per-robot configurations (mpc_episode_config_t, copied into the state by
// mpc_episodes_reset) carry the start, target and rules of each robot: the
// run_math_model episodes (stop_rule 1, no events) and math_mpc episodes
// (stop_rule 0, the operator schedule) can share one launch.
//
// Keep-out circles (mpc_episodes_run_obstacles) are the same kernel and the
// same pair rollout with an obstacle hook (Obs; NoObs without circles); the
// hooks of the modes: mpc_episodes_obs.h.  Robots as each other's circles
// (mpc_episodes_fleet_run) are the same kernel again, one launch per lockstep
// step, with a hook whose table each block forms from the other robots'
// positions: mpc_episodes_fleet.h.
#pragma once

#include <type_traits>

#include "mpc_argmin.h"
#include "mpc_device.h"
#include "mpc_episode.h"
#include "mpc_generated.h"
#include "mpc_lanes.h"
#include "mpc_timeline.h"
#include "mpc_winner.h"

namespace mpc {

// One robot's episode in HBM.
struct RobotState {
  EpisodeHead h;
  StaleTraj st;        // right after the head: staged with it
  int32_t stop;        // 0 running, else the MPC_EP_* bits of the step that ended it
                       // (MPC_EP_ARRIVED with calls == 0: on target at the start)
  int32_t calls;       // MPC steps run
  int64_t candidates;  // candidates rolled out (the steps' |V| * |B|)
};
static_assert(offsetof(RobotState, st) == sizeof(EpisodeHead), "stale trajectory follows the head");

// A hook that declares kFleet forms its table per call from a pose board
// (FleetObs, mpc_episodes_fleet.h); the others know nothing of it.
template <class Obs, class = void>
struct fleet_hook : std::false_type {};
template <class Obs>
struct fleet_hook<Obs, std::void_t<decltype(Obs::kFleet)>> : std::true_type {};
// A fleet hook that declares kMotion has one table per horizon step (the
// neighbours' circles move: FleetMotionObs): it is given the step's index
// (loop_step, world_step) and publishes the robot's displacement on exit.
template <class Obs, class = void>
struct motion_hook : std::false_type {};
template <class Obs>
struct motion_hook<Obs, std::void_t<decltype(Obs::kMotion)>> : std::true_type {};
// A motion hook that declares kPlan takes the neighbours' circles from their
// own plans (FleetPlanObs): on exit it publishes two layers of the robot's
// StaleTraj instead of the displacement.
template <class Obs, class = void>
struct plan_hook : std::false_type {};
template <class Obs>
struct plan_hook<Obs, std::void_t<decltype(Obs::kPlan)>> : std::true_type {};

// Two kernel arguments made live where this is called: their scalar loads are
// issued together and waited for once.  A fleet launch's arguments span two
// cache lines of the kernel-argument segment (the board and the counts behind
// the 512-B static table; cfgs .. count behind them), and the segment is cold
// in every scalar cache at every launch: loaded where each is first used, the
// two lines cost two misses in a row (0.7 us of a launch at 1000 robots;
// DESIGN.md section 5).
template <class T>
__device__ __forceinline__ void kernarg_touch(int a, T* b) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" ::"s"(a), "s"(b));
#else
  (void)a, (void)b;
#endif
}

constexpr int32_t kEpEnded = MPC_EP_ARRIVED | MPC_EP_BREAK | MPC_EP_LIMIT;
constexpr int32_t kEpMaxRobots = 65535;   // robots of one launch (one block each; the entries refuse more)
TL_BOUND(kRobots, kEpMaxRobots);

// The state of n robots: RobotState[n], then each robot's configuration
// (mpc_episodes_reset copies them in), so a run needs nothing but the state.
__host__ __device__ inline size_t episodes_cfg_offset(int n) {
  return (static_cast<size_t>(n) * sizeof(RobotState) + 255) & ~static_cast<size_t>(255);
}

#ifndef MPC_TEMPLATES_ONLY   // (a unit that is not mpc_rollout.hip: mpc_episodes_obs_launch.h)
__global__ void k_episodes_reset(const mpc_episode_config_t* __restrict__ cfgs, int n,
                                 RobotState* __restrict__ robots) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const mpc_episode_config_t c = cfgs[r];
  RobotState R = {};
  episode_restart(c, R.h);
  episode_prepare(c, R.h);
  // the loop's head (:542, run_math_model.py:261): an episode that starts on
  // its target runs no step
  const double ex = R.h.x_t - R.h.x, ey = R.h.y_t - R.h.y;
  R.stop = (ex * ex + ey * ey <= c.eps) ? MPC_EP_ARRIVED : 0;
  robots[r] = R;
}
#endif

// Two candidates with constant controls (v[j], b[j]) over n_steps, their
// recurrences in one loop — independent chains the scheduler interleaves —
// each exactly as the rollout kernels evaluate one candidate (rollout_candidate_l
// without the trajectory: the core recurrence, step_core, and for an irregular
// candidate the safe one, step_safe): the same bits per candidate.
// NS > 0: the horizon as a compile-time constant (the reference's N = 3):
// the loop unrolls, and the steps' sin/cos — which depend only on the heading
// chain, a sum of the candidate's constant increment — overlap.
// Obs: the obstacle hook of the rollout lanes (mpc_device.h: NoObs, the
// default, instantiates no obstacle statement; CircleObs / FrameObs test
// circles).  Two `blocked` flags sit next to `bad`; ONE loop<2> call after each
// step of the pair reads the table once for both candidates (the unrolled
// horizon and the generic one alike); a flagged candidate's recompute resets
// its flag and tests every step_safe state against the world table.
// blocked_out[2] (Obs::kOn only).
template <int INTEG, int ROT, bool PL2, int NS = 0, class Obs = NoObs>
__device__ __forceinline__ void const_pair_cost_l(const Consts& K, const double (&v)[2],
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
  auto one_step = [&]([[maybe_unused]] int st) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      step_core<INTEG, ROT, PL2>(x[j], y[j], ph[j], s[j], c[j], v[j], b[j], K, bad[j]);
    if constexpr (motion_hook<Obs>::value)
      obs.template loop_step<2>(st, x, y, blocked);   // (this step's table)
    else if constexpr (Obs::kOn)
      obs.template loop<2>(x, y, blocked);
  };
  if constexpr (NS > 0) {
#pragma unroll
    for (int st = 0; st < NS; ++st) one_step(st);
  } else {
    for (int st = 0; st < n_steps; ++st) one_step(st);
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
        if constexpr (motion_hook<Obs>::value)
          obs.world_step(st, x[j], y[j], blocked[j]);
        else if constexpr (Obs::kOn)
          obs.world(x[j], y[j], blocked[j]);
      }
    }
    cst[j] = cost(x[j], y[j], K);
    if constexpr (Obs::kOn) blocked_out[j] = blocked[j];
  }
}

template <int INTEG, int ROT, int NS = 0, class Obs = NoObs>
__device__ __forceinline__ void const_pair_cost(const Consts& K, const double (&v)[2],
                                                const double (&b)[2], int n_steps,
                                                double (&cst)[2], const Obs& obs = Obs{},
                                                bool* blocked_out = nullptr) {
  if (K.L_pow2)
    const_pair_cost_l<INTEG, ROT, true, NS, Obs>(K, v, b, n_steps, cst, obs, blocked_out);
  else
    const_pair_cost_l<INTEG, ROT, false, NS, Obs>(K, v, b, n_steps, cst, obs, blocked_out);
}

// The step's winner (constant controls v, b) re-derived by ONE lane with the
// rollout's own per-candidate recurrence — rollout_candidate_l's operations,
// the core form or, for a flagged candidate, the safe form — its layer states
// 0..2 (clamped to the horizon) into w.tr: the same bits as emit_winner's
// block-wide re-roll for the direct and rotation heading forms, without its
// barriers (kRotCum, whose sums run scaled, keeps emit_winner).
template <int INTEG, int ROT, bool PL2>
__device__ inline void const_winner_states_l(const Consts& K, double v, double b, int n_steps,
                                             Winner& w) {
  static_assert(ROT != kRotCum, "kRotCum winners are re-rolled by emit_winner");
  auto keep = [&](int st, double x, double y, double ph) {
    // (constant indices only: a dynamically indexed w.tr would live in scratch)
    if (st == 0) {
      w.tr[0][0] = x, w.tr[0][1] = y, w.tr[0][2] = ph;
    } else if (st == 1) {
      w.tr[1][0] = x, w.tr[1][1] = y, w.tr[1][2] = ph;
    } else if (st == 2) {
      w.tr[2][0] = x, w.tr[2][1] = y, w.tr[2][2] = ph;
    }
  };
  double x, y, ph, s, c;
  step_start<ROT>(K, x, y, ph, s, c);
  bool bad = false;
  for (int st = 0; st < n_steps; ++st) {
    step_core<INTEG, ROT, PL2>(x, y, ph, s, c, v, b, K, bad);
    keep(st, x, y, ph);
  }
  if (bad) {
    x = K.x;
    y = K.y;
    ph = K.phi;
    for (int st = 0; st < n_steps; ++st) {
      step_safe<INTEG>(x, y, ph, v, b, K);
      keep(st, x, y, ph);
    }
  }
  for (int k = n_steps; k < 3; ++k)   // a horizon below 3: the last layer repeated
    for (int q = 0; q < 3; ++q) {
      const double last = n_steps == 1 ? w.tr[0][q] : w.tr[1][q];
      if (k == 1) w.tr[1][q] = last;
      if (k == 2) w.tr[2][q] = last;
    }
}

// The same states for the direct heading form (ROT = 0), lane-parallel over
// the steps, by wave 0 (all 64 lanes, n_steps <= 64): the control is constant,
// so lane s forms its step's heading phi_s = phi + dphi (+ dphi ...) with
// exactly the serial chain's additions, its sin / cos and (QK21) position
// increments; lane 0 then only sums them in the serial order (QK21: x + inc;
// RECT: the fused fma(v h, cos, x)) — the serial recurrence's bits, its
// dependent chain cut from n_steps x (sin/cos + quadratures) to one.  A
// flagged candidate (|beta| > kTanMax, |phi_s| > kFastMax) takes lane 0's
// serial path (const_winner_states_l: the core form, then the safe one).
template <int INTEG, bool PL2>
__device__ inline void wave_winner_states_l(const Consts& K, double v, double b, int n_steps,
                                            Winner& w) {
  const int lane = threadIdx.x & 63;
  double ph = K.phi, sn = 0.0, cs = 0.0, ix = 0.0, iy = 0.0;
  bool bad = !(fabs(b) <= trig::kTanMax);
  const double t = trig::tan_small(b);
  double dphi, vh = 0.0;
  if constexpr (PL2 && INTEG == MPC_INTEG_RECT) {
    vh = v * K.h;
    dphi = (vh * K.inv_L) * t;                                 // step_core's form
  } else {
    const double wv = PL2 ? v * K.inv_L : v / K.L;
    dphi = heading_incr<INTEG>(wv, t, K);
  }
  if (lane < n_steps) {
    for (int j = 0; j <= lane; ++j) ph = ph + dphi;
    bad |= !(fabs(ph) <= trig::kFastMax);
    trig::sincos_core(ph, &sn, &cs);
    if constexpr (INTEG != MPC_INTEG_RECT) {
      ix = quad_const<INTEG>(v * cs, K);                      // position_step's increment
      iy = quad_const<INTEG>(v * sn, K);
    }
  }
  const bool any_bad = __ballot(lane < n_steps && bad) != 0;
  if (lane != 0) return;
  if (any_bad) {
    const_winner_states_l<INTEG, 0, PL2>(K, v, b, n_steps, w);
    return;
  }
  auto rl = [](double val, int src) {
    const uint64_t u = static_cast<uint64_t>(__double_as_longlong(val));
    const uint32_t lo = __builtin_amdgcn_readlane(static_cast<int>(u), src);
    const uint32_t hi = __builtin_amdgcn_readlane(static_cast<int>(u >> 32), src);
    return __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(hi) << 32) | lo));
  };
  double x = K.x, y = K.y;
  for (int st = 0; st < n_steps; ++st) {
    if constexpr (INTEG == MPC_INTEG_RECT) {
      const double vhs = PL2 ? vh : v * K.h;                  // = position_step<RECT>
      x = fma(vhs, rl(cs, st), x);
      y = fma(vhs, rl(sn, st), y);
    } else {
      x = x + rl(ix, st);
      y = y + rl(iy, st);
    }
    const double p = rl(ph, st);
    if (st == 0) {
      w.tr[0][0] = x, w.tr[0][1] = y, w.tr[0][2] = p;
    } else if (st == 1) {
      w.tr[1][0] = x, w.tr[1][1] = y, w.tr[1][2] = p;
    } else if (st == 2) {
      w.tr[2][0] = x, w.tr[2][1] = y, w.tr[2][2] = p;
    }
  }
  for (int k = n_steps; k < 3; ++k)
    for (int q = 0; q < 3; ++q) {
      const double last = n_steps == 1 ? w.tr[0][q] : w.tr[1][q];
      if (k == 1) w.tr[1][q] = last;
      if (k == 2) w.tr[2][q] = last;
    }
}

// The block's sum of the lanes' counts, valid in thread 0 (every thread of the
// block calls it).
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

// Block r = robot r (kBlock threads): up to max_calls MPC steps of its episode
// (fewer if it ends).  log: [n][cap] ring per robot; progress (optional):
// {calls, stop, candidates} per robot after the launch.
// Lane l rolls out candidates l, l + kBlock, ... two at a time, interleaved
// (const_pair_cost): two independent chains per lane cover the recurrence's
// latency, at the price of registers: the launch bound asks for 2 waves per
// SIMD (<= 256 VGPRs), so 2 robots per CU at a time.  A robot's serial phases
// (grid, re-roll, update: one wave or one lane) share their SIMD with the
// other resident robot's waves.  (One candidate at a time, and one wave per
// robot, were measured and not kept: DESIGN.md §1 and §6f.)
//
// With keep-out circles (mpc_episodes_run_obstacles; Obs = the mode's hook,
// mpc_episodes_obs.h) the kernel has two arguments more, through the packs:
// world (W = Obstacles), the one circle table of the launch, kernel argument 0
// (read through kernarg_world(): scalar loads), and count (B = int64_t; NULL:
// not counted), the last argument: [n] per robot the candidates blocked in
// the steps this launch ran for it (0 if none ran), written beside
// progress[r] by thread 0 — a lane-private add per pair, one block reduction
// at the end of the launch, no atomic.  (B* __restrict__: a pack deduced as
// B... would drop the qualifier, and hipcc then loads the argument elsewhere.)
// The semantics are mpc_rollout_partials_obstacles'
// (include/mpc_rollout.h): a blocked candidate never wins, an all-blocked step
// is the step without a finite cost (index -1, found 0, a stale step).  Every
// circle statement sits under `if constexpr (Obs::kOn)` in this one body: the
// plain instantiations (NoObs, empty packs) compile to what they were before
// the circles came (tools/kernel_digest.py).
// The hook is made by episode_obs(Obs*), found by argument-dependent lookup
// where the kernel is instantiated: this header, which the host replica's
// build parses, does not see FrameObs and the chained kernels it pulls in.
//
// A fleet call (mpc_episodes_fleet_run; Obs = FleetObs, W = FleetArgs,
// mpc_episodes_fleet.h) is a launch with max_calls = 1: a running robot's block
// first forms its table in LDS — the static circles and its chosen neighbours
// from this call's side of the pose board (obs.select) — and takes the NoObs
// pair rollout if the table is empty (a uniform branch); every block, stopped
// or not, writes its robot's position to the board's other side on exit, and
// count is added to, not written (the entry zeroes it before its launches).
// Every fleet statement sits under `if constexpr (kFleet)`.
// A predicted fleet call (mpc_episodes_fleet_run_predicted; Obs = FleetMotionObs,
// W = FleetMotionArgs) is a fleet call whose table has one part per horizon
// step: the pair rollout hands the hook the step's index, and the block writes
// the robot's displacement to the motion board's other side on exit.  Every
// such statement sits under `if constexpr (kMotion)` (motion_hook).
// A planned fleet call (mpc_episodes_fleet_run_planned; Obs = FleetPlanObs, W =
// FleetPlanArgs) is a predicted one whose tables follow the neighbours' plans:
// the kernel notes m at the start of the step beside from_x and, on exit, hands
// the hook the step's status, that m, the staged StaleTraj and the position for
// the plan board's other side.  Every such statement sits under
// `if constexpr (kPlan)` (plan_hook).
template <int INTEG, int ROT, class Obs = NoObs, class... W, class... B>
__global__ __launch_bounds__(kBlock, 2) void k_episodes_run(
    W... world, const mpc_episode_config_t* __restrict__ cfgs, RobotState* __restrict__ robots,
    int n_steps, int max_calls, mpc_episode_log_t* __restrict__ log, int cap,
    mpc_episodes_progress_t* __restrict__ progress, B* __restrict__... count) {
  static_assert(sizeof...(W) == (Obs::kOn ? 1 : 0) && sizeof...(B) == sizeof...(W),
                "the table and the count come with a hook, and only with one");
  constexpr bool kFleet = fleet_hook<Obs>::value;
  constexpr bool kMotion = motion_hook<Obs>::value;
  constexpr bool kPlan = plan_hook<Obs>::value;
  if constexpr (kFleet) kernarg_touch((world, ...).n, (count, ...));   // (both lines, one wait)
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
  [[maybe_unused]] Obs obs = [] {   // (FrameObs: its world table; the frame table per step)
    if constexpr (Obs::kOn)
      return episode_obs(static_cast<Obs*>(nullptr));
    else
      return Obs{};
  }();
  if constexpr (kFleet) obs.prefetch((world, ...));   // (the board's first chunk, in flight)
  int64_t cands = 0;                    // (thread 0)
  [[maybe_unused]] int64_t n_blk = 0;   // this lane's blocked candidates
  [[maybe_unused]] bool fleet_step = false;   // (kFleet) the robot took a step in this launch
  [[maybe_unused]] double from_x = 0.0, from_y = 0.0;   // (kMotion) where that step began
  [[maybe_unused]] int from_m = 0;                        // (kPlan) the finishing count m then
  TL_EP_BEGIN();
  for (int call = 0; call < max_calls; ++call) {
    __syncthreads();
    if (s_stop) break;   // uniform
    TL_EP_CALL();
    const EpisodeHead* Hs = reinterpret_cast<const EpisodeHead*>(s_head);
    if constexpr (kFleet) {   // this call's table (uniform: the whole block is here)
      obs.select((world, ...), r, Hs->x, Hs->y);
      fleet_step = true;
      if constexpr (kMotion) from_x = Hs->x, from_y = Hs->y;
      if constexpr (kPlan) from_m = Hs->m;
    }
    if (threadIdx.x < 64) {
      int nv, nb;
      episode_grids(c, *Hs, s_v, s_b, nv, nb);
      if (threadIdx.x == 0) {
        s_nv = nv;
        s_nb = nb;
      }
    }
    __syncthreads();
    TL_EP_MARK(0);
    const Consts K = uniform_consts(Hs->K);
    // rect+cum: the circles in the frame of THIS step's sums (uniform: the whole
    // block is here; the table's last readers passed the barriers above)
    if constexpr (Obs::kOn && ROT == kRotCum) obs.form(K, K.L_pow2 != 0);
    const double incumbent = Hs->incumbent;
    const int nv = s_nv, nb = s_nb, n_grid = nv * nb;
    uint64_t best_k = ~0ull;
    int64_t best_i = INT64_MAX;
    // lane l: candidates l, l + kBlock, l + 2 kBlock, ... two per pass (ascending
    // per lane: strict < keeps the first)
    for (int k0 = threadIdx.x; k0 < n_grid; k0 += 2 * kBlock) {
      const int k1 = k0 + kBlock;
      const bool has1 = k1 < n_grid;
      const int kq = has1 ? k1 : k0;   // (a valid stand-in: neither wins nor is counted)
      const double vv[2] = {s_v[k0 / nb], s_v[kq / nb]};
      const double bb[2] = {s_b[k0 % nb], s_b[kq % nb]};
      double cst[2];
      [[maybe_unused]] bool blk[2];
      if constexpr (kFleet) {
        if (obs.empty()) {   // uniform: no circle in this call — the loop without circles
          if (n_steps == 3)
            const_pair_cost<INTEG, ROT, 3>(K, vv, bb, n_steps, cst);
          else
            const_pair_cost<INTEG, ROT, 0>(K, vv, bb, n_steps, cst);
          blk[0] = blk[1] = false;
        } else if (n_steps == 3) {
          const_pair_cost<INTEG, ROT, 3, Obs>(K, vv, bb, n_steps, cst, obs, blk);
        } else {
          const_pair_cost<INTEG, ROT, 0, Obs>(K, vv, bb, n_steps, cst, obs, blk);
        }
      } else if (n_steps == 3)   // uniform: the reference's horizon, unrolled
        const_pair_cost<INTEG, ROT, 3, Obs>(K, vv, bb, n_steps, cst, obs, blk);
      else
        const_pair_cost<INTEG, ROT, 0, Obs>(K, vv, bb, n_steps, cst, obs, blk);
      if constexpr (Obs::kOn) {
        blk[1] = has1 && blk[1];
        n_blk += static_cast<int>(blk[0]) + static_cast<int>(blk[1]);
      }
      // (a blocked candidate: the key of a non-finite cost, which never wins)
      uint64_t kk;
      if constexpr (Obs::kOn)
        kk = blk[0] ? ~0ull : cost_key_nonneg(cst[0]);
      else
        kk = cost_key_nonneg(cst[0]);
      if (kk < best_k) {
        best_k = kk;
        best_i = k0;
      }
      if constexpr (Obs::kOn)
        kk = blk[1] ? ~0ull : cost_key_nonneg(cst[1]);
      else
        kk = cost_key_nonneg(cst[1]);
      if (has1 && kk < best_k) {
        best_k = kk;
        best_i = k1;
      }
    }
    TL_EP_MARK(1);
    block_argmin<true>(best_k, best_i);
    if (threadIdx.x == 0) {
      s_bk = best_k;
      s_bi = best_i;
      cands += n_grid;
    }
    __syncthreads();
    TL_EP_MARK(2);
    const uint64_t bk = s_bk;
    const int64_t bi = s_bi;
    // (in LDS: thread 0's private copy spilled to scratch, a memory round
    // trip per field on the step's serial path)
    __shared__ Winner s_win;
    Winner& win = s_win;
    if constexpr (ROT != kRotCum) {
      // wave 0 re-derives the winner itself (wave_winner_states_l for the
      // direct heading form, one lane's const_winner_states_l for the
      // rotation form): no block barriers
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
      // the winner's controls (constant over the horizon) staged for its re-roll
      if (bk != ~0ull && threadIdx.x < n_steps) {
        lds.pv[threadIdx.x] = s_v[bi / nb];
        lds.pb[threadIdx.x] = s_b[bi % nb];
      }
      // (v / b: the staged controls again, never read since pre_v / pre_b are
      // given — null constants there crash hipcc 7.2's inliner, which also
      // sees k_finalize's call of the same instantiation)
      emit_winner<INTEG, ROT>(K, lds.pv, lds.pb, 1, n_steps, bk, bi, bi, incumbent, &s_out,
                              &lds, &win, lds.pv, lds.pb, false);
    }
    TL_EP_MARK(3);
    if (threadIdx.x == 0) {   // (emit_winner, if it ran, ended with a barrier)
      EpisodeHead H;
      __builtin_memcpy(&H, s_head, sizeof(EpisodeHead));
      episode_advance<false>(c, H, *reinterpret_cast<StaleTraj*>(&s_head[kHeadWords]), win,
                             s_log);
      __builtin_memcpy(s_head, &H, sizeof(EpisodeHead));
      if (s_log.status & kEpEnded) s_stop = s_log.status;
      s_calls += 1;
    }
    TL_EP_MARK(4);
    __syncthreads();
    if (log && cap > 0 && threadIdx.x < kLogWords)
      reinterpret_cast<uint64_t*>(&log[static_cast<int64_t>(r) * cap + s_log.step % cap])
          [threadIdx.x] = reinterpret_cast<const uint64_t*>(&s_log)[threadIdx.x];
    TL_EP_MARK(5);
  }
  __syncthreads();
  for (int q = threadIdx.x; q < kStoredWords; q += kBlock)
    reinterpret_cast<uint64_t*>(R)[q] = s_head[q];
  [[maybe_unused]] int64_t* n_blocked = nullptr;
  [[maybe_unused]] int64_t blocked_all = 0;
  if constexpr (Obs::kOn) {
    n_blocked = (count, ...);
    if (n_blocked) blocked_all = block_sum_i64(n_blk);   // (uniform: a kernel argument)
  }
  if (threadIdx.x == 0) {
    R->stop = s_stop;
    R->calls = s_calls;
    R->candidates += cands;
    if (progress) {
      progress[r].calls = s_calls;
      progress[r].stop = s_stop;
      progress[r].candidates = R->candidates;
    }
    if constexpr (kFleet) {
      if (n_blocked) n_blocked[r] += blocked_all;
      const EpisodeHead* Hs = reinterpret_cast<const EpisodeHead*>(s_head);
      (world, ...).board_out[r] = {Hs->x, Hs->y};   // where the robot stands after this call
      if constexpr (kPlan)   // ... and where it means to go next, if it goes on with a winner
        Obs::publish((world, ...), r, fleet_step && !s_stop && !(s_log.status & MPC_EP_STALE),
                     from_m, *reinterpret_cast<const StaleTraj*>(&s_head[kHeadWords]), Hs->x,
                     Hs->y);
      else if constexpr (kMotion)   // ... and how far the call moved it, if it goes on
        Obs::publish((world, ...), r, fleet_step && !s_stop, from_x, from_y, Hs->x, Hs->y);
    } else if constexpr (Obs::kOn) {
      if (n_blocked) n_blocked[r] = blocked_all;
    }
  }
  if constexpr (kFleet) {
    if (!fleet_step) Obs::no_step((world, ...), r);   // uniform
  }
  TL_EP_END();
}

}  // namespace mpc
