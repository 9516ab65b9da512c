// mpc_device.h — the arithmetic of the MPC candidate expansion that compiles
// for host AND device (gfx950): the kernels run it, and the host replica
// (tests/replica_harness.cpp) calls the same functions.
//
//   Consts, consts_from_problem     per-problem constants, as the device derives them
//   quad_const, heading_incr, position_step, step_core, step_start, cum_pose,
//   step_safe, crit_sqrt, cost      one step and the criterion
//   Circle .. ObsTable, NoObs, CircleObs   keep-out circles: tables and lane hooks
//   frame_circle                    a circle in the frame of the rect+cum sums
//   fleet_d2                        the squared distance a fleet call ranks neighbours by
//   rollout_candidate_l, rollout_candidate  one candidate as the kernels evaluate it
//
// Every function here states one piece of ShittyWizard/DiplomJourney's
// math_model_tree.py in IEEE fp64 with the reference's operation order.  The
// translation unit is compiled with -ffp-contract=off so each + - * / is one
// rounding, exactly as in CPython; tan/sincos/sqrt are the ROCm device
// kernel's own fp64 routines (mpc_trig.h; faithfully rounded, <= 1 ulp from
// glibc's).  Nothing here is device-only: reductions, keys and the sampler's
// hash are in mpc_argmin.h and mpc_sampler.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_trig.h"

namespace mpc {

// Per-problem constants, derived once on the host (or per robot on device).
struct Consts {
  double x, y, phi;        // s0 = initial_coordinates (math_model_tree.py:294)
  double x_t, y_t;         // target globals (:65-66)
  double x_0, y_0;         // line origin globals (:57)
  double A, B, C1, C2;     // (y_t-y_0), (x_t-x_0), x_t*y_0, y_t*x_0   (:60)
  double inv_den;          // 1 / sqrt((y_t-y_0)**2 + (x_t-x_0)**2)    (:61): the line
                           // distance's division as a multiply (one rounding apart)
  double L, inv_L;         // wheelbase; 1/L when L is a power of two
  double h;                // (t+dt) - t, the quad interval length (RECT)
  double hlgth;            // 0.5*((t+dt) - t), QUADPACK's half length (QK21)
  double s0, c0;            // sin/cos of phi (heading-rotation mode)
  int32_t L_pow2;          // v/L == v*inv_L exactly
  int32_t pad_;
};

// Problem constants derived on the device (batched robots, episode).  The
// squares are x*x (glibc pow(x, 2.0) differs by 1 ulp in ~0.1% of inputs);
// the single-problem host path derives them with libm pow.
MPC_HD __forceinline__ Consts consts_from_problem(const mpc_problem_t& p) {
  Consts K;
  K.x = p.x;
  K.y = p.y;
  K.phi = p.phi;
  K.x_t = p.x_t;
  K.y_t = p.y_t;
  K.x_0 = p.x_0;
  K.y_0 = p.y_0;
  K.A = p.y_t - p.y_0;
  K.B = p.x_t - p.x_0;
  K.C1 = p.x_t * p.y_0;
  K.C2 = p.y_t * p.x_0;
  K.inv_den = 1.0 / sqrt(K.A * K.A + K.B * K.B);
  K.L = p.L;
  int e;
  const double m = frexp(p.L, &e);
  K.L_pow2 = (m == 0.5) ? 1 : 0;
  K.inv_L = K.L_pow2 ? 1.0 / p.L : 0.0;
  K.h = p.t_b - p.t_a;
  K.hlgth = 0.5 * (p.t_b - p.t_a);
  trig::sincos_fast(p.phi, &K.s0, &K.c0);
  K.pad_ = 0;
  return K;
}

// QUADPACK dqk21 Kronrod weights wgk(1..11).
constexpr double kWGK[11] = {
    0.011694638867371874278064396062192, 0.032558162307964727478818972459390,
    0.054755896574351996031381300244580, 0.075039674810919952767043140916190,
    0.093125454583697605535065465083366, 0.109387158802297641899210590325805,
    0.123491976262065851077208698889469, 0.134709217311473325928054001771707,
    0.142775938577060080797094273138717, 0.147739104901338491374841515972068,
    0.149445554002916905664936468389821};

// sp.quad(f, t, t+dt) of a constant integrand (math_model_tree.py:91-96).
template <int INTEG>
MPC_HD __forceinline__ double quad_const(double f, const Consts& K) {
  if constexpr (INTEG == MPC_INTEG_RECT) {
    return f * K.h;
  } else {
    double resk = kWGK[10] * f;
    const double fsum = f + f;
#pragma unroll
    for (int j = 1; j <= 9; j += 2) resk = resk + kWGK[j] * fsum;
#pragma unroll
    for (int j = 0; j <= 8; j += 2) resk = resk + kWGK[j] * fsum;
    return resk * K.hlgth;
  }
}

// The three integrals of one step.  QK21: the reference's quad() (bitwise
// dqk21 on the constant integrand).  RECT: the same integrals of the constant
// integrands evaluated directly, h * f, with one rounding fewer per position
// update: dphi = ((v/L) * h) * tan(beta), x' = fma(v * h, cos phi', x).  (For
// L a power of two (v * inv_L) * h == (v * h) * inv_L exactly, so both forms of
// v/L give the same dphi.)
template <int INTEG>
MPC_HD __forceinline__ double heading_incr(double w, double t, const Consts& K) {
  if constexpr (INTEG == MPC_INTEG_RECT)
    return (w * K.h) * t;
  else
    return quad_const<INTEG>(w * t, K);
}

template <int INTEG>
MPC_HD __forceinline__ double position_step(double p, double v, double trig, const Consts& K) {
  if constexpr (INTEG == MPC_INTEG_RECT)
    return fma(v * K.h, trig, p);
  else
    return p + quad_const<INTEG>(v * trig, K);
}

// iteration_of_predict (math_model_tree.py:111-115): heading first, then
// position with the updated heading (semi-implicit bicycle step).
//
// step_core is the hot-loop form.  It uses the range-limited trig cores and
// flags the candidate `bad` when an argument leaves their range (|beta| >
// kTanMax; in direct mode |phi| > kFastMax; in rotation mode |dphi| > kRotMax;
// NaN).
// A bad candidate is recomputed with step_safe (direct sin/cos, library
// fallbacks), so every candidate gets a well-defined, correct result while the
// hot loop carries no fallback code.
//   ROT = false: sin/cos of the new heading evaluated directly (the reference's
//                formula, :113-114)
//   ROT = 1:     (s, c) carry sin/cos of the heading and are rotated by the
//                increment (mpc_trig.h rotation_factors / rotate_by)
//   ROT = 2:     (kRotCum) the same recurrence started from the identity
//                rotation (s, c) = (0, 1) and positions (x, y) = (0, 0): it
//                accumulates the pose-independent sums A = sum vh cos(Phi_k),
//                B = sum vh sin(Phi_k) of the heading increments Phi_k since
//                the start; cum_pose() turns them into the pose.  The work
//                per step is ROT = 1's; only the start state and the final
//                transform differ, and nothing before the transform needs the
//                start pose (the chained episode step, k_episode_chain).
//   PL2:         L is a power of two (v / L == v * inv_L exactly).  A template
//                parameter, not a branch: a branch inside the step would split
//                the loop into basic blocks and stop the scheduler from
//                interleaving the lane's independent candidate chains.
//   PL2 + RECT:  (v * inv_L) * h is formed as (v * h) * inv_L — the same
//                value (scaling by a power of two commutes with rounding in the
//                normal range) — so v * h is shared with the position update.
//                kRotCum goes one step further: v * (h * inv_L) serves both, the
//                sums A, B are accumulated scaled by 1/L (every rounding scales
//                exactly) and cum_pose<true> scales them back: the same bits
//                as the unscaled sums, one multiply fewer per step.
//   ld:          VGPR-resident leading coefficients (trig::Leads), or nullptr.
constexpr int kRotCum = 2;

template <int INTEG, int ROT, bool PL2>
MPC_HD __forceinline__ void step_core(double& x, double& y, double& ph, double& s, double& c,
                                      double v, double beta, const Consts& K, bool& bad,
                                      const trig::Leads* ld = nullptr) {
  bad |= !(fabs(beta) <= trig::kTanMax);
  const double t = trig::tan_small(beta, ld);
  double dphi, vh = 0.0;
  if constexpr (PL2 && INTEG == MPC_INTEG_RECT && ROT == kRotCum) {
    vh = v * (K.h * K.inv_L);                                  // the sums scaled by 1/L
    dphi = vh * t;                                             // angle_phi (:107)
  } else if constexpr (PL2 && INTEG == MPC_INTEG_RECT) {
    vh = v * K.h;
    dphi = (vh * K.inv_L) * t;                                 // angle_phi (:107)
  } else {
    const double w = PL2 ? v * K.inv_L : v / K.L;              // _velocity / L   (:78)
    dphi = heading_incr<INTEG>(w, t, K);                       // angle_phi (:107)
  }
  ph = ph + dphi;                                              // phi + _phi      (:113)
  if constexpr (ROT) {
    bad |= !(fabs(dphi) <= trig::kRotMax);
    double sd, cd;
    trig::rotation_sc(dphi, sd, cd, ld);
    trig::rotate_sc(sd, cd, s, c);
  } else {
    bad |= !(fabs(ph) <= trig::kFastMax);
    trig::sincos_core(ph, &s, &c);
  }
  if constexpr (PL2 && INTEG == MPC_INTEG_RECT) {
    x = fma(vh, c, x);                                         // coordinate_x    (:99)
    y = fma(vh, s, y);                                         // coordinate_y    (:103)
  } else {
    x = position_step<INTEG>(x, v, c, K);                      // coordinate_x    (:99)
    y = position_step<INTEG>(y, v, s, K);                      // coordinate_y    (:103)
  }
}

// Start state of the step recurrence: the pose (ROT 0 / 1) or the identity
// rotation and empty sums (kRotCum).
template <int ROT>
MPC_HD __forceinline__ void step_start(const Consts& K, double& x, double& y, double& ph,
                                       double& s, double& c) {
  ph = K.phi;
  if constexpr (ROT == kRotCum) {
    x = 0.0;
    y = 0.0;
    s = 0.0;
    c = 1.0;
  } else {
    x = K.x;
    y = K.y;
    s = K.s0;
    c = K.c0;
  }
}

// kRotCum: position from the sums, x = x0 + (c0 A - s0 B), y = y0 + (s0 A + c0 B).
// SCALED: the sums of step_core<RECT, kRotCum, PL2 = true>, i.e. A/L and B/L.
template <bool SCALED>
MPC_HD __forceinline__ void cum_pose(const Consts& K, double A, double B, double& x, double& y) {
  if constexpr (SCALED) {
    A = A * K.L;
    B = B * K.L;
  }
  x = K.x + fma(K.c0, A, -(K.s0 * B));
  y = K.y + fma(K.s0, A, K.c0 * B);
}

template <int INTEG>
MPC_HD __forceinline__ void step_safe(double& x, double& y, double& ph, double v, double beta,
                                      const Consts& K) {
  const double w = K.L_pow2 ? v * K.inv_L : v / K.L;
  const double dphi = heading_incr<INTEG>(w, trig::tan_fast(beta), K);
  ph = ph + dphi;
  double s, c;
  trig::sincos_fast(ph, &s, &c);
  x = position_step<INTEG>(x, v, c, K);
  y = position_step<INTEG>(y, v, s, K);
}

// IEEE sqrt for the criteria: on the device, the rsq + Newton sequence hipcc
// emits for sqrt(double) (correctly rounded: the same bits as sqrt) without
// its input scaling and special-case selects, 11 instead of 18 VALU.  Exact
// for 0 and for every input >= 2^-767; below that (a terminal
// state closer to the target than 1e-115) and for +inf / NaN it returns NaN,
// which never wins the strict < of an arg-min (+inf and NaN never do either).
MPC_HD __forceinline__ double crit_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  // (the estimate of max(x, 2^-767): x itself in the exact range; for x = 0 a
  // finite estimate, so the sequence yields 0 exactly without a select; a NaN
  // x still propagates through the products)
  const double y = __builtin_amdgcn_rsq(fmax(x, 0x1p-767));
  double g = x * y, h = y * 0.5;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  double d = fma(-g, g, x);
  g = fma(d, h, g);
  d = fma(-g, g, x);
  return fma(d, h, g);
#else
  return sqrt(x);
#endif
}

// control_criterion (math_model_tree.py:82-87) on the layer-N state.
MPC_HD __forceinline__ double cost(double x, double y, const Consts& K) {
  const double ex = K.x_t - x, ey = K.y_t - y;
  const double dist_target = crit_sqrt(ex * ex + ey * ey);     // :66
  // :60-61, the division by the hypotenuse as a multiply by its reciprocal
  // (formed once per problem): <= 1 ulp from the quotient, and ~10 VALU
  // fewer per candidate than the IEEE division sequence.  Both sides of the
  // sentinel test are formed and one selected (no divergent branch).
  const double dl = fabs(K.A * x - K.B * y + K.C1 - K.C2) * K.inv_den;
  const double d = (x == K.x_0 && y == K.y_0) ? 1000.0 : dl;  // :57-58
  return 10000.0 * dist_target + 10000.0 * (d * d);            // :62, :87
}

// Keep-out circles (mpc_rollout_partials_obstacles; semantics in
// include/mpc_rollout.h).  One table per launch, a kernel argument: every
// entry is wave-uniform and reaches the test as a scalar operand, nothing per
// lane.  Entries past the call's count hold r2 = -1, which no squared distance
// is below, so a kernel instantiated for NOBS circles serves any count <= NOBS
// with straight-line code.
//   loop:  the circles in the frame of the step recurrence's (x, y): world
//          coordinates, or for kRotCum the start-pose frame of the sums (A, B)
//          — centres rotated by -phi about the start position, and with the
//          1/L-scaled sums of PL2 centres and radii scaled by 1/L (exact: L is
//          a power of two) — so the test needs no cum_pose per step.
//   world: world coordinates, for the irregular-candidate recompute
//          (step_safe), whose states replace the loop's.
struct Circle {
  double cx, cy, r2, pad_;   // 32 B
};
struct Obstacles {
  Circle c[MPC_MAX_OBSTACLES];
};
struct ObstacleArgs {
  Obstacles loop, world;
};
// The table as the kernels read it: in the kernel-argument segment (constant
// address space: scalar loads).
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) Obstacles* ObsTable;
#else
typedef const Obstacles* ObsTable;
#endif

// Obstacle hooks of the rollout lanes (the style of NoPre / NoSide): loop()
// after every step of the step_core recurrence, for the lane's CPL candidates
// together (one read of the table); world() after every step of the step_safe
// recompute.  Both OR into the candidates' `blocked` flags, which sit next to
// `bad`.  NoObs: the kernels without obstacles (no obstacle statement is
// instantiated: their code is unchanged).
struct NoObs {
  static constexpr bool kOn = false;
};

// (x, y) strictly inside any of the first NOBS circles.  Predicates only: no
// branch, no early exit; a NaN state compares false (its NaN cost never wins
// anyway).  Per circle and candidate 2 add, 1 mul, 1 fma, 1 compare; the lane
// masks are combined on the SALU.
// Up to 4 circles (24 SGPRs) stay in SGPRs across the rollout loop.  16 would
// need 96 of the ~100 SGPRs: hipcc hoists the loads out of the loop all the
// same and spills them to VGPR lanes, and the loop then reloads every operand
// with a v_readlane (146-171 of ~400 VALU per lane-step, counted in the ISA).
// So for NOBS > 4 the table pointer is made opaque per step: the step's
// scalar loads stay inside the step (32 s_load per lane-step, no VALU).
template <int NOBS>
struct CircleObs {
  static_assert(NOBS >= 1 && NOBS <= MPC_MAX_OBSTACLES, "circle count");
  static constexpr bool kOn = true;
  ObsTable loop_t, world_t;
  template <int CPL>
  __device__ __forceinline__ static void test(ObsTable t, const double (&x)[CPL],
                                              const double (&y)[CPL], bool (&blocked)[CPL]) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (NOBS > 4) asm volatile("" : "+s"(t));
#endif
    // (FrameObs::loop, mpc_episode_obs.h, has a copy of this loop: DESIGN.md §5)
#pragma unroll
    for (int i = 0; i < NOBS; ++i) {
      const double cx = t->c[i].cx, cy = t->c[i].cy, r2 = t->c[i].r2;
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const double dx = x[j] - cx, dy = y[j] - cy;
        blocked[j] |= fma(dy, dy, dx * dx) < r2;
      }
    }
  }
  template <int CPL>
  __device__ __forceinline__ void loop(const double (&x)[CPL], const double (&y)[CPL],
                                       bool (&blocked)[CPL]) const {
    test<CPL>(loop_t, x, y, blocked);
  }
  __device__ __forceinline__ void world(double x, double y, bool& blocked) const {
    const double xs[1] = {x}, ys[1] = {y};
    bool bl[1] = {blocked};
    test<1>(world_t, xs, ys, bl);
    blocked = bl[0];
  }
};

// One world-table circle (centre, r^2) in the frame of the kRotCum sums of the
// step that starts at K's pose: the `loop` entry host_obstacles forms on the
// host, for the entries whose pose exists only on the device (the episode
// steps, mpc_episode_obs.h).  A = c0 dx + s0 dy, B = c0 dy - s0 dx with (dx, dy)
// the centre minus the start position — the inverse of cum_pose — and, for the
// 1/L-scaled sums of PL2, centre times 1/L and r^2 times 1/L^2 (L a power of
// two: (r / L)^2 exactly).  An unused entry (r2 = -1) stays one.
MPC_HD __forceinline__ Circle frame_circle(const Consts& K, const Circle& w, bool scaled) {
  const double sc = scaled ? K.inv_L : 1.0;
  const double dx = w.cx - K.x, dy = w.cy - K.y;
  return Circle{(K.c0 * dx + K.s0 * dy) * sc, (K.c0 * dy - K.s0 * dx) * sc, w.r2 * (sc * sc), 0.0};
}

// The squared distance by which a robot of a fleet call ranks another
// (mpc_episodes_fleet_run, mpc_episodes_fleet.h): q's position minus r's, one
// fused operation — the form of the circle test above.  Never negative and
// never -0, so its bits order it.  The fleet model's host build calls this
// (tests/fleet_harness.cpp).
MPC_HD __forceinline__ double fleet_d2(double xr, double yr, double xq, double yq) {
  const double dx = xq - xr, dy = yq - yr;
  return fma(dy, dy, dx * dx);
}

// One coordinate of a neighbour's circle at horizon step j (1..N: the state
// after step j) of a predicted fleet call (mpc_episodes_fleet_run_predicted):
// where the neighbour stood when the call began plus j times its last call's
// displacement — the product rounded, then the sum (two roundings, never
// fused).  d = 0 gives x back bit for bit (x + 0.0; a position is never -0
// where it matters: the circle test takes differences).  The fleet model's
// host build calls this too (tests/fleet_harness.cpp).
MPC_HD __forceinline__ double fleet_predict(double x, double d, int j) {
  return x + static_cast<double>(j) * d;
}

// One candidate, exactly as the kernels evaluate it (the host replica in
// tests/replica_harness.cpp calls this): the core recurrence, and if that
// flags the candidate, the safe recurrence.  traj (optional) gets the
// per-step (x, y, phi).  Returns the cost.
template <int INTEG, int ROT, bool PL2>
MPC_HD inline double rollout_candidate_l(const Consts& K, const double* v, const double* b,
                                         int64_t ld, int64_t col, int n_steps, double* traj) {
  double x, y, ph, s, c;
  step_start<ROT>(K, x, y, ph, s, c);
  bool bad = false;
  for (int st = 0; st < n_steps; ++st) {
    step_core<INTEG, ROT, PL2>(x, y, ph, s, c, v[st * ld + col], b[st * ld + col], K, bad);
    if (traj) {
      if constexpr (ROT == kRotCum) {
        cum_pose<PL2>(K, x, y, traj[3 * st + 0], traj[3 * st + 1]);
      } else {
        traj[3 * st + 0] = x;
        traj[3 * st + 1] = y;
      }
      traj[3 * st + 2] = ph;
    }
  }
  if constexpr (ROT == kRotCum) {
    if (!bad) cum_pose<PL2>(K, x, y, x, y);
  }
  if (bad) {
    x = K.x;
    y = K.y;
    ph = K.phi;
    for (int st = 0; st < n_steps; ++st) {
      step_safe<INTEG>(x, y, ph, v[st * ld + col], b[st * ld + col], K);
      if (traj) {
        traj[3 * st + 0] = x;
        traj[3 * st + 1] = y;
        traj[3 * st + 2] = ph;
      }
    }
  }
  return cost(x, y, K);
}

template <int INTEG, int ROT>
MPC_HD inline double rollout_candidate(const Consts& K, const double* v, const double* b,
                                       int64_t ld, int64_t col, int n_steps, double* traj) {
  return K.L_pow2 ? rollout_candidate_l<INTEG, ROT, true>(K, v, b, ld, col, n_steps, traj)
                  : rollout_candidate_l<INTEG, ROT, false>(K, v, b, ld, col, n_steps, traj);
}

}  // namespace mpc
