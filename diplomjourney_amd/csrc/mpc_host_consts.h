// mpc_host_consts.h — the problem constants as the HOST derives them, for the
// one-shot entries of mpc_rollout.hip and for the host replica
// (tests/replica_harness.cpp): one source for both.  Host code only.
//
//   g_libm_pow, g_libm_sin, g_libm_cos   libm through volatile pointers
//   length_pow2          the wheelbase is a power of two
//   host_consts          Consts of a problem with the reference's libm calls
//   host_window_consts   Consts of a quad window alone (the full tree's shared
//                        control table, mpc_fulltree_argmin_batched)
//   world_obstacles, frame_obstacles   the keep-out circle tables of a call
// (The device's own derivation, x*x and sincos_fast, is consts_from_problem in
// mpc_device.h.)
#pragma once

#include <math.h>
#include <string.h>

#include "../../include/mpc_rollout.h"
#include "mpc_device.h"

namespace mpc {

// libm through volatile pointers: the compiler must not fold pow(x, 2.0) into
// x*x (Python's `a ** 2` is libm pow, which is not always x*x).
inline double (*volatile g_libm_pow)(double, double) = pow;
inline double (*volatile g_libm_sin)(double) = sin;
inline double (*volatile g_libm_cos)(double) = cos;

// The wheelbase is a power of two: sums scaled by 1/L are then exact, which the
// PL2 kernel instantiations and Consts::L_pow2 (consts_from_problem) rely on.
inline bool length_pow2(double L) {
  int e;
  return frexp(L, &e) == 0.5;
}

// Problem constants derived on the host with the reference's libm calls.
inline Consts host_consts(const mpc_problem_t& p) {
  Consts K;
  memset(&K, 0, sizeof(K));
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
  K.inv_den = 1.0 / sqrt(g_libm_pow(K.A, 2.0) + g_libm_pow(K.B, 2.0));
  K.L = p.L;
  K.L_pow2 = length_pow2(p.L) ? 1 : 0;
  K.inv_L = K.L_pow2 ? 1.0 / p.L : 0.0;
  K.h = p.t_b - p.t_a;
  K.hlgth = 0.5 * (p.t_b - p.t_a);
  K.s0 = g_libm_sin(p.phi);
  K.c0 = g_libm_cos(p.phi);
  return K;
}

// The constants of a quad window [t_a, t_b] and a wheelbase alone: what a
// control table shared by many robots is built from (no pose; a target off the
// origin so that the line terms stay finite).
inline Consts host_window_consts(double L, double t_a, double t_b) {
  mpc_problem_t q = {};
  q.x_t = 1.0;   // window-only constants for the shared control table
  q.y_t = 1.0;
  q.L = L;
  q.t_a = t_a;
  q.t_b = t_b;
  return host_consts(q);
}

// The circle tables of a call (mpc_device.h Obstacles), one-shot and episode
// entries alike.  world_obstacles: (x, y, r^2) in world coordinates; entries
// past n can never be entered (r2 = -1).
inline Obstacles world_obstacles(const mpc_obstacle_t* obs, int n) {
  Obstacles W;
  for (int i = 0; i < MPC_MAX_OBSTACLES; ++i) W.c[i] = Circle{0.0, 0.0, -1.0, 0.0};
  for (int i = 0; i < n; ++i) W.c[i] = Circle{obs[i].x, obs[i].y, obs[i].r * obs[i].r, 0.0};
  return W;
}

// frame_obstacles: the `loop` table of rect+cum for the step that starts at
// K's pose, frame_circle per entry (the episode kernels form the same table on
// the device from the state's pose, mpc_episode_obs.h).
inline Obstacles frame_obstacles(const Consts& K, const Obstacles& world, int n) {
  Obstacles F = world;
  for (int i = 0; i < n; ++i) F.c[i] = frame_circle(K, world.c[i], K.L_pow2 != 0);
  return F;
}

}  // namespace mpc
