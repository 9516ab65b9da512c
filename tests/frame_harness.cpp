// Host build of frame_circle (csrc/mpc_device.h): the rect+cum circle table of
// the device-resident episode steps, as the kernels form it, and the library's
// own table builder (csrc/mpc_host_consts.h), for
// tests/test_episode_obstacles_abi.py.
#include "../diplomjourney_amd/csrc/mpc_host_consts.h"

using namespace mpc;

extern "C" {

// The constants the table is formed from: x, y, s0, c0, inv_L, L_pow2, L.
void frame_consts(const mpc_problem_t* p, double* out) {
  const Consts K = consts_from_problem(*p);
  out[0] = K.x;
  out[1] = K.y;
  out[2] = K.s0;
  out[3] = K.c0;
  out[4] = K.inv_L;
  out[5] = K.L_pow2;
  out[6] = K.L;
}

// world: n circles (x, y, r) -> out: n frame entries (cx, cy, r2), from the
// world table's entry (x, y, r * r) as the episode entries build it; the
// table is scaled when L is a power of two.
void frame_circles(const mpc_problem_t* p, const double* world, int n, double* out) {
  const Consts K = consts_from_problem(*p);
  for (int i = 0; i < n; ++i) {
    const double r = world[3 * i + 2];
    const Circle f =
        frame_circle(K, Circle{world[3 * i], world[3 * i + 1], r * r, 0.0}, K.L_pow2 != 0);
    out[3 * i] = f.cx;
    out[3 * i + 1] = f.cy;
    out[3 * i + 2] = f.r2;
  }
}

// world_obstacles / frame_obstacles, the builder the entries call: n circles
// (x, y, r) -> all MPC_MAX_OBSTACLES entries (cx, cy, r2) of the world table and
// of the rect+cum loop table of the step that starts at p's pose.
void frame_tables(const mpc_problem_t* p, const mpc_obstacle_t* circles, int n, double* world,
                  double* loop) {
  const Consts K = consts_from_problem(*p);
  const Obstacles W = world_obstacles(circles, n), F = frame_obstacles(K, W, n);
  for (int i = 0; i < MPC_MAX_OBSTACLES; ++i) {
    const double w[3] = {W.c[i].cx, W.c[i].cy, W.c[i].r2}, f[3] = {F.c[i].cx, F.c[i].cy, F.c[i].r2};
    for (int q = 0; q < 3; ++q) world[3 * i + q] = w[q], loop[3 * i + q] = f[q];
  }
}

// cum_pose of n points (A, B) of the sums frame (scaled sums when L is a power of two).
void frame_cum_pose(const mpc_problem_t* p, const double* ab, int n, double* xy) {
  const Consts K = consts_from_problem(*p);
  for (int i = 0; i < n; ++i) {
    if (K.L_pow2)
      cum_pose<true>(K, ab[2 * i], ab[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
    else
      cum_pose<false>(K, ab[2 * i], ab[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
  }
}

}  // extern "C"
