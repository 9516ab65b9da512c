// Host build of the keep-out polygon tables (csrc/mpc_keepout.h): the entries'
// argument rule, the table builder with its rect+cum frame transform, and the
// inside predicate as the lane hook evaluates it, for
// tests/test_polygon_frame_cpu.py.
#include "../diplomjourney_amd/csrc/mpc_host_consts.h"
#include "../diplomjourney_amd/csrc/mpc_keepout.h"

using namespace mpc;

extern "C" {

int poly_check(const mpc_polygon_t* polygons, int n) { return check_polygons(polygons, n); }

// The constants the one-shot entries form the tables from: x, y, s0, c0, inv_L, L_pow2, L.
void poly_consts(const mpc_problem_t* p, double* out) {
  const Consts K = host_consts(*p);
  out[0] = K.x;
  out[1] = K.y;
  out[2] = K.s0;
  out[3] = K.c0;
  out[4] = K.inv_L;
  out[5] = K.L_pow2;
  out[6] = K.L;
}

// n checked polygons -> every slot (a, b, c) of the world table and of the
// rect+cum loop table of the step that starts at p's pose, as a launch gets them.
void poly_tables(const mpc_problem_t* p, const mpc_polygon_t* polygons, int n, double* world,
                 double* loop) {
  const Consts K = host_consts(*p);
  const KeepoutArgs O = keepout_args(K, ObstacleArgs{}, polygons, n, true);
  static_assert(sizeof(Polygons) == 3 * sizeof(double) * MPC_MAX_POLYGONS * MPC_MAX_POLYGON_VERTICES,
                "a table is its edges");
  memcpy(world, &O.pworld, sizeof(Polygons));
  memcpy(loop, &O.ploop, sizeof(Polygons));
}

// inside_polygons of n points (x, y) against the first n_poly polygons of a table.
void poly_inside(const double* table, int n_poly, const double* xy, int64_t n, uint8_t* out) {
  Polygons T;
  memcpy(&T, table, sizeof(T));
  for (int64_t i = 0; i < n; ++i) out[i] = inside_polygons(T, n_poly, xy[2 * i], xy[2 * i + 1]);
}

// cum_pose of n points (A, B) of the sums frame (scaled sums when L is a power of two).
void poly_cum_pose(const mpc_problem_t* p, const double* ab, int64_t n, double* xy) {
  const Consts K = host_consts(*p);
  for (int64_t i = 0; i < n; ++i) {
    if (K.L_pow2)
      cum_pose<true>(K, ab[2 * i], ab[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
    else
      cum_pose<false>(K, ab[2 * i], ab[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
  }
}

}  // extern "C"
