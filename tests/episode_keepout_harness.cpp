// Host build of what the device-resident episode's keep-out kernels judge a
// candidate by (csrc/mpc_episode_keepout.h), for tests/episode_keepout_cases.py:
// the polygon tables, the rect+cum sums they are evaluated on and cum_pose, all
// with the EPISODE's constants — consts_from_problem (mpc_device.h), which the
// device derives from the pose in its state — where tests/polygon_harness.cpp
// and replica_cum_sums (tests/replica_harness.cpp) use the one-shot entries'
// host_consts.  The frame table is frame_polygons, i.e. frame_edge per slot:
// the function FrameKeepoutObs::form calls on the device.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../diplomjourney_amd/csrc/mpc_device.h"
#include "../diplomjourney_amd/csrc/mpc_keepout.h"

#include <unordered_map>

using namespace mpc;

// The device's reciprocal estimates of the recurrence's denominators, as
// tests/replica_harness.cpp keeps them (replica_set_rcp_table): this library
// has its own copy of the hook they are read through (mpc_trig.h), so the
// table that harness.replica_rollout installs there is installed here as well.
static std::unordered_map<uint64_t, double> g_rcp;
static int64_t g_rcp_misses = 0;

static double rcp_from_table(double q) {
  uint64_t k;
  memcpy(&k, &q, 8);
  const auto it = g_rcp.find(k);
  if (it == g_rcp.end()) {
    ++g_rcp_misses;
    return 1.0 / q;
  }
  return it->second;
}

// The sums (A, B) of the rect+cum recurrence after every step and the
// candidate's `bad` flag: cum_sums of tests/replica_harness.cpp restated (it
// is static there, and replica_cum_sums calls it with host_consts), here with
// the episode's constants.  sums: [n_steps][2][n_cand].
template <bool PL2>
static void cum_sums(const Consts& K, const double* v, const double* b, int64_t n_cand,
                     int32_t n_steps, double* sums, uint8_t* bad_out) {
  for (int64_t col = 0; col < n_cand; ++col) {
    double x, y, ph, s, c;
    step_start<kRotCum>(K, x, y, ph, s, c);
    bool bad = false;
    for (int st = 0; st < n_steps; ++st) {
      step_core<MPC_INTEG_RECT, kRotCum, PL2>(x, y, ph, s, c, v[st * n_cand + col],
                                              b[st * n_cand + col], K, bad);
      sums[(st * 2 + 0) * n_cand + col] = x;
      sums[(st * 2 + 1) * n_cand + col] = y;
    }
    bad_out[col] = bad ? 1 : 0;
  }
}

extern "C" {

void ek_set_rcp_table(const double* q, const double* r, int64_t n) {
  g_rcp.clear();
  g_rcp_misses = 0;
  trig::g_host_rcp_estimate = n > 0 ? rcp_from_table : nullptr;
  for (int64_t i = 0; i < n; ++i) {
    uint64_t k;
    memcpy(&k, &q[i], 8);
    g_rcp[k] = r[i];
  }
}

int64_t ek_rcp_misses(void) { return g_rcp_misses; }

// x, y, s0, c0, inv_L, L_pow2, L of the episode's constants.
void ek_consts(const mpc_problem_t* p, double* out) {
  const Consts K = consts_from_problem(*p);
  out[0] = K.x;
  out[1] = K.y;
  out[2] = K.s0;
  out[3] = K.c0;
  out[4] = K.inv_L;
  out[5] = K.L_pow2;
  out[6] = K.L;
}

// n checked polygons -> every slot (a, b, c) of the world table (a launch's
// kernel argument) and of the frame table the rect+cum kernels form from it
// for the step that starts at p's pose.
void ek_tables(const mpc_problem_t* p, const mpc_polygon_t* polygons, int n, double* world,
               double* frame) {
  const Polygons W = world_polygons(polygons, n);
  const Polygons F = frame_polygons(consts_from_problem(*p), W);
  memcpy(world, &W, sizeof(Polygons));
  memcpy(frame, &F, sizeof(Polygons));
}

// cum_sums with the episode's constants.
void ek_cum_sums(const mpc_problem_t* p, const double* v, const double* b, int64_t n_cand,
                 int32_t n_steps, double* sums, uint8_t* bad_out) {
  const Consts K = consts_from_problem(*p);
  if (K.L_pow2)
    cum_sums<true>(K, v, b, n_cand, n_steps, sums, bad_out);
  else
    cum_sums<false>(K, v, b, n_cand, n_steps, sums, bad_out);
}

// cum_pose of n points (A, B) of the sums frame (scaled sums when L is a power of two).
void ek_cum_pose(const mpc_problem_t* p, const double* ab, int64_t n, double* xy) {
  const Consts K = consts_from_problem(*p);
  for (int64_t i = 0; i < n; ++i) {
    if (K.L_pow2)
      cum_pose<true>(K, ab[2 * i], ab[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
    else
      cum_pose<false>(K, ab[2 * i], ab[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
  }
}

}  // extern "C"
