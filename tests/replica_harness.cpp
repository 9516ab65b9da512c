// Host build of the kernel's own per-candidate arithmetic (mpc_device.h:
// problem constants, step, cost; mpc_trig.h) for tests/test_replica.py, and of
// the full tree's per-leaf arithmetic (mpc_ftdevice.h) for
// tests/fulltree_cases.py.  The GPU must reproduce these states and costs bit
// for bit: same source, same IEEE operations, fma and rint are exact on both
// sides.  The host-derived constants are the library's too
// (mpc_host_consts.h).  One body is repeated here, not shared: the
// per-control lines of k_ft_controls (mpc_fulltree.h), marked below -- as a
// shared function they changed the kernel's code.  Test infrastructure only.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <unordered_map>

#include "../diplomjourney_amd/csrc/mpc_device.h"
#include "../diplomjourney_amd/csrc/mpc_host_consts.h"

// The device's reciprocal estimates (v_rcp_f64 is not an IEEE operation):
// a GPU test fetches them for every denominator the rollout will form
// (replica_tan_q -> mpc_rcp_estimate) and installs them here; without a table
// the host build uses 1.0 / q.
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

extern "C" void replica_set_rcp_table(const double* q, const double* r, int64_t n) {
  g_rcp.clear();
  g_rcp_misses = 0;
  if (n <= 0) {
    mpc::trig::g_host_rcp_estimate = nullptr;
    return;
  }
  g_rcp.reserve(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    uint64_t k;
    memcpy(&k, &q[i], 8);
    g_rcp[k] = r[i];
  }
  mpc::trig::g_host_rcp_estimate = rcp_from_table;
}

extern "C" int64_t replica_rcp_misses(void) { return g_rcp_misses; }

// The denominators tan_small forms for these steering angles.
extern "C" void replica_tan_q(const double* beta, int64_t n, double* q) {
  for (int64_t i = 0; i < n; ++i) q[i] = mpc::trig::tan_small_q(beta[i] * beta[i]);
}

// device_consts: the problem constants as the DEVICE derives them from a
// problem (consts_from_problem, mpc_device.h: the episode entries and the
// batched entry) instead of the one-shot entries' host derivation
// (host_consts, mpc_host_consts.h).  Both are the library's own functions.
static mpc::Consts problem_consts(const mpc_problem_t& p, bool device_consts) {
  return device_consts ? mpc::consts_from_problem(p) : mpc::host_consts(p);
}

static int rollout_impl(const mpc_problem_t* p, const double* v, const double* b, int64_t n_cand,
                        int32_t n_steps, int32_t integ, bool device_consts, double* states,
                        double* costs) {
  const mpc::Consts K = problem_consts(*p, device_consts);
  const bool rot = (integ & MPC_HEADING_ROTATE) != 0;
  const bool cum = (integ & MPC_HEADING_CUMULATIVE) != 0;
  const int ig = integ & 0xff;
  double traj[3 * MPC_MAX_STEPS];
  for (int64_t c = 0; c < n_cand; ++c) {
    double cst;
    if (ig == MPC_INTEG_RECT && cum)
      cst = mpc::rollout_candidate<MPC_INTEG_RECT, mpc::kRotCum>(K, v, b, n_cand, c, n_steps, traj);
    else if (ig == MPC_INTEG_RECT)
      cst = rot ? mpc::rollout_candidate<MPC_INTEG_RECT, 1>(K, v, b, n_cand, c, n_steps, traj)
                : mpc::rollout_candidate<MPC_INTEG_RECT, 0>(K, v, b, n_cand, c, n_steps, traj);
    else
      cst = rot ? mpc::rollout_candidate<MPC_INTEG_QK21, 1>(K, v, b, n_cand, c, n_steps, traj)
                : mpc::rollout_candidate<MPC_INTEG_QK21, 0>(K, v, b, n_cand, c, n_steps, traj);
    if (states)
      for (int s = 0; s < n_steps; ++s)
        for (int k = 0; k < 3; ++k) states[(s * 3 + k) * n_cand + c] = traj[3 * s + k];
    if (costs) costs[c] = cst;
  }
  return 0;
}

extern "C" int replica_rollout(const mpc_problem_t* p, const double* v, const double* b,
                               int64_t n_cand, int32_t n_steps, int32_t integ, double* states,
                               double* costs) {
  return rollout_impl(p, v, b, n_cand, n_steps, integ, false, states, costs);
}

extern "C" int replica_rollout_device_consts(const mpc_problem_t* p, const double* v,
                                             const double* b, int64_t n_cand, int32_t n_steps,
                                             int32_t integ, double* states, double* costs) {
  return rollout_impl(p, v, b, n_cand, n_steps, integ, true, states, costs);
}

// The sums (A, B) of the rect+cum recurrence after every step — what a lane
// hook's loop() is handed (tests/test_ranking_polygons_gpu.py: the keep-out
// polygons' frame table is evaluated on them), scaled by 1/L when L is a power
// of two — and the candidate's `bad` flag (its states then come from step_safe
// and the hook tests those).  rollout_candidate_l's own loop, which keeps only
// what cum_pose makes of the sums.  sums: [n_steps][2][n_cand].
template <bool PL2>
static void cum_sums(const mpc::Consts& K, const double* v, const double* b, int64_t n_cand,
                     int32_t n_steps, double* sums, uint8_t* bad_out) {
  for (int64_t col = 0; col < n_cand; ++col) {
    double x, y, ph, s, c;
    mpc::step_start<mpc::kRotCum>(K, x, y, ph, s, c);
    bool bad = false;
    for (int st = 0; st < n_steps; ++st) {
      mpc::step_core<MPC_INTEG_RECT, mpc::kRotCum, PL2>(x, y, ph, s, c, v[st * n_cand + col],
                                                        b[st * n_cand + col], K, bad);
      sums[(st * 2 + 0) * n_cand + col] = x;
      sums[(st * 2 + 1) * n_cand + col] = y;
    }
    bad_out[col] = bad ? 1 : 0;
  }
}

extern "C" void replica_cum_sums(const mpc_problem_t* p, const double* v, const double* b,
                                 int64_t n_cand, int32_t n_steps, double* sums, uint8_t* bad_out) {
  const mpc::Consts K = mpc::host_consts(*p);
  if (K.L_pow2)
    cum_sums<true>(K, v, b, n_cand, n_steps, sums, bad_out);
  else
    cum_sums<false>(K, v, b, n_cand, n_steps, sums, bad_out);
}

// ---------------------------------------------------------------------------
// The full tree (mpc_ftdevice.h): every leaf's cost in leaf order
// j = (k0 * S1 + k1) * S1 + k2, by the functions the kernels run.
#include <vector>

#include "../diplomjourney_amd/csrc/mpc_ftdevice.h"

template <int INTEG, bool ROT>
static void fulltree_leaves(const mpc::Consts& K, const mpc::FtCrit& F,
                            const std::vector<mpc::FtCtl>& ctl, double* costs,
                            const int64_t* leaves, int64_t n_leaves, double* traj) {
  const int64_t s1 = static_cast<int64_t>(ctl.size());
  const mpc::FtState s0{K.x, K.y, K.phi, K.s0, K.c0};
  if (costs) {
    int64_t j = 0;
    for (int64_t k0 = 0; k0 < s1; ++k0) {
      const mpc::FtState l0 = mpc::ft_apply<INTEG, ROT>(s0, ctl[k0], K);
      for (int64_t k1 = 0; k1 < s1; ++k1) {
        const mpc::FtState l1 = mpc::ft_apply<INTEG, ROT>(l0, ctl[k1], K);
        for (int64_t k2 = 0; k2 < s1; ++k2) {
          const mpc::FtState lf = mpc::ft_apply<INTEG, ROT>(l1, ctl[k2], K);
          costs[j++] = mpc::cost_fulltree(lf.x, lf.y, lf.ph, F);
        }
      }
    }
  }
  for (int64_t n = 0; n < n_leaves; ++n, traj += 9) {   // k_ft_finalize's re-derivation
    const int64_t leaf = leaves[n];
    if (leaf < 0 || leaf >= s1 * s1 * s1) continue;
    const int64_t kk[3] = {leaf / (s1 * s1), (leaf / s1) % s1, leaf % s1};
    mpc::FtState st = s0;
    for (int l = 0; l < 3; ++l) {
      st = mpc::ft_apply<INTEG, ROT>(st, ctl[kk[l]], K);
      traj[3 * l] = st.x;
      traj[3 * l + 1] = st.y;
      traj[3 * l + 2] = st.ph;
    }
  }
}

template <int INTEG>
static int fulltree_impl(const mpc_fulltree_problem_t* p, const double* V, int32_t nv,
                         const double* B, int32_t nb, bool want_rot, bool device_consts,
                         double* costs, int32_t* no_rot, const int64_t* leaves, int64_t n_leaves,
                         double* traj) {
  const mpc_problem_t q{p->x, p->y, p->phi, p->x_t, p->y_t, p->x_0, p->y_0, p->L, p->t_a, p->t_b};
  const mpc::Consts K = problem_consts(q, device_consts);
  // the control table's constants: the one-shot entry's are the problem's; the
  // batched entry derives window-only ones on the host (mpc_fulltree_argmin_batched)
  const mpc::Consts Kw = device_consts ? mpc::host_window_consts(p->L, p->t_a, p->t_b) : K;
  const int64_t s1 = static_cast<int64_t>(nv) * nb;
  std::vector<mpc::FtCtl> ctl(static_cast<size_t>(s1));
  bool over = false;   // the launch-wide flag *no_rot
  for (int64_t k = 0; k < s1; ++k) {
    // k_ft_controls (mpc_fulltree.h), its body from `FtCtl u` to `ctl[k] = u`,
    // with K = Kw: factored into a shared function the kernel's code changed,
    // so the lines are repeated here
    mpc::FtCtl u;
    u.v = V[k / nb];
    u.beta = B[k % nb];
    u.vh = u.v * Kw.h;
    const double w = Kw.L_pow2 ? u.v * Kw.inv_L : u.v / Kw.L;
    u.dphi = mpc::heading_incr<INTEG>(w, mpc::trig::tan_fast(u.beta), Kw);
    if (fabs(u.dphi) <= mpc::trig::kRotMax) {
      mpc::trig::rotation_sc(u.dphi, u.sd, u.cd);
    } else {
      u.sd = u.cd = 0.0;
      over = true;
    }
    ctl[k] = u;
  }
  if (no_rot) *no_rot = over ? 1 : 0;
  const mpc::FtCrit F = mpc::ft_crit(K, p->atan_target);
  if (want_rot && !over)   // the kernels' `ROT && *no_rot == 0u`
    fulltree_leaves<INTEG, true>(K, F, ctl, costs, leaves, n_leaves, traj);
  else
    fulltree_leaves<INTEG, false>(K, F, ctl, costs, leaves, n_leaves, traj);
  return 0;
}

// costs: S1^3 doubles or null; no_rot: the flag; traj: 9 doubles per entry of
// `leaves`, which receive that leaf's three layer states (x, y, phi).
extern "C" int replica_fulltree(const mpc_fulltree_problem_t* p, const double* V, int32_t nv,
                                const double* B, int32_t nb, int32_t integ, int32_t device_consts,
                                double* costs, int32_t* no_rot, const int64_t* leaves,
                                int64_t n_leaves, double* traj) {
  if (integ & MPC_HEADING_CUMULATIVE) return 1;
  const bool rot = (integ & MPC_HEADING_ROTATE) != 0;
  if ((integ & 0xff) == MPC_INTEG_RECT)
    return fulltree_impl<MPC_INTEG_RECT>(p, V, nv, B, nb, rot, device_consts != 0, costs, no_rot,
                                         leaves, n_leaves, traj);
  return fulltree_impl<MPC_INTEG_QK21>(p, V, nv, B, nb, rot, device_consts != 0, costs, no_rot,
                                       leaves, n_leaves, traj);
}

// ---------------------------------------------------------------------------
// The device-resident episode's state (mpc_episode.h) for tests/episode_state.py
// and tests/episode_model.py: the layout of its structs as this compiler lays
// them out, and the two host-buildable functions the episode's bookkeeping
// takes its constants and its restart incumbent from.  Only the struct
// definitions of mpc_episode.h are used: no device function is called.
#include <stddef.h>

// (mpc_episode.h also defines one kernel, k_episode_reset.  A host-only build
// has no device image for a kernel's launch stub to register, so here it is
// parsed as an ordinary device function, which the host build does not emit.
// The macro is the HIP headers' own, already defined by the includes above,
// and is put back right after this one include.)
#include <hip/hip_runtime.h>
#pragma push_macro("__global__")
#undef __global__
#define __global__ __device__
#include "../diplomjourney_amd/csrc/mpc_episode.h"
// (mpc_episodes.h: the batched robots' RobotState, for its layout alone; its
// two kernels and those of the headers it includes are parsed the same way,
// without their launch bounds, which only a kernel may carry.  The price:
// mpc_episodes.h and everything it includes (mpc_argmin.h, mpc_generated.h,
// mpc_lanes.h, mpc_sampler.h, mpc_winner.h) are now part of EVERY build of
// this harness, so a construct in one of them that the host pass cannot
// parse breaks all replica tests, not only the RobotState layout check.  If
// that happens, move this include and replica_robot_layout into a harness of
// their own rather than weaken the header.)
#pragma push_macro("__launch_bounds__")
#undef __launch_bounds__
#define __launch_bounds__(...)
#include "../diplomjourney_amd/csrc/mpc_episodes.h"
#pragma pop_macro("__launch_bounds__")
#pragma pop_macro("__global__")

// out[0..8): sizeof(RobotState), offsetof of h, st, stop, calls, candidates,
// sizeof(mpc_episode_config_t), episodes_cfg_offset(1) (check_robot_layout of
// tests/episode_state.py states the same order).  Kept apart from
// replica_episode_layout, whose value count tests/test_episode_model_cpu.py pins.
extern "C" void replica_robot_layout(int64_t* out) {
  using namespace mpc;
  out[0] = sizeof(RobotState);
  out[1] = offsetof(RobotState, h);
  out[2] = offsetof(RobotState, st);
  out[3] = offsetof(RobotState, stop);
  out[4] = offsetof(RobotState, calls);
  out[5] = offsetof(RobotState, candidates);
  out[6] = sizeof(mpc_episode_config_t);
  out[7] = static_cast<int64_t>(episodes_cfg_offset(1));
}

// out[0..n): sizeof of EpisodeHead, StaleTraj, EarlyPub, EpisodeState, Consts;
// offsetof of every field of Consts, EpisodeHead, StaleTraj, EarlyPub,
// EpisodeState, each in declaration order; kEpMaxGrid, kPubWords,
// kStoredWords; last, the number of values before it (layout_names() of
// tests/episode_state.py states the same order).
extern "C" void replica_episode_layout(int64_t* out, int32_t n) {
  using namespace mpc;
#define OFF(S, f) static_cast<int64_t>(offsetof(S, f))
  const int64_t v[] = {
      sizeof(EpisodeHead), sizeof(StaleTraj), sizeof(EarlyPub), sizeof(EpisodeState),
      sizeof(Consts),
      OFF(Consts, x), OFF(Consts, y), OFF(Consts, phi), OFF(Consts, x_t), OFF(Consts, y_t),
      OFF(Consts, x_0), OFF(Consts, y_0), OFF(Consts, A), OFF(Consts, B), OFF(Consts, C1),
      OFF(Consts, C2), OFF(Consts, inv_den), OFF(Consts, L), OFF(Consts, inv_L), OFF(Consts, h),
      OFF(Consts, hlgth), OFF(Consts, s0), OFF(Consts, c0), OFF(Consts, L_pow2),
      OFF(Consts, pad_),
      OFF(EpisodeHead, K), OFF(EpisodeHead, incumbent), OFF(EpisodeHead, x), OFF(EpisodeHead, y),
      OFF(EpisodeHead, phi), OFF(EpisodeHead, v), OFF(EpisodeHead, beta), OFF(EpisodeHead, x_t),
      OFF(EpisodeHead, y_t), OFF(EpisodeHead, x_0), OFF(EpisodeHead, y_0), OFF(EpisodeHead, t),
      OFF(EpisodeHead, seed), OFF(EpisodeHead, step), OFF(EpisodeHead, p), OFF(EpisodeHead, m),
      OFF(EpisodeHead, steps_for_slowing), OFF(EpisodeHead, episodes), OFF(EpisodeHead, nv),
      OFF(EpisodeHead, nb), OFF(EpisodeHead, recursive), OFF(EpisodeHead, has_traj),
      OFF(StaleTraj, ot), OFF(StaleTraj, v), OFF(StaleTraj, beta),
      OFF(EarlyPub, step), OFF(EarlyPub, k), OFF(EarlyPub, alt), OFF(EarlyPub, t),
      OFF(EarlyPub, h), OFF(EarlyPub, hl), OFF(EarlyPub, x), OFF(EarlyPub, y), OFF(EarlyPub, ph),
      OFF(EpisodeState, h), OFF(EpisodeState, st), OFF(EpisodeState, early),
      OFF(EpisodeState, grid_v), OFF(EpisodeState, grid_b), OFF(EpisodeState, done),
      OFF(EpisodeState, chain_error), OFF(EpisodeState, p2p_seq), OFF(EpisodeState, chain_pub),
      OFF(EpisodeState, gathered_tag),
      kEpMaxGrid, kPubWords, kStoredWords};
#undef OFF
  const int32_t count = static_cast<int32_t>(sizeof(v) / sizeof(v[0]));
  for (int32_t i = 0; i < n && i < count; ++i) out[i] = v[i];
  if (n > count) out[count] = count;
}

// consts_from_problem (mpc_device.h), raw bytes: sizeof(Consts) at consts_out.
extern "C" void replica_consts(const mpc_problem_t* p, void* consts_out) {
  const mpc::Consts K = mpc::consts_from_problem(*p);
  memcpy(consts_out, &K, sizeof(K));
}

// cost (mpc_device.h) of (x, y) under the constants replica_consts wrote.
extern "C" double replica_cost(const void* consts, double x, double y) {
  mpc::Consts K;
  memcpy(&K, consts, sizeof(K));
  return mpc::cost(x, y, K);
}
