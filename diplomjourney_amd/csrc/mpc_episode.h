// mpc_episode.h — device-resident MPC episode, its data and its update: the
// reference's math_mpc loop (math_model_tree.py:515-635) with its state in
// HBM, so that an MPC step is enqueued without a host round-trip (gfx950).
//
//   EpisodeHead, StaleTraj, EarlyPub, EpisodeHook, k*Words   the scalars, as staged in LDS
//   log_slot, early_pose_ok  (used by the update and by mpc_finalize.h)
//   EpisodeState             head + sampler grids + the launches' hand-off words
//   episode_consts, episode_restart, episode_seed, episode_prepare,
//   episode_early_prepare, k_episode_reset   start of an episode / of a step
//   turn_target, episode_advance, episode_hook   the update after a step's winner
//
// The episode update mirrors diplomjourney_amd/episode.py Episode._advance:
// finishing logic (:392-414), operator events (:564-569), arrival restart.
// Who calls it: k_finalize<..., KDEV> (mpc_finalize.h, one GPU),
// k_episode_advance* and the mailbox exchange (mpc_exchange.h, multi-GPU),
// k_episode_chain (mpc_chain.h).  The step's sampler: mpc_generated.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_device.h"
#include "mpc_timeline.h"
#include "mpc_winner.h"

namespace mpc {

// The device-resident episode's scalars (EpisodeState, below = this head + the
// sampler grids).
struct EpisodeHead {
  Consts K;            // this step's problem constants
  double incumbent;    // optimal_criterion at the start of this step
  double x, y, phi, v, beta;
  double x_t, y_t, x_0, y_0;
  double t;
  uint64_t seed;       // this step's sampler seed
  int64_t step;
  int32_t p, m, steps_for_slowing, episodes;
  int32_t nv, nb;
  // math_mpc's stuck detector (:559-563); x_previous / y_previous (:540-541,
  // :570-571) are always the pose the step starts from, (x, y) above
  int32_t recursive;
  int32_t has_traj;    // optimal_trajectory holds a winner (not the initial [[[0]]])
};

// The module globals optimal_trajectory[0] (layer states 0..2), result_v,
// result_beta: what a step in which no candidate beats the incumbent returns
// (stale: :351-359 not taken; the post-processing :366-429 as usual).  Stored
// right after the head in HBM and staged with it in LDS; the update reads and
// writes it there (a register copy of head + trajectory would not fit
// thread 0's registers and lands in scratch).
struct StaleTraj {
  double ot[3][3];
  double v, beta;
};

// What a chained step's early publication needs of the update it makes,
// formed when the previous step's update is done (episode_early_prepare):
// the finishing layer k when the step can only be a common one (no event,
// break or limit; -1 otherwise), the next step's t and step sizes, and the
// pose a step without winner returns (stale layer k, or the pose) and whether
// it passes the end-of-step checks.  `step`: the head's
// step count it was formed for (a step completed by another path leaves it
// stale, and the next chained step then publishes after its update).
// Stored right after StaleTraj, staged with the head.
struct EarlyPub {
  int64_t step;
  int32_t k, alt;
  double t, h, hl;
  double x, y, ph;   // (its sin / cos are evaluated when used: a step without winner is rare)
};

struct EpisodeHook {  // single-GPU episode: finalize also advances it
  EpisodeHead* H;     // nullptr: no hook
  mpc_episode_log_t* log;
  int cap;
  uint64_t* chain_pub = nullptr;   // cleared with the update (ends a chain of chained steps) ...
  int chain_pub_words = 0;
  uint32_t publish_epoch = 0;      // ... or, nonzero, the next step's constants published
  uint32_t* chain_error = nullptr; // (publish_epoch: the early publication's self-check, code 6)
};
constexpr int kHeadWords = static_cast<int>(sizeof(EpisodeHead) / 8);
constexpr int kStaleWords = static_cast<int>(sizeof(StaleTraj) / 8);
constexpr int kEarlyWords = static_cast<int>(sizeof(EarlyPub) / 8);
constexpr int kStoredWords = kHeadWords + kStaleWords;   // head + stale trajectory
constexpr int kStagedWords = kStoredWords + kEarlyWords; // ... + the early-publication inputs
static_assert(kStagedWords <= 64, "staged head: one word per lane");
constexpr int kLogWords = static_cast<int>(sizeof(mpc_episode_log_t) / 8);
static_assert(sizeof(EpisodeHead) % 8 == 0 && kHeadWords <= 64, "head: one word per lane");
static_assert(sizeof(mpc_episode_log_t) % 8 == 0 && kLogWords <= 64, "log: one word per lane");

__device__ __forceinline__ mpc_episode_log_t* log_slot(mpc_episode_log_t* log, int cap,
                                                       int64_t step) {
  return (log && cap > 0) ? &log[step % cap] : nullptr;
}

// The end-of-step checks of a candidate next pose that episode_advance makes
// after the events (none in the early publication's steps): the
// run_math_model stuck break (:266-272) and the arrival (:542).
__device__ __forceinline__ bool early_pose_ok(const mpc_episode_config_t& c, const EpisodeHead& H,
                                              double x, double y) {
  if (c.stop_rule == 1 && x == H.x && y == H.y && H.recursive >= 1) return false;
  const double ex = H.x_t - x, ey = H.y_t - y;
  return !(ex * ex + ey * ey <= c.eps);
}

constexpr int kEpMaxGrid = 64;

constexpr int kConstsWords = static_cast<int>(sizeof(Consts) / 4);
constexpr int kPubWords = kConstsWords + 2;   // Consts, then t
static_assert(sizeof(Consts) % 4 == 0 && kPubWords <= 64, "published words: one wave");

// EpisodeHead: the scalars; the grids only feed the sampler.
// The stale trajectory follows the head (staged and stored with it as one
// run of kStoredWords words), then the early-publication inputs (staged with
// both by a chained step's block 0: kStagedWords).
struct EpisodeState {
  EpisodeHead h;
  StaleTraj st;        // right after the head: staged and stored with it
  EarlyPub early;      // right after the stale trajectory: staged with both
  double grid_v[kEpMaxGrid];
  double grid_b[kEpMaxGrid];
  uint32_t done;       // blocks of the running fused launch that have finished
  uint32_t chain_error;   // a chained step's wait timed out (k_episode_chain)
  // P2P exchange: completions so far; completion c uses mailbox slot c & 1.
  // Counted on the device (every rank completes the same steps), not taken
  // from the launch's epoch: a replayed HIP graph repeats its epochs, and a
  // captured sequence of odd length would start its next replay in the slot
  // its flush was still reading on a slower rank.
  uint32_t p2p_seq;
  // Constants published by a chained launch's block 0 (k_episode_chain): the
  // dwords of the step's Consts and of t, each in a 64-bit word tagged with
  // the launch's epoch ((dword << 32) | epoch), so one coherent load per word
  // says whether its value is this step's.  Tag 0: none.
  alignas(128) uint64_t chain_pub[kPubWords];
  // Overlapped exchange (mpc_episode_exchange_step2 with wait_tag): the epoch
  // of the step whose candidates the last all_gather delivered, stored by
  // k_exchange_mark on the collective's stream after the collective; block 0
  // of the next launch polls it instead of the launch waiting on a stream edge.
  alignas(128) uint64_t gathered_tag;
};
static_assert(offsetof(EpisodeState, st) == sizeof(EpisodeHead), "stale trajectory follows the head");
static_assert(offsetof(EpisodeState, early) == kStoredWords * 8, "EarlyPub follows the stale trajectory");

__device__ inline Consts episode_consts(const EpisodeHead& S, double x, double y, double phi,
                                        double L, double t_a, double t_b) {
  mpc_problem_t p;
  p.x = x;
  p.y = y;
  p.phi = phi;
  p.x_t = S.x_t;
  p.y_t = S.y_t;
  p.x_0 = S.x_0;
  p.y_0 = S.y_0;
  p.L = L;
  p.t_a = t_a;
  p.t_b = t_b;
  return consts_from_problem(p);
}

// Episode.reset() / math_mpc's prologue (:521-541): start pose, target, line
// origin at the start, t = 0, p = 1, m = 0 (the script resets m between its
// two runs, :737), recursive = False;
// incumbent = cfg.incumbent0, or control_criterion of the line origin with
// the episode's target (the reference's first optimal_criterion is that of
// config.py's target, :676).  optimal_trajectory / result_v / result_beta
// are module globals the reference never resets: they carry over.
__device__ inline void episode_restart(const mpc_episode_config_t& c, EpisodeHead& S) {
  S.x = c.start_x;
  S.y = c.start_y;
  S.phi = c.start_phi;
  S.v = c.start_v;
  S.beta = c.start_beta;
  S.x_t = c.target_x;
  S.y_t = c.target_y;
  S.x_0 = c.start_x;
  S.y_0 = c.start_y;
  S.t = 0.0;
  S.p = 1;
  S.m = 0;
  S.steps_for_slowing = 0;
  S.episodes += 1;
  S.recursive = 0;
  if (c.incumbent0 != 0.0) {
    S.incumbent = c.incumbent0;
  } else {
    const Consts K0 = episode_consts(S, S.x_0, S.y_0, 0.0, c.L, 0.0, c.delta_t);
    S.incumbent = cost(S.x_0, S.y_0, K0);
  }
}

__device__ __forceinline__ uint64_t episode_seed(const mpc_episode_config_t& c,
                                                 const EpisodeHead& S) {
  return c.seed + 0x9E3779B9ull * static_cast<uint64_t>(S.p + 1000 * S.episodes);
}

// Start of an MPC step (math_mpc :302): t += dt, this step's problem
// constants (quad window [t, t+dt]) and sampler seed.  Run by reset and at
// the end of every advance, so a step's rollout needs no preparation launch.
__device__ inline void episode_prepare(const mpc_episode_config_t& c, EpisodeHead& S) {
  const double t = S.t + c.delta_t;
  S.K = episode_consts(S, S.x, S.y, S.phi, c.L, t, t + c.delta_t);
  S.t = t;
  S.seed = episode_seed(c, S);
}

// The head's early_* fields (EpisodeHead): the next step's early-publication
// inputs that do not depend on its winner — episode_advance's decisions
// (:559-569, :542 and the step limit) as far as the head alone fixes them,
// with st the stale trajectory the step will return without a winner.
__device__ inline void episode_early_prepare(const mpc_episode_config_t& c, const EpisodeHead& S,
                                             const StaleTraj& st, EarlyPub& E) {
  E.step = S.step;
  E.t = S.t + c.delta_t;
  E.h = (E.t + c.delta_t) - E.t;             // consts_from_problem
  E.hl = 0.5 * ((E.t + c.delta_t) - E.t);
  const bool common = !(c.stop_rule == 0 && S.recursive) && S.p != c.p_turn_right &&
                      S.p != c.p_turn_left && S.p != c.p_new_target &&
                      !(c.max_steps > 0 && S.p + 1 > c.max_steps);
  const int k = S.m == 2 ? 2 : (S.m == 1 ? 1 : 0);
  E.k = common ? k : -1;
  E.x = S.has_traj ? st.ot[k][0] : S.x;
  E.y = S.has_traj ? st.ot[k][1] : S.y;
  E.ph = S.has_traj ? st.ot[k][2] : S.phi;
  E.alt = early_pose_ok(c, S, E.x, E.y) ? 1 : 0;
}

#ifndef MPC_TEMPLATES_ONLY   // (a unit that is not mpc_rollout.hip: mpc_episodes_obs_launch.h)
__global__ void k_episode_reset(mpc_episode_config_t c, EpisodeState* __restrict__ S) {
  if (threadIdx.x != 0) return;
  EpisodeHead H = {};
  episode_restart(c, H);
  episode_prepare(c, H);
  EarlyPub E;
  episode_early_prepare(c, H, S->st, E);
  S->early = E;
  S->h = H;
  S->done = 0u;
  S->chain_error = 0u;
  S->p2p_seq = 0u;
  for (int q = 0; q < kPubWords; ++q) S->chain_pub[q] = 0ull;
  S->gathered_tag = 0ull;
}
#endif

// _turn_target (math_model_tree.py:142-215 sectors; sign = +1 left, -1 right).
__device__ inline void turn_target(double ax, double ay, double aphi, double d, double R,
                                   double sign, double& tx, double& ty) {
  const double pi = 3.141592653589793;
  double sn, cs;
  if (pi / 2 <= aphi && aphi <= 3 * pi / 2) {
    if (aphi <= pi) {
      trig::sincos_fast(aphi - pi / 2, &sn, &cs);
      tx = ax - sign * d * cs - R * sn;
      ty = ay - sign * d * sn + R * cs;
    } else {
      trig::sincos_fast(aphi - pi, &sn, &cs);
      tx = ax + sign * d * sn - R * cs;
      ty = ay - sign * d * cs - R * sn;
    }
  } else if (aphi <= 2 * pi) {
    trig::sincos_fast(aphi - 3 * pi / 2, &sn, &cs);
    tx = ax + sign * d * cs + R * sn;
    ty = ay + sign * d * sn - R * cs;
  } else {
    trig::sincos_fast(aphi, &sn, &cs);
    tx = ax - sign * d * sn + R * cs;
    ty = ay + sign * d * cs + R * sn;
  }
}

// Episode._advance = the rest of math_mpc's loop body after predictive_control
// (:542-574 with :351-429): the returned pose is the winner's layer state
// picked by the finishing logic (:392-414) — or, when no candidate beat the
// incumbent, the STALE optimal_trajectory / result_v / result_beta of the
// last improving step (the globals :351-359 did not touch), with the same
// finishing logic; then the stuck detector (:559-563: a pose equal to the
// previous one sets `recursive`, the next step with it set ends the episode
// before the events), the operator events (:564-569), p += 1, and the loop
// condition (:542: on target ends the episode).  An ended episode restarts
// (the bench's episode stream; the reference's loop returns).
// Operates on a register copy of the episode scalars (the caller loads it
// once and stores it back once).  The step's log record is filled in `L`
// (LDS); the caller stores it (log_slot) together with the head.
// RESTART = false (the batched robots of mpc_episodes.h): an ended episode
// stays ended (the caller stops the robot) instead of restarting.
// c.stop_rule 1: run_math_model.py's stuck detector instead of math_mpc's —
// `recursive` counts the episode's non-moving steps and the second one ends
// it at once (:266-272, before the on-target test of the loop head).
// early (a chained step's block 0 that published early, finalize_block):
// the next step's Consts and t as published (8-B aligned LDS words) — the
// step cannot end then, and the update takes t from them and leaves H.K to
// the caller (it stores the published words as the head's constants); a
// step that ends anyway sets *early_bad (chain error 6) and is prepared in
// full.
template <bool RESTART = true>
__device__ inline void episode_advance(const mpc_episode_config_t& c, EpisodeHead& H,
                                       StaleTraj& st, const Winner& r, mpc_episode_log_t& L,
                                       const uint32_t* early = nullptr,
                                       bool* early_bad = nullptr) {
  TL_B0(9);
  EpisodeHead* S = &H;
  S->steps_for_slowing -= 1;
  S->incumbent = 9223372036854775808.0;  // float(sys.maxsize), :428
  L.step = S->step;
  L.index = r.found ? r.index : -1;
  L.p = S->p;
  L.episode = S->episodes;
  L.found = r.found;
  L.cost = r.cost;
  int32_t status = 0;
  S->step += 1;
  if (r.found) {   // :352-359: the globals take the winner
    const int last = r.n_steps - 1;
    for (int k = 0; k < 3; ++k)
      for (int q = 0; q < 3; ++q) st.ot[k][q] = tr_at(r, k < last ? k : last, q);
    st.v = r.v;
    st.beta = r.beta;
    S->has_traj = 1;
  } else {
    status |= MPC_EP_STALE;
    if (!S->has_traj) {
      // the reference's initial optimal_trajectory [[[0]]] has no layer
      // states (it would raise IndexError): stay at the pose
      for (int k = 0; k < 3; ++k) {
        st.ot[k][0] = S->x;
        st.ot[k][1] = S->y;
        st.ot[k][2] = S->phi;
      }
      st.v = S->v;
      st.beta = S->beta;
    }
  }
  // finishing logic on optimal_trajectory[0] (:388-414): probe layer 2 (the
  // last layer for horizons < 3), return layer k
  int k = 0;
  if (S->m == 2) {
    k = 2;
  } else if (S->m == 1) {
    k = 1;
    S->m += 1;
  } else {
    const double ex = S->x_t - st.ot[2][0], ey = S->y_t - st.ot[2][1];
    if (ex * ex + ey * ey <= c.eps) S->m += 1;
  }
  TL_B0(10);
  const double x_prev = S->x, y_prev = S->y;   // x_previous / y_previous (:570-571)
  S->x = st.ot[k][0];   // (st lives in LDS: a dynamic index is an LDS address)
  S->y = st.ot[k][1];
  S->phi = st.ot[k][2];
  S->v = st.v;
  S->beta = st.beta;
  bool ended = false;
  if (c.stop_rule == 0 && S->recursive) {   // :559-561 "Recursive error." -> break
    status |= MPC_EP_BREAK;
    ended = true;
  } else if (S->x == x_prev && S->y == y_prev && c.stop_rule == 1 && S->recursive >= 1) {
    S->recursive += 1;                      // run_math_model.py:266-272: k == 2
    status |= MPC_EP_STUCK | MPC_EP_BREAK;
    ended = true;
  } else {
    if (S->x == x_prev && S->y == y_prev) {   // :562-563 (stop_rule 1: k += 1)
      S->recursive += 1;
      status |= MPC_EP_STUCK;
    }
    double tx, ty;
    if (S->p == c.p_turn_right) {
      turn_target(S->x, S->y, S->phi, c.turn_distance, c.radius_u_turn, -1.0, tx, ty);
      S->x_t = tx;
      S->y_t = ty;
      S->x_0 = S->x;
      S->y_0 = S->y;
      S->steps_for_slowing = c.slow_turn;
      status |= MPC_EP_EVENT;
    }
    if (S->p == c.p_turn_left) {
      turn_target(S->x, S->y, S->phi, c.turn_distance, c.radius_u_turn, +1.0, tx, ty);
      S->x_t = tx;
      S->y_t = ty;
      S->x_0 = S->x;
      S->y_0 = S->y;
      S->steps_for_slowing = c.slow_turn;
      status |= MPC_EP_EVENT;
    }
    if (S->p == c.p_new_target) {
      S->x_t = c.event_target_x;
      S->y_t = c.event_target_y;
      S->x_0 = S->x;
      S->y_0 = S->y;
      S->steps_for_slowing = c.slow_new_target;
      status |= MPC_EP_EVENT;
    }
    S->p += 1;
    const double ex = S->x_t - S->x, ey = S->y_t - S->y;
    if (ex * ex + ey * ey <= c.eps) {                   // :542
      status |= MPC_EP_ARRIVED;
      ended = true;
    } else if (c.max_steps > 0 && S->p > c.max_steps) {
      status |= MPC_EP_LIMIT;
      ended = true;
    }
  }
  L.x = S->x;
  L.y = S->y;
  L.phi = S->phi;
  L.v = S->v;
  L.beta = S->beta;
  L.status = status;
  TL_B0(6);
  if (ended) {
    if constexpr (!RESTART) return;
    episode_restart(c, *S);
  }
  TL_B0(11);
  if (early && (ended || reinterpret_cast<const Consts*>(early)->x != S->x ||
                reinterpret_cast<const Consts*>(early)->y != S->y ||
                reinterpret_cast<const Consts*>(early)->phi != S->phi))
    *early_bad = true;   // (never expected: the early decisions are this update's)
  if (early && !ended) {
    // K: the published words (= episode_prepare's; the caller stores them)
    S->t = *reinterpret_cast<const double*>(early + sizeof(Consts) / 4);
    S->seed = episode_seed(c, *S);
  } else {
    episode_prepare(c, *S);
  }
  TL_B0(12);
}

__device__ void episode_hook(const mpc_episode_config_t& c, const EpisodeHook& h,
                             const Winner& r, EpisodeHead& H, StaleTraj& st,
                             mpc_episode_log_t& L, mpc_episode_log_t*& slot,
                             const uint32_t* early, bool* early_bad) {
  slot = log_slot(h.log, h.cap, H.step);
  episode_advance(c, H, st, r, L, early, early_bad);
}

}  // namespace mpc
