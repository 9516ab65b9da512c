// mpc_episodes_obs.h — keep-out circles in the batched robots' device-resident
// episodes (mpc_episodes_run_obstacles; gfx950): which hook a mode's
// k_episodes_run<INTEG, ROT, Obs, Obstacles> (mpc_episodes.h, the one kernel
// with and without circles) takes, and how the kernel makes it.
//
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

template <int ROT, int NOBS>
using EpisodesObs = std::conditional_t<ROT == kRotCum, FrameObs<NOBS>, CircleObs<NOBS>>;

// The kernel's hook on the launch's table, kernel argument 0 (the overload is
// chosen by the hook's type; FrameObs: its world table, the frame table per step).
template <int NOBS>
__device__ __forceinline__ CircleObs<NOBS> episode_obs(CircleObs<NOBS>*) {
  return CircleObs<NOBS>{kernarg_world(), kernarg_world()};
}
template <int NOBS>
__device__ __forceinline__ FrameObs<NOBS> episode_obs(FrameObs<NOBS>*) {
  return FrameObs<NOBS>{kernarg_world()};
}

}  // namespace mpc
