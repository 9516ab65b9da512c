// mpc_episodes_obs_launch.h — the launch of k_episodes_run with keep-out
// circles, declared for mpc_rollout.hip and defined in mpc_episodes_obs.hip, a
// translation unit of its own: with the circle instantiations in
// mpc_rollout.hip's, hipcc allocated the registers of the plain
// k_episodes_run<RECT, 0> and <RECT, 1> differently although no statement of
// theirs changed (tools/kernel_digest.py), and the plain kernels
// are to stay what was measured.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_device.h"
#include "mpc_episodes.h"

namespace mpc {

// k_episodes_run<mode of `integrator`, its hook for dispatch_nobs<true>(n_obs)> on st,
// one block per robot; every argument checked by the caller (episodes_run).
void launch_episodes_run_obs(hipStream_t st, int32_t integrator, const Obstacles& world, int n_obs,
                             int n_robots, const mpc_episode_config_t* cfgs, RobotState* robots,
                             int n_steps, int max_calls, mpc_episode_log_t* log, int cap,
                             mpc_episodes_progress_t* progress, int64_t* n_blocked);

}  // namespace mpc
