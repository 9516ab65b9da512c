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

struct FtCtl;        // mpc_ftdevice.h
struct FtRobot;      // mpc_fulltree.h
struct FtLockstep;   // mpc_ftepisodes.h
struct Rec;          // mpc_argmin.h

// k_episodes_run<mode of `integrator`, its hook for dispatch_nobs<true>(n_obs)> on st,
// one block per robot; every argument checked by the caller (episodes_run).
void launch_episodes_run_obs(hipStream_t st, int32_t integrator, const Obstacles& world, int n_obs,
                             int n_robots, const mpc_episode_config_t* cfgs, RobotState* robots,
                             int n_steps, int max_calls, mpc_episode_log_t* log, int cap,
                             mpc_episodes_progress_t* progress, int64_t* n_blocked);

// The full tree's leaf kernels with circles (mpc_fulltree_obs.h), each after
// k_ft_reach on st: the launch of the plain entry's leaf kernel with the same
// grid, so the block records and everything after them are the plain entry's.
// reach2: MPC_MAX_OBSTACLES doubles of the call's workspace / state; n_blocked:
// nullable, zeroed by the caller.  Every argument checked by the caller.
void launch_ft_leaves_obs(hipStream_t st, int32_t integrator, const Obstacles& world, int n_obs,
                          const Consts& K, double atan_t, const FtCtl* ctl, const uint32_t* no_rot,
                          double* reach2, int64_t s1, int64_t u_lo, int64_t u_hi, int64_t grid,
                          Rec* part, int64_t* n_blocked);
void launch_ft_leaves_batched_obs(hipStream_t st, int32_t integrator, const Obstacles& world,
                                  int n_obs, const FtRobot* robots, int n_robots,
                                  const FtCtl* ctl, const uint32_t* no_rot, double* reach2,
                                  int64_t s1, int64_t blocks_per_robot, Rec* part,
                                  int64_t* n_blocked);
void launch_ftl_leaves_obs(hipStream_t st, int32_t integrator, const Obstacles& world, int n_obs,
                           const FtLockstep* ls, const FtCtl* ctl, const int32_t* live,
                           const FtRobot* robots, double* reach2, int64_t s1, int grid, Rec* part,
                           int64_t* n_blocked);

}  // namespace mpc
