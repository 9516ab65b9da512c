// mpc_episodes_obs.hip — the second translation unit of libmpc_rollout.so: the
// circle instantiations of the batched robots' episode kernel (k_episodes_run,
// mpc_episodes.h, with the hooks of mpc_episodes_obs.h) and their launch, and
// the fleet instantiations of the same kernel (the hooks of mpc_episodes_fleet.h:
// FleetObs, FleetMotionObs for the predicted fleet call and FleetPlanObs for the
// planned one), the kernels that fill the pose board and the plan board's side
// 0, and their launches; and the full tree's leaf kernels with circles
// (mpc_fulltree_obs.h) with theirs.  The entries, their
// checks and the plain instantiations stay in mpc_rollout.hip (episodes_run,
// episodes_fleet_run); why the two are compiled apart: mpc_episodes_obs_launch.h.
// (the headers' plain, non-template kernels are mpc_rollout.hip's: one definition
// per library)
#define MPC_TEMPLATES_ONLY
#include "mpc_episodes_obs_launch.h"

#include "mpc_dispatch.h"
#include "mpc_episodes_fleet.h"
#include "mpc_episodes_obs.h"
#include "mpc_fulltree_obs.h"

namespace mpc {

void launch_episodes_run_obs(hipStream_t st, int32_t integrator, const Obstacles& world, int n_obs,
                             int n_robots, const mpc_episode_config_t* cfgs, RobotState* robots,
                             int n_steps, int max_calls, mpc_episode_log_t* log, int cap,
                             mpc_episodes_progress_t* progress, int64_t* n_blocked) {
  dispatch_mode(integrator, [&](auto I, auto R) {
    dispatch_nobs<true>(n_obs, [&](auto NOBS) {
      k_episodes_run<I, R, EpisodesObs<R, NOBS>, Obstacles><<<n_robots, kBlock, 0, st>>>(
          world, cfgs, robots, n_steps, max_calls, log, cap, progress, n_blocked);
    });
  });
}

void launch_fleet_begin(hipStream_t st, const RobotState* robots, int n_robots, FleetPos* board) {
  k_fleet_begin<<<(n_robots + 255) / 256, 256, 0, st>>>(robots, n_robots, board);
}

void launch_episodes_fleet(hipStream_t st, int32_t integrator, const FleetArgs& A, int n_robots,
                           const mpc_episode_config_t* cfgs, RobotState* robots, int n_steps,
                           mpc_episode_log_t* log, int cap, mpc_episodes_progress_t* progress,
                           int64_t* n_blocked) {
  dispatch_mode(integrator, [&](auto I, auto R) {
    k_episodes_run<I, R, FleetObs<R>, FleetArgs><<<n_robots, kBlock, 0, st>>>(
        A, cfgs, robots, n_steps, 1, log, cap, progress, n_blocked);
  });
}

void launch_episodes_fleet_predicted(hipStream_t st, int32_t integrator, const FleetMotionArgs& A,
                                     int n_robots, const mpc_episode_config_t* cfgs,
                                     RobotState* robots, mpc_episode_log_t* log, int cap,
                                     mpc_episodes_progress_t* progress, int64_t* n_blocked) {
  dispatch_mode(integrator, [&](auto I, auto R) {
    k_episodes_run<I, R, FleetMotionObs<R>, FleetMotionArgs><<<n_robots, kBlock, 0, st>>>(
        A, cfgs, robots, A.n_steps, 1, log, cap, progress, n_blocked);
  });
}

void launch_fleet_plan_begin(hipStream_t st, const FleetPos* board, int n_robots, FleetPlan* plan) {
  k_fleet_plan_begin<<<(n_robots + 255) / 256, 256, 0, st>>>(board, n_robots, plan);
}

void launch_episodes_fleet_planned(hipStream_t st, int32_t integrator, const FleetPlanArgs& A,
                                   int n_robots, const mpc_episode_config_t* cfgs,
                                   RobotState* robots, mpc_episode_log_t* log, int cap,
                                   mpc_episodes_progress_t* progress, int64_t* n_blocked) {
  dispatch_mode(integrator, [&](auto I, auto R) {
    k_episodes_run<I, R, FleetPlanObs<R>, FleetPlanArgs><<<n_robots, kBlock, 0, st>>>(
        A, cfgs, robots, A.n_steps, 1, log, cap, progress, n_blocked);
  });
}

// The full tree with circles (mpc_fulltree_obs.h): the reach radii of the call's
// control table, then the leaf kernel of the plain entry's grid.
void launch_ft_leaves_obs(hipStream_t st, int32_t integrator, const Obstacles& world, int n_obs,
                          const Consts& K, double atan_t, const FtCtl* ctl, const uint32_t* no_rot,
                          double* reach2, int64_t s1, int64_t u_lo, int64_t u_hi, int64_t grid,
                          Rec* part, int64_t* n_blocked) {
  k_ft_reach<<<1, 64, 0, st>>>(world, ctl, s1, n_obs, reach2);
  dispatch_integ_rot(integrator, [&](auto I, auto R) {
    k_ft_leaves_obs<I, R><<<static_cast<unsigned>(grid), kBlock, 0, st>>>(
        world, K, atan_t, ctl, no_rot, reach2, n_obs, s1, u_lo, u_hi, part, n_blocked);
  });
}

void launch_ft_leaves_batched_obs(hipStream_t st, int32_t integrator, const Obstacles& world,
                                  int n_obs, const FtRobot* robots, int n_robots,
                                  const FtCtl* ctl, const uint32_t* no_rot, double* reach2,
                                  int64_t s1, int64_t blocks_per_robot, Rec* part,
                                  int64_t* n_blocked) {
  k_ft_reach<<<1, 64, 0, st>>>(world, ctl, s1, n_obs, reach2);
  dispatch_integ_rot(integrator, [&](auto I, auto R) {
    k_ft_leaves_batched_obs<I, R>
        <<<dim3(static_cast<unsigned>(blocks_per_robot), n_robots), kBlock, 0, st>>>(
            world, robots, ctl, no_rot, reach2, n_obs, s1, part, n_blocked);
  });
}

void launch_ftl_leaves_obs(hipStream_t st, int32_t integrator, const Obstacles& world, int n_obs,
                           const FtLockstep* ls, const FtCtl* ctl, const int32_t* live,
                           const FtRobot* robots, double* reach2, int64_t s1, int grid, Rec* part,
                           int64_t* n_blocked) {
  // (a call without a live robot leaves the table of the last one: reach radii
  // nobody reads)
  k_ft_reach<<<1, 64, 0, st>>>(world, ctl, s1, n_obs, reach2);
  dispatch_integ_rot(integrator, [&](auto I, auto R) {
    k_ftl_leaves_obs<I, R><<<grid, kBlock, 0, st>>>(world, ls, ctl, live, robots, reach2, n_obs,
                                                    s1, part, n_blocked);
  });
}

#ifdef MPC_TIMELINE
const void* fleet_timeline_table(size_t* bytes) {
  *bytes = sizeof(g_tl_ep);
  return &g_tl_ep;
}
#endif

}  // namespace mpc
