// mpc_episodes_fleet_launch.h — the launches of a fleet call
// (mpc_episodes_fleet_begin / _run), declared for mpc_rollout.hip and defined
// in mpc_episodes_obs.hip, the library's second translation unit, for the
// reason mpc_episodes_obs_launch.h gives: the kernels mpc_rollout.hip
// instantiates are to stay what was measured.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_device.h"
#include "mpc_episodes.h"

namespace mpc {

// One robot's position on the pose board (16 B).
struct FleetPos {
  double x, y;
};
static_assert(sizeof(FleetPos) == 16, "the board: 16 B per robot per side");

// The board: two sides of n positions.  Fleet call c reads side c & 1 and
// writes side (c + 1) & 1; mpc_episodes_fleet_begin fills side 0.
inline size_t fleet_board_bytes(int n) { return 2 * static_cast<size_t>(n) * sizeof(FleetPos); }

// What one fleet launch reads besides the robots, kernel argument 0 (the
// static table first: kernarg_world() finds it there).
struct FleetArgs {
  Obstacles world;             // the static circles; r2 = -1 past n_static
  const FleetPos* board_in;    // this call's side: every robot's position at its start
  FleetPos* board_out;         // the other side: block r writes entry r on exit
  double r2;                   // clearance * clearance
  double reach2;               // reach * reach
  int32_t n_static;            // static circles
  int32_t n;                   // robots (board entries)
  int32_t* neighbours;         // [n][1 + MPC_MAX_OBSTACLES], or NULL
};

// A predicted fleet launch's arguments (mpc_episodes_fleet_run_predicted): the
// fleet launch's, first and unchanged — the plain fleet kernels keep their
// argument segment — then the motion board's sides, entries {dx, dy} with the
// pose board's layout and parity, and the horizon (select() forms one table
// per step).
struct FleetMotionArgs : FleetArgs {
  const FleetPos* motion_in;   // this call's side: every robot's last displacement
  FleetPos* motion_out;        // the other side: block r writes entry r on exit
  int32_t n_steps;             // the horizon N: tables for steps 1..N
};

// One robot's entry of the plan board (32 B): where it means to be after the
// next fleet call and after the one behind it — two layers of its StaleTraj,
// or its position twice if it stands (mpc_episodes_fleet_run_planned).
struct FleetPlan {
  double x1, y1, x2, y2;
};
static_assert(sizeof(FleetPlan) == 32, "the plan board: 32 B per robot per side");

// The plan board: two sides of n entries, the pose board's parity.
inline size_t fleet_plan_bytes(int n) { return 2 * static_cast<size_t>(n) * sizeof(FleetPlan); }

// A planned fleet launch's arguments (mpc_episodes_fleet_run_planned): the
// fleet launch's, first and unchanged, then the plan board's sides and the
// horizon, as FleetMotionArgs has the motion board's.
struct FleetPlanArgs : FleetArgs {
  const FleetPlan* plan_in;    // this call's side: every robot's next two plan points
  FleetPlan* plan_out;         // the other side: block r writes entry r on exit
  int32_t n_steps;             // the horizon N: tables for steps 1..N
};

// side 0 of the board from the robots' states
void launch_fleet_begin(hipStream_t st, const RobotState* robots, int n_robots, FleetPos* board);

// side 0 of the plan board from side 0 of the pose board: everybody stands
// (x, y, x, y), before planned fleet call 0
void launch_fleet_plan_begin(hipStream_t st, const FleetPos* board, int n_robots, FleetPlan* plan);

// k_episodes_run<mode of `integrator`, FleetObs> for ONE MPC step of every
// running robot (max_calls = 1), one block per robot; n_blocked[r] (or NULL) is
// added to.  Every argument checked by the caller (mpc_episodes_fleet_run).
void launch_episodes_fleet(hipStream_t st, int32_t integrator, const FleetArgs& A, int n_robots,
                           const mpc_episode_config_t* cfgs, RobotState* robots, int n_steps,
                           mpc_episode_log_t* log, int cap, mpc_episodes_progress_t* progress,
                           int64_t* n_blocked);

// The same with FleetMotionObs: one PREDICTED fleet call (A.motion_in / _out set).
void launch_episodes_fleet_predicted(hipStream_t st, int32_t integrator, const FleetMotionArgs& A,
                                     int n_robots, const mpc_episode_config_t* cfgs,
                                     RobotState* robots, mpc_episode_log_t* log, int cap,
                                     mpc_episodes_progress_t* progress, int64_t* n_blocked);

// The same with FleetPlanObs: one PLANNED fleet call (A.plan_in / _out set).
void launch_episodes_fleet_planned(hipStream_t st, int32_t integrator, const FleetPlanArgs& A,
                                   int n_robots, const mpc_episode_config_t* cfgs,
                                   RobotState* robots, mpc_episode_log_t* log, int cap,
                                   mpc_episodes_progress_t* progress, int64_t* n_blocked);

#ifdef MPC_TIMELINE
// The second unit's copy of workload R's phase table (mpc_timeline.h: a table is
// static to its translation unit), for mpc_debug_timeline(3, ...): the last
// fleet launch's phases, select() inside phase 0.
const void* fleet_timeline_table(size_t* bytes);
#endif

}  // namespace mpc
