// mpc_episodes_fleet.h — robots as each other's keep-out circles
// (mpc_episodes_fleet_begin / _run; gfx950): the hook k_episodes_run
// (mpc_episodes.h, the one kernel) takes for a fleet call, and the kernel that
// fills the pose board.
//
// A fleet call is ONE launch of k_episodes_run<INTEG, ROT, FleetObs<ROT>,
// FleetArgs> with max_calls = 1: every running robot takes one MPC step, and
// lockstep is the stream's order — no block waits for another, none reads what
// another writes in the same launch.  Call c reads side c & 1 of the board
// (every robot's position at the start of the call) and every block, stopped or
// not, writes its robot's position after the step to the other side.
//
// Robot r's table of the call, in LDS (FleetLds): the launch's static circles,
// then a circle (x_q, y_q, clearance) for each chosen neighbour — of the robots
// q != r with d2 = fleet_d2(r, q) < reach^2, the K = MPC_MAX_OBSTACLES -
// n_static smallest by (d2, q).  select() finds them in one pass over the board,
// kBlock entries at a time: the entries within reach are compacted (ballot and
// the waves' counts) behind the at most K kept so far, every entry of that list
// (at most K + kBlock) counts the entries below it — (d2 bits, q), a total
// order — and those of rank < K move to their rank.  What stays after the last
// chunk is the chosen set for every n and every crowding, in ascending order
// (neighbours_out wants it so), with no sort, no atomic and nothing that grows
// with the crowd; a chunk with nobody within reach costs one barrier.
//
// The rollout's hook reads the table as broadcast LDS operands (all lanes one
// address), in groups of kFleetGroup padded with r2 = -1, a runtime number of
// groups: the count m differs per robot and per call.  m = 0 is the kernel's
// business: it takes the NoObs pair rollout for that call (empty()).  rect+cum
// tests in the frame of the step's sums: form() makes the second table with
// frame_circle, as FrameObs does.
//
// FleetMotionObs, below: the hook of a predicted fleet call
// (mpc_episodes_fleet_run_predicted), the same selection with one table per
// horizon step, the neighbours' circles moved by their last displacement.
// FleetPlanObs, below it: the hook of a planned fleet call
// (mpc_episodes_fleet_run_planned), the same tables with the circles on the
// neighbours' own plans, read from a plan board.
#pragma once

#include "mpc_episode_obs.h"
#include "mpc_episodes.h"
#include "mpc_episodes_fleet_launch.h"

namespace mpc {

constexpr int kFleetGroup = 4;
constexpr int kFleetList = MPC_MAX_OBSTACLES + kBlock;   // kept so far + one chunk
constexpr int kFleetRow = 1 + MPC_MAX_OBSTACLES;         // neighbours_out per robot
static_assert(MPC_MAX_OBSTACLES % kFleetGroup == 0 && MPC_MAX_OBSTACLES <= 64, "table groups");

struct FleetLds {
  Circle world[MPC_MAX_OBSTACLES];   // static circles, then the chosen neighbours
  Circle frame[MPC_MAX_OBSTACLES];   // rect+cum: the same in the frame of the step's sums
  uint64_t key[kFleetList];          // d2's bits
  int32_t idx[kFleetList];           // the robot
  int32_t wcnt[2][kWaves];           // the waves' counts of a chunk (two chunks' turns)
};

__device__ __forceinline__ FleetLds* fleet_lds() {
  __shared__ FleetLds s_fleet;
  return &s_fleet;
}

__global__ void k_fleet_begin(const RobotState* __restrict__ robots, int n,
                              FleetPos* __restrict__ board) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) board[r] = FleetPos{robots[r].h.x, robots[r].h.y};
}

template <int ROT>
struct FleetObs {
  static constexpr bool kOn = true;
  static constexpr bool kFleet = true;
  uint32_t loop_at = 0, world_at = 0;   // LDS addresses of the tables
  int m = 0;                            // this call's circles (block-uniform)
  FleetPos first{0.0, 0.0};             // this thread's entry of the board's first chunk

  // The first chunk's load, issued when the kernel starts: it is in flight
  // while the head is staged, not waited for at the head of select().
  __device__ __forceinline__ void prefetch(const FleetArgs& A) {
    if (static_cast<int>(threadIdx.x) < A.n) first = A.board_in[threadIdx.x];
  }

  __device__ __forceinline__ bool empty() const { return m == 0; }
  __device__ __forceinline__ int groups() const { return (m + kFleetGroup - 1) / kFleetGroup; }

  // Robot r at (x, y): its table of this call.  Every thread of the block calls
  // it at the same point (barriers inside).
  __device__ __forceinline__ void select(const FleetArgs& A, int r, double x, double y) {
    FleetLds* S = fleet_lds();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n, n_static = A.n_static, keep = MPC_MAX_OBSTACLES - n_static;
    const FleetPos* __restrict__ in = A.board_in;
    const double reach2 = A.reach2;
    int len = 0, total = 0, turn = 0;   // (uniform: every thread counts the same)
    FleetPos p = first, next{0.0, 0.0};
    for (int base = 0; base < n; base += kBlock, turn ^= 1, p = next) {
      const int q = base + tid;
      // (the next chunk's entry is in flight over this chunk's barriers)
      if (q + kBlock < n) next = in[q + kBlock];
      bool near = false;
      double d2 = 0.0;
      if (q < n && q != r) {
        d2 = fleet_d2(x, y, p.x, p.y);
        near = d2 < reach2;
      }
      const uint64_t bal = __ballot(near);
      if (lane == 0) S->wcnt[turn][wave] = __popcll(bal);
      __syncthreads();
      int c = 0, before = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const int cw = S->wcnt[turn][w];
        c += cw;
        before += w < wave ? cw : 0;
      }
      total += c;
      if (c == 0 || keep == 0) continue;   // uniform (wcnt: the next chunk writes the other turn)
      if (near) {
        const int slot = len + before + __popcll(bal & ((1ull << lane) - 1ull));
        S->key[slot] = static_cast<uint64_t>(__double_as_longlong(d2));
        S->idx[slot] = q;
      }
      __syncthreads();
      const int e = len + c;   // <= keep + kBlock <= kFleetList
      uint64_t mk[2] = {0, 0};
      int32_t mi[2] = {0, 0};
      int rank[2] = {keep, keep};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = tid + h * kBlock;
        if (i < e) {
          mk[h] = S->key[i];
          mi[h] = S->idx[i];
          int below = 0;
          for (int j = 0; j < e; ++j) {
            const uint64_t kj = S->key[j];
            const int32_t ij = S->idx[j];
            below += (kj < mk[h] || (kj == mk[h] && ij < mi[h])) ? 1 : 0;
          }
          rank[h] = below;
        }
      }
      __syncthreads();   // every rank is counted before an entry moves
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (rank[h] < keep) {
          S->key[rank[h]] = mk[h];
          S->idx[rank[h]] = mi[h];
        }
      len = e < keep ? e : keep;
      __syncthreads();
    }
    m = n_static + len;
    if (tid < MPC_MAX_OBSTACLES) {
      Circle cq{0.0, 0.0, -1.0, 0.0};
      if (tid < n_static) {
        const ObsTable W = kernarg_world();
        cq = Circle{W->c[tid].cx, W->c[tid].cy, W->c[tid].r2, 0.0};
      } else if (tid < m) {
        const FleetPos p = in[S->idx[tid - n_static]];
        cq = Circle{p.x, p.y, A.r2, 0.0};
      }
      S->world[tid] = cq;
    }
    if (A.neighbours && tid < kFleetRow)
      A.neighbours[r * kFleetRow + tid] = tid == 0 ? total : (tid - 1 < len ? S->idx[tid - 1] : -1);
    __syncthreads();
  }

  // A robot that takes no step in this launch: nobody counted, nobody chosen.
  __device__ __forceinline__ static void no_step(const FleetArgs& A, int r) {
    if (A.neighbours && threadIdx.x < kFleetRow)
      A.neighbours[r * kFleetRow + threadIdx.x] = threadIdx.x == 0 ? 0 : -1;
  }

  // rect+cum: the table in the frame of the sums of the step that starts at K's
  // pose (every thread of the block, at the same point).
  __device__ __forceinline__ void form(const Consts& K, bool scaled) {
    FleetLds* S = fleet_lds();
    if (static_cast<int>(threadIdx.x) < groups() * kFleetGroup)
      S->frame[threadIdx.x] = frame_circle(K, S->world[threadIdx.x], scaled);
    __syncthreads();
  }

  template <int CPL>
  __device__ __forceinline__ static void test(uint32_t at, int n_groups, const double (&x)[CPL],
                                              const double (&y)[CPL], bool (&blocked)[CPL]) {
#if defined(__HIP_DEVICE_COMPILE__)
    const auto* t = (const __attribute__((address_space(3))) Circle*)at;
#else
    const Circle* t = nullptr;   // (the host pass only parses the kernels)
    (void)at;
#endif
    for (int g = 0; g < n_groups; ++g, t += kFleetGroup) {
#pragma unroll
      for (int i = 0; i < kFleetGroup; ++i) {
        const double cx = t[i].cx, cy = t[i].cy, r2 = t[i].r2;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          const double dx = x[j] - cx, dy = y[j] - cy;
          blocked[j] |= fma(dy, dy, dx * dx) < r2;
        }
      }
    }
  }
  template <int CPL>
  __device__ __forceinline__ void loop(const double (&x)[CPL], const double (&y)[CPL],
                                       bool (&blocked)[CPL]) const {
    test<CPL>(loop_at, groups(), x, y, blocked);
  }
  __device__ __forceinline__ void world(double x, double y, bool& blocked) const {
    const double xs[1] = {x}, ys[1] = {y};
    bool bl[1] = {blocked};
    test<1>(world_at, groups(), xs, ys, bl);
    blocked = bl[0];
  }
};

// The kernel's hook (mpc_episodes_obs.h has the circle modes'): the tables'
// addresses; select() fills them per call.
template <int ROT>
__device__ __forceinline__ FleetObs<ROT> episode_obs(FleetObs<ROT>*) {
  FleetLds* S = fleet_lds();
  FleetObs<ROT> o;
  o.world_at = lds_addr(S->world);
  o.loop_at = ROT == kRotCum ? lds_addr(S->frame) : o.world_at;
  return o;
}

// ---------------------------------------------------------------------------
// A predicted fleet call (mpc_episodes_fleet_run_predicted): each chosen
// neighbour's circle moves with the neighbour's last displacement, read from
// this call's side of the motion board.  The selection is FleetObs' own
// (positions at the start of the call); after it the block forms ONE TABLE PER
// HORIZON STEP in LDS — step j's (1..N) holds the static circles unmoved and
// each neighbour's circle at (fleet_predict(x, dx, j), fleet_predict(y, dy, j))
// — at a fixed stride of MPC_MAX_OBSTACLES circles, one entry per thread (a
// second pass when n_steps * groups * 4 > kBlock).  The lanes' test is
// FleetObs::test with the table's address advanced by the step's stride: the
// same broadcast operands, nothing more per lane and step.  rect+cum: form()
// makes every step's table in the frame of the call's sums.
constexpr uint32_t kFleetStepStride = MPC_MAX_OBSTACLES * sizeof(Circle);

struct FleetStepTable {
  Circle c[MPC_MAX_STEPS][MPC_MAX_OBSTACLES];
};

__device__ __forceinline__ FleetStepTable* fleet_step_world() {
  __shared__ FleetStepTable s_fleet_step_world;
  return &s_fleet_step_world;
}
__device__ __forceinline__ FleetStepTable* fleet_step_frame() {   // (rect+cum only)
  __shared__ FleetStepTable s_fleet_step_frame;
  return &s_fleet_step_frame;
}

template <int ROT>
struct FleetMotionObs : FleetObs<ROT> {
  static constexpr bool kMotion = true;   // (the kernel: the step index at the hook, the motion write)
  int entries = 0;                        // n_steps * groups * 4 (block-uniform)

  // FleetObs::select, then the per-step tables.  Entry e = (j - 1) * g4 + i:
  // circle i of step j.
  __device__ __forceinline__ void select(const FleetMotionArgs& A, int r, double x, double y) {
    FleetObs<ROT>::select(A, r, x, y);
    if (this->m == 0) {   // uniform: the call runs without circles
      entries = 0;
      return;
    }
    FleetLds* S = fleet_lds();
    FleetStepTable* T = fleet_step_world();
    const int g4 = this->groups() * kFleetGroup, n_static = A.n_static, m = this->m;
    entries = A.n_steps * g4;
    for (int e = threadIdx.x; e < entries; e += kBlock) {
      const int j = e / g4, i = e - j * g4;
      Circle cq = S->world[i];
      if (i >= n_static && i < m) {
        const FleetPos d = A.motion_in[S->idx[i - n_static]];
        cq.cx = fleet_predict(cq.cx, d.x, j + 1);
        cq.cy = fleet_predict(cq.cy, d.y, j + 1);
      }
      T->c[j][i] = cq;
    }
    __syncthreads();
  }

  __device__ __forceinline__ void form(const Consts& K, bool scaled) {
    FleetStepTable* T = fleet_step_world();
    FleetStepTable* F = fleet_step_frame();
    const int g4 = this->groups() * kFleetGroup;
    for (int e = threadIdx.x; e < entries; e += kBlock) {
      const int j = e / g4, i = e - j * g4;
      F->c[j][i] = frame_circle(K, T->c[j][i], scaled);
    }
    __syncthreads();
  }

  // st: the step's index from 0 (the state after step st + 1).
  template <int CPL>
  __device__ __forceinline__ void loop_step(int st, const double (&x)[CPL], const double (&y)[CPL],
                                            bool (&blocked)[CPL]) const {
    FleetObs<ROT>::template test<CPL>(this->loop_at + static_cast<uint32_t>(st) * kFleetStepStride,
                                      this->groups(), x, y, blocked);
  }
  __device__ __forceinline__ void world_step(int st, double x, double y, bool& blocked) const {
    const double xs[1] = {x}, ys[1] = {y};
    bool bl[1] = {blocked};
    FleetObs<ROT>::template test<1>(this->world_at + static_cast<uint32_t>(st) * kFleetStepStride,
                                    this->groups(), xs, ys, bl);
    blocked = bl[0];
  }

  // Block r's entry of the motion board's out side (one thread): the step's
  // displacement of a robot that goes on, zero of one that does not.
  __device__ __forceinline__ static void publish(const FleetMotionArgs& A, int r, bool moves,
                                                 double x0, double y0, double x1, double y1) {
    A.motion_out[r] = moves ? FleetPos{x1 - x0, y1 - y0} : FleetPos{0.0, 0.0};
  }
};

template <int ROT>
__device__ __forceinline__ FleetMotionObs<ROT> episode_obs(FleetMotionObs<ROT>*) {
  FleetMotionObs<ROT> o;
  o.world_at = lds_addr(fleet_step_world()->c);
  o.loop_at = ROT == kRotCum ? lds_addr(fleet_step_frame()->c) : o.world_at;
  return o;
}

// ---------------------------------------------------------------------------
// A planned fleet call (mpc_episodes_fleet_run_planned): each chosen
// neighbour's circle follows the neighbour's own plan, two points (a1, a2) read
// from this call's side of the plan board — where the neighbour means to be
// after this call and after the next: layers of its StaleTraj, the arc it
// drives, or its position twice if it stands.  Step 1's centre is a1, step 2's
// a2, step j >= 3's fleet_predict(a2, a2 - a1, j - 2) per coordinate.  The
// selection, the per-step tables, form() and the lanes' tests are
// FleetMotionObs'; only where a centre comes from differs.  The chosen
// neighbours' entries are staged in LDS first — one 32-B load each, by the
// first `len` threads, which form a2 - a1 there once — and the tables' entries
// are formed from LDS: no entry waits for a global load of its own, and the
// difference is not made N times.  k_fleet_plan_begin fills the board's side 0
// before planned call 0: everybody stands.
struct FleetPlanLds {
  FleetPlan a[MPC_MAX_OBSTACLES];   // the chosen neighbours' entries
  FleetPos d[MPC_MAX_OBSTACLES];    // a2 - a1
};

__device__ __forceinline__ FleetPlanLds* fleet_plan_lds() {
  __shared__ FleetPlanLds s_fleet_plan;
  return &s_fleet_plan;
}

__global__ void k_fleet_plan_begin(const FleetPos* __restrict__ board, int n,
                                   FleetPlan* __restrict__ plan) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const FleetPos p = board[r];
  plan[r] = FleetPlan{p.x, p.y, p.x, p.y};
}

template <int ROT>
struct FleetPlanObs : FleetMotionObs<ROT> {
  static constexpr bool kPlan = true;   // (the kernel: m at the start of the step, the plan write)

  // FleetObs::select, the chosen neighbours' entries staged, then the per-step
  // tables (entry e = (j - 1) * g4 + i: circle i of step j).
  __device__ __forceinline__ void select(const FleetPlanArgs& A, int r, double x, double y) {
    FleetObs<ROT>::select(A, r, x, y);
    if (this->m == 0) {   // uniform: the call runs without circles
      this->entries = 0;
      return;
    }
    FleetLds* S = fleet_lds();
    FleetPlanLds* P = fleet_plan_lds();
    FleetStepTable* T = fleet_step_world();
    const int g4 = this->groups() * kFleetGroup, n_static = A.n_static, m = this->m;
    if (static_cast<int>(threadIdx.x) < m - n_static) {
      const FleetPlan a = A.plan_in[S->idx[threadIdx.x]];
      P->a[threadIdx.x] = a;
      P->d[threadIdx.x] = FleetPos{a.x2 - a.x1, a.y2 - a.y1};
    }
    __syncthreads();
    this->entries = A.n_steps * g4;
    for (int e = threadIdx.x; e < this->entries; e += kBlock) {
      const int j = e / g4, i = e - j * g4;
      Circle cq = S->world[i];
      if (i >= n_static && i < m) {
        const FleetPlan a = P->a[i - n_static];
        const FleetPos d = P->d[i - n_static];
        cq.cx = j == 0 ? a.x1 : (j == 1 ? a.x2 : fleet_predict(a.x2, d.x, j - 1));
        cq.cy = j == 0 ? a.y1 : (j == 1 ? a.y2 : fleet_predict(a.y2, d.y, j - 1));
      }
      T->c[j][i] = cq;
    }
    __syncthreads();
  }

  // Block r's entry of the plan board's out side (one thread).  plans: the
  // robot took a step in this call, goes on after it, and the step had a
  // winner; its entry is then layers min(k + 1, 2) and min(k + 2, 2) of its
  // plan, k the layer the update returned (m0: m when the step began).
  // Everyone else stands at (x, y).  Copies, no arithmetic.
  __device__ __forceinline__ static void publish(const FleetPlanArgs& A, int r, bool plans, int m0,
                                                 const StaleTraj& st, double x, double y) {
    const int k = m0 == 2 ? 2 : (m0 == 1 ? 1 : 0);
    const int k1 = k == 0 ? 1 : 2, k2 = 2;   // min(k + 1, 2); min(k + 2, 2) = 2 for every k
    A.plan_out[r] = plans ? FleetPlan{st.ot[k1][0], st.ot[k1][1], st.ot[k2][0], st.ot[k2][1]}
                          : FleetPlan{x, y, x, y};
  }
};

template <int ROT>
__device__ __forceinline__ FleetPlanObs<ROT> episode_obs(FleetPlanObs<ROT>*) {
  FleetPlanObs<ROT> o;
  o.world_at = lds_addr(fleet_step_world()->c);
  o.loop_at = ROT == kRotCum ? lds_addr(fleet_step_frame()->c) : o.world_at;
  return o;
}

}  // namespace mpc
