// mpc_timeline.h — the phase stamps of the developer timelines, compiled in
// behind one macro (gfx950).
// Without MPC_TIMELINE (the product) every stamp is ((void)0) and this header
// declares and includes nothing: the machine code is the same with or without
// them (tools/kernel_digest.py).  With it (tools/tl_variant.so) a stamp reads
// the 100-MHz clock (s_memrealtime); tools/timeline.py names the phases and
// reads the tables through mpc_debug_timeline (mpc_rollout.hip, variant only).
//   TL_B0(q), TL_B0_IF(cond, q)   chained step, block 0 (thread 0 / the thread
//                                 `cond` picks): g_tl[8 * kChainBlocks + q]
//   TL_TILE(q), TL_TILE_STORED(q) chained step, a block's thread 0: g_tl[8 *
//                                 blockIdx.x + q]; _STORED: after its stores
//   TL_EP_BEGIN / _CALL / _MARK(q) / _END   workload R: thread 0 sums each
//                                 phase's ticks over its calls in registers,
//                                 g_tl_ep[8 * blockIdx.x + q] at the end (6: calls)
//   RUN_SET / _MIN / _MAX / _ADD(j, f)   persistent run: g_run_tl[j][f]
// A table is static to its translation unit: the circle instantiations of
// k_episodes_run and its fleet instantiations (mpc_episodes_obs.hip) stamp a
// copy that mpc_debug_timeline reads as its table 3 (a fleet call is a launch:
// the last call's phases).
// Bounds: the tables are sized by the constants that bound the grids (TL_BOUND
// beside each), and every stamp tests its own index as well: none writes past
// its table whatever launches the code it sits in.
#pragma once

#ifdef MPC_TIMELINE
namespace mpc {
namespace tl {
constexpr int kChainBlocks = 2049;   // block 0 + kMaxBlocks tile blocks
constexpr int kB0Slots = 32;         // block 0's own, after the blocks' 8 each
constexpr int kRobots = 65535;       // kEpMaxRobots: one block per robot
constexpr int kRunSteps = 64;        // kRunMaxSteps
}  // namespace tl
static __device__ unsigned long long g_tl[8 * tl::kChainBlocks + tl::kB0Slots];
static __device__ unsigned long long g_tl_ep[8 * tl::kRobots];
// per step of the last launch: 0 selector step start, 1 records complete,
// 2 step done (selector), 3 first unit start (min), 4 last loop end (max),
// 5 last wait end (max), 6 last record stored (max), 7 units that waited
static __device__ unsigned long long g_run_tl[tl::kRunSteps][8];
}  // namespace mpc

#define TL_BOUND(name, value) static_assert(mpc::tl::name == (value), "timeline table size")
#define TL_NOW() __builtin_amdgcn_s_memrealtime()
// one stamp: g_tl[base + q], q < n a constant, if `cond`
#define TL_PUT(cond, base, q, n)                                                        \
  do {                                                                                  \
    static_assert((q) >= 0 && (q) < (n), "timeline slot");                              \
    if (cond)                                                                           \
      __hip_atomic_store(&mpc::g_tl[(base) + (q)], TL_NOW(), __ATOMIC_RELAXED,          \
                         __HIP_MEMORY_SCOPE_AGENT);                                     \
  } while (0)
#define TL_B0_IF(cond, q) \
  TL_PUT(blockIdx.x == 0 && (cond), 8 * mpc::tl::kChainBlocks, q, mpc::tl::kB0Slots)
#define TL_B0(q) TL_B0_IF(threadIdx.x == 0, q)
#define TL_TILE(q) \
  TL_PUT(threadIdx.x == 0 && blockIdx.x < mpc::tl::kChainBlocks, 8 * blockIdx.x, q, 8)
#define TL_TILE_STORED(q) \
  do { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TL_TILE(q); } while (0)
#define TL_EP_BEGIN() unsigned long long tl_acc[6] = {}, tl_prev = TL_NOW(), tl_n = 0
#define TL_EP_CALL() \
  do { if (threadIdx.x == 0) { tl_prev = TL_NOW(); tl_n++; } } while (0)
#define TL_EP_MARK(q)                                                                   \
  do {                                                                                  \
    static_assert((q) >= 0 && (q) < 6, "timeline phase");                               \
    if (threadIdx.x == 0) {                                                             \
      const unsigned long long tl_now = TL_NOW();                                       \
      tl_acc[q] += tl_now - tl_prev;                                                    \
      tl_prev = tl_now;                                                                 \
    }                                                                                   \
  } while (0)
#define TL_EP_END()                                                                     \
  do {                                                                                  \
    if (threadIdx.x == 0 && blockIdx.x < mpc::tl::kRobots) {                            \
      for (int q = 0; q < 6; ++q) mpc::g_tl_ep[8 * blockIdx.x + q] = tl_acc[q];         \
      mpc::g_tl_ep[8 * blockIdx.x + 6] = tl_n;                                          \
    }                                                                                   \
  } while (0)
#define RUN_AT(j, f, op)                                                               \
  do {                                                                                  \
    static_assert((f) >= 0 && (f) < 8, "timeline field");                               \
    if (static_cast<unsigned>(j) < static_cast<unsigned>(mpc::tl::kRunSteps)) op;       \
  } while (0)
#define RUN_SET(j, f) RUN_AT(j, f, mpc::g_run_tl[j][f] = TL_NOW())
#define RUN_MIN(j, f) RUN_AT(j, f, atomicMin(&mpc::g_run_tl[j][f], TL_NOW()))
#define RUN_MAX(j, f) RUN_AT(j, f, atomicMax(&mpc::g_run_tl[j][f], TL_NOW()))
#define RUN_ADD(j, f) RUN_AT(j, f, atomicAdd(&mpc::g_run_tl[j][f], 1ull))
#else
#define TL_BOUND(name, value) static_assert(true, "")
#define TL_B0_IF(cond, q) ((void)0)
#define TL_B0(q) ((void)0)
#define TL_TILE(q) ((void)0)
#define TL_TILE_STORED(q) ((void)0)
#define TL_EP_BEGIN() ((void)0)
#define TL_EP_CALL() ((void)0)
#define TL_EP_MARK(q) ((void)0)
#define TL_EP_END() ((void)0)
#define RUN_SET(j, f) ((void)0)
#define RUN_MIN(j, f) ((void)0)
#define RUN_MAX(j, f) ((void)0)
#define RUN_ADD(j, f) ((void)0)
#endif
