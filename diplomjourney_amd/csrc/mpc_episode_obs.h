// mpc_episode_obs.h — keep-out circles in the device-resident episode steps
// (mpc_episode_partials_obstacles, mpc_episode_chain_step_obstacles; gfx950).
//
//   kernarg_world            the call's world-frame circle table (kernel argument 0)
//   frame_slots, FrameObs<NOBS>   the lane hook of rect+cum: the table in the frame
//                            of the sums, formed on the device from the step's
//                            pose (its loop repeats CircleObs::test's, mpc_device.h)
//   episode_obs_body, k_episode_stream_obs, k_episode_argmin_obs   the streaming /
//                            scalar rollout of mpc_episode_partials with circles
//   chain_obs_waves, k_episode_chain_obs   k_episode_chain<kChainFin> with circles
//                            (block 0: a copy of that kernel's, mpc_chain.h)
//
// The world-frame modes (qk21, rect, +rot) test the kernel-argument table as
// the one-shot kernels do (CircleObs).  rect+cum accumulates sums that know no
// pose, so its circles are moved into the start-pose frame (frame_circle,
// mpc_device.h): the one-shot entry does that on the host, here the pose
// exists only in the episode state, or, in a chained launch, only once block 0
// has published it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_chain.h"
#include "mpc_device.h"
#include "mpc_kernels.h"
#include "mpc_lanes.h"

namespace mpc {

// The world table: the kernels' FIRST argument `W`, read through the segment
// pointer (constant address space, scalar loads; see kernarg_obs).
__device__ __forceinline__ ObsTable kernarg_world() {
#if defined(__HIP_DEVICE_COMPILE__)
  return (ObsTable)__builtin_amdgcn_kernarg_segment_ptr();
#else
  return nullptr;   // (the host pass only parses the kernels)
#endif
}

// The frame table of the 16-circle instantiations (LDS only in the kernels
// that call this).
__device__ __forceinline__ Circle* frame_slots() {
  __shared__ Circle s_frame[MPC_MAX_OBSTACLES];
  return s_frame;
}

// The rect+cum hook.  form(K, scaled): the world table in the frame of the sums
// of the step that starts at K's pose; every thread of the block calls it at
// the same point (the LDS form has a barrier).
// Up to 4 circles: every lane computes the (uniform) entries and they move to
// SGPRs with readfirstlane, as consts_from_words does with the constants; the
// loop's test then has scalar operands, as CircleObs<4>'s.
// 16 circles: 96 SGPRs do not survive the loop (CircleObs), so lanes 0..15
// write one entry each to LDS and every step reads them back as broadcast
// operands (all lanes one address: no bank conflict); the table's address is
// made opaque per step, so that the 48 loads are not hoisted into 96 VGPRs.
// world(): the irregular-candidate recompute, on the kernel-argument table.
template <int NOBS>
struct FrameObs {
  static_assert(NOBS >= 1 && NOBS <= MPC_MAX_OBSTACLES, "circle count");
  static constexpr bool kOn = true;
  static constexpr bool kRegs = NOBS <= 4;
  ObsTable world_t;
  Circle reg[kRegs ? NOBS : 1];
  uint32_t lds = 0;

  __device__ __forceinline__ void form(const Consts& K, bool scaled) {
    if constexpr (kRegs) {
#pragma unroll
      for (int i = 0; i < NOBS; ++i) {
        const Circle f = frame_circle(
            K, Circle{world_t->c[i].cx, world_t->c[i].cy, world_t->c[i].r2, 0.0}, scaled);
        reg[i] = Circle{uniform_d(f.cx), uniform_d(f.cy), uniform_d(f.r2), 0.0};
      }
    } else {
      Circle* t = frame_slots();
      if (threadIdx.x < NOBS) {
        const int i = threadIdx.x;
        t[i] = frame_circle(K, Circle{world_t->c[i].cx, world_t->c[i].cy, world_t->c[i].r2, 0.0},
                            scaled);
      }
      __syncthreads();
      lds = lds_addr(t);
    }
  }

  template <int CPL>
  __device__ __forceinline__ void loop(const double (&x)[CPL], const double (&y)[CPL],
                                       bool (&blocked)[CPL]) const {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t at = lds;
    if constexpr (!kRegs) asm volatile("" : "+v"(at));
    [[maybe_unused]] const auto* t = (const __attribute__((address_space(3))) Circle*)at;
#else
    [[maybe_unused]] const Circle* t = nullptr;
#endif
    // (a copy of CircleObs::test's loop, mpc_device.h: DESIGN.md §5)
#pragma unroll
    for (int i = 0; i < NOBS; ++i) {
      double cx, cy, r2;
      if constexpr (kRegs) {
        cx = reg[i].cx, cy = reg[i].cy, r2 = reg[i].r2;
      } else {
        cx = t[i].cx, cy = t[i].cy, r2 = t[i].r2;
      }
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const double dx = x[j] - cx, dy = y[j] - cy;
        blocked[j] |= fma(dy, dy, dx * dx) < r2;
      }
    }
  }

  __device__ __forceinline__ void world(double x, double y, bool& blocked) const {
    CircleObs<NOBS>{world_t, world_t}.world(x, y, blocked);
  }
};

// mpc_episode_partials with circles: rollout_argmin_body<KDEV> with the hook
// of the mode.
template <int CPL, int INTEG, int ROT, int NOBS>
__device__ __forceinline__ void episode_obs_body(const Consts* __restrict__ Kdev,
                                                 const double* __restrict__ v,
                                                 const double* __restrict__ b, int64_t n_cand,
                                                 int n_steps, Rec* __restrict__ part,
                                                 unsigned long long* __restrict__ n_blocked) {
  const ObsTable W = kernarg_world();
  const Consts K = *Kdev;
  if constexpr (ROT == kRotCum) {
    FrameObs<NOBS> obs{W};
    obs.form(K, K.L_pow2 != 0);
    rollout_argmin_body<CPL, INTEG, ROT, false, true>(K, Kdev, v, b, n_cand, n_steps, part,
                                                      nullptr, obs, n_blocked);
  } else {
    rollout_argmin_body<CPL, INTEG, ROT, false, true>(K, Kdev, v, b, n_cand, n_steps, part,
                                                      nullptr, CircleObs<NOBS>{W, W}, n_blocked);
  }
}

// The aligned path (the one-shot variant's launch bound: 76-90 VGPRs, no scratch).
template <int INTEG, int ROT, int NOBS>
__global__ __launch_bounds__(kBlock, kObsStreamWaves) void k_episode_stream_obs(
    Obstacles W, const Consts* __restrict__ Kdev, const double* __restrict__ v,
    const double* __restrict__ b, int64_t n_cand, int n_steps, Rec* __restrict__ part,
    unsigned long long* __restrict__ n_blocked) {
  episode_obs_body<kCplWide, INTEG, ROT, NOBS>(Kdev, v, b, n_cand, n_steps, part, n_blocked);
}

// The scalar path (one candidate per lane).
template <int INTEG, int ROT, int NOBS>
__global__ __launch_bounds__(kBlock, 1) void k_episode_argmin_obs(
    Obstacles W, const Consts* __restrict__ Kdev, const double* __restrict__ v,
    const double* __restrict__ b, int64_t n_cand, int n_steps, Rec* __restrict__ part,
    unsigned long long* __restrict__ n_blocked) {
  episode_obs_body<1, INTEG, ROT, NOBS>(Kdev, v, b, n_cand, n_steps, part, n_blocked);
}

// The chained step (one GPU, kChainFin) with circles: block 0 completes the
// previous step exactly as k_episode_chain's does; the tile blocks test this
// step's candidates (chain_tiles<..., FrameObs<NOBS>>).
// Launch bound: the one-GPU chained kernel's for 4 circles (86 VGPRs); with the
// 16-circle table's LDS operands the loop held 96 VGPRs and 12-20 B of scratch
// per lane at 5 waves per SIMD, none at 4.
template <int NOBS>
constexpr int chain_obs_waves() {
  return NOBS > 4 ? 4 : chain_waves<kChainFin>();
}
template <bool PL2, bool TILED, int NOBS>
__global__ __launch_bounds__(kBlock, chain_obs_waves<NOBS>()) void k_episode_chain_obs(
    Obstacles W, EpisodeState* __restrict__ S, uint32_t epoch, const double* __restrict__ v,
    const double* __restrict__ b, int64_t n_cand, int n_steps, Rec* __restrict__ part,
    int has_prev, const Rec* __restrict__ part_prev, int n_part_prev,
    const double* __restrict__ v_prev, const double* __restrict__ b_prev, int64_t index_base,
    mpc_result_t* __restrict__ out_prev, mpc_episode_config_t ecfg,
    mpc_episode_log_t* __restrict__ log, int cap, unsigned long long* __restrict__ n_blocked) {
  constexpr int INTEG = MPC_INTEG_RECT, ROT = kRotCum;
  if (blockIdx.x == 0) {
    // (a copy of k_episode_chain's kChainFin block-0 body, mpc_chain.h: DESIGN.md §5)
    if (has_prev) {
      const Consts Kp = S->h.K;
      const EpisodeHook hook{&S->h, log, cap, S->chain_pub, kPubWords, epoch, &S->chain_error};
      finalize_block<INTEG, ROT, true, kBlock, false, false, TILED>(
          part_prev, n_part_prev, Kp, v_prev, b_prev, n_cand, n_steps, index_base, S->h.incumbent,
          out_prev, ecfg, hook, ring_lds());
      __syncthreads();   // (the wheelbase check below reads the stored head)
    } else {
      chain_publish(S, epoch);
    }
    if (threadIdx.x == 0 && (S->h.K.L_pow2 != 0) != PL2) S->chain_error = 2u;
    return;
  }
  chain_tiles<INTEG, ROT, PL2, false, kChainWaitTicks, TILED>(
      S, epoch, v, b, n_cand, n_steps, part, has_prev, ecfg, FrameObs<NOBS>{kernarg_world()},
      n_blocked);
}

}  // namespace mpc
