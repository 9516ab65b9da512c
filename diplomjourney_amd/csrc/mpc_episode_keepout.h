// mpc_episode_keepout.h — keep-out polygons (beside the circles) in the
// device-resident episode steps (mpc_episode_partials_keepout,
// mpc_episode_chain_step_keepout; gfx950).
//
//   EpisodeKeepoutArgs, kernarg_episode_keepout   the call's world tables
//                            (kernel argument 0: the circles where
//                            kernarg_world reads them, then the polygons)
//   frame_edge_slots, FrameKeepoutObs<NOBS>   the lane hook of rect+cum: the
//                            edge table in the frame of the sums, formed on the
//                            device from the step's pose (frame_edge,
//                            mpc_keepout.h: the function the host calls)
//   episode_keepout_body, k_episode_stream_keepout, k_episode_argmin_keepout
//                            the streaming / scalar rollout of
//                            mpc_episode_partials with circles and polygons
//   k_episode_chain_keepout  k_episode_chain<kChainFin> with both (block 0: a
//                            copy of that kernel's, mpc_chain.h)
// (their launches: launch_episode_keepout, launch_episode_chain_keepout in
// mpc_rollout.hip)
//
// The world-frame modes (qk21, rect, +rot) test the kernel-argument tables as
// the one-shot kernels do (KeepoutObs, mpc_keepout.h).  rect+cum accumulates
// sums that know no pose: its circles move into the start-pose frame as
// FrameObs's do (mpc_episode_obs.h) and its edge lines by frame_edge, on the
// device, because the pose exists only in the episode state, or, in a chained
// launch, only once block 0 has published it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_chain.h"
#include "mpc_device.h"
#include "mpc_episode_obs.h"
#include "mpc_keepout.h"
#include "mpc_kernels.h"
#include "mpc_lanes.h"

namespace mpc {

// The kernels' FIRST argument: the circles' world table at offset 0 (where
// kernarg_world reads it), the polygons' after it, then the polygon count.
struct EpisodeKeepoutArgs {
  Obstacles world;
  Polygons pworld;
  int32_t n_polygons, pad_[3];
};
static_assert(offsetof(EpisodeKeepoutArgs, world) == 0 &&
                  offsetof(EpisodeKeepoutArgs, pworld) == 512 &&
                  sizeof(EpisodeKeepoutArgs) == 1296,
              "table layout");
// HIP passes at most 4 KB of kernel arguments: the tables, the chained
// kernel's mpc_episode_config_t by value and its pointers and sizes (136 B,
// rounded up) fit.
static_assert(sizeof(EpisodeKeepoutArgs) + sizeof(mpc_episode_config_t) + 160 <= 4096,
              "kernel-argument segment");

#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) EpisodeKeepoutArgs* EpisodeKeepoutTable;
#else
typedef const EpisodeKeepoutArgs* EpisodeKeepoutTable;
#endif
__device__ __forceinline__ EpisodeKeepoutTable kernarg_episode_keepout() {
#if defined(__HIP_DEVICE_COMPILE__)
  return (EpisodeKeepoutTable)__builtin_amdgcn_kernarg_segment_ptr();
#else
  return nullptr;   // (the host pass only parses the kernels)
#endif
}

// The world-frame hook on the kernel-argument tables (the one-shot kernels'
// KeepoutObs with `loop` = `world`).
template <int NOBS>
__device__ __forceinline__ KeepoutObs<NOBS> world_keepout(EpisodeKeepoutTable a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return KeepoutObs<NOBS>{&a->world, &a->world, &a->pworld, &a->pworld, a->n_polygons};
#else
  return KeepoutObs<NOBS>{nullptr, nullptr, nullptr, nullptr, 0};
#endif
}

// The frame table of the polygons: all 32 edge slots, 768 B (LDS only in the
// kernels that call this).
__device__ __forceinline__ Edge* frame_edge_slots() {
  __shared__ Edge s_pframe[MPC_MAX_POLYGONS * MPC_MAX_POLYGON_VERTICES];
  return s_pframe;
}

// The rect+cum hook of the keep-out steps: the circles as FrameObs<16> has
// them (NOBS = 0: no circle statement), then the polygons.
// form(K, scaled): threads 0..31 move one world edge each into the frame of the
// sums of the step that starts at K's pose (frame_edge: a padded edge keeps its
// sign) and write it to LDS; threads 0..15 write FrameObs<16>'s circle entries
// beside them; one barrier for both.  Every thread of the block calls it at the
// same point.
// loop(): KeepoutObs::test's polygon loop (mpc_keepout.h) with the edge
// operands read from that table: wave-uniform over the call's polygon count,
// never unrolled, the 8 edge slots of a polygon straight-line code, the
// compares combined as wave masks.  The operands are uniform values in VGPRs
// (all lanes read one address: a broadcast, no bank conflict), 6 per edge.
// The table's address is made opaque per step, so that no load is hoisted out
// of the rollout loop, and again per edge together with the polygon's running
// mask of the lane's FIRST candidate (in[0]; one tie orders the read, whose
// address is the tied value, also with two candidates per lane), so that edge
// i + 1 is read once edge i has been judged: gathered at the head of a polygon
// its 24 doubles are 48 VGPRs.  Moving them to SGPRs (readfirstlane)
// would cost 6 VALU per edge, as many as the test of the lane's two candidates.
// world(): the irregular-candidate recompute, KeepoutObs's on the
// kernel-argument tables.
template <int NOBS>
struct FrameKeepoutObs {
  static_assert(NOBS == 0 || NOBS == MPC_MAX_OBSTACLES, "circle count");
  static constexpr bool kOn = true;
  EpisodeKeepoutTable args;
  int n_poly = 0;   // (wave-uniform: a kernel argument)
  uint32_t lds_c = 0, lds_p = 0;

  __device__ __forceinline__ void form(const Consts& K, bool scaled) {
#if defined(__HIP_DEVICE_COMPILE__)
    n_poly = args->n_polygons;
    Edge* t = frame_edge_slots();
    constexpr int kEdges = MPC_MAX_POLYGONS * MPC_MAX_POLYGON_VERTICES;
    if (threadIdx.x < kEdges) {
      const int i = threadIdx.x;
      const int p = i / MPC_MAX_POLYGON_VERTICES, q = i % MPC_MAX_POLYGON_VERTICES;
      t[i] = frame_edge(
          K, Edge{args->pworld.e[p][q].a, args->pworld.e[p][q].b, args->pworld.e[p][q].c}, scaled);
    }
    if constexpr (NOBS > 0) {
      Circle* tc = frame_slots();
      if (threadIdx.x < NOBS) {
        const int i = threadIdx.x;
        tc[i] = frame_circle(
            K, Circle{args->world.c[i].cx, args->world.c[i].cy, args->world.c[i].r2, 0.0}, scaled);
      }
      lds_c = lds_addr(tc);
    }
    __syncthreads();
    lds_p = lds_addr(t);
#endif
  }

  template <int CPL>
  __device__ __forceinline__ void loop(const double (&x)[CPL], const double (&y)[CPL],
                                       bool (&blocked)[CPL]) const {
    static_assert(CPL == 1 || CPL == 2, "candidates per lane");
    if constexpr (NOBS > 0) {
      FrameObs<NOBS> circles{&args->world};
      circles.lds = lds_c;
      circles.template loop<CPL>(x, y, blocked);
    }
    uint64_t any[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) any[j] = wave_mask(blocked[j]);
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t at = lds_p;
    if constexpr (CPL == 2)
      asm volatile("" : "+v"(at), "+s"(any[0]), "+s"(any[1]));
    else
      asm volatile("" : "+v"(at), "+s"(any[0]));
#pragma unroll 1
    for (int p = 0; p < n_poly; ++p) {
      uint64_t in[CPL];
#pragma unroll
      for (int j = 0; j < CPL; ++j) in[j] = ~uint64_t{0};
#pragma unroll
      for (int i = 0; i < MPC_MAX_POLYGON_VERTICES; ++i) {
        asm volatile("" : "+v"(at), "+s"(in[0]));
        const auto* e = (const __attribute__((address_space(3))) Edge*)at + i;
        const double a = e->a, b = e->b, c = e->c;
#pragma unroll
        for (int j = 0; j < CPL; ++j) in[j] &= wave_mask(edge_inner(a, b, c, x[j], y[j]));
      }
#pragma unroll
      for (int j = 0; j < CPL; ++j) any[j] |= in[j];
      at += MPC_MAX_POLYGON_VERTICES * sizeof(Edge);
    }
#endif
#pragma unroll
    for (int j = 0; j < CPL; ++j) blocked[j] = lane_of(any[j]);
  }

  __device__ __forceinline__ void world(double x, double y, bool& blocked) const {
    world_keepout<NOBS>(args).world(x, y, blocked);
  }
};

// mpc_episode_partials with circles and polygons: rollout_argmin_body<KDEV>
// with the hook of the mode.
template <int CPL, int INTEG, int ROT, int NOBS>
__device__ __forceinline__ void episode_keepout_body(const Consts* __restrict__ Kdev,
                                                     const double* __restrict__ v,
                                                     const double* __restrict__ b, int64_t n_cand,
                                                     int n_steps, Rec* __restrict__ part,
                                                     unsigned long long* __restrict__ n_blocked) {
  const EpisodeKeepoutTable A = kernarg_episode_keepout();
  const Consts K = *Kdev;
  if constexpr (ROT == kRotCum) {
    FrameKeepoutObs<NOBS> obs{A};
    obs.form(K, K.L_pow2 != 0);
    rollout_argmin_body<CPL, INTEG, ROT, false, true>(K, Kdev, v, b, n_cand, n_steps, part,
                                                      nullptr, obs, n_blocked);
  } else {
    rollout_argmin_body<CPL, INTEG, ROT, false, true>(K, Kdev, v, b, n_cand, n_steps, part,
                                                      nullptr, world_keepout<NOBS>(A), n_blocked);
  }
}

// The aligned path (the circle kernels' launch bound).
template <int INTEG, int ROT, int NOBS>
__global__ __launch_bounds__(kBlock, kObsStreamWaves) void k_episode_stream_keepout(
    EpisodeKeepoutArgs A, const Consts* __restrict__ Kdev, const double* __restrict__ v,
    const double* __restrict__ b, int64_t n_cand, int n_steps, Rec* __restrict__ part,
    unsigned long long* __restrict__ n_blocked) {
  episode_keepout_body<kCplWide, INTEG, ROT, NOBS>(Kdev, v, b, n_cand, n_steps, part, n_blocked);
}

// The scalar path (one candidate per lane).
template <int INTEG, int ROT, int NOBS>
__global__ __launch_bounds__(kBlock, 1) void k_episode_argmin_keepout(
    EpisodeKeepoutArgs A, const Consts* __restrict__ Kdev, const double* __restrict__ v,
    const double* __restrict__ b, int64_t n_cand, int n_steps, Rec* __restrict__ part,
    unsigned long long* __restrict__ n_blocked) {
  episode_keepout_body<1, INTEG, ROT, NOBS>(Kdev, v, b, n_cand, n_steps, part, n_blocked);
}

// The chained step (one GPU, kChainFin) with circles and polygons: block 0
// completes the previous step exactly as k_episode_chain's does; the tile
// blocks wait for the published pose, form the tables and test this step's
// candidates (chain_tiles<..., FrameKeepoutObs<NOBS>>), as with circles alone.
// Launch bound: k_episode_chain_obs's for the same circle count.
template <bool PL2, bool TILED, int NOBS>
__global__ __launch_bounds__(kBlock, chain_obs_waves<NOBS>()) void k_episode_chain_keepout(
    EpisodeKeepoutArgs A, EpisodeState* __restrict__ S, uint32_t epoch,
    const double* __restrict__ v, const double* __restrict__ b, int64_t n_cand, int n_steps,
    Rec* __restrict__ part, int has_prev, const Rec* __restrict__ part_prev, int n_part_prev,
    const double* __restrict__ v_prev, const double* __restrict__ b_prev, int64_t index_base,
    mpc_result_t* __restrict__ out_prev, mpc_episode_config_t ecfg,
    mpc_episode_log_t* __restrict__ log, int cap, unsigned long long* __restrict__ n_blocked) {
  constexpr int INTEG = MPC_INTEG_RECT, ROT = kRotCum;
  if (blockIdx.x == 0) {
    // (a copy of k_episode_chain's kChainFin block-0 body, mpc_chain.h, as
    // k_episode_chain_obs carries one, mpc_episode_obs.h: DESIGN.md §5)
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
      S, epoch, v, b, n_cand, n_steps, part, has_prev, ecfg,
      FrameKeepoutObs<NOBS>{kernarg_episode_keepout()}, n_blocked);
}

}  // namespace mpc
