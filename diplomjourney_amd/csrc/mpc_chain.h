// mpc_chain.h — the chained episode step: one launch = this step's streaming
// rollout + the completion of the previous step (gfx950).
//
//   kChainFin, kChainXchg, kChainP2P   what block 0 completes the previous step with
//   consts_from_words, chain_read      the published constants, as a tile block reads them
//   chain_waves, chain_tiles           the tile blocks (with an obstacle hook: the
//                                      blocked-count epilogue of mpc_kernels.h)
//   k_episode_chain                    block 0 (mpc_finalize.h / mpc_exchange.h) + the tiles;
//                                      its kChainFin block 0 is repeated in
//                                      k_episode_chain_obs (mpc_episode_obs.h)
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_argmin.h"
#include "mpc_device.h"
#include "mpc_episode.h"
#include "mpc_exchange.h"
#include "mpc_finalize.h"
#include "mpc_kernels.h"
#include "mpc_lanes.h"
#include "mpc_timeline.h"
#include "mpc_winner.h"

namespace mpc {

// ---------------------------------------------------------------------------
// Chained episode step (heading mode kRotCum): ONE launch = this step's
// streaming rollout + the completion of the PREVIOUS step.  Block 0 completes
// step k-1 — kChainFin (one GPU): k_finalize's record reduction, winner
// re-roll and episode update; kChainXchg (multi-GPU): the selection over the
// gathered per-rank candidates, the winner's re-roll and the update — and
// publishes step k's constants as epoch-tagged words (EpisodeState::chain_pub);
// kChainXchg's block 0 then collects this launch's tagged block records into
// the rank's candidate (collect_local_candidate), which the caller gathers.
// The other blocks do not wait for it: in kRotCum mode a candidate's rollout
// needs no start pose, only the step size h (and the constant wheelbase
// terms).  A block reads the published words once, right after its first
// control loads are in flight: if all carry this launch's epoch (block 0 is
// done: every block after the first round) the constants are final; else it
// speculates h as the next step of the same episode (from the previous
// step's published t, + dt, as episode_prepare forms it) and reads the words
// again after its loop, for the final pose transform and the criterion.  If h
// turns out different (the previous step restarted the episode and reset t)
// the lane recomputes with the published constants (rollout_lane_glds).
// Records of tile-block b go to part[b - 1].  Consecutive chained launches
// carry different epochs and the update that ends a chain (k_finalize's hook,
// k_episode_advance) clears the tags.  The wait is bounded: if the words
// never came, chain_error is set instead of hanging the GPU.
// kChainP2P (multi-GPU, no collective): kChainFin's structure (records to
// part, the next launch's block 0 reduces them) with the per-rank candidates
// exchanged through the mailboxes by block 0 (p2p_complete).
constexpr int kChainFin = 1, kChainXchg = 3, kChainP2P = 4;
TL_BOUND(kChainBlocks, kMaxBlocks + 1);   // a chained grid: block 0 + rollout_grid() tile blocks

// LDS dwords (Consts layout) -> wave-uniform Consts, field by field (no
// memory view of the struct: it stays in SGPRs).
__device__ __forceinline__ Consts consts_from_words(const uint32_t* w) {
  auto d = [&](size_t off) {
    const int q = static_cast<int>(off / 4);
    // (readfirstlane returns int: through uint32_t, not sign-extended)
    const uint64_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(w[q]));
    const uint64_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(w[q + 1]));
    return __longlong_as_double(static_cast<long long>((hi << 32) | lo));
  };
  auto i32 = [&](size_t off) {
    return static_cast<int32_t>(__builtin_amdgcn_readfirstlane(w[off / 4]));
  };
  Consts K;
  K.x = d(offsetof(Consts, x));
  K.y = d(offsetof(Consts, y));
  K.phi = d(offsetof(Consts, phi));
  K.x_t = d(offsetof(Consts, x_t));
  K.y_t = d(offsetof(Consts, y_t));
  K.x_0 = d(offsetof(Consts, x_0));
  K.y_0 = d(offsetof(Consts, y_0));
  K.A = d(offsetof(Consts, A));
  K.B = d(offsetof(Consts, B));
  K.C1 = d(offsetof(Consts, C1));
  K.C2 = d(offsetof(Consts, C2));
  K.inv_den = d(offsetof(Consts, inv_den));
  K.L = d(offsetof(Consts, L));
  K.inv_L = d(offsetof(Consts, inv_L));
  K.h = d(offsetof(Consts, h));
  K.hlgth = d(offsetof(Consts, hlgth));
  K.s0 = d(offsetof(Consts, s0));
  K.c0 = d(offsetof(Consts, c0));
  K.L_pow2 = i32(offsetof(Consts, L_pow2));
  K.pad_ = 0;
  return K;
}

// Wave 0 of a tile block: one coherent load of every published word into
// s_w / s_tag; returns (wave-uniform) whether all carry `epoch`.
__device__ __forceinline__ bool chain_read(const EpisodeState* S, uint32_t epoch,
                                           uint32_t* s_w, uint32_t* s_tag) {
  const int q = threadIdx.x;
  bool ok = true;
  if (q < kPubWords) {
    const uint64_t w = __hip_atomic_load(const_cast<uint64_t*>(&S->chain_pub[q]),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_w[q] = static_cast<uint32_t>(w >> 32);
    s_tag[q] = static_cast<uint32_t>(w);
    ok = static_cast<uint32_t>(w) == epoch;
  }
  return __ballot(!ok) == 0;
}

// Launch bound of the chained kernel (waves per SIMD).  The one-GPU form runs
// 5 since round 6 (87 VGPRs, no scratch): at 6 it held 80 VGPRs with 4 spilled
// (12 B of scratch per lane) and ran 0.2-0.6 us slower per launch at config C
// and 0.7 us at D (same-box A/Bs, profiles/r06/ab_chain_waves.txt); the
// exchange and P2P forms run 5
// (at 6 they keep scratch: the P2P form spilled the work-item id at entry, a
// 4-B store per lane in EVERY wave — 2 MB of writes per config-C launch, the
// round-4 traffic excess; measured, 3 interleaved pairs each: exchange 36.73
// (6 waves) vs 36.31 us, profiles/r04/exchange_waves_ab.txt; P2P 31.17-31.47
// vs 30.83-31.11 us, profiles/r05/p2p_waves_ab.txt).
#ifndef MPC_CHAIN_FIN_WAVES
#define MPC_CHAIN_FIN_WAVES 5
#endif
template <int MODE>
constexpr int chain_waves() {
  return MODE == kChainFin ? MPC_CHAIN_FIN_WAVES : 5;
}

// PL2 (wheelbase a power of two) is a template parameter, not a runtime
// branch: with both rollout variants inlined the kernel held 119 VGPRs and
// spilled 191 SGPRs; one variant per instantiation: 108-112 VGPRs, 81-86.
// The tile blocks of a chained launch (blocks 1..): stream this step's
// controls through the LDS ring, speculating the step size until block 0 has
// published the step's constants (see k_episode_chain), then the criterion
// and the block's record into part[blockIdx.x - 1] (TAGGED: the exchange
// form, whose records block 0 of the SAME launch collects).  WAIT_TICKS bounds
// the wait for block 0's constants (kChainWaitTicks on one GPU,
// kXchgWaitTicks when block 0 itself waits for peers or a collective).
// Obs (mpc_episode_obs.h FrameObs; NoObs: none): keep-out circles.  The loop
// tests them in the frame of the sums, so the table needs the step's final
// pose before the loop: an obstacle block that does not find the constants
// final in pre0 waits for them there (the same bounded wait, the same
// chain_error) and speculates nothing; obs.form() then makes the table.
// n_blocked: as in rollout_argmin_body.
template <int INTEG, int ROT, bool PL2, bool TAGGED, uint64_t WAIT_TICKS, bool TILED,
          class Obs = NoObs>
__device__ __forceinline__ void chain_tiles(EpisodeState* __restrict__ S, uint32_t epoch,
                                            const double* __restrict__ v,
                                            const double* __restrict__ b, int64_t n_cand,
                                            int n_steps, Rec* __restrict__ part, int has_prev,
                                            const mpc_episode_config_t& ecfg, Obs obs = Obs{},
                                            unsigned long long* __restrict__ n_blocked = nullptr) {
  TL_TILE(0);
  constexpr int CPL = 2;
  __shared__ __attribute__((aligned(16))) uint32_t s_w[kPubWords];
  __shared__ uint32_t s_tag[kPubWords];
  __shared__ int s_final;
  // The step's final constants as the tile's epilogue reads them (the pose
  // transform, the criterion, an irregular candidate's recompute): straight
  // from the published words in LDS (s_w holds Consts' dwords), as VGPR
  // operands loaded where they are used.  Formed in SGPRs (readfirstlane)
  // they did not fit beside the loop's trig coefficients and spilled to VGPR
  // lanes: ~100 v_writelane / v_readlane per wave and tile.
  static_assert(offsetof(Consts, x) == 0 && alignof(Consts) <= 16, "Consts over s_w");
  const Consts& K = *reinterpret_cast<const Consts*>(s_w);
  Consts Kl;
  bool waited = false;
  // After the block's first control loads are in flight: the loop constants.
  // (K itself is formed only after the loop, from the LDS words, so that it
  // is not live in SGPRs across the loop.)
  auto pre0 = [&]() {
    if (threadIdx.x < 64) {
      bool fin = true;
      if (has_prev) {
        fin = chain_read(S, epoch, s_w, s_tag);
      } else if (threadIdx.x < kConstsWords) {   // block 0 only republishes the head
        s_w[threadIdx.x] = reinterpret_cast<const uint32_t*>(&S->h.K)[threadIdx.x];
      }
      if (threadIdx.x == 0) s_final = fin;
    }
    __syncthreads();
    TL_TILE(1);
    Kl = consts_from_words(s_w);
    if constexpr (Obs::kOn) return;   // (first(), below: waits instead of speculating)
    if (s_final) return;
    // speculate h from the published t: the previous step's (+ dt) or, if
    // block 0 already published it, this step's; torn -> NaN (recompute)
    const uint32_t g0 = __builtin_amdgcn_readfirstlane(s_tag[kConstsWords]);
    const uint32_t g1 = __builtin_amdgcn_readfirstlane(s_tag[kConstsWords + 1]);
    const uint64_t tb =
        (static_cast<uint64_t>(static_cast<uint32_t>(
             __builtin_amdgcn_readfirstlane(s_w[kConstsWords + 1]))) << 32) |
        static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(s_w[kConstsWords]));
    double t = __longlong_as_double(static_cast<long long>(tb));
    if (g0 == g1 && g0 == epoch - 1u)
      t = t + ecfg.delta_t;                                   // episode_prepare
    else if (!(g0 == g1 && g0 == epoch))
      t = __builtin_nan("");
    Kl.h = (t + ecfg.delta_t) - t;                            // consts_from_problem: t_b - t_a
  };
  // Three steps before the loop ends (blocks whose constants were not final
  // at the start): wave 0 loads the published words again, in flight with
  // the last control loads, so the end of the loop normally finds them there.
  uint64_t w_pre = 0;
  bool pre_issued = false;
  auto mid = [&]() {
    if (waited || pre_issued || s_final) return;
    pre_issued = true;
    if (threadIdx.x < kPubWords)
      w_pre = __hip_atomic_load(&S->chain_pub[threadIdx.x], __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
  };
  // After the loop: the final constants (called by every thread of the block
  // at the same point, see the clamp below).
  auto wait = [&]() {
    if (waited) return;
    waited = true;
    __syncthreads();   // LDS reuse
    if (!s_final) {
      if (threadIdx.x < 64) {
        bool fin = false;
        if (pre_issued) {
          const bool ok = threadIdx.x >= kPubWords || static_cast<uint32_t>(w_pre) == epoch;
          fin = __ballot(!ok) == 0;
          if (fin && threadIdx.x < kPubWords) s_w[threadIdx.x] = static_cast<uint32_t>(w_pre >> 32);
        }
        // (wave 0 only: its clock reads are uniform)
        // Two polls in flight, issued ~0.1 us apart: a poll's answer is as of
        // when it reached memory, so the words are seen about half a round
        // trip after they land instead of up to one and a half.
        if (!fin) {
          const uint32_t deadline = wall_deadline(WAIT_TICKS);
          const int q = threadIdx.x;
          uint64_t* const pw = &S->chain_pub[q < kPubWords ? q : 0];
          auto ld = [&]() {
            return __hip_atomic_load(pw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          };
          auto here = [&](uint64_t w) {
            return __ballot(q < kPubWords && static_cast<uint32_t>(w) != epoch) == 0;
          };
          uint64_t a = ld(), b = 0, got = 0;
          for (;;) {
            __builtin_amdgcn_s_sleep(2);
            b = ld();
            if (here(a)) { got = a; fin = true; break; }
            if (wall_passed(deadline)) break;
            __builtin_amdgcn_s_sleep(2);
            a = ld();
            if (here(b)) { got = b; fin = true; break; }
            if (wall_passed(deadline)) break;
          }
          if (fin && q < kPubWords) s_w[q] = static_cast<uint32_t>(got >> 32);
        }
        if (!fin && threadIdx.x == 0) S->chain_error = 1u;
      }
      __syncthreads();
    }
    TL_TILE(2);
  };
  // What the lane calls once its first control loads are in flight.
  auto first = [&]() {
    pre0();
    if constexpr (Obs::kOn) {
      if (!s_final) {   // (uniform over the block)
        wait();
        Kl = consts_from_words(s_w);
      }
      obs.form(Kl, PL2);
    }
  };
  // 32-bit candidate indices (the aligned path's rows are < 2^28 candidates,
  // wide_ok): the clamp below is one v_min with a scalar operand, no 64-bit
  // select holding its own registers across the loop
  const int32_t n32 = static_cast<int32_t>(n_cand);
  const int32_t n_tiles = (n32 + kBlock * CPL - 1) / (kBlock * CPL);
  uint64_t best_k = ~0ull;
  int64_t best_i = INT64_MAX;
  [[maybe_unused]] uint32_t wave_blocked = 0;   // (wave-uniform)
  for (int32_t tile = blockIdx.x - 1; tile < n_tiles; tile += gridDim.x - 1) {
    const int32_t c0 = tile * (kBlock * CPL) + static_cast<int32_t>(threadIdx.x) * CPL;
    // lanes past the end of a partial tile roll the last pair again (result
    // ignored), so every lane reaches the barriers of pre0 / wait on the same path
    const int32_t cl = min(c0, n32 - CPL);
    double cst[CPL];
    [[maybe_unused]] bool blocked[CPL];
    // leading trig coefficients not pinned: the fifth wave per SIMD needs the
    // registers more (as the rect+cum stream kernel)
    // TILED: the tile's rows are one contiguous run (tile base + s * 1024
    // doubles), the lane's column its offset within the tile
    const int64_t tb0 = TILED ? static_cast<int64_t>(tile) * (2 * MPC_TILE) * n_steps : 0;
    rollout_lane_glds_k<INTEG, ROT, PL2, decltype(wait), decltype(first), decltype(mid), false,
                        Obs>(K, Kl, v + tb0, b + tb0, TILED ? 2 * MPC_TILE : n_cand,
                             TILED ? cl - tile * MPC_TILE : cl, n_steps, cst, wait, first, mid, obs,
                             blocked);
    if constexpr (Obs::kOn) {   // (every lane: the clamped lanes' repeats are not counted)
#pragma unroll
      for (int j = 0; j < CPL; ++j)
        wave_blocked +=
            __builtin_popcountll(__builtin_amdgcn_ballot_w64(blocked[j] && c0 < n32));
    }
    if (c0 < n32) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        uint64_t kk = cost_key_nonneg(cst[j]);
        if constexpr (Obs::kOn) kk = blocked[j] ? ~0ull : kk;
        if (kk < best_k) {
          best_k = kk;
          best_i = c0 + j;
        }
      }
    }
  }
  if constexpr (Obs::kOn) store_wave_blocked(wave_blocked);
  TL_TILE(4);
  block_argmin<true>(best_k, best_i);   // (indices < n_cand < 2^31)
  TL_TILE(5);
  if (threadIdx.x == 0) {
    if constexpr (TAGGED)
      store_tagged_rec(&part[blockIdx.x - 1], best_k, best_i, epoch);
    else
      part[blockIdx.x - 1] = Rec{best_k, best_i};
    TL_TILE_STORED(3);
  }
  if constexpr (Obs::kOn) add_block_blocked(n_blocked);
}

template <int INTEG, int ROT, int MODE, bool PL2, bool TILED = false>
__global__ __launch_bounds__(kBlock, chain_waves<MODE>()) void k_episode_chain(
    EpisodeState* __restrict__ S, uint32_t epoch, const double* __restrict__ v,
    const double* __restrict__ b, int64_t n_cand, int n_steps, Rec* __restrict__ part,
    int has_prev, const Rec* __restrict__ part_prev, int n_part_prev,
    const double* __restrict__ v_prev, const double* __restrict__ b_prev, int64_t index_base,
    mpc_result_t* __restrict__ out_prev, const mpc_candidate_t* __restrict__ gathered,
    int n_gathered, mpc_episode_config_t ecfg, mpc_episode_log_t* __restrict__ log, int cap,
    uint32_t wait_tag) {
  static_assert(ROT == kRotCum, "chained steps need the pose-independent recurrence");
  if (blockIdx.x == 0) {
    TL_TILE(0);
    if (has_prev) {
      // the completion of step k-1 publishes step k's constants itself, from
      // its LDS copy of the updated head (store_update)
      if constexpr (MODE == kChainP2P) {
        // the previous launch's records -> this rank's candidate, posted to
        // every mailbox; the world's awaited; selection and update.
        // (`gathered` carries the mailbox, n_gathered the world size, wait_tag
        // the previous step's epoch)
        p2p_complete<INTEG, ROT, TILED>(ecfg, S, const_cast<mpc_candidate_t*>(gathered), n_gathered,
                                 wait_tag, part_prev, n_part_prev, v_prev, b_prev, n_cand,
                                 n_steps, index_base, out_prev, log, cap, epoch);
      } else if constexpr (MODE == kChainFin) {
        // (this block-0 body has a copy in k_episode_chain_obs, mpc_episode_obs.h: DESIGN.md §5)
        const Consts Kp = S->h.K;
        const EpisodeHook hook{&S->h, log, cap, S->chain_pub, kPubWords, epoch, &S->chain_error};
        // (block 0 never fills the control ring: its LDS holds the re-roll)
        finalize_block<INTEG, ROT, true, kBlock, false, false, TILED>(
            part_prev, n_part_prev, Kp, v_prev, b_prev, n_cand, n_steps, index_base,
            S->h.incumbent, out_prev, ecfg, hook, ring_lds());
      } else {
        // overlapped exchange: the gathered candidates come from a collective
        // that ran beside this launch — wait for its mark, stage them in LDS.
        // P2P: wait for them in this rank's mailbox (`gathered` carries it,
        // n_gathered the world size, wait_tag the previous step's epoch).
        const mpc_candidate_t* g =
            wait_tag ? wait_gathered(S, wait_tag, gathered, n_gathered) : gathered;
        if (g)
          advance_from_candidates<INTEG, ROT>(ecfg, S, g, n_gathered, out_prev, log, cap,
                                              epoch, ring_lds());
        else   // timed out (chain error 4): publish the unchanged head so no tile hangs
          chain_publish(S, epoch);
      }
      __syncthreads();   // (the wheelbase check below reads the stored head)
    } else {
      chain_publish(S, epoch);   // no previous step: the head as reset / last updated
    }
    // The host picked PL2 from the caller's cfg; the tile blocks use the
    // published head's wheelbase terms.  If those disagree (a cfg other than
    // the one the state was reset with) every dphi would be formed with the
    // wrong form: flag it (chain_error = 2) instead of returning wrong costs
    // silently.  (chain_publish ended with a barrier after the head store.)
    if (threadIdx.x == 0 && (S->h.K.L_pow2 != 0) != PL2) S->chain_error = 2u;
    // kChainXchg passes the rank's candidate record in part_prev's slot (one
    // kernel argument fewer: a further SGPR pair spilled a VGPR)
    if constexpr (MODE == kChainXchg)
      collect_local_candidate(part, gridDim.x - 1, epoch, v, b, n_cand, n_steps, index_base,
                              reinterpret_cast<mpc_candidate_t*>(const_cast<Rec*>(part_prev)),
                              &S->chain_error);
    return;
  }
  static_assert(!TILED || MODE != kChainXchg, "the all_gather form reads SoA controls");
  chain_tiles<INTEG, ROT, PL2, MODE == kChainXchg,
              MODE == kChainFin ? kChainWaitTicks : kXchgWaitTicks, TILED>(
      S, epoch, v, b, n_cand, n_steps, part, has_prev, ecfg);
}

}  // namespace mpc
