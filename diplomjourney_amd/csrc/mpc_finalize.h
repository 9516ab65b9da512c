// mpc_finalize.h — a step's completion: the block records' reduction, the
// winner's re-roll and, on one GPU, the episode update (gfx950).
//
//   store_update       the episode update's stores, one word per lane
//   u64x2, load8_rec_sc1, load8_rec_sc1_sbase   block records read `sc1`
//   NoRecSrc, finalize_block   arg-min over the block records; the winner
//                      re-rolled (mpc_winner.h); the update (mpc_episode.h) and
//                      a chained step's early publication
//   k_finalize_gen, k_finalize   the selection as a kernel of its own
//   k_rollout_episode  the streaming rollout whose last block finalizes
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/mpc_rollout.h"
#include "mpc_argmin.h"
#include "mpc_device.h"
#include "mpc_episode.h"
#include "mpc_lanes.h"
#include "mpc_timeline.h"
#include "mpc_winner.h"

namespace mpc {

// The episode update's stores, one 8-B word per lane (called by every thread
// after a barrier; thread 0 staged the head and the log record in LDS): a
// single lane's ~40 stores serialise in the address path for ~0.7 us.
// epoch != 0 (a chained launch's block 0): instead of clearing the chain
// tags, publish the updated head's Consts and t as epoch-tagged words (the
// layout of EpisodeState::chain_pub: Consts' dwords, then t's two) straight
// from the LDS copy — not re-read from HBM after the head's stores, which
// would put a store drain and a load round trip in front of the publication.
// published: the head's Consts are the published words `pub` (the early
// publication's), not s_head's.
__device__ __forceinline__ void store_update(EpisodeHead* H, const uint64_t* s_head,
                                             mpc_episode_log_t* slot, const uint64_t* s_log,
                                             uint64_t* chain_pub, int chain_words,
                                             uint32_t epoch = 0, bool published = false,
                                             const uint32_t* pub = nullptr) {
  const int q = threadIdx.x;
  if (chain_pub && q < chain_words && !published) {
    if (epoch) {
      constexpr int kKWords = static_cast<int>(sizeof(Consts) / 4);
      const uint32_t* dw = reinterpret_cast<const uint32_t*>(s_head);
      const uint32_t d =
          q < kKWords ? dw[q] : dw[offsetof(EpisodeHead, t) / 4 + (q - kKWords)];
      __hip_atomic_store(&chain_pub[q], (static_cast<uint64_t>(d) << 32) | epoch,
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      chain_pub[q] = 0ull;
    }
  }
  constexpr int kKQ = static_cast<int>(sizeof(Consts) / 8);
  if (q < kStoredWords)   // head, then StaleTraj
    reinterpret_cast<uint64_t*>(H)[q] =
        (published && q < kKQ) ? reinterpret_cast<const uint64_t*>(pub)[q] : s_head[q];
  if (slot && q < kLogWords) reinterpret_cast<uint64_t*>(slot)[q] = s_log[q];
}

// Block-record reduction + winner re-roll (+ episode update), run by every
// thread of one block of NT threads.  SC1: the records were written by
// blocks of the SAME launch (fused path): they were stored `sc1` and are read
// `sc1` (L1 bypassed; the counter hand-off of rollout_episode).
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// Eight records, `sc1`, in ONE statement that also waits for them: an asm
// load's destination is written whenever the data arrives, so it must never
// leave the statement un-waited (hipcc may copy or reuse the register).
__device__ __forceinline__ void load8_rec_sc1(const Rec* const (&p)[8], u64x2 (&r)[8]) {
  asm volatile(
      "global_load_dwordx4 %0, %8, off sc1\n\t"
      "global_load_dwordx4 %1, %9, off sc1\n\t"
      "global_load_dwordx4 %2, %10, off sc1\n\t"
      "global_load_dwordx4 %3, %11, off sc1\n\t"
      "global_load_dwordx4 %4, %12, off sc1\n\t"
      "global_load_dwordx4 %5, %13, off sc1\n\t"
      "global_load_dwordx4 %6, %14, off sc1\n\t"
      "global_load_dwordx4 %7, %15, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(r[4]), "=&v"(r[5]),
        "=&v"(r[6]), "=&v"(r[7])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7])
      : "memory");
}

// The same from a wave-uniform base (SGPR pair) and 32-bit byte offsets: one
// VGPR per address instead of two (block 0 of the chained exchange step polls
// its records with these, and its register peak is the kernel's).
__device__ __forceinline__ void load8_rec_sc1_sbase(const Rec* base, const uint32_t (&o)[8],
                                                    u64x2 (&r)[8]) {
  // (the base through readfirstlane: uniform for the compiler whatever loop
  // the call sits in, so the "s" operand is an SGPR pair)
  const uint64_t ab = reinterpret_cast<uint64_t>(base);
  base = reinterpret_cast<const Rec*>(
      (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(
           static_cast<int>(ab >> 32)))) << 32) |
      static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(ab))));
  asm volatile(
      "s_nop 4\n\t"   // VALU-written SGPR -> VMEM: see glds_pair
      "global_load_dwordx4 %0, %8, %16 sc1\n\t"
      "global_load_dwordx4 %1, %9, %16 sc1\n\t"
      "global_load_dwordx4 %2, %10, %16 sc1\n\t"
      "global_load_dwordx4 %3, %11, %16 sc1\n\t"
      "global_load_dwordx4 %4, %12, %16 sc1\n\t"
      "global_load_dwordx4 %5, %13, %16 sc1\n\t"
      "global_load_dwordx4 %6, %14, %16 sc1\n\t"
      "global_load_dwordx4 %7, %15, %16 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(r[4]), "=&v"(r[5]),
        "=&v"(r[6]), "=&v"(r[7])
      : "v"(o[0]), "v"(o[1]), "v"(o[2]), "v"(o[3]), "v"(o[4]), "v"(o[5]), "v"(o[6]), "v"(o[7]),
        "s"(base)
      : "memory");
}

// GEN (generated controls, k_rollout_generated): v / b are [n_part][MPC_MAX_STEPS]
// — the controls of each rollout block's best candidate — instead of the
// [n_steps][n_cand] candidate arrays; the winner's are those of its block.
// Src: where the block records come from.  NoRecSrc: `part` / `n_part` as
// below; otherwise src(k, i) leaves in every thread the lexicographic minimum
// of its share of the records (the persistent run's selector, which polls the
// tagged records of the same launch: mpc_run.h).
struct NoRecSrc {};
template <int INTEG, int ROT, bool KDEV, int NT, bool SC1, bool GEN = false, bool TILED = false,
          class Src = NoRecSrc>
__device__ __forceinline__ void finalize_block(
    const Rec* __restrict__ part, int n_part, const Consts& K, const double* __restrict__ v,
    const double* __restrict__ b, int64_t n_cand, int n_steps, int64_t index_base,
    double incumbent, mpc_result_t* __restrict__ out, const mpc_episode_config_t& ecfg,
    const EpisodeHook& hook, EmitLds* lds, const Src& src = Src{}) {
  // One-GPU episode: the episode scalars are staged in LDS by wave 1 (one
  // 8-B vector load per lane, issued after its record loads) and updated by
  // thread 0 once the winner is known.  (Loading them into thread 0's SGPRs
  // serialised three scalar round trips in front of wave 0's record loads.)
  static_assert(NT >= 128, "head staging by wave 1");
  static_assert(MPC_MAX_STEPS * 3 <= NT, "trajectory stored one value per lane");
  __shared__ uint64_t s_head[kStagedWords];
  __shared__ mpc_episode_log_t s_log;   // filled field by field by the update
  __shared__ mpc_episode_log_t* s_slot;
  __shared__ uint64_t s_key[NT / 64];
  __shared__ int64_t s_idx[NT / 64];
  // the early publication (chained step's block 0, below)
  constexpr int kKWords = static_cast<int>(sizeof(Consts) / 4);
  __shared__ __attribute__((aligned(8))) uint32_t s_pub[64];
  __shared__ double2 s_sc[3];
  __shared__ int s_early, s_pose, s_sc_ready;
  uint64_t k = ~0ull;
  int64_t i = INT64_MAX;
  // wave 1's head words, loaded BEFORE its records so that both are in flight
  // together (the block barrier after the reduction waits for the staging)
  const bool stage = KDEV && hook.H && threadIdx.x >= 64 && threadIdx.x < 64 + kStagedWords;
  const uint64_t head_word =
      stage ? reinterpret_cast<const uint64_t*>(hook.H)[threadIdx.x - 64] : 0ull;
  if constexpr (!std::is_same_v<Src, NoRecSrc>) {
    src(k, i);
  } else if constexpr (SC1) {
    // n_part <= kMaxBlocks = 8 * NT: eight loads per thread, addresses of
    // out-of-range slots clamped to a valid record and their values ignored
    static_assert(kMaxBlocks <= 8 * NT, "load8_rec_sc1 covers 8 records per thread");
    const Rec* ptr[8];
    u64x2 r[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int p = threadIdx.x + q * NT;
      ptr[q] = part + (p < n_part ? p : n_part - 1);
    }
    load8_rec_sc1(ptr, r);
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (threadIdx.x + q * NT < n_part &&
          rec_less(r[q].x, static_cast<int64_t>(r[q].y), k, i)) {
        k = r[q].x;
        i = static_cast<int64_t>(r[q].y);
      }
  } else if (n_part <= NT) {
    // at most one record per thread (a small launch, config B's 196): no
    // compare chain over seven sentinel records on the selection's path
    if (static_cast<int>(threadIdx.x) < n_part) {
      const Rec r = part[threadIdx.x];
      k = r.key;
      i = r.idx;
    }
  } else {
    // all of this thread's records are loaded before any is compared, so
    // the loads overlap (one memory round trip)
    constexpr int kPer = (kMaxBlocks + NT - 1) / NT;
    Rec r[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int p = threadIdx.x + q * NT;
      r[q] = p < n_part ? part[p] : Rec{~0ull, INT64_MAX};
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q)
      if (rec_less(r[q].key, r[q].idx, k, i)) {
        k = r[q].key;
        i = r[q].idx;
      }
  }
  TL_B0(1);
  if (stage) s_head[threadIdx.x - 64] = head_word;
  // record indices are local candidate indices: below 2^31 for any row the
  // candidate arrays can hold in practice -> three 32-bit DPP minima
  if (!GEN && n_cand < (int64_t{1} << 31))
    wave_argmin32(k, i);
  else
    wave_argmin(k, i);
  TL_B0(2);
  // Each wave's best candidate's controls, loaded while the waves' minima are
  // combined: the block's winner is one of them, so its re-roll starts
  // without a dependent load of its own (one memory round trip fewer on the
  // selection's critical path; the same values, so the same arithmetic).
  double* s_pv = lds->pv;
  double* s_pb = lds->pb;
  double pv = 0.0, pb = 0.0;
  const int ln = threadIdx.x & 63;
  if constexpr (!GEN) {
    if (k != ~0ull && ln < n_steps) {
      const int64_t o = ctl_off<TILED>(ln, i, TILED ? n_steps : n_cand);
      pv = v[o];
      pb = b[o];
    }
  }
  if (ln == 0) {
    s_key[threadIdx.x >> 6] = k;
    s_idx[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  // every thread forms the block's winner (thread 0's result as before), so
  // the wave that holds it knows to stage its controls
  TL_B0(3);
  int wbest = 0;
  k = s_key[0];
  i = s_idx[0];
  for (int w = 1; w < NT / 64; ++w)
    if (rec_less(s_key[w], s_idx[w], k, i)) {
      k = s_key[w];
      i = s_idx[w];
      wbest = w;
    }
  if constexpr (!GEN) {
    if ((threadIdx.x >> 6) == wbest && ln < n_steps) {
      s_pv[ln] = pv;
      s_pb[ln] = pb;
    }
  }   // (emit_winner's first barrier orders these stores before its reads)
  Winner w;
  if constexpr (GEN) {
    // (thread 0 holds the winner; emit_winner takes its column from thread 0)
    // (k_rollout_generated: 2 candidates per lane, tiles dealt round-robin)
    const int64_t col = k == ~0ull ? 0 : ((i / (kBlock * 2)) % n_part) * MPC_MAX_STEPS;
    emit_winner<INTEG, ROT>(K, v, b, 1, n_steps, k, col, index_base + i, incumbent, out, lds, &w);
  } else {
    // A chained step's block 0: in the common step (no event, no end of the
    // episode) the next step's published words follow from the new pose
    // alone, so they go out before the rest of the update — the tile blocks
    // waiting for them do not also wait for the log record, the stale
    // trajectory, the event and restart logic and the head's stores.  What
    // does not need the winner was formed by the previous update (the head's
    // early_* fields); wave 3 lays out the words that carry over while wave 0
    // forms the per-step factors, and wave 1 evaluates sin / cos of the
    // winner's layer headings (the pass's own sums, in its order) during lane
    // 0's serial pass.
    const EpisodeHead& Hs = *reinterpret_cast<const EpisodeHead*>(s_head);
    const EarlyPub& Es = *reinterpret_cast<const EarlyPub*>(&s_head[kStoredWords]);
    const bool early_on = KDEV && hook.H && hook.publish_epoch;
    auto side_a = [&]() {
      const int q = threadIdx.x - 192;
      if (!early_on || q < 0 || q >= 64) return;
      constexpr int kH = static_cast<int>(offsetof(Consts, h) / 4);
      constexpr int kHl = static_cast<int>(offsetof(Consts, hlgth) / 4);
      static_assert(kHl == kH + 2, "h, hlgth adjacent");
      const uint32_t* kw = reinterpret_cast<const uint32_t*>(s_head);   // Hs.K's dwords
      const uint32_t* ew = reinterpret_cast<const uint32_t*>(&Es.t);   // t, h, hl
      if (q < kKWords)
        s_pub[q] = (q >= kH && q < kH + 4) ? ew[2 + (q - kH)] : kw[q];
      else if (q < kKWords + 2)
        s_pub[q] = ew[q - kKWords];
    };
    // The pick: the winner's layer jj = min(k, N-1) as lane 0 forms it in the
    // serial pass (on_layer: the end-of-step checks, the pose into s_pub,
    // s_pose = 1 publish / 2 not), or the no-winner pose (decided by wave 3
    // alone); wave 3 then adds sin / cos and publishes — while lane 0 goes on
    // with the remaining layers.
    const bool can_early =
        early_on && Es.step == Hs.step && Es.k >= 0;   // (uniform: LDS words, all threads)
    const bool valid_w = k != ~0ull;
    const bool found_w = valid_w && key_cost(k) < incumbent;   // emit_winner's `found`
    const int jj_w = can_early ? (Es.k < n_steps - 1 ? Es.k : n_steps - 1) : -1;
    if (threadIdx.x == 0) {   // (LDS starts undefined; read only after emit_winner's barriers)
      s_pose = 0;
      s_sc_ready = 0;
    }
    auto on_layer = [&](int st, double x, double y, double ph) {
      if (!can_early || !found_w || st != jj_w) return;
      const bool ok = early_pose_ok(ecfg, Hs, x, y);
      if (ok) {
        Consts& Kp = *reinterpret_cast<Consts*>(s_pub);
        Kp.x = x;
        Kp.y = y;
        Kp.phi = ph;
      }
      __hip_atomic_store(&s_pose, ok ? 1 : 2, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      TL_B0_IF(true, 19);
    };
    auto side_b = [&](bool fast) {
      const int q = threadIdx.x;
      if (early_on && q >= 64 && q < 64 + 3) {
        const int last = n_steps - 1, jj = q - 64 < last ? q - 64 : last;
        double ph;
        if (fast) {   // emit_winner's fast pass: K.phi + dphi_0 + ... in step order
          ph = K.phi;
          for (int st = 0; st <= jj; ++st) ph = ph + lds->dphi[st];
        } else {
          ph = lds->phi[jj];
        }
        // sincos_fast's own core (the same bits) on its range; beyond it (a
        // heading of more than 2^19 pi / 2, never in practice) no early
        // publication — the large reduction's code would cost the kernel
        // scratch memory
        double sn = 0.0, cs = 0.0;
        const bool in = fabs(ph) <= trig::kFastMax;
        if (in) trig::sincos_core(ph, &sn, &cs);
        s_sc[q - 64] = make_double2(sn, cs);
        const bool all_in = __ballot(!in) == 0;
        if (q == 64)   // (the wave's three LDS stores are in order before it)
          __hip_atomic_store(&s_sc_ready, all_in ? 1 : 2, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
        TL_B0_IF(q == 64, 18);
      }
      if (early_on && q >= 192 && q < 256) {   // wave 3: the pick's last part, the publication
        if (q == 192) {
          int pub = 0;
          if (can_early) {
            Consts& Kp = *reinterpret_cast<Consts*>(s_pub);
            if (!found_w) {   // the no-winner pose: the stale layer k, or the pose
              if (Es.alt && fabs(Es.ph) <= trig::kFastMax) {
                double sn, cs;
                trig::sincos_core(Es.ph, &sn, &cs);   // (= sincos_fast on its range)
                Kp.x = Es.x;
                Kp.y = Es.y;
                Kp.phi = Es.ph;
                Kp.s0 = sn;
                Kp.c0 = cs;
                pub = 1;
              }
            } else {
              // lane 0's pose and wave 1's sin / cos (bounded waits: an
              // unanswered one only forgoes the early publication)
              int pose = 0, sc = 0;
              for (uint32_t it = 0; it < (1u << 22) && (pose == 0 || sc == 0); ++it) {
                pose = __hip_atomic_load(&s_pose, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                sc = __hip_atomic_load(&s_sc_ready, __ATOMIC_ACQUIRE,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                if (pose == 2 || sc == 2) break;
                if (pose == 0 || sc == 0) __builtin_amdgcn_s_sleep(1);
              }
              if (pose == 1 && sc == 1) {
                Kp.s0 = s_sc[jj_w].x;
                Kp.c0 = s_sc[jj_w].y;
                pub = 1;
              }
            }
          }
          s_early = pub;
        }
        // thread 192's LDS stores, then wave 3's reads (one wave)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int w3 = q - 192;
        if (s_early && w3 < hook.chain_pub_words)
          __hip_atomic_store(&hook.chain_pub[w3],
                             (static_cast<uint64_t>(s_pub[w3]) << 32) | hook.publish_epoch,
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        TL_B0_IF(q == 192, 13);
      }
    };
    emit_winner<INTEG, ROT>(K, v, b, n_cand, n_steps, k, i, index_base + i, incumbent, out, lds,
                            &w, s_pv, s_pb, KDEV && hook.H, side_a, side_b, on_layer);
  }
  TL_B0(5);
  if (KDEV && hook.H) {
    const bool early = hook.publish_epoch && s_early;   // (uniform)
    if (threadIdx.x == 0) {
      // on the LDS copy itself: the update touches a few of its words, and a
      // copy into registers and back costs more than it saves; after an early
      // publication the constants are left as published
      bool bad = false;
      episode_hook(ecfg, hook, w, *reinterpret_cast<EpisodeHead*>(s_head),
                   *reinterpret_cast<StaleTraj*>(&s_head[kHeadWords]), s_log, s_slot,
                   early ? s_pub : nullptr, &bad);
      TL_B0(7);
      if (bad && hook.chain_error) *hook.chain_error = 6u;
    }
    __syncthreads();
    if (hook.publish_epoch && threadIdx.x == 64) {
      // the next step's early-publication inputs, beside the head's stores
      // (an EarlyPub follows the stale trajectory in the state)
      EarlyPub E;
      episode_early_prepare(ecfg, *reinterpret_cast<const EpisodeHead*>(s_head),
                            *reinterpret_cast<const StaleTraj*>(&s_head[kHeadWords]), E);
      *reinterpret_cast<EarlyPub*>(reinterpret_cast<uint64_t*>(hook.H) + kStoredWords) = E;
      TL_B0_IF(true, 15);
    }
    // the head and the log record back to HBM, the chain tags cleared (or the
    // next step's constants published, unless they already are)
    store_update(hook.H, s_head, s_slot, reinterpret_cast<const uint64_t*>(&s_log),
                 hook.chain_pub, hook.chain_pub_words, hook.publish_epoch, early, s_pub);
    TL_B0(8);
    // the record's remaining trajectory, off the update's critical path
    emit_winner_tail<INTEG, ROT>(K, n_steps, lds, out);
    TL_B0(14);
  }
}

// The selection of a generated-controls step (GEN finalize_block).
template <int INTEG, int ROT>
__global__ __launch_bounds__(kFinBlock) void k_finalize_gen(
    const Rec* __restrict__ part, int n_part, const Consts* __restrict__ Kdev,
    const double* __restrict__ part_v, const double* __restrict__ part_b, int n_steps,
    int64_t index_base, const double* __restrict__ incumbent_dev,
    mpc_result_t* __restrict__ out, mpc_episode_config_t ecfg, EpisodeHook hook) {
  const Consts K = *Kdev;
  __shared__ EmitLds lds;
  finalize_block<INTEG, ROT, true, kFinBlock, false, true>(part, n_part, K, part_v, part_b, 0,
                                                           n_steps, index_base, *incumbent_dev,
                                                           out, ecfg, hook, &lds);
}

template <int INTEG, int ROT, bool KDEV, bool TILED = false>
__global__ __launch_bounds__(kFinBlock) void k_finalize(
    const Rec* __restrict__ part, int n_part, Consts Karg, const Consts* __restrict__ Kdev,
    const double* __restrict__ v, const double* __restrict__ b, int64_t n_cand, int n_steps,
    int64_t index_base, double incumbent_arg, const double* __restrict__ incumbent_dev,
    mpc_result_t* __restrict__ out, mpc_episode_config_t ecfg, EpisodeHook hook) {
  const Consts K = KDEV ? *Kdev : Karg;
  const double incumbent = KDEV ? *incumbent_dev : incumbent_arg;
  __shared__ EmitLds lds;
  finalize_block<INTEG, ROT, KDEV, kFinBlock, false, false, TILED>(
      part, n_part, K, v, b, n_cand, n_steps, index_base, incumbent, out, ecfg, hook, &lds);
}

// Device-resident episode, one launch per MPC step: the streaming rollout +
// block arg-min of k_rollout_argmin, then the LAST block to finish runs the
// finalize (record reduction, winner re-roll, and on one GPU the episode
// update).  Hand-off (MI355X_MICROARCH.md, inter-workgroup visibility): each
// block's thread 0 stores its record `sc1`, waits for it (vmcnt(0)), then adds
// to the launch counter (agent-scope atomic); the block whose add returns
// gridDim-1 is last, and its threads read every record `sc1` after a
// workgroup barrier.  The last block re-arms the counter for the next launch.
template <int CPL, int INTEG, int ROT>
__global__ __launch_bounds__(kBlock, 1) void k_rollout_episode(
    const Consts* __restrict__ Kdev, const double* __restrict__ v, const double* __restrict__ b,
    int64_t n_cand, int n_steps, int64_t index_base, Rec* __restrict__ part,
    uint32_t* __restrict__ done, const double* __restrict__ incumbent_dev,
    mpc_result_t* __restrict__ out, mpc_episode_config_t ecfg, EpisodeHook hook) {
  const Consts K = *Kdev;
  const int64_t n_tiles = (n_cand + kBlock * CPL - 1) / (kBlock * CPL);
  uint64_t best_k = ~0ull;
  int64_t best_i = INT64_MAX;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t c0 = tile * (kBlock * CPL) + threadIdx.x * CPL;
    if (c0 < n_cand) {
      double cst[CPL];
      rollout_lane<CPL, INTEG, ROT, false>(K, v, b, n_cand, c0, n_steps, cst, nullptr, n_cand);
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const uint64_t kk = cost_key_nonneg(cst[j]);
        if (kk < best_k) {
          best_k = kk;
          best_i = c0 + j;
        }
      }
    }
  }
  block_argmin(best_k, best_i);
  __shared__ int s_last;
  if (threadIdx.x == 0) {
    Rec* dst = part + blockIdx.x;
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)"
                 :
                 : "v"(dst),
                   "v"(u64x2{best_k, static_cast<uint64_t>(best_i)})
                 : "memory");
    const uint32_t prev =
        __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  // (the block's control ring is drained: its LDS holds the re-roll)
  finalize_block<INTEG, ROT, true, kBlock, true>(part, gridDim.x, K, v, b, n_cand, n_steps,
                                                 index_base, *incumbent_dev, out, ecfg, hook,
                                                 ring_lds());
  if (threadIdx.x == 0) *done = 0u;
}

}  // namespace mpc
