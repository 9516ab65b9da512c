// mpc_exchange.h — the multi-GPU episode: per-rank winners or candidates
// exchanged by a collective or through P2P mailboxes, then the update (gfx950).
//
//   kWallHz .. block_wall_passed   bounded device waits on the wall clock
//   advance_from_results, k_episode_advance   selection over the gathered
//                      per-rank winners, then the episode update
//   advance_from_candidates, k_episode_advance_cand   the same over gathered
//                      candidates, the winner re-rolled from its controls
//   rec_tag .. tagged_rec_index, collect_local_candidate   a launch's tagged
//                      block records -> the rank's candidate
//   k_exchange_mark, wait_gathered   the overlapped all_gather's hand-off
//   chain_publish      the head's constants as epoch-tagged words (here, not in
//                      mpc_chain.h: a timed-out mailbox wait publishes too)
//   MailHdr .. p2p_complete, k_mailbox_ping, k_episode_p2p_flush   the mailbox exchange
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_argmin.h"
#include "mpc_episode.h"
#include "mpc_finalize.h"
#include "mpc_kernels.h"
#include "mpc_lanes.h"
#include "mpc_timeline.h"
#include "mpc_winner.h"

namespace mpc {

// Bounded device waits, measured on the GPU's constant-rate wall clock
// (wall_clock64: s_memrealtime, 100 MHz on gfx950) rather than in poll passes,
// so that waits of different loops compare: a wait that runs out sets
// chain_error instead of hanging the GPU.
//   kChainWaitTicks   one GPU: a chained launch's tiles wait for block 0,
//                     which waits for nothing outside the launch
//   kPeerWaitTicks    block 0 waits for other ranks (P2P mailbox, error 5) or
//                     for a collective beside the launch (error 4); ranks are
//                     not barrier-aligned between steps, so a peer may start
//                     the same step a host hiccup later
//   kXchgWaitTicks    an exchange launch's tiles wait for THAT block 0: longer
//                     than its peer wait, so a late peer surfaces as block 0's
//                     error (or not at all), never as tiles scoring the step on
//                     speculated constants (error 1)
constexpr uint64_t kWallHz = 100000000ull;
constexpr uint64_t kChainWaitTicks = kWallHz / 5;        // 0.2 s
constexpr uint64_t kPeerWaitTicks = 2 * kWallHz;         // 2 s
constexpr uint64_t kXchgWaitTicks = 3 * kWallHz;         // 3 s
static_assert(kXchgWaitTicks > kPeerWaitTicks, "tiles outwait their block 0");

// 32-bit deadlines (one register; the low word wraps after 42 s, far beyond
// any budget here, and the comparison is wrap-safe)
__device__ __forceinline__ uint32_t wall_deadline(uint64_t ticks) {
  return static_cast<uint32_t>(wall_clock64()) + static_cast<uint32_t>(ticks);
}
__device__ __forceinline__ bool wall_passed(uint32_t deadline) {
  return static_cast<int32_t>(static_cast<uint32_t>(wall_clock64()) - deadline) > 0;
}
// Block-wide (all threads, same pass): has the deadline passed?  Thread 0's
// clock decides, so every wave leaves a __syncthreads_* poll on the same pass.
__device__ __forceinline__ bool block_wall_passed(uint32_t deadline) {
  // (readfirstlane: the compiler sees a uniform value, so a loop that leaves
  // on it stays uniform and its loop-invariant pointers stay in SGPRs)
  return __builtin_amdgcn_readfirstlane(
             __syncthreads_or(threadIdx.x == 0 && wall_passed(deadline))) != 0;
}

// Multi-GPU: lexicographic (cost, global index) selection over the gathered
// per-rank winners (the all-reduce(min+index)), then the episode update.
// Called by every thread of a block (>= 64 threads): thread 0 updates a
// register copy of the head, which goes back to HBM through LDS one word per
// lane (a single lane's stores serialise); end_chain clears the chain tags.
__device__ inline void advance_from_results(const mpc_episode_config_t& c, EpisodeState* S,
                                            const mpc_result_t* __restrict__ res, int n,
                                            mpc_episode_log_t* __restrict__ log, int cap,
                                            bool end_chain = true) {
  __shared__ uint64_t s_head[kStoredWords];
  __shared__ mpc_episode_log_t s_log;
  __shared__ mpc_episode_log_t* s_slot;
  if (threadIdx.x < kStaleWords)   // the stale trajectory, staged beside the head
    s_head[kHeadWords + threadIdx.x] = reinterpret_cast<const uint64_t*>(&S->st)[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    EpisodeHead H = S->h;
    uint64_t bk;
    const int best = select_index(res, n, bk);
    const mpc_result_t& r = res[best];
    Winner w;
    w.cost = r.cost;
    w.index = r.index;
    w.found = (bk != ~0ull && r.cost < H.incumbent) ? 1 : 0;
    w.n_steps = r.n_steps;
    w.v = r.v;
    w.beta = r.beta;
    for (int k = 0; k < 3; ++k)
      for (int q = 0; q < 3; ++q) w.tr[k][q] = r.traj[k < r.n_steps ? k : 0][q];
    s_slot = log_slot(log, cap, H.step);
    episode_advance(c, H, *reinterpret_cast<StaleTraj*>(&s_head[kHeadWords]), w, s_log);
    __builtin_memcpy(s_head, &H, sizeof(EpisodeHead));
  }
  __syncthreads();
  store_update(&S->h, s_head, s_slot, reinterpret_cast<const uint64_t*>(&s_log),
               end_chain ? S->chain_pub : nullptr, kPubWords);
}

// Multi-GPU chained exchange: the global winner of a step among the gathered
// per-rank candidates (lexicographic (cost, global index)), re-rolled from its
// gathered controls with the step's constants (emit_winner: the same
// operations as the rollout that scored it) into `out`, then the episode
// update.  Every thread of a block of kFinBlock threads.
template <int INTEG, int ROT>
__device__ void advance_from_candidates(const mpc_episode_config_t& c, EpisodeState* S,
                                        const mpc_candidate_t* __restrict__ g, int n,
                                        mpc_result_t* __restrict__ out,
                                        mpc_episode_log_t* __restrict__ log, int cap,
                                        uint32_t publish_epoch, EmitLds* lds) {
  __shared__ uint64_t s_head[kStoredWords];
  __shared__ mpc_episode_log_t s_log;
  __shared__ mpc_episode_log_t* s_slot;
  __shared__ int s_best;
  __shared__ uint64_t s_bk;
  if (threadIdx.x < kStoredWords)
    s_head[threadIdx.x] = reinterpret_cast<const uint64_t*>(&S->h)[threadIdx.x];
  if (threadIdx.x == 0) {
    int best = 0;
    uint64_t bk = ~0ull;
    int64_t bi = INT64_MAX;
    for (int r = 0; r < n; ++r) {
      const uint64_t k = g[r].index < 0 ? ~0ull : cost_key(g[r].cost);
      const int64_t i = g[r].index < 0 ? INT64_MAX : g[r].index;
      if (r == 0 || rec_less(k, i, bk, bi)) {
        best = r;
        bk = k;
        bi = i;
      }
    }
    s_best = best;
    s_bk = bk;
  }
  __syncthreads();
  const mpc_candidate_t* w = &g[s_best];
  const EpisodeHead* Hs = reinterpret_cast<const EpisodeHead*>(s_head);
  const Consts K = Hs->K;                // the step's constants (before the update)
  Winner win;
  emit_winner<INTEG, ROT>(K, nullptr, nullptr, 0, w->n_steps, s_bk, 0, w->index, Hs->incumbent,
                          out, lds, &win, w->v, w->beta, true);
  if (threadIdx.x == 0) {   // emit_winner ended with a barrier; lane 0 holds `win`
    EpisodeHead H;
    __builtin_memcpy(&H, s_head, sizeof(EpisodeHead));
    s_slot = log_slot(log, cap, H.step);
    episode_advance(c, H, *reinterpret_cast<StaleTraj*>(&s_head[kHeadWords]), win, s_log);
    __builtin_memcpy(s_head, &H, sizeof(EpisodeHead));
  }
  __syncthreads();
  // publish_epoch 0: the update ends the chain (tags cleared); else it
  // publishes the next step's constants (a chained exchange step's block 0)
  store_update(&S->h, s_head, s_slot, reinterpret_cast<const uint64_t*>(&s_log), S->chain_pub,
               kPubWords, publish_epoch);
  TL_B0(8);
  emit_winner_tail<INTEG, ROT>(K, w->n_steps, lds, out);   // the rest of the record
}

template <int INTEG, int ROT>
__global__ __launch_bounds__(kFinBlock) void k_episode_advance_cand(
    mpc_episode_config_t c, EpisodeState* __restrict__ S, const mpc_candidate_t* __restrict__ g,
    int n, mpc_result_t* __restrict__ out, mpc_episode_log_t* __restrict__ log, int cap) {
  __shared__ EmitLds lds;
  advance_from_candidates<INTEG, ROT>(c, S, g, n, out, log, cap, 0u, &lds);
}

// A tile block's record in an exchange step: ONE 16-B `sc1` store that block
// 0 of the same launch polls for (no counter, no wait in the tile block).
// Freshness must not rest on the 16-B store and load being single-copy
// atomic (the memory model promises that only up to 8 B), so EACH 8-B half
// carries the launch's 16-bit tag in its low bits and block 0 accepts the
// record only when both halves show it:
//   word 0 = key[63:16] << 16 | tag
//   word 1 = key[15:0] << 48 | index[31:0] << 16 | tag
// (the 64-bit cost key and a 32-bit local index; no candidate: index
// 0xffffffff).  A half torn from an older record carries another tag (or the
// 0 of a consumed record) and is polled again.
__device__ __forceinline__ uint32_t rec_tag(uint32_t epoch) {
  return epoch % 0xffffu + 1u;   // in [1, 0xffff]; consecutive epochs differ, 0 = untagged
}

__device__ __forceinline__ void store_tagged_rec(Rec* dst, uint64_t key, int64_t idx,
                                                 uint32_t epoch) {
  const uint64_t ix = idx == INT64_MAX ? 0xffffffffull
                                       : static_cast<uint64_t>(static_cast<uint32_t>(idx));
  const uint64_t tag = rec_tag(epoch);
  const uint64_t w0 = (key & ~0xffffull) | tag;
  const uint64_t w1 = (key << 48) | (ix << 16) | tag;
  // (s_nop 1: the store must read its data registers before the compiler's
  // next instruction may overwrite them)
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1"
               :
               : "v"(dst), "v"(u64x2{w0, w1})
               : "memory");
}

__device__ __forceinline__ bool tagged_rec_fresh(const u64x2& r, uint32_t tag) {
  return static_cast<uint32_t>(r.x & 0xffffu) == tag && static_cast<uint32_t>(r.y & 0xffffu) == tag;
}

__device__ __forceinline__ uint64_t tagged_rec_key(const u64x2& r) {
  return (r.x & ~0xffffull) | (r.y >> 48);
}

__device__ __forceinline__ uint32_t tagged_rec_index(const u64x2& r) {
  return static_cast<uint32_t>(r.y >> 16);
}

// Block 0 of an exchange step, after publishing: wait until every tile
// block's record of THIS launch has landed (tags == epoch; `sc1` loads, a
// bounded poll), reduce them and write this rank's best candidate — its
// (cost, global index) and its controls, one step per lane — to `out`.
__device__ void collect_local_candidate(const Rec* __restrict__ part, int n_part, uint32_t epoch,
                                        const double* __restrict__ v,
                                        const double* __restrict__ b, int64_t n_cand,
                                        int n_steps, int64_t index_base,
                                        mpc_candidate_t* __restrict__ out, uint32_t* err) {
  static_assert(kMaxBlocks <= 8 * kBlock, "eight records per thread");
  uint32_t off[8];   // byte offsets from the (uniform) record base
  u64x2 r[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int p = threadIdx.x + q * kBlock;
    off[q] = static_cast<uint32_t>(p < n_part ? p : n_part - 1) * sizeof(Rec);
  }
  bool timed_out = false;
  const uint32_t tag = rec_tag(epoch);
  // Bounded in passes (~1-2 us each: 2^20 passes, >= 1 s; the tiles may share
  // the GPU with other processes' launches).  A clock check here (a second
  // block-wide barrier per check) kept 52 B of VGPR spills in this form.
  for (uint32_t it = 0;; ++it) {
    load8_rec_sc1_sbase(part, off, r);
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (threadIdx.x + q * kBlock < n_part) ok = ok && tagged_rec_fresh(r[q], tag);
    if (__syncthreads_and(ok)) break;
    if (it >= (1u << 20)) {   // uniform: every thread counts the same passes
      timed_out = true;
      break;
    }
    __builtin_amdgcn_s_sleep(16);
  }
  uint64_t k = ~0ull;
  int64_t i = INT64_MAX;
  if (!timed_out) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint32_t lo = tagged_rec_index(r[q]);
      const int64_t idx = lo == 0xffffffffu ? INT64_MAX : static_cast<int64_t>(lo);
      const uint64_t key = tagged_rec_key(r[q]);
      if (threadIdx.x + q * kBlock < n_part) {
        if (rec_less(key, idx, k, i)) {
          k = key;
          i = idx;
        }
        // consumed: untag both halves.  A replayed HIP graph repeats its
        // launches' epochs, so a record left tagged would pass for the
        // replay's own before that launch's tile block stores it.  Coherent
        // (`sc1`) stores: a plain store could stay dirty in this XCD's L2 and
        // be written back over a later record stored there by a block on
        // another XCD with no kernel boundary in between (measured: a
        // persistent multi-step variant of this collection timed out so).
        uint64_t* h = reinterpret_cast<uint64_t*>(
            const_cast<char*>(reinterpret_cast<const char*>(part)) + off[q]);
        __hip_atomic_store(h, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(h + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  } else if (threadIdx.x == 0) {
    *err = 3u;
  }
  block_argmin(k, i);
  __shared__ uint64_t s_k;
  __shared__ int64_t s_i;
  if (threadIdx.x == 0) {
    s_k = k;
    s_i = i;
  }
  __syncthreads();
  k = s_k;
  i = s_i;
  const bool valid = k != ~0ull;
  const int q = threadIdx.x;
  if (q < MPC_MAX_STEPS) {   // one value per lane
    out->v[q] = (valid && q < n_steps) ? v[q * n_cand + i] : 0.0;
    out->beta[q] = (valid && q < n_steps) ? b[q * n_cand + i] : 0.0;
  }
  if (q == 0) {
    out->cost = valid ? key_cost(k) : __builtin_inf();
    out->index = valid ? index_base + i : -1;
    out->n_steps = n_steps;
    out->reserved_ = 0;
  }
}

// The overlapped exchange's hand-off: after the all_gather of step `tag`'s
// candidates (same stream, so the collective's stores are complete), publish
// the tag.  One coherent 8-B store (relaxed, agent scope: `sc1`).
#ifndef MPC_TEMPLATES_ONLY   // (a unit that is not mpc_rollout.hip: mpc_episodes_obs_launch.h)
__global__ void k_exchange_mark(EpisodeState* __restrict__ S, uint32_t tag) {
  if (threadIdx.x == 0) __hip_atomic_store(&S->gathered_tag, static_cast<uint64_t>(tag),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif

constexpr int kXchgLdsRanks = 32;   // gathered candidates staged in the ring's LDS
static_assert(kXchgLdsRanks * sizeof(mpc_candidate_t) + sizeof(EmitLds) <= sizeof(g_ring),
              "staged candidates + the re-roll's LDS fit in the control ring");

// Block 0 of an overlapped exchange step, all threads: wait (bounded) until
// the all_gather of step `tag` has been marked, then copy the n gathered
// candidates into LDS with coherent 8-B loads (the collective wrote them
// while this launch was already running: no stream edge orders them for
// it).  Returns the LDS copy, or nullptr if the wait timed out (error 4).
__device__ const mpc_candidate_t* wait_gathered(EpisodeState* S, uint32_t tag,
                                                const mpc_candidate_t* __restrict__ g, int n) {
  __shared__ int s_ok;
  if (threadIdx.x < 64) {   // one wave: its clock reads are uniform
    bool ok = false;
    const uint32_t deadline = wall_deadline(kPeerWaitTicks);
    for (;;) {
      const uint64_t w = __hip_atomic_load(&S->gathered_tag, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
      if (static_cast<uint32_t>(w) == tag) {
        ok = true;
        break;
      }
      if (wall_passed(deadline)) break;
      __builtin_amdgcn_s_sleep(2);
    }
    if (threadIdx.x == 0) {
      s_ok = ok;
      if (!ok) S->chain_error = 4u;
    }
  }
  __syncthreads();
  if (!s_ok) return nullptr;
  mpc_candidate_t* dst = reinterpret_cast<mpc_candidate_t*>(
      reinterpret_cast<char*>(ring_lds()) + ((sizeof(EmitLds) + 15) & ~size_t{15}));
  const int words = n * static_cast<int>(sizeof(mpc_candidate_t) / 8);
  for (int q = threadIdx.x; q < words; q += blockDim.x)
    reinterpret_cast<uint64_t*>(dst)[q] =
        __hip_atomic_load(reinterpret_cast<const uint64_t*>(g) + q, __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  return dst;
}

#ifndef MPC_TEMPLATES_ONLY   // (a unit that is not mpc_rollout.hip: mpc_episodes_obs_launch.h)
__global__ __launch_bounds__(64) void k_episode_advance(mpc_episode_config_t c,
                                                        EpisodeState* __restrict__ S,
                                                        const mpc_result_t* __restrict__ res,
                                                        int n, mpc_episode_log_t* __restrict__ log,
                                                        int cap) {
  advance_from_results(c, S, res, n, log, cap);
}
#endif

// Block 0, all threads, after the episode head is stored: publish its Consts
// and t as tagged words (relaxed agent-scope atomic stores: coherent, and each
// word validates itself).
__device__ __forceinline__ void chain_publish(EpisodeState* S, uint32_t epoch) {
  __syncthreads();   // the head (stored by thread 0) is visible to the block
  const int q = threadIdx.x;
  if (q < kPubWords) {
    const uint32_t d = q < kConstsWords
                           ? reinterpret_cast<const uint32_t*>(&S->h.K)[q]
                           : reinterpret_cast<const uint32_t*>(&S->h.t)[q - kConstsWords];
    __hip_atomic_store(&S->chain_pub[q], (static_cast<uint64_t>(d) << 32) | epoch,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------
// Peer-to-peer exchange (mpc_episode_p2p_step): no collective launch.  Every
// rank owns a MAILBOX in its HBM (uncached device memory, mpc_mailbox_alloc:
// each access goes to HBM, so stores a peer GPU makes over xGMI are what this
// GPU's loads see).  Block 0 of rank q's launch with epoch e+1 — the launch
// that completes step e — reduces step e's block records (the previous
// launch's, stream-ordered: plain loads) into q's candidate and stores it into
// slot c&1 (c = the episode's P2P completions so far, EpisodeState::p2p_seq),
// row q, of EVERY rank's mailbox (its own included); it then waits
// until the world's candidates of step e are complete in its own mailbox,
// stages them in LDS, clears them, selects the global winner and updates the
// episode.  The tile blocks meanwhile stream step e+1 (its constants are
// speculated until block 0 publishes them, as in the one-GPU chain): the
// exchange runs beside the rollout, not between launches.
// Self-validating granules: each 8-B word of a candidate travels as one 16-B
// granule whose two 8-B halves both carry the step's 16-bit tag (word[63:16]
// | tag, word[15:0] << 48 | tag — the tagged block records' encoding), so a
// reader accepts a word only when both halves are this step's, never relying
// on store ordering, on a fence or on 16-B single-copy atomicity: the writer
// issues its stores and goes on (no completion wait, no flag store), the
// reader polls the granules themselves.  Only the words a step needs move:
// cost, index, (n_steps, reserved), v[0..n_steps), beta[0..n_steps).
// A consumed granule is zeroed by its reader.  Two slots suffice: rank q
// writes slot c&1 again only for completion c+2, after it has read every
// rank's completion-(c+1) candidate — each posted in a launch that began after
// the launch whose zeroing stores had completed (a kernel boundary).  This
// holds across graph replays whatever the captured length (the count lives on
// the device; the epochs only tag the granules).
//   layout: MailHdr (the peers' mailbox pointers as mapped in this process,
//           this rank, the world size, ping words), then granule
//           [2][world][kCandWords] of 16 B
constexpr int kMailMaxRanks = kXchgLdsRanks;
struct MailHdr {
  uint64_t peers[kMailMaxRanks];
  int32_t rank, world;
  uint64_t ping[kMailMaxRanks];   // mpc_mailbox_ping: rank r's ping word
};
constexpr size_t kMailHdrBytes = (sizeof(MailHdr) + 255) & ~size_t{255};
constexpr int kCandWords = static_cast<int>(sizeof(mpc_candidate_t) / 8);
constexpr size_t kMailRecBytes = kCandWords * sizeof(u64x2);
static_assert(sizeof(mpc_candidate_t) % 8 == 0, "candidates move as 8-B words");
static_assert(offsetof(mpc_candidate_t, v) == 24 && offsetof(mpc_candidate_t, beta) ==
                  24 + 8 * MPC_MAX_STEPS, "candidate word map (cand_word)");
// Peers' launches are not stream-ordered with this one: a rank may start its
// step a host-side hiccup later.  kPeerWaitTicks (2 s) before chain error 5.

__host__ __device__ inline size_t mailbox_bytes(int world) {
  return kMailHdrBytes + 2 * static_cast<size_t>(world) * kMailRecBytes;
}

__device__ __forceinline__ u64x2* mail_rec(void* mb, uint32_t slot, int rank, int world) {
  return reinterpret_cast<u64x2*>(static_cast<char*>(mb) + kMailHdrBytes +
                                  (static_cast<size_t>(slot) * world + rank) * kMailRecBytes);
}

// The j-th posted word of a candidate of n_steps steps: its word index in
// mpc_candidate_t (3 header words, then v[0..n), then beta[0..n)).
__device__ __forceinline__ int cand_word(int j, int n_steps) {
  return j < 3 + n_steps ? j : j + (MPC_MAX_STEPS - n_steps);
}

// Where block 0 stages candidates: the control ring's LDS after the re-roll's
// EmitLds (the ring is idle in block 0).
__device__ __forceinline__ mpc_candidate_t* cand_lds() {
  return reinterpret_cast<mpc_candidate_t*>(reinterpret_cast<char*>(ring_lds()) +
                                            ((sizeof(EmitLds) + 15) & ~size_t{15}));
}

// Block 0, all threads: this rank's best candidate of the previous launch —
// the lexicographic (cost, local index) minimum of its n_part block records
// (plain 16-B records of a stream-ordered earlier launch), its global index
// and its controls — into `out` (LDS).  Each wave loads its own best's
// controls while the waves' minima are combined (finalize_block's prefetch:
// no dependent load after the block's winner is known).
template <bool TILED = false>
__device__ void records_candidate(const Rec* __restrict__ part, int n_part,
                                  const double* __restrict__ v, const double* __restrict__ b,
                                  int64_t n_cand, int n_steps, int64_t index_base,
                                  mpc_candidate_t* out) {
  constexpr int kPer = static_cast<int>((kMaxBlocks + kBlock - 1) / kBlock);
  Rec r[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) {   // every load issued before any compare
    const int p = threadIdx.x + q * kBlock;
    r[q] = p < n_part ? part[p] : Rec{~0ull, INT64_MAX};
  }
  uint64_t k = ~0ull;
  int64_t i = INT64_MAX;
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (rec_less(r[q].key, r[q].idx, k, i)) {
      k = r[q].key;
      i = r[q].idx;
    }
  wave_argmin(k, i);   // every lane: its wave's best
  const int ln = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double pv = 0.0, pb = 0.0;
  if (k != ~0ull && ln < n_steps) {
    const int64_t o = ctl_off<TILED>(ln, i, TILED ? n_steps : n_cand);
    pv = v[o];
    pb = b[o];
  }
  __shared__ uint64_t s_k[kWaves];
  __shared__ int64_t s_i[kWaves];
  if (ln == 0) {
    s_k[wave] = k;
    s_i[wave] = i;
  }
  __syncthreads();
  int wbest = 0;
  k = s_k[0];
  i = s_i[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w)
    if (rec_less(s_k[w], s_i[w], k, i)) {
      k = s_k[w];
      i = s_i[w];
      wbest = w;
    }
  const bool valid = k != ~0ull;
  if (wave == wbest && ln < MPC_MAX_STEPS) {   // one value per lane
    out->v[ln] = (valid && ln < n_steps) ? pv : 0.0;
    out->beta[ln] = (valid && ln < n_steps) ? pb : 0.0;
  }
  if (threadIdx.x == 0) {
    out->cost = valid ? key_cost(k) : __builtin_inf();
    out->index = valid ? index_base + i : -1;
    out->n_steps = n_steps;
    out->reserved_ = 0;
  }
}

// Block 0, all threads: post this rank's candidate (in LDS) of step `epoch`
// to every rank's mailbox as tagged granules (16-B `sc0 sc1` stores; nothing
// waits for them).
__device__ void post_candidate(const uint64_t* s_peers, int rank, int world, uint32_t epoch,
                               uint32_t slot, int n_steps, const mpc_candidate_t* cand) {
  const uint64_t tag = rec_tag(epoch);
  const int words = 3 + 2 * n_steps;
  __syncthreads();   // the candidate is complete in LDS
  const uint64_t* src = reinterpret_cast<const uint64_t*>(cand);
  for (int q = threadIdx.x; q < world * words; q += blockDim.x) {
    const int r = q / words, j = q - r * words;
    const uint64_t w = src[cand_word(j, n_steps)];
    u64x2* dst = mail_rec(reinterpret_cast<void*>(s_peers[r]), slot, rank, world) + j;
    // (s_nop 1: the store reads its data registers before hipcc's next
    // instruction may overwrite them)
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1"
                 :
                 : "v"(dst), "v"(u64x2{(w & ~0xffffull) | tag, (w << 48) | tag})
                 : "memory");
  }
}

// Block 0, all threads: wait (bounded; chain error 5) until every rank's
// candidate of step `epoch` is complete in this rank's mailbox, decode them
// into LDS (cand_lds) and zero the granules.  Returns the LDS copy, or nullptr
// on a timeout.
__device__ const mpc_candidate_t* wait_mailbox(EpisodeState* S, void* mb, uint32_t epoch,
                                               uint32_t slot, int world, int n_steps,
                                               uint64_t ticks) {
  const uint32_t tag = rec_tag(epoch);
  const int words = 3 + 2 * n_steps, total = world * words;
  mpc_candidate_t* dst = cand_lds();
  const uint32_t deadline = wall_deadline(ticks);
  uint32_t it = 0;
  // one granule per thread and pass (world * words <= 256 in one pass: up to
  // 11 ranks at N = 10); a later chunk is polled after the earlier is in
#pragma unroll 1
  for (int base = 0; base < total; base += kBlock) {
    const int q = base + static_cast<int>(threadIdx.x);
    const int r = q / words, j = q - r * words;
    uint64_t* h = q < total ? reinterpret_cast<uint64_t*>(mail_rec(mb, slot, r, world) + j)
                            : nullptr;
    u64x2 g = {0, 0};
    for (;; ++it) {
      bool ok = true;
      if (h) {
        g.x = __hip_atomic_load(h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        g.y = __hip_atomic_load(h + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        ok = tagged_rec_fresh(g, tag);
      }
      if (__syncthreads_and(ok)) break;
      // uniform: every thread counts the same passes, thread 0's clock decides
      if ((it & 63) == 63 && block_wall_passed(deadline)) {
        if (threadIdx.x == 0) S->chain_error = 5u;
        return nullptr;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (h) {
      reinterpret_cast<uint64_t*>(&dst[r])[cand_word(j, n_steps)] = tagged_rec_key(g);
      __hip_atomic_store(h, uint64_t{0}, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(h + 1, uint64_t{0}, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  __syncthreads();
  return dst;
}

// Block 0 of a P2P launch (and the flush): complete step `tag` = prev: this
// rank's candidate from the previous launch's records, posted; the world
// candidates awaited; the global winner re-rolled into out_prev and the
// episode updated, publishing `publish_epoch` (0: end of the chain).
template <int INTEG, int ROT, bool TILED = false>
__device__ void p2p_complete(const mpc_episode_config_t& c, EpisodeState* S, void* mb, int world,
                             uint32_t prev, const Rec* __restrict__ part_prev, int n_part_prev,
                             const double* __restrict__ v_prev, const double* __restrict__ b_prev,
                             int64_t n_cand, int n_steps, int64_t index_base,
                             mpc_result_t* __restrict__ out_prev,
                             mpc_episode_log_t* __restrict__ log, int cap, uint32_t publish_epoch) {
  // the header (peers, rank: uncached, so a full memory round trip) loaded
  // before the records, its values parked in LDS after them
  __shared__ uint64_t s_peers[kMailMaxRanks];
  __shared__ int s_rank;
  const MailHdr* hdr = static_cast<const MailHdr*>(mb);
  __shared__ uint32_t s_err, s_seq;
  const uint64_t my_peer = static_cast<int>(threadIdx.x) < world ? hdr->peers[threadIdx.x] : 0;
  const int my_rank = threadIdx.x == 0 ? hdr->rank : 0;
  // an earlier step of this episode already timed out waiting for its peers
  // (error 5: a peer gone): fail fast instead of waiting the full budget
  // again on every later step.  Other errors say nothing about the peers.
  const uint32_t prior_err = threadIdx.x == 0 ? S->chain_error : 0u;
  const uint32_t seq = threadIdx.x == 0 ? S->p2p_seq : 0u;
  mpc_candidate_t* lc = cand_lds();
  records_candidate<TILED>(part_prev, n_part_prev, v_prev, b_prev, n_cand, n_steps, index_base,
                           lc);
  TL_B0(1);
  if (static_cast<int>(threadIdx.x) < world) s_peers[threadIdx.x] = my_peer;
  if (threadIdx.x == 0) {
    s_rank = my_rank;
    s_err = prior_err;
    s_seq = seq;
  }
  __syncthreads();
  const uint32_t slot = s_seq & 1u;
  post_candidate(s_peers, s_rank, world, prev, slot, n_steps, lc);
  TL_B0(2);
  const mpc_candidate_t* g =
      wait_mailbox(S, mb, prev, slot, world, n_steps, s_err == 5u ? 0ull : kPeerWaitTicks);
  TL_B0(3);
  if (threadIdx.x == 0) S->p2p_seq = s_seq + 1u;   // read by the next launch
  if (g) {
    advance_from_candidates<INTEG, ROT>(c, S, g, world, out_prev, log, cap, publish_epoch,
                                        ring_lds());
  } else if (publish_epoch) {   // timed out (error 5): publish the unchanged head
    chain_publish(S, publish_epoch);
  } else if (threadIdx.x < kPubWords) {   // ... or still end the chain
    __hip_atomic_store(&S->chain_pub[threadIdx.x], uint64_t{0}, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The mailboxes' self-test (mpc_mailbox_ping): lane r stores `tag` into
// rank r's ping word for this rank, then every lane waits (~0.1 s at most)
// for its rank's word in this mailbox; ok[0] = 1 if all `world` arrived.
#ifndef MPC_TEMPLATES_ONLY   // (a unit that is not mpc_rollout.hip: mpc_episodes_obs_launch.h)
__global__ __launch_bounds__(64) void k_mailbox_ping(void* mb, uint32_t tag, int32_t* ok) {
  MailHdr* hdr = static_cast<MailHdr*>(mb);
  const int world = hdr->world, rank = hdr->rank;
  const int r = threadIdx.x;
  if (r < world)
    __hip_atomic_store(&static_cast<MailHdr*>(reinterpret_cast<void*>(hdr->peers[r]))->ping[rank],
                       static_cast<uint64_t>(tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  bool seen = r >= world;
  const uint32_t deadline = wall_deadline(kPeerWaitTicks);   // one wave: uniform clock
  while (__ballot(!seen) != 0 && !wall_passed(deadline)) {
    if (!seen)
      seen = __hip_atomic_load(&hdr->ping[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) ==
             static_cast<uint64_t>(tag);
    __builtin_amdgcn_s_sleep(8);
  }
  const bool all = __ballot(!seen) == 0;
  if (r == 0) ok[0] = all ? 1 : 0;
}
#endif

template <int INTEG, int ROT, bool TILED>
__global__ __launch_bounds__(kBlock) void k_episode_p2p_flush(
    mpc_episode_config_t c, EpisodeState* __restrict__ S, void* mailbox, uint32_t tag, int world,
    const Rec* __restrict__ part, int n_part, const double* __restrict__ v,
    const double* __restrict__ b, int64_t n_cand, int n_steps, int64_t index_base,
    mpc_result_t* __restrict__ out, mpc_episode_log_t* __restrict__ log, int cap) {
  p2p_complete<INTEG, ROT, TILED>(c, S, mailbox, world, tag, part, n_part, v, b, n_cand, n_steps,
                           index_base, out, log, cap, 0u);
}

}  // namespace mpc
