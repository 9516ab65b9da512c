// mpc_lanes.h — one lane's rollout of its candidates, and the LDS-DMA control
// ring that feeds it (gfx950).
//
//   kCplWide, kPrefetch, kMaxBlocks, kFinBlock   tuning constants
//   ctl_off                  where a candidate's control sits (SoA or tiled)
//   uniform_d, uniform_consts   block-uniform constants moved to SGPRs
//   rollout_lane_l           CPL adjacent candidates, N steps in registers with
//                            the controls of the next kPrefetch-1 steps in
//                            flight; terminal cost
//   g_ring, lds_addr, glds_pair, glds_refill, wait_vm, NoPre
//                            the ring: kRing step slots per wave, filled by
//                            global_load_lds_dwordx4
//   rollout_lane_glds_k, rollout_lane_glds   the wide path (CPL = 2: every
//                            control load is 16 B per lane = 1 KiB per wave
//                            instruction) over the ring
//   rollout_lane             picks the path and the wheelbase form
//
// Template modes: INTEG (MPC_INTEG_QK21 | MPC_INTEG_RECT), ROT (heading
// rotation recurrence instead of a per-step sincos), STATES (write every
// candidate's per-step states: the CoordinateTree payload).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/mpc_rollout.h"
#include "mpc_argmin.h"
#include "mpc_device.h"

namespace mpc {

// Tuning constants (DESIGN.md §5 records the A/B measurements behind them).
constexpr int kCplWide = 2;    // candidates per lane on the aligned path (16-B control loads)
constexpr int kPrefetch = 2;   // register-ring depth in steps of the scalar / states path
constexpr int64_t kMaxBlocks = 2048;   // rollout grid cap: 256 CUs x 8 resident blocks
constexpr int kFinBlock = 256;         // one-block selection kernels (A/B: 1024 -> 256 = -0.7 us)

// Offset of candidate c's control at step s: step-major SoA (pitch = the row
// pitch ld) or TILED (MPC_LAYOUT_TILED, pitch = n_steps: tile c / 512 holds
// per step 512 v then 512 beta; the beta pointer is the v pointer + 512).
template <bool TILED>
__host__ __device__ __forceinline__ int64_t ctl_off(int64_t s, int64_t c, int64_t pitch) {
  if constexpr (TILED)
    return (c >> 9) * (pitch << 10) + (s << 10) + (c & 511);
  else
    return s * pitch + c;
}
static_assert(MPC_TILE == 512, "ctl_off's shifts");

// Block-uniform constants computed on the VALU (consts_from_problem) moved to
// SGPRs: hipcc keeps VALU results in VGPRs even when every lane holds the same
// value, which costs the batched kernel its fifth wave (120 VGPRs -> spills).
__device__ __forceinline__ double uniform_d(double a) {
  const uint64_t u = static_cast<uint64_t>(__double_as_longlong(a));
  const uint64_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(u)));
  const uint64_t hi =
      static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(u >> 32)));
  return __longlong_as_double(static_cast<long long>((hi << 32) | lo));
}

__device__ __forceinline__ Consts uniform_consts(const Consts& k) {
  Consts K;
  K.x = uniform_d(k.x);
  K.y = uniform_d(k.y);
  K.phi = uniform_d(k.phi);
  K.x_t = uniform_d(k.x_t);
  K.y_t = uniform_d(k.y_t);
  K.x_0 = uniform_d(k.x_0);
  K.y_0 = uniform_d(k.y_0);
  K.A = uniform_d(k.A);
  K.B = uniform_d(k.B);
  K.C1 = uniform_d(k.C1);
  K.C2 = uniform_d(k.C2);
  K.inv_den = uniform_d(k.inv_den);
  K.L = uniform_d(k.L);
  K.inv_L = uniform_d(k.inv_L);
  K.h = uniform_d(k.h);
  K.hlgth = uniform_d(k.hlgth);
  K.s0 = uniform_d(k.s0);
  K.c0 = uniform_d(k.c0);
  K.L_pow2 = __builtin_amdgcn_readfirstlane(k.L_pow2);
  K.pad_ = 0;
  return K;
}

// Rollout of CPL adjacent candidates starting at column c0; costs in cst.
// obs: the obstacle hook (NoObs: none); blocked_out[CPL] (Obs::kOn only):
// the candidates that entered a keep-out circle.
template <int CPL, int INTEG, int ROT, bool STATES, bool PL2, class Obs = NoObs>
__device__ __forceinline__ void rollout_lane_l(const Consts& K, const double* __restrict__ v,
                                             const double* __restrict__ b, int64_t ld, int64_t c0,
                                             int n_steps, double (&cst)[CPL],
                                             double* __restrict__ states, int64_t n_cand,
                                             const Obs& obs = Obs{},
                                             bool* blocked_out = nullptr) {
  double x[CPL], y[CPL], ph[CPL], sn[CPL], cs[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) step_start<ROT>(K, x[j], y[j], ph[j], sn[j], cs[j]);
  // Controls of step sr for this lane's CPL candidates: 16 B per lane per
  // array on the wide path (one 1 KiB wave-instruction each).
  auto load = [&](int sr, double (&vv)[CPL], double (&bb)[CPL]) {
    if constexpr (CPL >= 2) {
#pragma unroll
      for (int h = 0; h < CPL; h += 2) {
        const double2 v2 = *reinterpret_cast<const double2*>(v + sr * ld + c0 + h);
        const double2 b2 = *reinterpret_cast<const double2*>(b + sr * ld + c0 + h);
        vv[h] = v2.x;
        vv[h + 1] = v2.y;
        bb[h] = b2.x;
        bb[h + 1] = b2.y;
      }
    } else {
      vv[0] = v[sr * ld + c0];
      bb[0] = b[sr * ld + c0];
    }
  };
  bool bad[CPL];
  [[maybe_unused]] bool blocked[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    bad[j] = false;
    if constexpr (Obs::kOn) blocked[j] = false;
  }
  auto body = [&](int sr, const double (&vv)[CPL], const double (&bb)[CPL]) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      step_core<INTEG, ROT, PL2>(x[j], y[j], ph[j], sn[j], cs[j], vv[j], bb[j], K, bad[j]);
      if constexpr (STATES) {
        double px = x[j], py = y[j];
        if constexpr (ROT == kRotCum) cum_pose<PL2>(K, x[j], y[j], px, py);
        states[(sr * 3 + 0) * n_cand + c0 + j] = px;
        states[(sr * 3 + 1) * n_cand + c0 + j] = py;
        states[(sr * 3 + 2) * n_cand + c0 + j] = ph[j];
      }
    }
    if constexpr (Obs::kOn) obs.loop(x, y, blocked);
  };
  // Software pipeline: the controls of the next kPrefetch-1 steps are in
  // flight while this step's trig chain runs (rotating register buffers,
  // kPrefetch steps per trip, static indices, no copies).  One step of VALU
  // work is far shorter than the loaded HBM latency, so one step of lookahead
  // leaves the loop waiting on memory.
  constexpr int D = kPrefetch;
  double vq[D][CPL], bq[D][CPL];
#pragma unroll
  for (int u = 0; u < D - 1; ++u)
    if (u < n_steps) load(u, vq[u], bq[u]);
#pragma unroll 1
  for (int s = 0; s < n_steps; s += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int st = s + u;
      if (st < n_steps) {
        if (st + D - 1 < n_steps) load(st + D - 1, vq[(u + D - 1) % D], bq[(u + D - 1) % D]);
        body(st, vq[u], bq[u]);
      }
    }
  }
  // Irregular candidates (argument outside the trig cores' range, or NaN):
  // recompute with the safe recurrence.  Never taken for the reference's
  // arguments; kept out of the loop so the loop carries no fallback code.
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    if constexpr (ROT == kRotCum) {
      if (!bad[j]) cum_pose<PL2>(K, x[j], y[j], x[j], y[j]);
    }
    if (bad[j]) {
      x[j] = K.x;
      y[j] = K.y;
      ph[j] = K.phi;
      if constexpr (Obs::kOn) blocked[j] = false;   // the recompute's states replace the loop's
      for (int sr = 0; sr < n_steps; ++sr) {
        step_safe<INTEG>(x[j], y[j], ph[j], v[sr * ld + c0 + j], b[sr * ld + c0 + j], K);
        if constexpr (Obs::kOn) obs.world(x[j], y[j], blocked[j]);
        if constexpr (STATES) {
          states[(sr * 3 + 0) * n_cand + c0 + j] = x[j];
          states[(sr * 3 + 1) * n_cand + c0 + j] = y[j];
          states[(sr * 3 + 2) * n_cand + c0 + j] = ph[j];
        }
      }
    }
    cst[j] = cost(x[j], y[j], K);
    if constexpr (Obs::kOn) blocked_out[j] = blocked[j];
  }
}

// ---------------------------------------------------------------------------
// Wide path with an LDS-DMA control ring.  Each wave streams its own 128
// candidates: per step one global_load_lds_dwordx4 for v and one for beta
// (1 KiB each, lane-linear: lane l's 16 B land at slot + 16*l) into a ring of
// kRing step slots per wave, kRing-1 steps ahead of the step being computed.
// The loads need no VGPRs while in flight (the register ring of rollout_lane_l
// holds 8 per step of lookahead), so the lookahead is deeper at a lower VGPR
// count.  The DMA is issued by inline asm, which hipcc neither counts nor
// orders against the LDS reads: the waits are explicit (vmcnt for "slot
// landed", lgkmcnt(0) before a slot is refilled) and every asm statement
// clobbers memory.
// The control DMA is streamed once: non-temporal (A/B: -1.5 us/step on config C).
#define MPC_GLDS_POLICY " nt"
constexpr int kRing = 3;   // LDS ring depth in steps (kRing-1 steps in flight)

// One ring for every instantiation (namespace scope: allocated once per kernel).
__shared__ double2 g_ring[kWaves][kRing][2][64];  // [wave][slot][v|beta][lane]

__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return static_cast<uint32_t>(
      reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) char*)p));
}

// Inline asm whose VMEM instruction takes an SGPR operand (the `saddr` base)
// must itself provide the wait states the hardware needs between a VALU that
// writes that SGPR and the VMEM that reads it (5 on CDNA): hipcc's hazard
// recognizer does not look inside asm statements, and it reloads spilled SGPRs
// with v_readlane — measured: a v_readlane of the base right before the load,
// 0 wait states, faulted.  Hence the `s_nop 4` ahead of the first such VMEM in
// every statement below (the M0 write's own 1-wait-state need is covered too).
// Both control rows of one step into LDS (v at dst_v, beta at dst_b).  The
// addresses are SGPR base + 32-bit VGPR offset (the `saddr` form): the row
// bases gv / gb (step s's rows: wave-uniform) advance per step on the SALU,
// the lane's byte offset `voff` is fixed for the tile — no 64-bit per-lane
// address arithmetic on the VALU in the loop.  The statement writes only M0
// (saved and restored) and `keep`: no SCC-setting instruction (s_add etc.),
// since hipcc may hold a live SCC across it.
// Refilling a slot must not overtake the LDS reads of its previous contents:
// `read_v`/`read_b` are the registers those reads produced, taken as inputs
// so hipcc completes the reads (lgkmcnt) before the DMA is issued — without a
// blanket lgkmcnt(0), which would also wait for unrelated scalar loads.
__device__ __forceinline__ void glds_pair(const double* gv, const double* gb, uint32_t voff,
                                          uint32_t dst_v, uint32_t dst_b) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %4\n\t"
      "s_nop 4\n\t"
      "global_load_lds_dwordx4 %1, %2" MPC_GLDS_POLICY "\n\t"
      "s_mov_b32 m0, %5\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %3" MPC_GLDS_POLICY "\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(gv), "s"(gb), "s"(dst_v), "s"(dst_b)
      : "memory");
}

__device__ __forceinline__ void glds_refill(const double* gv, const double* gb, uint32_t voff,
                                            uint32_t dst_v, uint32_t dst_b,
                                            const double2& read_v, const double2& read_b) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %4\n\t"
      "s_nop 4\n\t"
      "global_load_lds_dwordx4 %1, %2" MPC_GLDS_POLICY "\n\t"
      "s_mov_b32 m0, %5\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %3" MPC_GLDS_POLICY "\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(gv), "s"(gb), "s"(dst_v), "s"(dst_b), "v"(read_v.x), "v"(read_v.y),
        "v"(read_b.x), "v"(read_b.y)
      : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  if constexpr (N == 0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 2)
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 4)
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 6)
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 8)
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 10)
    asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  else if constexpr (N == 12)
    asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else
    asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
}

struct NoPre {
  __device__ void operator()() const {}
};

// pre(): called before K is first read (the chained episode step waits there
// for this step's constants): ROT 0 / 1 once the first ring slots are in
// flight; kRotCum only after the loop, which reads Kloop (the step size h and
// the wheelbase terms; = K except in the chained step, which speculates them
// in pre0(), called once the first ring slots are in flight).
// mid(): kRotCum, called right after the wait of step n_steps - 3: loads it
// issues complete with that step's last control DMA (the tail waits for both).
// PIN: the leading trig coefficients pinned in VGPRs (8 VGPRs for ~8 VALU per
// lane-step); off where the register budget is tighter than the VALU budget.
// obs / blocked_out[2]: as in rollout_lane_l.
template <int INTEG, int ROT, bool PL2, class Pre = NoPre, class Pre0 = NoPre,
          class Mid = NoPre, bool PIN = true, class Obs = NoObs>
__device__ __forceinline__ void rollout_lane_glds_k(const Consts& K, const Consts& Kloop,
                                                    const double* __restrict__ v,
                                                    const double* __restrict__ b, int64_t ld,
                                                    int64_t c0, int n_steps, double (&cst)[2],
                                                    const Pre& pre = Pre{},
                                                    const Pre0& pre0 = Pre0{},
                                                    const Mid& mid = Mid{},
                                                    const Obs& obs = Obs{},
                                                    bool* blocked_out = nullptr) {
  constexpr int CPL = 2;
  constexpr int R = kRing;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t ring0 = __builtin_amdgcn_readfirstlane(lds_addr(&g_ring[wv][0][0][0]));
  constexpr uint32_t kSlot = 2 * 64 * sizeof(double2);  // 2 KiB
  auto dst = [&](int slot) { return ring0 + slot * kSlot; };
  // the lane's byte offset in every control row (< 2^31: the host checks
  // 8 * ld < 2^31 for the aligned path)
  const uint32_t voff = static_cast<uint32_t>(c0) * 8u;
  // leading trig coefficients pinned in VGPRs (opaque to the compiler, so not
  // re-materialised per step)
  trig::Leads lead = trig::const_leads();
  if constexpr (PIN)
    asm volatile("" : "+v"(lead.tp), "+v"(lead.rs), "+v"(lead.rc));
  // The loop constants: Kloop (read after pre0), or K when a speculated step
  // size turns out wrong (kRotCum with a real pre(): the chained step after an
  // episode restart) and the loop runs again from the controls with the final
  // constants — the same code, bitwise the lane's arithmetic, and no second
  // copy of the recurrence to hold registers for.
  Consts KL;
  double x[CPL], y[CPL], ph[CPL], sn[CPL], cs[CPL];
  bool bad[CPL];
  [[maybe_unused]] bool blocked[CPL];
  for (int pass = 0;; ++pass) {
#pragma unroll
    for (int u = 0; u < R - 1; ++u)
      if (u < n_steps) glds_pair(v + u * ld, b + u * ld, voff, dst(u), dst(u) + kSlot / 2);
    if (pass == 0) {
      if constexpr (ROT != kRotCum)
        pre();
      else
        pre0();   // kRotCum: the loop constants Kloop (the chained step reads them here)
      KL = Kloop;
    }
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      step_start<ROT>(KL, x[j], y[j], ph[j], sn[j], cs[j]);
      bad[j] = false;
      if constexpr (Obs::kOn) blocked[j] = false;
    }
    double2 v2 = make_double2(0.0, 0.0), b2 = v2;   // the last slot's contents as read
#pragma unroll 1
    for (int s = 0; s < n_steps; s += R) {
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int st = s + u;
        if (st < n_steps) {
          if (st + R - 1 < n_steps) {
            const int sr = st + R - 1, slot = (u + R - 1) % R;   // = the slot read last step
            glds_refill(v + sr * ld, b + sr * ld, voff, dst(slot), dst(slot) + kSlot / 2, v2,
                        b2);
            wait_vm<2 * (R - 1)>();   // this step's pair has landed
          } else {
            wait_vm<0>();             // pipeline tail
          }
          if constexpr (!std::is_same_v<Mid, NoPre>) {
            if (st == n_steps - 3) mid();
          }
          v2 = g_ring[wv][u][0][lane];
          b2 = g_ring[wv][u][1][lane];
          // the heading itself is not needed here (rotation mode carries sin/cos;
          // an irregular candidate is recomputed from K.phi), so no phi chain
          double ph0 = ROT ? 0.0 : ph[0], ph1 = ROT ? 0.0 : ph[1];
          step_core<INTEG, ROT, PL2>(x[0], y[0], ph0, sn[0], cs[0], v2.x, b2.x, KL, bad[0],
                                     &lead);
          step_core<INTEG, ROT, PL2>(x[1], y[1], ph1, sn[1], cs[1], v2.y, b2.y, KL, bad[1],
                                     &lead);
          if constexpr (Obs::kOn) obs.loop(x, y, blocked);
          if (!ROT) {
            ph[0] = ph0;
            ph[1] = ph1;
          }
        }
      }
    }
    if constexpr (ROT == kRotCum) {
      // the start pose is first needed here (chained step: this step's
      // constants are waited for now; if the step size speculated for the loop
      // turns out different — an episode restart reset t — the loop runs again)
      if (pass == 0) pre();
      if constexpr (!std::is_same_v<Pre, NoPre>) {
        // (the chained step's K lives in LDS: its h and, on the rare rerun,
        // the loop's terms are moved to SGPRs; nothing else of K is)
        if (KL.h != uniform_d(K.h)) {   // rare (episode restart); uniform over the block
          KL = uniform_consts(K);
          continue;
        }
      }
#pragma unroll
      for (int j = 0; j < CPL; ++j)
        if (!bad[j]) cum_pose<PL2>(K, x[j], y[j], x[j], y[j]);
    }
    break;
  }
  // The criterion first (an irregular candidate's value is replaced below),
  // then the rare recompute: nothing of the criterion (the target and line
  // terms of K, which the chained step reads from LDS into VGPRs) is live
  // across the recompute's register-hungry trig.
#pragma unroll
  for (int j = 0; j < CPL; ++j) cst[j] = cost(x[j], y[j], K);
  if (bad[0] || bad[1]) {
    // (wave-uniform SGPR copies: the recompute's trig needs the VGPRs)
    const Consts Ks = uniform_consts(K);
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      if (bad[j]) {
        x[j] = Ks.x;
        y[j] = Ks.y;
        ph[j] = Ks.phi;
        if constexpr (Obs::kOn) blocked[j] = false;   // the recompute's states replace the loop's
        for (int sr = 0; sr < n_steps; ++sr) {
          step_safe<INTEG>(x[j], y[j], ph[j], v[sr * ld + c0 + j], b[sr * ld + c0 + j], Ks);
          if constexpr (Obs::kOn) obs.world(x[j], y[j], blocked[j]);
        }
        cst[j] = cost(x[j], y[j], Ks);
      }
    }
  }
  if constexpr (Obs::kOn) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) blocked_out[j] = blocked[j];
  }
}

// kRotCum keeps the start pose's terms live across the loop: with pinned
// leads it needs > 96 VGPRs and spills at 5 waves/SIMD (any scratch costs far
// more than the fifth wave gains), unpinned it fits.
template <int INTEG, int ROT, bool PL2, class Obs = NoObs>
__device__ __forceinline__ void rollout_lane_glds(const Consts& K, const double* __restrict__ v,
                                                  const double* __restrict__ b, int64_t ld,
                                                  int64_t c0, int n_steps, double (&cst)[2],
                                                  const Obs& obs = Obs{},
                                                  bool* blocked_out = nullptr) {
  rollout_lane_glds_k<INTEG, ROT, PL2, NoPre, NoPre, NoPre, ROT != kRotCum, Obs>(
      K, K, v, b, ld, c0, n_steps, cst, NoPre{}, NoPre{}, NoPre{}, obs, blocked_out);
}

// L a power of two or not: one loop body each (see step_core).
template <int CPL, int INTEG, int ROT, bool STATES, class Obs = NoObs>
__device__ __forceinline__ void rollout_lane(const Consts& K, const double* __restrict__ v,
                                             const double* __restrict__ b, int64_t ld, int64_t c0,
                                             int n_steps, double (&cst)[CPL],
                                             double* __restrict__ states, int64_t n_cand,
                                             const Obs& obs = Obs{},
                                             bool* blocked_out = nullptr) {
  if constexpr (CPL == 2 && !STATES) {
    if (K.L_pow2)
      rollout_lane_glds<INTEG, ROT, true, Obs>(K, v, b, ld, c0, n_steps, cst, obs, blocked_out);
    else
      rollout_lane_glds<INTEG, ROT, false, Obs>(K, v, b, ld, c0, n_steps, cst, obs, blocked_out);
    return;
  }
  if (K.L_pow2)
    rollout_lane_l<CPL, INTEG, ROT, STATES, true, Obs>(K, v, b, ld, c0, n_steps, cst, states,
                                                       n_cand, obs, blocked_out);
  else
    rollout_lane_l<CPL, INTEG, ROT, STATES, false, Obs>(K, v, b, ld, c0, n_steps, cst, states,
                                                        n_cand, obs, blocked_out);
}

}  // namespace mpc
