// mpc_winner.h — the winner's re-roll: its states and result record, lane-
// parallel, bitwise the arithmetic the lane scored (gfx950).
//
//   Winner, tr_at            what the episode update needs of a winner
//   EmitLds, ring_lds        the re-roll's LDS (its own, or the idle control ring)
//   NoSide                   no side work beside the re-roll
//   emit_winner, emit_winner_tail   the re-roll, and the rest of a deferred one
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_argmin.h"
#include "mpc_device.h"
#include "mpc_lanes.h"
#include "mpc_timeline.h"

namespace mpc {

// What the episode update needs of a winner (kept in registers by the
// finalize kernel instead of being re-read from the result record).
struct Winner {
  double cost;
  int64_t index;
  int32_t found, n_steps;
  double v, beta;
  double tr[3][3];     // states of steps 0..2 (clamped to the horizon)
};

// r.tr[k][q] for a runtime k in {0, 1, 2} by selects: a dynamically indexed
// local array would live in scratch memory (a ~µs round trip per access).
__device__ __forceinline__ double tr_at(const Winner& r, int k, int q) {
  const double a = r.tr[0][q], b = r.tr[1][q], c = r.tr[2][q];
  return k == 0 ? a : (k == 1 ? b : c);
}

// Re-roll the winner and fill the result record.  Called by ALL threads of
// the block once thread 0 holds the winner (key, col).  The N-step recurrence
// is split so that only cheap accumulations stay serial: lane s computes the
// state-free heading increment dphi_s = Q((v_s/L) tan(beta_s)); lane 0
// accumulates the headings; lane s evaluates sincos(phi_s) (direct mode) or
// the rotation factors of dphi_s (ROT); lane 0 rotates (ROT) and accumulates
// x and y.  The winner is regular or irregular exactly as in rollout_lane
// (same tests), and each branch repeats that path's operations in the same
// order, so the emitted states are bitwise those the arg-min scored.
// LDS of the winner's re-roll (emit_winner) and of the selection's staged
// controls (finalize_block), provided by the caller: a kernel that owns LDS
// it is not using at that point — the chained step's block 0 and the fused
// finalize have the control ring — lends that instead of adding 2.5 KiB to
// the kernel's LDS (which decides how many blocks fit on a CU).
struct EmitLds {
  double v[MPC_MAX_STEPS], dphi[MPC_MAX_STEPS], phi[MPC_MAX_STEPS];
  double a[MPC_MAX_STEPS], c[MPC_MAX_STEPS];
  double tr[MPC_MAX_STEPS * 3];
  double pv[MPC_MAX_STEPS], pb[MPC_MAX_STEPS];
  double tail[5];      // deferred re-roll: lane 0's state (x, y, sin, cos, phi) ...
  int tail_from;       // ... after this many steps (== n_steps: nothing deferred)
};

// The control ring's LDS lent to the re-roll (a block whose ring is idle).
__device__ __forceinline__ EmitLds* ring_lds() {
  static_assert(sizeof(EmitLds) <= sizeof(g_ring), "the re-roll's LDS fits in the ring");
  return reinterpret_cast<EmitLds*>(&g_ring[0][0][0][0]);
}

// Side work for the threads that have no part in a phase of the re-roll (every
// thread >= 64: n_steps <= 32): side_a() runs beside the per-step factors,
// side_b(fast) beside lane 0's serial pass; both are called by every thread
// and pick their own threads.
struct NoSide {
  __device__ void operator()() const {}
  __device__ void operator()(bool) const {}
  __device__ void operator()(int, double, double, double) const {}
};

// on_layer(st, x, y, phi): lane 0, in the serial pass, as each of the first
// three layer states is formed.
template <int INTEG, int ROT, class SideA = NoSide, class SideB = NoSide, class OnLayer = NoSide>
__device__ void emit_winner(const Consts& K, const double* __restrict__ v,
                            const double* __restrict__ b, int64_t ld, int n_steps, uint64_t key,
                            int64_t col, int64_t reported_index, double incumbent,
                            mpc_result_t* __restrict__ out, EmitLds* lds, Winner* win = nullptr,
                            const double* pre_v = nullptr, const double* pre_b = nullptr,
                            bool defer_tail = false, const SideA& side_a = SideA{},
                            const SideB& side_b = SideB{}, const OnLayer& on_layer = OnLayer{}) {
  double* s_v = lds->v;
  double* s_dphi = lds->dphi;
  double* s_phi = lds->phi;
  double* s_a = lds->a;
  double* s_c = lds->c;
  __shared__ double s_b0;
  __shared__ uint64_t s_key;
  __shared__ int64_t s_col, s_rep;
  __shared__ int s_bad;
  if (threadIdx.x == 0) {
    s_key = key;
    s_col = col;
    s_rep = reported_index;
    s_bad = 0;
  }
  __syncthreads();
  TL_B0(16);
  key = s_key;
  col = s_col;
  const int lane = threadIdx.x;
  const bool valid = key != ~0ull;
  // Regular pass (step_core's forms and range checks), then — if any step is
  // irregular — the safe pass (step_safe's forms) for the whole candidate,
  // exactly as rollout_candidate / the rollout kernels decide.
  double vs = 0.0, w = 0.0, bs = 0.0, d = 0.0, ra = 0.0, rc = 0.0;
  if (valid && lane < n_steps) {
    // pre_v / pre_b: the winner's controls already staged in LDS by the caller
    // (finalize_block prefetches each wave's best during the block reduction)
    vs = pre_v ? pre_v[lane] : v[lane * ld + col];
    bs = pre_b ? pre_b[lane] : b[lane * ld + col];
    s_v[lane] = vs;
    if (lane == 0) s_b0 = bs;
    w = K.L_pow2 ? vs * K.inv_L : vs / K.L;
    d = heading_incr<INTEG>(w, trig::tan_small(bs), K);
    s_dphi[lane] = d;
    const bool lane_bad =
        !(fabs(bs) <= trig::kTanMax) || (ROT && !(fabs(d) <= trig::kRotMax));
    if (lane_bad) s_bad = 1;
    // rotation mode: the factors depend on this step's increment only, so
    // they are formed here, in the same phase (no heading chain needed)
    if (ROT && !lane_bad) {
      trig::rotation_sc(d, ra, rc);
      s_a[lane] = ra;
      s_c[lane] = rc;
    }
  }
  TL_B0(17);
  side_a();
  __syncthreads();
  TL_B0(4);
  // Regular rotation-mode winner: ONE serial pass on lane 0 (heading, rotation,
  // position); every other case keeps the heading chain / sincos phases.
  const bool fast = ROT && s_bad == 0;
  if (!fast) {
    if (valid && lane == 0) {
      double ph = K.phi;
      for (int st = 0; st < n_steps; ++st) {
        ph = ph + s_dphi[st];
        s_phi[st] = ph;
        if (!ROT && !(fabs(ph) <= trig::kFastMax)) s_bad = 1;
      }
    }
    __syncthreads();
    if (s_bad) {
      if (valid && lane < n_steps)
        s_dphi[lane] = heading_incr<INTEG>(w, trig::tan_fast(bs), K);
      __syncthreads();
      if (valid && lane == 0) {
        double ph = K.phi;
        for (int st = 0; st < n_steps; ++st) {
          ph = ph + s_dphi[st];
          s_phi[st] = ph;
        }
      }
      __syncthreads();
    }
    if (valid && lane < n_steps)
      trig::sincos_fast(s_phi[lane], &s_a[lane], &s_c[lane]);  // == sincos_core if regular
    __syncthreads();
  }
  // Lane 0 runs the serial pass into LDS; the record's trajectory is then
  // stored by one lane per value (a single lane's ~30 stores would serialise
  // in the address path for ~1 us).
  // defer_tail (a regular rotation-mode winner): the pass stops after the
  // three layer states the episode update needs; emit_winner_tail() finishes
  // the record's trajectory once the update is out (same operations, same
  // order, continued from the saved state).
  double* s_tr = lds->tr;
  const int n_run = (defer_tail && fast && n_steps > 3) ? 3 : n_steps;
  if (lane == 0) {
    lds->tail_from = n_steps;
    out->n_steps = n_steps;
    if (win) win->n_steps = n_steps;
    if (!valid) {
      out->cost = __builtin_inf();
      out->index = -1;
      out->found = 0;
      out->v = 0.0;
      out->beta = 0.0;
      if (win) {
        win->cost = __builtin_inf();
        win->index = -1;
        win->found = 0;
      }
    } else {
      const double c = key_cost(key);
      const int found = c < incumbent ? 1 : 0;
      out->cost = c;
      out->index = s_rep;
      out->found = found;
      out->v = s_v[0];
      out->beta = s_b0;
      if (win) {
        win->cost = c;
        win->index = s_rep;
        win->found = found;
        win->v = s_v[0];
        win->beta = s_b0;
      }
      double x, y, sn, cs, ph;
      if (fast)
        step_start<ROT>(K, x, y, ph, sn, cs);    // kRotCum: identity rotation, empty sums
      else
        step_start<0>(K, x, y, ph, sn, cs);
      // the fast pass takes step st's values from lane st's registers
      // (v_readlane: no LDS round trip per step on the serial path)
      auto rl = [](double val, int src) {
        const uint64_t u = static_cast<uint64_t>(__double_as_longlong(val));
        const uint32_t lo = __builtin_amdgcn_readlane(static_cast<int>(u), src);
        const uint32_t hi = __builtin_amdgcn_readlane(static_cast<int>(u >> 32), src);
        return __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(hi) << 32) | lo));
      };
      for (int st = 0; st < n_run; ++st) {
        double vst;
        if (fast) {
          ph = ph + rl(d, st);
          trig::rotate_sc(rl(ra, st), rl(rc, st), sn, cs);
          vst = rl(vs, st);
        } else {
          ph = s_phi[st];
          sn = s_a[st];
          cs = s_c[st];
          vst = s_v[st];
        }
        x = position_step<INTEG>(x, vst, cs, K);
        y = position_step<INTEG>(y, vst, sn, K);
        double px = x, py = y;
        if (ROT == kRotCum && fast) cum_pose<false>(K, x, y, px, py);
        s_tr[3 * st] = px;
        s_tr[3 * st + 1] = py;
        s_tr[3 * st + 2] = ph;
        if (win && st < 3) {
          win->tr[st][0] = px;
          win->tr[st][1] = py;
          win->tr[st][2] = ph;
        }
        if (st < 3) on_layer(st, px, py, ph);
      }
      if (n_run < n_steps) {
        lds->tail[0] = x;
        lds->tail[1] = y;
        lds->tail[2] = sn;
        lds->tail[3] = cs;
        lds->tail[4] = ph;
        lds->tail_from = n_run;
      }
    }
  }
  side_b(fast);
  __syncthreads();
  if (valid && lane < 3 * lds->tail_from) (&out->traj[0][0])[lane] = s_tr[lane];
}

// The rest of a deferred re-roll (emit_winner with defer_tail): every thread,
// after a barrier that follows emit_winner; K = the constants it was given.
template <int INTEG, int ROT>
__device__ void emit_winner_tail(const Consts& K, int n_steps, EmitLds* lds,
                                 mpc_result_t* __restrict__ out) {
  const int from = lds->tail_from;   // uniform
  if (from >= n_steps) return;
  double* s_tr = lds->tr;
  if (threadIdx.x == 0) {
    double x = lds->tail[0], y = lds->tail[1], sn = lds->tail[2], cs = lds->tail[3],
           ph = lds->tail[4];
    for (int st = from; st < n_steps; ++st) {
      ph = ph + lds->dphi[st];
      trig::rotate_sc(lds->a[st], lds->c[st], sn, cs);
      x = position_step<INTEG>(x, lds->v[st], cs, K);
      y = position_step<INTEG>(y, lds->v[st], sn, K);
      double px = x, py = y;
      if (ROT == kRotCum) cum_pose<false>(K, x, y, px, py);
      s_tr[3 * st] = px;
      s_tr[3 * st + 1] = py;
      s_tr[3 * st + 2] = ph;
    }
  }
  __syncthreads();
  const int q = threadIdx.x;
  if (q >= 3 * from && q < 3 * n_steps) (&out->traj[0][0])[q] = s_tr[q];
}

}  // namespace mpc
