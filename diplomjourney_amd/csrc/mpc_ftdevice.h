// mpc_ftdevice.h — the full tree's per-layer and per-leaf arithmetic
// (mpc_fulltree.h's kernels run it on the device; the host build of
// tests/replica_harness.cpp runs the same functions, so the two agree bit for
// bit).  No kernels here: a host-only build of this header links without a
// device code object.  (The per-control derivation stays in k_ft_controls.)
#pragma once

#include "mpc_device.h"

namespace mpc {

struct FtCtl {
  double v, beta, dphi, sd, cd;   // sd, cd = sin / cos of dphi (ROT)
  double vh;   // v * h (RECT's position increment factor, formed once per control)
};

struct FtState {
  double x, y, ph, s, c;
};

// The criterion's per-problem terms, folded once per problem (ft_crit) so that
// a leaf spends 27 VALU on it instead of 35:
//   10000*dist_target + 10*(arctan(x_t/y_t) - phi)^2 + 100*dist_line^2
// (run_math_model.py:82-86) with dist_line = |A x - B y + C1 - C2| / hyp
// (:53-61) evaluated as lin = fma(A, x, fma(-B, y, C1 - C2)) and
// 100*dist_line^2 = (lin * K2) * lin, K2 = 100 / hyp^2; the sum as
// fma(10000, dist_target, fma(lin * K2, lin, (10 a) a)).  Other roundings than
// the script's order (a few ulps of the cost; the tests' 1e-12 bar).  The
// line-origin sentinel (:57-58, dist_line = 1000) replaces lin by
// S = sqrt(1e8 / K2): its term is 1e8 to within an ulp or two, and such a
// leaf (the state AT the line origin, cost >= 1e8) never wins.
struct FtCrit {
  double x_t, y_t, x_0, y_0, A, nB, C, K2, S, atan_t;
};

MPC_HD __forceinline__ FtCrit ft_crit(const Consts& K, double atan_t) {
  FtCrit F;
  F.x_t = K.x_t;
  F.y_t = K.y_t;
  F.x_0 = K.x_0;
  F.y_0 = K.y_0;
  F.A = K.A;
  F.nB = -K.B;
  F.C = K.C1 - K.C2;
  F.K2 = 100.0 * (K.inv_den * K.inv_den);
  F.S = sqrt(1e8 / F.K2);
  F.atan_t = atan_t;
  return F;
}

MPC_HD __forceinline__ double cost_fulltree(double x, double y, double ph, const FtCrit& F) {
  const double a = F.atan_t - ph;
  const double ex = F.x_t - x, ey = F.y_t - y;
  const double dist_target = crit_sqrt(fma(ex, ex, ey * ey));
  const double lin0 = fma(F.A, x, fma(F.nB, y, F.C));
  const double lin = (x == F.x_0 && y == F.y_0) ? F.S : lin0;
  return fma(10000.0, dist_target, fma(lin * F.K2, lin, (a * 10.0) * a));
}

// iteration_of_predict (:111-115) with a precomputed control: heading first,
// then the position with the new heading.  ROT: (s, c) rotated by the
// control's sin / cos (the candidate rollout's complex product, 4 VALU).
template <int INTEG, bool ROT>
MPC_HD __forceinline__ FtState ft_apply(const FtState& in, const FtCtl& u, const Consts& K) {
  FtState o;
  o.ph = in.ph + u.dphi;
  if constexpr (ROT) {
    o.s = in.s;
    o.c = in.c;
    trig::rotate_sc(u.sd, u.cd, o.s, o.c);
  } else {
    trig::sincos_fast(o.ph, &o.s, &o.c);
  }
  if constexpr (INTEG == MPC_INTEG_RECT) {   // = position_step: fma(v * h, trig, p)
    o.x = fma(u.vh, o.c, in.x);
    o.y = fma(u.vh, o.s, in.y);
  } else {
    o.x = position_step<INTEG>(in.x, u.v, o.c, K);
    o.y = position_step<INTEG>(in.y, u.v, o.s, K);
  }
  return o;
}

// Keep-out circles (mpc_fulltree_argmin_obstacles): a layer state (x, y) lies
// strictly inside the circle (cx, cy, r2 = r * r) — the predicate of the
// rollout's CircleObs (mpc_device.h), in world coordinates.  A NaN state is
// inside nothing.
MPC_HD __forceinline__ bool ft_inside(double x, double y, double cx, double cy, double r2) {
  const double dx = x - cx, dy = y - cy;
  return fma(dy, dy, dx * dx) < r2;
}

// Reach culling.  vh_max: the largest |v * h| of the control table (NaN entries
// ignored; +inf if some |v * h| is).  One ft_apply moves a state by
//   |d| <= |v h| (1 + e) + 2^-53 (|x'| + |y'|)
// — the trig pair's norm and, for QK21, the quadrature's eleven roundings are
// within e << 2^-20 of 1; the last term is the rounding of the new position
// itself.  A leaf state inside circle (c, r) has |x'| <= |cx| + r, |y'| <= |cy| + r,
// and ft_inside evaluates its squared distance to within 4 ulp.  So a layer-1
// state whose leaf can be inside lies nearer to c than
//   R = (r + vh_max (1 + 2^-20) + 2^-50 (|cx| + |cy| + r)) (1 + 2^-20),
// the slack 2^-20 covering e, the roundings of R and of R * R, and those of the
// test that compares against it.  Returns R * R: a layer-1 state with
// d2 >= R * R (ft_inside's d2) has no leaf inside the circle.  +inf for an
// infinite vh_max: nothing is culled.
MPC_HD __forceinline__ double ft_reach_r2(double cx, double cy, double r2, double vh_max) {
  constexpr double kSlack = 1.0 + 0x1p-20;
  const double r = sqrt(r2);
  const double R = (r + vh_max * kSlack + 0x1p-50 * (fabs(cx) + fabs(cy) + r)) * kSlack;
  return R * R;
}

}  // namespace mpc
