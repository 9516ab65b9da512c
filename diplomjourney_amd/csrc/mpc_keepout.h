// mpc_keepout.h — keep-out polygons of the one-shot entries
// (mpc_rollout_partials_keepout; semantics in include/mpc_rollout.h): the edge
// tables, their host builder and checks, and the lane hook that applies a
// call's circles and then its polygons.  Compiles for host and device; the
// host test build is tests/polygon_harness.cpp.
//
//   Edge, Polygons, KeepoutArgs      the tables of a launch
//   check_polygons                   the entries' argument rule (host)
//   world_polygons, frame_edge, frame_polygons   the tables of a call (host)
//   edge_inner, inside_polygons      the predicate, as the hook evaluates it
//   KeepoutObs<NOBS>                 the lane hook (the style of CircleObs)
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/mpc_rollout.h"
#include "mpc_device.h"

namespace mpc {

// One edge as a half-plane: a point is on the edge's inner side iff
// a x + b y + c > 0.  (a, b) is the unit inner normal of the edge's line and
// c = -(a Px + b Py) for its first endpoint P, so the value is the point's
// signed distance from the line.  A positive common factor changes no sign:
// the rect+cum frame uses that (frame_edge).
struct Edge {
  double a, b, c;   // 24 B
};
// Every slot of every polygon holds an edge, so any vertex count is served by
// straight-line code over a polygon's 8 slots: an unused edge of a used
// polygon is always true (0, 0, 1).  The hook loops over the call's polygon
// count; the polygons past it are padded all the same, every edge always false
// (0, 0, -1), so a reader of all four never enters one.  A NaN
// state makes every edge value NaN — 0 * NaN included — which is not > 0: it
// is inside nothing, padded or not.
struct Polygons {
  Edge e[MPC_MAX_POLYGONS][MPC_MAX_POLYGON_VERTICES];   // 768 B
};
// The kernels' first argument: the circle tables (mpc_device.h ObstacleArgs'
// members, at the same offsets) and the polygon tables, `loop` and `world` of
// each as described at Circle.
struct KeepoutArgs {
  Obstacles loop, world;
  Polygons ploop, pworld;
  int32_t n_polygons, pad_[3];
};
// HIP passes at most 4 KB of kernel arguments: the tables, Consts and the
// launch's pointers and sizes (64 B) fit.
static_assert(sizeof(Polygons) == 768 && sizeof(KeepoutArgs) == 2576, "table layout");
static_assert(sizeof(KeepoutArgs) + sizeof(Consts) + 64 <= 4096, "kernel-argument segment");
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) Polygons* PolyTable;
#else
typedef const Polygons* PolyTable;
#endif

// The edge test: two fused operations and a compare.  With unit normals the
// computed value differs from the signed distance by a few ulps of
// |x| + |y| + |c| (mpc_rollout.h gives the bound).
MPC_HD __forceinline__ bool edge_inner(double a, double b, double c, double x, double y) {
  return fma(a, x, fma(b, y, c)) > 0.0;
}

// (x, y) strictly inside any of the table's first n_poly polygons: edges
// ANDed, polygons ORed — the hook's rule, for the host (polygon_harness.cpp).
inline bool inside_polygons(const Polygons& T, int n_poly, double x, double y) {
  bool any = false;
  for (int p = 0; p < n_poly; ++p) {
    bool in = true;
    for (int i = 0; i < MPC_MAX_POLYGON_VERTICES; ++i)
      in &= edge_inner(T.e[p][i].a, T.e[p][i].b, T.e[p][i].c, x, y);
    any |= in;
  }
  return any;
}

// The argument rule of the keep-out entries, one condition per polygon: after
// normalising the orientation by the sign of the shoelace area, every vertex
// other than an edge's two endpoints lies strictly on the inner side of that
// edge's line.  That refuses a zero or non-finite area, a repeated vertex, a
// collinear triple, a reflex vertex, a bow-tie and a pentagram (whose turns
// all have one sign).  Vertex differences are taken first, so a polygon far
// from the origin is judged by its shape.
inline bool polygon_ok(const mpc_polygon_t& g) {
  const int n = g.n_vertices;
  if (n < 3 || n > MPC_MAX_POLYGON_VERTICES) return false;
  for (int i = 0; i < n; ++i)
    if (!isfinite(g.x[i]) || !isfinite(g.y[i])) return false;
  double area2 = 0.0;   // twice the signed area, about vertex 0
  for (int i = 1; i + 1 < n; ++i)
    area2 += (g.x[i] - g.x[0]) * (g.y[i + 1] - g.y[0]) - (g.x[i + 1] - g.x[0]) * (g.y[i] - g.y[0]);
  if (!isfinite(area2) || area2 == 0.0) return false;
  const double sgn = area2 > 0 ? 1.0 : -1.0;
  for (int i = 0; i < n; ++i) {
    const int j = (i + 1) % n;
    const double dx = g.x[j] - g.x[i], dy = g.y[j] - g.y[i];
    for (int k = 0; k < n; ++k) {
      if (k == i || k == j) continue;
      if (!(sgn * (dx * (g.y[k] - g.y[i]) - dy * (g.x[k] - g.x[i])) > 0.0)) return false;
    }
  }
  return true;
}

inline int check_polygons(const mpc_polygon_t* polygons, int32_t n) {
  if (n < 0 || n > MPC_MAX_POLYGONS || (n > 0 && !polygons)) return MPC_ERR_ARG;
  for (int i = 0; i < n; ++i)
    if (!polygon_ok(polygons[i])) return MPC_ERR_ARG;
  return MPC_OK;
}

// The world table of n checked polygons.  A clockwise vertex list is reversed
// first, so both orientations of one list give the same table bit for bit.
inline Polygons world_polygons(const mpc_polygon_t* polygons, int n) {
  Polygons W;
  for (int p = 0; p < MPC_MAX_POLYGONS; ++p)
    for (int i = 0; i < MPC_MAX_POLYGON_VERTICES; ++i)
      W.e[p][i] = Edge{0.0, 0.0, p < n ? 1.0 : -1.0};
  for (int p = 0; p < n; ++p) {
    const mpc_polygon_t& g = polygons[p];
    const int m = g.n_vertices;
    double area2 = 0.0;
    for (int i = 1; i + 1 < m; ++i)
      area2 += (g.x[i] - g.x[0]) * (g.y[i + 1] - g.y[0]) - (g.x[i + 1] - g.x[0]) * (g.y[i] - g.y[0]);
    double x[MPC_MAX_POLYGON_VERTICES], y[MPC_MAX_POLYGON_VERTICES];
    for (int i = 0; i < m; ++i) {
      const int q = area2 > 0 ? i : m - 1 - i;
      x[i] = g.x[q];
      y[i] = g.y[q];
    }
    for (int i = 0; i < m; ++i) {   // counter-clockwise: the inner side is on the left
      const int j = (i + 1) % m;
      const double dx = x[j] - x[i], dy = y[j] - y[i], len = hypot(dx, dy);
      const double a = -dy / len, b = dx / len;
      W.e[p][i] = Edge{a, b, -fma(a, x[i], b * y[i])};
    }
  }
  return W;
}

// One world edge in the frame of the kRotCum sums (A, B) of the step that
// starts at K's pose.  cum_pose gives x = Kx + c0 A - s0 B, y = Ky + s0 A +
// c0 B, so a x + b y + c = (a c0 + b s0) A + (b c0 - a s0) B + (a Kx + b Ky + c):
// a line stays a line.  The 1/L-scaled sums of PL2 are A / L and B / L: the
// constant term times 1/L (exact, L a power of two) is the same test divided
// by L > 0.  A padded edge (a = b = 0) keeps its sign.
MPC_HD __forceinline__ Edge frame_edge(const Consts& K, const Edge& w, bool scaled) {
  const double c = fma(w.a, K.x, fma(w.b, K.y, w.c));
  return Edge{w.a * K.c0 + w.b * K.s0, w.b * K.c0 - w.a * K.s0, scaled ? c * K.inv_L : c};
}

inline Polygons frame_polygons(const Consts& K, const Polygons& world) {
  Polygons F;
  for (int p = 0; p < MPC_MAX_POLYGONS; ++p)
    for (int i = 0; i < MPC_MAX_POLYGON_VERTICES; ++i)
      F.e[p][i] = frame_edge(K, world.e[p][i], K.L_pow2 != 0);
  return F;
}

// The tables of a one-shot launch: `world` as given, `loop` in the frame of
// the recurrence's (x, y) (the circles: host_obstacles' pair).
inline KeepoutArgs keepout_args(const Consts& K, const ObstacleArgs& circles,
                                const mpc_polygon_t* polygons, int n_polygons, bool cum) {
  const Polygons W = world_polygons(polygons, n_polygons);
  return KeepoutArgs{circles.loop, circles.world, cum ? frame_polygons(K, W) : W, W, n_polygons,
                     {0, 0, 0}};
}

// A lane predicate as the wave's mask, and a mask's bit of this lane: SGPR
// pairs both ways, no instruction.  (The host pass only parses the hook.)
__device__ __forceinline__ uint64_t wave_mask(bool lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ballot_w64(lane);
#else
  return lane ? ~uint64_t{0} : 0;
#endif
}
__device__ __forceinline__ bool lane_of(uint64_t mask) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_inverse_ballot_w64(mask);
#else
  return mask != 0;
#endif
}

// The lane hook of the keep-out entries: the call's circles (CircleObs<NOBS>'s
// test; NOBS = 0: no circle statement), then its polygons.  Per edge and
// candidate 2 fma and 1 compare; the compares' lane masks are ANDed within a
// polygon and ORed into `blocked` on the SALU.  The tables are wave-uniform
// (kernel arguments, scalar loads): nothing here is per lane.
// One polygon is 24 scalar operands (48 SGPRs), four are 192: as with
// CircleObs<16> they do not survive the rollout loop in SGPRs, and with the
// four polygons' tests unrolled into one block hipcc gathers all their loads
// at its head and spills them (1000 to 2000 SGPR spills and scratch, counted
// with the unrolled form).  So the polygons are a wave-uniform loop over the
// call's count, never unrolled: one polygon's 24 operands are live at a time,
// the step's scalar loads stay inside the step, and a call pays for the
// polygons it has.  Within a polygon the 8 edge slots are straight-line code.
template <int NOBS>
struct KeepoutObs {
  static_assert(NOBS >= 0 && NOBS <= MPC_MAX_OBSTACLES, "circle count");
  static constexpr bool kOn = true;
  ObsTable loop_c, world_c;
  PolyTable loop_p, world_p;
  int n_poly;   // (wave-uniform: a kernel argument)
  template <int CPL>
  __device__ __forceinline__ static void test(ObsTable tc, PolyTable tp, int n_poly,
                                              const double (&x)[CPL], const double (&y)[CPL],
                                              bool (&blocked)[CPL]) {
    if constexpr (NOBS > 0) CircleObs<NOBS>::template test<CPL>(tc, x, y, blocked);
    // The edge compares as wave masks (a ballot of a compare is the compare
    // itself, written to an SGPR pair), ANDed and ORed as 64-bit scalars and
    // turned back into the lane predicate once, for free.  As bool chains the
    // SLP vectoriser packed the 16 predicates of a polygon into byte vectors
    // (v_cndmask / shifts / v_bitop3 per polygon) and kept three copies of
    // every candidate's (x, y) in VGPRs: two of the streaming kernels spilled.
    uint64_t any[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) any[j] = wave_mask(blocked[j]);
    // The table pointer opaque per step, as CircleObs<16>'s — and the circles'
    // result with it: the polygons' loads then cannot rise above the circle
    // test, whose 96 SGPRs of operands would be spilled across the polygon loop.
    static_assert(CPL == 1 || CPL == 2, "candidates per lane");
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (CPL == 2)
      asm volatile("" : "+s"(tp), "+s"(any[0]), "+s"(any[1]));
    else
      asm volatile("" : "+s"(tp), "+s"(any[0]));
#endif
#pragma unroll 1
    for (int p = 0; p < n_poly; ++p) {
      uint64_t in[CPL];
#pragma unroll
      for (int j = 0; j < CPL; ++j) in[j] = ~uint64_t{0};
#pragma unroll
      for (int i = 0; i < MPC_MAX_POLYGON_VERTICES; ++i) {
        const double a = tp->e[p][i].a, b = tp->e[p][i].b, c = tp->e[p][i].c;
#pragma unroll
        for (int j = 0; j < CPL; ++j) in[j] &= wave_mask(edge_inner(a, b, c, x[j], y[j]));
      }
#pragma unroll
      for (int j = 0; j < CPL; ++j) any[j] |= in[j];
    }
#pragma unroll
    for (int j = 0; j < CPL; ++j) blocked[j] = lane_of(any[j]);
  }
  template <int CPL>
  __device__ __forceinline__ void loop(const double (&x)[CPL], const double (&y)[CPL],
                                       bool (&blocked)[CPL]) const {
    test<CPL>(loop_c, loop_p, n_poly, x, y, blocked);
  }
  __device__ __forceinline__ void world(double x, double y, bool& blocked) const {
    const double xs[1] = {x}, ys[1] = {y};
    bool bl[1] = {blocked};
    test<1>(world_c, world_p, n_poly, xs, ys, bl);
    blocked = bl[0];
  }
};

}  // namespace mpc
