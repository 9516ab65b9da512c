// mpc_dispatch.h — runtime options -> template arguments, on the host: the one
// vocabulary of every translation unit that launches kernels (mpc_rollout.hip,
// mpc_episodes_obs.hip).
#pragma once

#include <stdint.h>

#include <type_traits>

#include "../../include/mpc_rollout.h"
#include "mpc_device.h"

namespace mpc {

template <int V>
using IC = std::integral_constant<int, V>;
template <bool V>
using BC = std::integral_constant<bool, V>;

inline bool is_cum(int32_t integrator) { return (integrator & MPC_HEADING_CUMULATIVE) != 0; }

// Runtime bools -> f(BC<b0>{}, BC<b1>{}, ...): one call per combination, so a
// kernel's bool template parameters can follow runtime decisions.
template <class F, class... Bs>
void dispatch_bools(F&& f, bool b, Bs... rest) {
  if constexpr (sizeof...(rest) == 0) {
    b ? f(BC<true>{}) : f(BC<false>{});
  } else {
    b ? dispatch_bools([&](auto... t) { f(BC<true>{}, t...); }, rest...)
      : dispatch_bools([&](auto... t) { f(BC<false>{}, t...); }, rest...);
  }
}

// integrator -> f(IC<INTEG>, BC<ROT>): the integrator and whether the heading is
// a rotation.  As it stands, the full-tree kernels' dispatch (direct or rotation
// heading only: their entries refuse MPC_HEADING_CUMULATIVE).  The tags convert
// to their values, so a lambda's (auto I, auto R) go straight into k<I, R>.
template <class F>
void dispatch_integ_rot(int32_t integrator, F&& f) {
  dispatch_bools(
      [&](auto rect, auto rot) { f(IC<rect ? MPC_INTEG_RECT : MPC_INTEG_QK21>{}, rot); },
      (integrator & 0xff) == MPC_INTEG_RECT, (integrator & MPC_HEADING_ROTATE) != 0);
}

// integrator -> f(IC<INTEG>, IC<ROT>), ROT as described above mode_ok
// (mpc_rollout.hip).
template <class F>
void dispatch_mode(int32_t integrator, F&& f) {
  if ((integrator & 0xff) == MPC_INTEG_RECT && is_cum(integrator))
    f(IC<MPC_INTEG_RECT>{}, IC<kRotCum>{});
  else
    dispatch_integ_rot(integrator, [&](auto integ, auto rot) { f(integ, IC<rot ? 1 : 0>{}); });
}

// n_obs -> f(IC<NOBS>) over the instantiations: 4 or all, and with ONE also 1.
template <bool ONE, class F>
void dispatch_nobs(int n_obs, F&& f) {
  if constexpr (ONE) {
    if (n_obs <= 1) return f(IC<1>{});
  }
  if (n_obs <= 4)
    f(IC<4>{});
  else
    f(IC<MPC_MAX_OBSTACLES>{});
}

}  // namespace mpc
