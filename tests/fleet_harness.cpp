// The host build of the fleet call's distance (fleet_d2, csrc/mpc_device.h): the
// function the kernel ranks neighbours by, compiled for the host with the
// library's -ffp-contract=off, so that tests/fleet_model.py chooses neighbours
// by the device's own bits.  Test infrastructure only.
#include "../diplomjourney_amd/csrc/mpc_device.h"

extern "C" {

// out[q] = fleet_d2(robot r's position, robot q's) for every q of the board
void fleet_d2_row(const double* x, const double* y, int64_t n, int64_t r, double* out) {
  for (int64_t q = 0; q < n; ++q) out[q] = mpc::fleet_d2(x[r], y[r], x[q], y[q]);
}

}  // extern "C"
