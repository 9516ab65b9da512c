// The host builds of the fleet calls' two device functions (fleet_d2 and
// fleet_predict, csrc/mpc_device.h): the distance the kernel ranks neighbours
// by and the centre it forms a predicted call's per-step tables with, compiled
// for the host with the library's -ffp-contract=off, so that
// tests/fleet_model.py chooses neighbours and places the moving circles by the
// device's own bits.  Test infrastructure only.
#include "../diplomjourney_amd/csrc/mpc_device.h"

extern "C" {

// out[q] = fleet_d2(robot r's position, robot q's) for every q of the board
void fleet_d2_row(const double* x, const double* y, int64_t n, int64_t r, double* out) {
  for (int64_t q = 0; q < n; ++q) out[q] = mpc::fleet_d2(x[r], y[r], x[q], y[q]);
}

// out[q] = fleet_predict(x[q], d[q], j) for every q
void fleet_predict_row(const double* x, const double* d, int64_t n, int64_t j, double* out) {
  for (int64_t q = 0; q < n; ++q) out[q] = mpc::fleet_predict(x[q], d[q], static_cast<int>(j));
}

}  // extern "C"
