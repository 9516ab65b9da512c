// The host build of a predicted fleet call's circle centre (fleet_predict,
// csrc/mpc_device.h): the function the kernel forms the per-step tables with,
// compiled for the host with the library's -ffp-contract=off, so that
// tests/fleet_motion_model.py places the moving circles by the device's own
// bits.  Test infrastructure only.
#include "../diplomjourney_amd/csrc/mpc_device.h"

extern "C" {

// out[q] = fleet_predict(x[q], d[q], j) for every q
void fleet_predict_row(const double* x, const double* d, int64_t n, int64_t j, double* out) {
  for (int64_t q = 0; q < n; ++q) out[q] = mpc::fleet_predict(x[q], d[q], static_cast<int>(j));
}

}  // extern "C"
