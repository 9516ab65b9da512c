// CPU sanitizer driver (ASan/UBSan on the CPU restatement) — test
// infrastructure only.  One executable holds the C oracle (oracle/
// mpc_oracle.c, compiled separately as C) and the host replica of the
// kernels' arithmetic (tests/replica_harness.cpp, included below), and runs:
//   synth    edge-size synthetic cases: n_cand 0..4097 (odd, wave +-1), horizons
//            1..32, every integrator, costs + layer states out (the oracle's
//            states_out indexing), the batched scan, the sampler with
//            index_base / ld, the full tree with every per-leaf output, and
//            the replica with and without an installed estimate table
//   calls F  the reference's recorded predictive_control calls, as written by
//            tests/test_sanitizers.py into F (binary, see read_calls), through
//            the oracle in qk21: one mpc_result_t per call appended to F.out
// and prints a 64-bit FNV-1a checksum of every output byte, so that the test
// can compare a plain and an -fsanitize=address,undefined build bit for bit.
// The restated reference code lives in mpc_oracle.c (math_model_tree.py:56-115,
// run_math_model.py:82-197) and mpc_device.h (the host-derived constants:
// mpc_host_consts.h); nothing here restates it.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "replica_harness.cpp"

extern "C" {
int mpc_oracle_rollout_argmin(const mpc_problem_t* p, const double* v, const double* beta,
                              int64_t n_cand, int32_t n_steps, int64_t index_base,
                              double incumbent, int32_t integ, mpc_result_t* out,
                              double* costs_out, double* states_out);
int mpc_oracle_rollout_argmin_batched(const mpc_problem_t* problems, const double* incumbents,
                                      int32_t n_problems, const double* v, const double* beta,
                                      int64_t cand, int32_t n_steps, int32_t integ,
                                      mpc_result_t* out);
void mpc_oracle_sample_controls(const double* v_grid, int32_t n_v, const double* beta_grid,
                                int32_t n_beta, int64_t n_cand, int32_t n_steps, uint64_t seed,
                                int64_t index_base, int32_t const_prefix, double* v_sc,
                                double* beta_sc, int64_t ld);
int64_t mpc_oracle_fulltree_argmin(const double* V, int32_t nv, const double* B, int32_t nb,
                                   double x, double y, double phi, double x_t, double y_t,
                                   double x_0, double y_0, double atan_target, double L,
                                   double t_a, double t_b, double incumbent, int32_t integ,
                                   double* best_cost, int32_t* found, double* res,
                                   double* out_costs, double* out_leaf, double* out_l0,
                                   double* out_l1);
}

static uint64_t g_fnv = 1469598103934665603ull;
static void mix(const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) g_fnv = (g_fnv ^ b[i]) * 1099511628211ull;
}
template <class T>
static void mixv(const std::vector<T>& v) {
  if (!v.empty()) mix(v.data(), v.size() * sizeof(T));
}

static const int kIntegs[] = {MPC_INTEG_QK21, MPC_INTEG_RECT,
                              MPC_INTEG_QK21 | MPC_HEADING_ROTATE,
                              MPC_INTEG_RECT | MPC_HEADING_ROTATE,
                              MPC_INTEG_RECT | MPC_HEADING_CUMULATIVE};

static mpc_problem_t problem(double x, double y, double phi, double L, double t) {
  mpc_problem_t p;
  p.x = x; p.y = y; p.phi = phi;
  p.x_t = 2.0; p.y_t = 3.0; p.x_0 = 0.0; p.y_0 = 0.0;
  p.L = L; p.t_a = t; p.t_b = t + 0.05;
  return p;
}

static int synth() {
  const double V[] = {0.0, 0.1, 0.25, 0.5, 0.75, 1.0};
  const double B[] = {-1.047, -0.6, -0.2, 0.0, 0.3, 0.7, 1.047, 1.3};   // 1.3: |beta| > 1.1
  const int nv = 6, nb = 8;
  const int64_t sizes[] = {0, 1, 2, 3, 63, 64, 65, 1000, 4097};
  const int horizons[] = {1, 3, 10, 32};
  for (int64_t n : sizes)
    for (int ns : horizons) {
      const int64_t ld = n + 5;   // a row pitch wider than the row
      std::vector<double> v(static_cast<size_t>(ns * ld + 1)), b(v.size());
      mpc_oracle_sample_controls(V, nv, B, nb, n, ns, 20261015u + n, 7, 1, v.data(), b.data(),
                                 ld);
      // the scans read [ns][n] rows: repack
      // (one spare element: an empty shard still passes non-null pointers)
      std::vector<double> vv(static_cast<size_t>(ns * n + 1)), bb(vv.size());
      for (int s = 0; s < ns; ++s)
        for (int64_t c = 0; c < n; ++c) {
          vv[s * n + c] = v[s * ld + c];
          bb[s * n + c] = b[s * ld + c];
        }
      mixv(vv);
      mixv(bb);
      for (int ig : kIntegs) {
        for (double L : {0.5, 0.45}) {
          const mpc_problem_t p = problem(0.2, -0.1, 0.4, L, 0.35);
          mpc_result_t r;
          std::vector<double> costs(static_cast<size_t>(n)),
              states(static_cast<size_t>(ns * 3 * n));
          const int st = mpc_oracle_rollout_argmin(&p, vv.data(), bb.data(), n, ns, 11, 1e300,
                                                   ig & 0xff, &r, costs.data(), states.data());
          if (st != 0) return 10;
          mix(&r, sizeof r);
          mixv(costs);
          mixv(states);
          std::vector<double> rc(static_cast<size_t>(n)), rs(static_cast<size_t>(ns * 3 * n));
          replica_rollout(&p, vv.data(), bb.data(), n, ns, ig, rs.data(), rc.data());
          mixv(rc);
          mixv(rs);
        }
      }
    }
  // the reciprocal-estimate table path of the replica (installed, then removed)
  {
    const int64_t n = 129;
    const int ns = 5;
    std::vector<double> v(ns * n), b(ns * n);
    mpc_oracle_sample_controls(V, nv, B, nb, n, ns, 99, 0, 0, v.data(), b.data(), n);
    std::vector<double> q(b.size()), r(b.size());
    replica_tan_q(b.data(), static_cast<int64_t>(b.size()), q.data());
    for (size_t i = 0; i < q.size(); ++i) r[i] = 1.0 / q[i];
    replica_set_rcp_table(q.data(), r.data(), static_cast<int64_t>(q.size()));
    const mpc_problem_t p = problem(0.0, 0.0, 0.0, 0.5, 0.05);
    std::vector<double> rc(n), rs(ns * 3 * n);
    replica_rollout(&p, v.data(), b.data(), n, ns, MPC_INTEG_RECT | MPC_HEADING_CUMULATIVE,
                    rs.data(), rc.data());
    const int64_t miss = replica_rcp_misses();
    replica_set_rcp_table(nullptr, nullptr, 0);
    mixv(rc);
    mixv(rs);
    mix(&miss, sizeof miss);
  }
  // batched robots (config E's layout: robot r owns columns [r*cand, (r+1)*cand))
  {
    const int R = 7, ns = 4;
    const int64_t cand = 33;
    std::vector<double> v(ns * R * cand), b(v.size());
    for (int r = 0; r < R; ++r)
      mpc_oracle_sample_controls(V, nv, B, nb, cand, ns, 500 + r, 0, 1, v.data() + r * cand,
                                 b.data() + r * cand, R * cand);
    std::vector<mpc_problem_t> probs;
    std::vector<double> inc;
    for (int r = 0; r < R; ++r) {
      probs.push_back(problem(0.1 * r, -0.05 * r, 0.3 - 0.1 * r, 0.5, 0.05));
      inc.push_back(r == 3 ? 0.0 : 1e300);   // robot 3: nothing beats its incumbent
    }
    for (int ig : kIntegs) {
      std::vector<mpc_result_t> out(R);
      if (mpc_oracle_rollout_argmin_batched(probs.data(), inc.data(), R, v.data(), b.data(), cand,
                                            ns, ig & 0xff, out.data()) != 0)
        return 11;
      for (const auto& o : out) mix(&o, sizeof o);
    }
  }
  // full tree with every per-leaf output (run_math_model.py:158-197)
  {
    const double FV[] = {0.0, 0.5, 1.0};
    const double FB[] = {-0.5, 0.0, 0.5};
    const int64_t s1 = 9, leaves = s1 * s1 * s1;
    for (int ig : {MPC_INTEG_QK21, MPC_INTEG_RECT}) {
      std::vector<double> costs(leaves), leaf(3 * leaves), l0(3 * s1), l1(3 * s1 * s1);
      double best = 0, res[9];
      int32_t found = 0;
      const int64_t j = mpc_oracle_fulltree_argmin(FV, 3, FB, 3, 0.1, 0.2, 0.3, 4.0, 5.0, 0.0,
                                                   0.0, 0.6747409422235527, 0.5, 0.05, 0.1,
                                                   1e18, ig, &best, &found, res, costs.data(),
                                                   leaf.data(), l0.data(), l1.data());
      mix(&j, sizeof j);
      mix(&best, sizeof best);
      mix(&found, sizeof found);
      mix(res, sizeof res);
      mixv(costs);
      mixv(leaf);
      mixv(l0);
      mixv(l1);
    }
  }
  return 0;
}

// calls file: int64 count, then per call: int64 n_cand, 10 doubles problem,
// double incumbent, v[3 * n_cand], beta[3 * n_cand] (step-major, N = 3)
static int calls(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 20;
  int64_t count = 0;
  if (fread(&count, 8, 1, f) != 1 || count < 0 || count > 100000) return 21;
  std::vector<mpc_result_t> out(static_cast<size_t>(count));
  for (int64_t i = 0; i < count; ++i) {
    int64_t n = 0;
    double pd[11];
    if (fread(&n, 8, 1, f) != 1 || n < 0 || n > 1000000 || fread(pd, 8, 11, f) != 11) return 22;
    mpc_problem_t p;
    memcpy(&p, pd, sizeof p);
    static_assert(sizeof(mpc_problem_t) == 10 * sizeof(double), "problem = 10 doubles");
    std::vector<double> v(static_cast<size_t>(3 * n)), b(v.size());
    if (fread(v.data(), 8, v.size(), f) != v.size() || fread(b.data(), 8, b.size(), f) != b.size())
      return 23;
    if (mpc_oracle_rollout_argmin(&p, v.data(), b.data(), n, 3, 0, pd[10], MPC_INTEG_QK21,
                                  &out[static_cast<size_t>(i)], nullptr, nullptr) != 0)
      return 24;
  }
  fclose(f);
  std::string o = std::string(path) + ".out";
  FILE* g = fopen(o.c_str(), "wb");
  if (!g) return 25;
  fwrite(out.data(), sizeof(mpc_result_t), out.size(), g);
  fclose(g);
  mixv(out);
  return 0;
}

int main(int argc, char** argv) {
  int rc = 2;
  if (argc >= 2 && !strcmp(argv[1], "synth")) rc = synth();
  else if (argc >= 3 && !strcmp(argv[1], "calls")) rc = calls(argv[2]);
  else if (argc >= 2 && !strcmp(argv[1], "canary")) {   // proves the instrumentation is live
    std::vector<double> x(4, 1.0);
    volatile const double* q = x.data();
    rc = static_cast<int>(q[argc + 2]);   // one past the end: ASan must stop here
  }
  printf("fnv %016llx rc %d\n", static_cast<unsigned long long>(g_fnv), rc);
  return rc;
}
