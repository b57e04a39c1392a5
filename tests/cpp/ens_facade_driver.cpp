// Monte-Carlo ensembles through the facade, on the GPU: altro::problems::UnicycleProblem (kTurn90's cost, bound and goal
// constraint) with a different initial state per instance.  Solve, TrackEnsemble, FillNoise, PerturbControlsGaussian
// (include/altro/altro.hpp; thin calls of include/altro_ensemble.h).  The repository's own driver;
// tests/test_ensemble_facade_gpu.py gives it the inputs and compares what it prints -- every number as a hexadecimal float --
// with the C calls' results.
//
//   ens_facade_driver <inputs file> <batch> <N> <samples> <seed> <instance_base> <viol_tol>
// inputs file: doubles x0[B][3] | Sigma0[B][3][3] | W[B][N][3][3] | u_lo[2] | u_hi[2] | sigma[2].
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "altro/problems.hpp"

static void PrintRow(const char* tag, const std::vector<double>& v) {
  std::printf("%s", tag);
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const int B = std::atoi(argv[2]), N = std::atoi(argv[3]), S = std::atoi(argv[4]);
  const unsigned long long seed = std::strtoull(argv[5], nullptr, 10), base = std::strtoull(argv[6], nullptr, 10);
  const double tol = std::atof(argv[7]);
  const size_t n0 = (size_t)B * 3, nS = (size_t)B * 9, nW = (size_t)B * N * 9;
  std::vector<double> in(n0 + nS + nW + 6);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  const double *x0 = in.data(), *Sigma0 = x0 + n0, *W = Sigma0 + nS, *lo = W + nW, *hi = lo + 2, *sigma = hi + 2;
  try {
    altro::problems::UnicycleProblem def;
    def.SetScenario(altro::problems::UnicycleProblem::kTurn90);
    def.N = N;
    def.batch = B;
    def.x0.assign(x0, x0 + n0);
    altro::problem::Problem prob = def.MakeProblem(true);
    altro::augmented_lagrangian::AugmentedLagrangianiLQR<3, 2> solver(prob);
    auto Z = std::make_shared<altro::Trajectory<3, 2>>(def.InitialTrajectory());
    solver.SetTrajectory(Z);
    solver.Solve();
    std::printf("status %d\n", (int)solver.GetStatus());
    const int mode = ALTRO_COV_W_PER_INSTANCE | ALTRO_COV_W_PER_KNOT;
    const size_t K1 = (size_t)N + 1;
    std::vector<double> mean((size_t)B * K1 * 3), mom2((size_t)B * K1 * 9);
    std::vector<int> alive((size_t)B * K1), viol((size_t)B * K1);
    std::vector<altro_ensemble_stats> sum((size_t)B);
    std::vector<altro_track_stats> st((size_t)B * S);
    solver.TrackEnsemble(N, S, seed, base, Sigma0, true, W, mode, lo, hi, tol, mean.data(), mom2.data(), alive.data(), viol.data(), sum.data(),
                         st.data());
    PrintRow("dev_mean", mean);
    PrintRow("dev_mom2", mom2);
    PrintRow("alive", std::vector<double>(alive.begin(), alive.end()));
    PrintRow("viol_count", std::vector<double>(viol.begin(), viol.end()));
    std::vector<double> flat;
    for (const altro_ensemble_stats& s : sum)
      for (double v : {(double)s.samples, (double)s.stopped_state, (double)s.stopped_control, (double)s.violated, s.cost_mean, s.cost_max,
                       s.violation_max, s.max_dx, s.max_du})
        flat.push_back(v);
    PrintRow("summary", flat);
    flat.clear();
    for (const altro_track_stats& s : st)
      for (double v : {(double)s.status, (double)s.steps_done, s.cost, s.violation, s.max_dx, s.max_du}) flat.push_back(v);
    PrintRow("stats", flat);
    std::vector<double> dx0((size_t)B * S * 3), w((size_t)B * S * N * 3);
    solver.FillNoise(N, S, seed, base, Sigma0, true, W, mode, dx0.data(), w.data());
    PrintRow("dx0", dx0);
    PrintRow("w", w);
    solver.PerturbControlsGaussian(1, seed, base, sigma, false);
    std::vector<double> X((size_t)B * K1 * 3), U((size_t)B * N * 2);
    if (altro_get_trajectory(solver.Handle(), X.data(), U.data()) != ALTRO_OK) return 4;
    PrintRow("U", U);
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
