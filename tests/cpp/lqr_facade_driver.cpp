// Time-varying LQR tracking gains through the facade, on the GPU: altro::problems::UnicycleProblem (kTurn90's cost, bound and
// goal constraint) with a different initial state per instance.  SetLqrGainPolicy, Solve (which ends with the pass and
// installs its gains), ClearLqrGainPolicy, ComputeLqrGains without installing (include/altro/altro.hpp; thin calls of
// include/altro_lqr.h).  The repository's own driver; tests/test_lqr_facade_gpu.py gives it the inputs and compares what it
// prints -- every number as a hexadecimal float -- with the C calls' results.
//
//   lqr_facade_driver <inputs file> <batch> <N>
// inputs file: doubles x0[B][3] | Q[3][3] | R[2][2] | Qf[3][3].
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
  if (argc < 4) return 2;
  const int B = std::atoi(argv[2]), N = std::atoi(argv[3]);
  const size_t n0 = (size_t)B * 3;
  std::vector<double> in(n0 + 9 + 4 + 9);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  const double *x0 = in.data(), *Q = x0 + n0, *R = Q + 9, *Qf = R + 4;
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
    solver.SetLqrGainPolicy(Q, R, Qf);
    solver.Solve();
    std::printf("status %d\n", (int)solver.GetStatus());
    std::vector<double> K((size_t)B * N * 6), d((size_t)B * N * 2), P((size_t)B * (N + 1) * 9);
    if (altro_get_gains(solver.Handle(), K.data(), d.data()) != ALTRO_OK) return 4;
    PrintRow("policy_K", K);
    PrintRow("policy_d", d);
    solver.ClearLqrGainPolicy();
    int on = 1;
    if (altro_lqr_get_policy(solver.Handle(), &on, nullptr, nullptr, nullptr) != ALTRO_OK || on != 0) return 5;
    std::vector<int> fail(B, 7);
    solver.ComputeLqrGains(Q, R, Qf, false, K.data(), P.data(), fail.data());
    PrintRow("K", K);
    PrintRow("P", P);
    PrintRow("fail", std::vector<double>(fail.begin(), fail.end()));
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
