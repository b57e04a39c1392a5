// The closed-loop covariance through the facade, on the GPU: altro::problems::UnicycleProblem (kTurn90's cost, bound and goal
// constraint) with a different initial state per instance and a CircleConstraint per knot of [1, N) that is never active (one far
// circle whose centre differs from knot to knot, so the facade emits the loop as ONE knot constraint).  Solve,
// PropagateCovariance, InflateCircleTrack (include/altro/altro.hpp; thin calls of include/altro_covariance.h).  The repository's
// own driver; tests/test_cov_facade_gpu.py gives it the inputs and compares what it prints -- every number as a hexadecimal
// float -- with the C calls' results.
//
//   cov_facade_driver <inputs file> <batch> <N> <rows> <kappa>
// inputs file: doubles x0[B][3] | Sigma0[B][3][3] | W[B][N][3][3] | base[rows][3].
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
  if (argc < 6) return 2;
  const int B = std::atoi(argv[2]), N = std::atoi(argv[3]), rows = std::atoi(argv[4]);
  const double kappa = std::atof(argv[5]);
  const size_t n0 = (size_t)B * 3, nS = (size_t)B * 9, nW = (size_t)B * N * 9, nb = (size_t)rows * 3;
  std::vector<double> in(n0 + nS + nW + nb);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  const double *x0 = in.data(), *Sigma0 = x0 + n0, *W = Sigma0 + nS, *base = W + nW;
  try {
    altro::problems::UnicycleProblem def;
    def.SetScenario(altro::problems::UnicycleProblem::kTurn90);
    def.N = N;
    def.batch = B;
    def.x0.assign(x0, x0 + n0);
    altro::problem::Problem prob = def.MakeProblem(true);
    for (int k = 1; k < N; ++k) {
      altro::examples::CircleConstraint far;
      far.AddObstacle(5.0 + 1e-3 * k, 5.0, 0.1);
      std::shared_ptr<altro::constraints::Constraint<altro::constraints::Inequality>> con =
          std::make_shared<altro::examples::CircleConstraint>(far);
      prob.SetConstraint(con, k);
    }
    altro::augmented_lagrangian::AugmentedLagrangianiLQR<3, 2> solver(prob);
    auto Z = std::make_shared<altro::Trajectory<3, 2>>(def.InitialTrajectory());
    solver.SetTrajectory(Z);
    solver.Solve();
    std::printf("status %d\n", (int)solver.GetStatus());
    std::vector<double> Sigma((size_t)B * (N + 1) * 9), sx((size_t)B * (N + 1) * 3), su((size_t)B * N * 2), rpos((size_t)B * (N + 1));
    solver.PropagateCovariance(N, Sigma0, true, W, ALTRO_COV_W_PER_INSTANCE | ALTRO_COV_W_PER_KNOT, Sigma.data(), sx.data(), su.data(),
                               rpos.data());
    PrintRow("Sigma", Sigma);
    PrintRow("sx", sx);
    PrintRow("su", su);
    PrintRow("rpos", rpos);
    // the registration index of the knot constraint: the only one altro_get_knot_params answers for
    std::vector<double> par((size_t)B * (N - 1) * 3);
    int index = -1;
    for (int i = 0; i < 8 && index < 0; ++i)
      if (altro_get_knot_params(solver.Handle(), i, par.data()) == ALTRO_OK) index = i;
    if (index < 0) return 4;
    std::printf("index %d\n", index);
    solver.InflateCircleTrack(index, base, rows, false, kappa, rpos.data());
    if (altro_get_knot_params(solver.Handle(), index, par.data()) != ALTRO_OK) return 4;
    PrintRow("params", par);
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
