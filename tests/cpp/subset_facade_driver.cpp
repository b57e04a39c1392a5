// The solve mask and sequential team rounds through the facade, on the GPU: the ring scenario of team_facade_driver.cpp
// (altro::problems::UnicycleProblem with kTurn90's cost, bound and goal constraint, a CircleConstraint per knot of [1, N) for the
// team-mates).  Solve, FillTeamTracks, SetSolveMask + Solve, GetSolveMask, SolveTeamSequential, ClearSolveMask
// (include/altro/altro.hpp; thin calls of include/altro_subset.h).  The repository's own driver;
// tests/test_subset_facade_gpu.py gives it the inputs and compares what it prints -- the masks, and every state and control as
// a hexadecimal float -- with the C calls' results.
//
//   subset_facade_driver <inputs file> <teams> <agents> <N> <sweeps>
// inputs file: doubles x0[B][3] | xf[B][3] | radius[agents] | mask[B] (non-zero: takes part), B = teams * agents.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "altro/problems.hpp"

static void DumpTrajectory(const char* tag, const altro::Trajectory<3, 2>& Z, int B, int N) {
  for (int b = 0; b < B; ++b)
    for (int k = 0; k <= N; ++k) {
      std::printf("%s x %d %d %a %a %a\n", tag, b, k, Z.State(k, b)[0], Z.State(k, b)[1], Z.State(k, b)[2]);
      if (k < N) std::printf("%s u %d %d %a %a\n", tag, b, k, Z.Control(k, b)[0], Z.Control(k, b)[1]);
    }
}
static void PrintMask(const char* tag, int count, const std::vector<unsigned char>& m) {
  std::printf("%s %d", tag, count);
  for (unsigned char x : m) std::printf(" %d", (int)x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  const int T = std::atoi(argv[2]), A = std::atoi(argv[3]), N = std::atoi(argv[4]), sweeps = std::atoi(argv[5]), B = T * A;
  std::vector<double> in((size_t)B * 7 + A);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  const double *x0 = in.data(), *xf = x0 + (size_t)B * 3, *radius = xf + (size_t)B * 3, *maskd = radius + A;
  std::vector<unsigned char> mask((size_t)B), got((size_t)B);
  for (int b = 0; b < B; ++b) mask[b] = maskd[b] != 0.0 ? 7 : 0;  // (any non-zero byte counts)
  try {
    altro::problems::UnicycleProblem def;
    def.SetScenario(altro::problems::UnicycleProblem::kTurn90);
    def.N = N;
    def.batch = B;
    def.x0.assign(x0, x0 + (size_t)B * 3);
    def.xf.assign(xf, xf + (size_t)B * 3);
    def.u0 = {0.1, 0.0};
    altro::problem::Problem prob = def.MakeProblem(true);
    // the placeholder circles of team_facade_driver.cpp: ONE knot constraint, which the team calls fill on the device
    const int np = 3 * (A - 1);
    for (int k = 1; k < N; ++k) {
      altro::examples::CircleConstraint seed;
      for (int i = 0; i < A - 1; ++i) seed.AddObstacle(1e-3 * k, 0.0, 0.0);
      std::shared_ptr<altro::constraints::Constraint<altro::constraints::Inequality>> con =
          std::make_shared<altro::examples::CircleConstraint>(seed);
      prob.SetConstraint(con, k);
    }
    altro::augmented_lagrangian::AugmentedLagrangianiLQR<3, 2> solver(prob);
    auto Z = std::make_shared<altro::Trajectory<3, 2>>(def.InitialTrajectory());
    solver.SetTrajectory(Z);
    solver.Solve();
    std::vector<double> par((size_t)B * (N - 1) * np);
    int index = -1;
    for (int i = 0; i < 8 && index < 0; ++i)
      if (altro_get_knot_params(solver.Handle(), i, par.data()) == ALTRO_OK) index = i;
    if (index < 0) return 4;
    std::printf("index %d\n", index);
    PrintMask("nomask", solver.GetSolveMask(got.data()), got);
    solver.FillTeamTracks(A, index, radius, false, ALTRO_TEAM_ALL, 1.0);
    solver.SetSolveMask(mask.data());
    PrintMask("mask", solver.GetSolveMask(got.data()), got);
    solver.Solve();
    DumpTrajectory("masked", *Z, B, N);
    solver.SolveTeamSequential(A, index, radius, false, sweeps);
    DumpTrajectory("sequential", *Z, B, N);
    PrintMask("after", solver.GetSolveMask(got.data()), got);
    solver.ClearSolveMask();
    PrintMask("cleared", solver.GetSolveMask(got.data()), got);
    std::printf("status %d\n", (int)solver.GetStatus());
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
