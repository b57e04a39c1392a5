// Teams through the facade, on the GPU: altro::problems::UnicycleProblem (kTurn90's cost, bound and goal constraint) with
// `teams` x `agents` unicycles that swap sides of a ring and a CircleConstraint per knot of [1, N) for the team-mates.  Solve (against
// placeholder circles of radius 0), TeamClearance, FillTeamTracks, SolveTeam (include/altro/altro.hpp; thin calls of
// include/altro_team.h).  The repository's own driver; tests/test_team_gpu.py gives it the inputs and compares what it prints
// -- clearances, the filled parameters, and every state and control as a hexadecimal float -- with the C calls' results.
//
//   team_facade_driver <inputs file> <teams> <agents> <N> <mode> <blend> <rounds>
// inputs file: doubles x0[B][3] | xf[B][3] | radius[agents], B = teams * agents.
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
static void PrintRow(const char* tag, const std::vector<double>& v) {
  std::printf("%s", tag);
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const int T = std::atoi(argv[2]), A = std::atoi(argv[3]), N = std::atoi(argv[4]), mode = std::atoi(argv[5]), B = T * A;
  const double blend = std::atof(argv[6]);
  const int rounds = std::atoi(argv[7]);
  std::vector<double> in((size_t)B * 6 + A);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  const double *x0 = in.data(), *xf = x0 + (size_t)B * 3, *radius = xf + (size_t)B * 3;
  try {
    altro::problems::UnicycleProblem def;
    def.SetScenario(altro::problems::UnicycleProblem::kTurn90);
    def.N = N;
    def.batch = B;
    def.x0.assign(x0, x0 + (size_t)B * 3);
    def.xf.assign(xf, xf + (size_t)B * 3);
    def.u0 = {0.1, 0.0};
    altro::problem::Problem prob = def.MakeProblem(true);
    // the caller's idiom: a CircleConstraint of its own on every knot of [1, N), one circle per team-mate.  Nothing is known
    // of the team-mates yet: radius 0 (never active), the centre a placeholder that differs from knot to knot.  The facade
    // emits the loop as ONE knot constraint (include/altro_knot_params.h), which the team calls then fill on the device.
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
    // the registration index of the knot constraint: the only one altro_get_knot_params answers for
    std::vector<double> par((size_t)B * (N - 1) * np);
    int index = -1;
    for (int i = 0; i < 8 && index < 0; ++i)
      if (altro_get_knot_params(solver.Handle(), i, par.data()) == ALTRO_OK) index = i;
    if (index < 0) return 4;
    std::printf("index %d\n", index);
    std::vector<double> clear((size_t)T);
    solver.TeamClearance(A, index, radius, false, clear.data());
    PrintRow("uncoupled", clear);
    solver.FillTeamTracks(A, index, radius, false, mode, 1.0);
    if (altro_get_knot_params(solver.Handle(), index, par.data()) != ALTRO_OK) return 4;
    PrintRow("params", par);
    solver.SolveTeam(A, index, radius, false, mode, blend, rounds);
    DumpTrajectory("team", *Z, B, N);
    solver.TeamClearance(A, index, radius, false, clear.data());
    PrintRow("coupled", clear);
    std::printf("status %d\n", (int)solver.GetStatus());
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
