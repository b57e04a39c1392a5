// The reference's moving-obstacle idiom through the facade, on the GPU: prob.SetConstraint(std::make_shared<CircleConstraint>(
// ...), k) and prob.SetConstraint(std::make_shared<ControlBound>(...), k) in a loop over the knots, an object of its own on
// each (altro/problem/problem.hpp:66-133), beside the per-knot SetCostFunction loop.  24 distinct knots: more than the library
// holds as knot classes, so the facade emits them as knot constraints with the parameters as tracks on the device
// (include/altro_knot_params.h).  The repository's own driver; tests/test_knot_params_gpu.py gives it the rows and compares
// what it prints -- every state and control as a hexadecimal float -- with the C call's results.
//
//   knot_params_facade_driver <rows file> <B> <N> <h>
// rows file: doubles [B][N + 1][15], row k = xref (3), uref (2), two circles (6), lb (2), ub (2) of knot k.  Solves, prints,
// advances the horizon by 5 knots and reports where the windows then stand.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "altro/augmented_lagrangian/al_solver.hpp"
#include "altro/problem/problem.hpp"
#include "examples/problems/unicycle.hpp"

namespace al = altro::augmented_lagrangian;
namespace pb = altro::problem;
namespace ex = altro::examples;

static std::vector<double> Diag3(double a, double b, double c) { return {a, 0, 0, 0, b, 0, 0, 0, c}; }

template <class Solver>
static void Dump(const char* tag, Solver& solver, const altro::Trajectory<3, 2>& Z, int B, int N) {
  std::printf("%s iterations %d outer %d status %d offset %d\n", tag, solver.GetStats().iterations_total, solver.GetStats().iterations_outer,
              static_cast<int>(solver.GetStatus()), solver.GetTrackOffset());
  for (int b = 0; b < B; ++b)
    for (int k = 0; k <= N; ++k) {
      std::printf("%s x %d %d %a %a %a\n", tag, b, k, Z.State(k, b)[0], Z.State(k, b)[1], Z.State(k, b)[2]);
      if (k < N) std::printf("%s u %d %d %a %a\n", tag, b, k, Z.Control(k, b)[0], Z.Control(k, b)[1]);
    }
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const int B = std::atoi(argv[2]), N = std::atoi(argv[3]), W = 15;
  const float h = static_cast<float>(std::atof(argv[4]));
  std::vector<double> path((size_t)B * (N + 1) * W);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(path.data(), sizeof(double), path.size(), f) != path.size()) return 3;
  std::fclose(f);
  const double hd = h;
  const std::vector<double> Q = Diag3(10.0 * hd, 10.0 * hd, 1.0 * hd), R = {0.1 * hd, 0, 0, 0.1 * hd}, Qf = Diag3(10.0, 10.0, 1.0),
                            R0 = {0, 0, 0, 0};
  try {
    pb::Problem prob(N);
    prob.SetBatch(B);
    for (int k = 0; k <= N; ++k) {  // the per-knot loop of the reference
      std::vector<double> xref((size_t)B * 3), uref((size_t)B * 2);
      for (int b = 0; b < B; ++b) {
        const double* row = path.data() + ((size_t)b * (N + 1) + k) * W;
        for (int i = 0; i < 3; ++i) xref[(size_t)b * 3 + i] = row[i];
        for (int i = 0; i < 2; ++i) uref[(size_t)b * 2 + i] = row[3 + i];
      }
      prob.SetCostFunction(ex::QuadraticCost::LQRCost(k < N ? Q : Qf, k < N ? R : R0, xref, uref, k == N), k);
    }
    using Model = pb::DiscretizedModel<ex::Unicycle>;
    const Model model{ex::Unicycle()};
    for (int k = 0; k < N; ++k) prob.SetDynamics(std::make_shared<Model>(model), k);
    for (int k = 0; k < N; ++k) {  // the per-knot loop of the reference: the circles before the bound on every knot
      std::vector<double> circles((size_t)B * 6), bound((size_t)B * 4);
      for (int b = 0; b < B; ++b) {
        const double* row = path.data() + ((size_t)b * (N + 1) + k) * W;
        for (int i = 0; i < 6; ++i) circles[(size_t)b * 6 + i] = row[5 + i];
        for (int i = 0; i < 4; ++i) bound[(size_t)b * 4 + i] = row[11 + i];
      }
      if (k >= 1) {
        auto obs = std::make_shared<ex::CircleConstraint>();
        obs->SetBatchObstacles(circles, 6);
        prob.SetConstraint(obs, k);
      }
      auto bnd = std::make_shared<ex::ControlBound>(std::vector<double>{-1, -1}, std::vector<double>{1, 1});
      bnd->params = bound;  // (per instance: batch blocks of lb, ub back to back)
      bnd->nparams = 4;
      prob.SetConstraint(bnd, k);
    }
    std::vector<double> x0((size_t)B * 3);
    for (int b = 0; b < B; ++b)
      for (int i = 0; i < 3; ++i) x0[(size_t)b * 3 + i] = path[(size_t)b * (N + 1) * W + i] + (i == 1 ? 0.1 : 0.0);
    prob.SetInitialState(x0);
    al::AugmentedLagrangianiLQR<3, 2> solver(prob);
    auto Z = std::make_shared<altro::Trajectory<3, 2>>(N, B);
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < N; ++k) {
        Z->Control(k, b)[0] = 0.1;
        Z->Control(k, b)[1] = 0.1;
      }
    Z->SetUniformStep(h);
    solver.SetTrajectory(Z);
    solver.Solve();
    Dump("first", solver, *Z, B, N);
    solver.AdvanceHorizon(5);
    std::printf("advanced offset %d reference %d\n", solver.GetTrackOffset(), solver.GetReferenceOffset());
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
