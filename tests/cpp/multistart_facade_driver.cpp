// Multi-start through the facade, on the GPU: altro::problems::UnicycleProblem (kTurn90) with `problems` goals and `starts`
// adjacent instances per goal, each start from constant controls of its own.  Solve, SelectStarts, GetBestStarts,
// PerturbControls, SpreadBestStart (include/altro/altro.hpp; thin calls of include/altro_multistart.h).  The repository's own
// driver; tests/test_multistart_gpu.py gives it the inputs and compares what it prints -- winners, and every state and control
// as a hexadecimal float -- with the C calls' results.
//
//   multistart_facade_driver <inputs file> <problems> <starts> <N>
// inputs file: doubles xf[B][3] | u0[B][2] | dU[starts][N][2], B = problems * starts.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "altro/problems.hpp"

static void DumpRows(const char* tag, const double* X, const double* U, int rows, int N) {
  for (int b = 0; b < rows; ++b)
    for (int k = 0; k <= N; ++k) {
      const double* x = X + ((size_t)b * (N + 1) + k) * 3;
      std::printf("%s x %d %d %a %a %a\n", tag, b, k, x[0], x[1], x[2]);
      if (k < N) std::printf("%s u %d %d %a %a\n", tag, b, k, U[((size_t)b * N + k) * 2], U[((size_t)b * N + k) * 2 + 1]);
    }
}
static void DumpTrajectory(const char* tag, const altro::Trajectory<3, 2>& Z, int B, int N) {
  for (int b = 0; b < B; ++b)
    for (int k = 0; k <= N; ++k) {
      std::printf("%s x %d %d %a %a %a\n", tag, b, k, Z.State(k, b)[0], Z.State(k, b)[1], Z.State(k, b)[2]);
      if (k < N) std::printf("%s u %d %d %a %a\n", tag, b, k, Z.Control(k, b)[0], Z.Control(k, b)[1]);
    }
}
static void PrintWinners(const char* tag, const std::vector<int>& w) {
  std::printf("%s", tag);
  for (int v : w) std::printf(" %d", v);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const int P = std::atoi(argv[2]), G = std::atoi(argv[3]), N = std::atoi(argv[4]), B = P * G;
  std::vector<double> in((size_t)B * 5 + (size_t)G * N * 2);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  const double *xf = in.data(), *u0 = xf + (size_t)B * 3, *dU = u0 + (size_t)B * 2;
  try {
    altro::problems::UnicycleProblem def;
    def.SetScenario(altro::problems::UnicycleProblem::kTurn90);
    def.N = N;
    def.batch = B;
    def.xf.assign(xf, xf + (size_t)B * 3);
    altro::problem::Problem prob = def.MakeProblem(true);
    altro::augmented_lagrangian::AugmentedLagrangianiLQR<3, 2> solver(prob);
    auto Z = std::make_shared<altro::Trajectory<3, 2>>(def.InitialTrajectory());
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < N; ++k) {
        Z->Control(k, b)[0] = u0[2 * b];
        Z->Control(k, b)[1] = u0[2 * b + 1];
      }
    solver.SetTrajectory(Z);
    solver.Solve();
    std::vector<int> win(P), bwin(P), swin(P);
    solver.SelectStarts(G, win.data());
    PrintWinners("select", win);
    std::vector<double> X((size_t)P * (N + 1) * 3), U((size_t)P * N * 2);
    solver.GetBestStarts(G, X.data(), U.data(), nullptr, bwin.data());
    PrintWinners("bestwin", bwin);
    DumpRows("best", X.data(), U.data(), P, N);
    solver.PerturbControls(G, dU);
    DumpTrajectory("perturbed", *Z, B, N);
    solver.SpreadBestStart(G, swin.data());
    PrintWinners("spreadwin", swin);
    DumpTrajectory("spread", *Z, B, N);
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
