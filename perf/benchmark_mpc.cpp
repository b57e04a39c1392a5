// perf/benchmark_mpc.cpp -- a receding-horizon loop through the C++ facade: the kTurn90 batch (BASELINE config 3) is solved,
// the first `shift` controls are "applied" (the plan's own state plus a small disturbance becomes the new initial state),
// the horizon moves forward on the device (AugmentedLagrangianiLQR::AdvanceHorizon, include/altro_mpc.h) and the next
// solve starts warm (reset_duals = false).
//   usage: benchmark_mpc [cycles] [batch] [shift] [--check]
// Prints per-cycle iterations and times; exits non-zero when a cycle after the first needs more iterations than the first --
// iterations of a cycle = iterations_total summed over ALL instances of the batch, the same instances in every cycle (an
// instance that ends the cold solve at an iteration limit counts there with that limit, and with what it then needs warm).
// --check: prints one line "iterations <cycle> <instance> <iterations_total> <status>" per solve instead of the times
// (tests/test_mpc_gpu.py compares them with the Python loop).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "altro/problems.hpp"

using namespace altro;

int main(int argc, char* argv[]) {
  bool check = false;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--check")) check = true;
    else pos.push_back(argv[i]);
  }
  const int cycles = pos.size() > 0 ? std::stoi(pos[0]) : 6;
  const int B = pos.size() > 1 ? std::stoi(pos[1]) : 16;
  const int shift = pos.size() > 2 ? std::stoi(pos[2]) : 5;
  try {
    problems::UnicycleProblem def;
    def.MakeTurn90Batch(B);
    problem::Problem prob = def.MakeProblem(true);
    augmented_lagrangian::AugmentedLagrangianiLQR<3, 2> solver(prob);
    solver.GetiLQRSolver().SetRecordCostToGo(false);
    auto traj = std::make_shared<Trajectory<3, 2>>(def.InitialTrajectory());
    solver.SetTrajectory(traj);
    solver.GetOptions().reset_duals = false;  // warm start: the duals the advance carried stay (al_solver.hpp:292-297)
    std::vector<double> w((size_t)B * 3);
    int first_sum = 0, failures = 0;
    for (int c = 0; c < cycles; ++c) {
      const auto t0 = std::chrono::high_resolution_clock::now();
      solver.Solve();
      const auto t1 = std::chrono::high_resolution_clock::now();
      // the disturbance of the closed-loop tests: w[c][b][i] = 1e-2 sin(1 + 3c + 5b + 7i)
      for (int b = 0; b < B; ++b)
        for (int i = 0; i < 3; ++i) w[(size_t)b * 3 + i] = 1e-2 * std::sin(1.0 + 3.0 * c + 5.0 * b + 7.0 * i);
      const auto t2 = std::chrono::high_resolution_clock::now();
      solver.AdvanceHorizon(shift, nullptr, w.data());
      const auto t3 = std::chrono::high_resolution_clock::now();
      int it_max = 0, it_sum = 0, solved = 0, b = 0;
      for (const altro_stats& s : solver.GetStats().AllInstances()) {
        if (check) std::printf("iterations %d %d %d %d\n", c, b, s.iterations_total, s.status);
        it_max = s.iterations_total > it_max ? s.iterations_total : it_max;
        solved += s.status == 0;
        it_sum += s.iterations_total;
        ++b;
      }
      if (c == 0) first_sum = it_sum;
      if (c > 0 && it_sum > first_sum) ++failures;
      if (!check)
        std::printf("cycle %d: solved %d/%d, iterations sum %d max %d, solve %.3f ms, advance %.3f ms\n", c, solved, B, it_sum,
                    it_max, std::chrono::duration<double, std::milli>(t1 - t0).count(),
                    std::chrono::duration<double, std::milli>(t3 - t2).count());
    }
    if (failures) {
      std::fprintf(stderr, "%d cycle(s) after the first needed more iterations than the first (%d)\n", failures, first_sum);
      return 2;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
