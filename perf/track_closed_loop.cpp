// perf/track_closed_loop.cpp -- the plant under the solved plan's feedback policy, through the C++ facade: the kTurn90 batch
// (BASELINE config 3) is solved once, then AugmentedLagrangianiLQR::TrackClosedLoop (include/altro_mpc.h) simulates
// `samples` disturbed copies of every instance for `steps` knots on the device, the controls clipped to the problem's own
// bounds.
//   usage: track_closed_loop [batch] [samples] [steps] [--dump]
// The disturbances are closed formulas: dx0[b][s][i] = 1e-2 sin(1 + 3 s + 5 b + 7 i),
// w[b][s][k][i] = 1e-2 sin(2 + 3 s + 5 b + 7 i + 11 k).  Prints a summary; --dump prints every state, control and
// statistic as a hexadecimal float, one line per row (tests/test_mpc_track_gpu.py compares them with the C call's bit for
// bit):  "x <b> <s> <k> <x_0> .. "   "u <b> <s> <k> <u_0> .. "   "stats <b> <s> <status> <steps_done> <cost> <violation>
// <max_dx> <max_du>".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "altro/problems.hpp"

using namespace altro;

int main(int argc, char* argv[]) {
  bool dump = false;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--dump")) dump = true;
    else pos.push_back(argv[i]);
  }
  const int B = pos.size() > 0 ? std::stoi(pos[0]) : 16;
  const int S = pos.size() > 1 ? std::stoi(pos[1]) : 8;
  constexpr int n = 3, m = 2;
  try {
    problems::UnicycleProblem def;
    def.MakeTurn90Batch(B);
    problem::Problem prob = def.MakeProblem(true);
    augmented_lagrangian::AugmentedLagrangianiLQR<n, m> solver(prob);
    solver.GetiLQRSolver().SetRecordCostToGo(false);
    auto traj = std::make_shared<Trajectory<n, m>>(def.InitialTrajectory());
    solver.SetTrajectory(traj);
    solver.Solve();
    const int N = solver.NumSegments();
    const int steps = pos.size() > 2 ? std::stoi(pos[2]) : N;
    const size_t L = (size_t)B * S;
    std::vector<double> dx0(L * n), w(L * steps * n), X(L * (steps + 1) * n), U(L * steps * m);
    std::vector<altro_track_stats> stats(L);
    for (int b = 0; b < B; ++b)
      for (int s = 0; s < S; ++s)
        for (int i = 0; i < n; ++i) {
          const size_t l = (size_t)b * S + s;
          dx0[l * n + i] = 1e-2 * std::sin(1.0 + 3.0 * s + 5.0 * b + 7.0 * i);
          for (int k = 0; k < steps; ++k) w[(l * steps + k) * n + i] = 1e-2 * std::sin(2.0 + 3.0 * s + 5.0 * b + 7.0 * i + 11.0 * k);
        }
    const double u_lo[m] = {-1.5, -1.5}, u_hi[m] = {1.5, 1.5};  // (the bound of kTurn90: problems.hpp)
    solver.TrackClosedLoop(steps, S, dx0.data(), w.data(), u_lo, u_hi, X.data(), U.data(), stats.data());
    double worst_dx = 0.0, worst_viol = 0.0;
    int stopped = 0;
    for (const altro_track_stats& st : stats) {
      worst_dx = st.max_dx > worst_dx ? st.max_dx : worst_dx;
      worst_viol = st.violation > worst_viol ? st.violation : worst_viol;
      stopped += st.steps_done != steps;
    }
    std::printf("tracked %d instances x %d samples for %d of %d knots: stopped %d, max |x - Xbar| %.3g, max violation %.3g\n", B, S,
                steps, N, stopped, worst_dx, worst_viol);
    if (dump) {
      for (size_t l = 0; l < L; ++l) {
        const int b = (int)(l / S), s = (int)(l % S);
        for (int k = 0; k <= steps; ++k) {
          std::printf("x %d %d %d", b, s, k);
          for (int i = 0; i < n; ++i) std::printf(" %a", X[(l * (steps + 1) + k) * n + i]);
          std::printf("\n");
        }
        for (int k = 0; k < steps; ++k) {
          std::printf("u %d %d %d", b, s, k);
          for (int i = 0; i < m; ++i) std::printf(" %a", U[(l * steps + k) * m + i]);
          std::printf("\n");
        }
        std::printf("stats %d %d %d %d %a %a %a %a\n", b, s, stats[l].status, stats[l].steps_done, stats[l].cost, stats[l].violation,
                    stats[l].max_dx, stats[l].max_du);
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
