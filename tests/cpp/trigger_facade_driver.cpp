// Event-triggered re-planning through the facade, on the GPU: altro::problems::UnicycleProblem (kTurn90's cost, bound and
// goal constraint) with a different initial state per instance.  Solve, TrackClosedLoop, EvaluateTrigger, RunTriggered
// (include/altro/altro.hpp; thin calls of include/altro_trigger.h).  The repository's own driver;
// tests/test_trigger_gpu.py gives it the inputs and compares what it prints -- every floating-point number as a hexadecimal
// float -- with the C calls' results.
//
//   trigger_facade_driver <inputs file> <batch> <N> <cycles> <shift> <max_age> <dx_tol>
// inputs file: doubles x0[B][3] | w[cycles][B][shift][3] | age[B].
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
static void PrintInts(const char* tag, const std::vector<int>& v) {
  std::printf("%s", tag);
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}
static void PrintStats(const char* tag, const std::vector<altro_track_stats>& v) {
  std::printf("%s", tag);
  for (const altro_track_stats& s : v)
    std::printf(" %d %d %a %a %a %a", s.status, s.steps_done, s.cost, s.violation, s.max_dx, s.max_du);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const int B = std::atoi(argv[2]), N = std::atoi(argv[3]), cycles = std::atoi(argv[4]), shift = std::atoi(argv[5]);
  altro_trigger_rule rule;
  rule.max_age = std::atoi(argv[6]);
  rule.dx_tol = std::atof(argv[7]);
  rule.viol_tol = -1.0;
  rule.on_unsolved = 1;
  rule.lookahead = 0;
  rule.ahead_tol = 0.0;
  const size_t n0 = (size_t)B * 3, nw = (size_t)cycles * B * shift * 3;
  std::vector<double> in(n0 + nw + (size_t)B);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  const double *x0 = in.data(), *w = x0 + n0;
  std::vector<int> age(B);
  for (int b = 0; b < B; ++b) age[b] = (int)in[n0 + nw + b];
  const double lo[2] = {-1.5, -1.5}, hi[2] = {1.5, 1.5};
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
    std::printf("solved %d\n", (int)solver.GetStatus());
    // the rule over a tracked segment: cycle 0's disturbance, one sample
    std::vector<altro_track_stats> seg(B);
    solver.TrackClosedLoop(shift, 1, nullptr, w, lo, hi, nullptr, nullptr, seg.data());
    std::vector<unsigned char> mask(B);
    std::vector<int> why(B);
    solver.EvaluateTrigger(rule, seg.data(), age.data(), lo, hi, mask.data(), why.data());
    PrintInts("mask", std::vector<int>(mask.begin(), mask.end()));
    PrintInts("why", why);
    // ... and the run
    const size_t L = (size_t)cycles * shift;
    std::vector<double> X((size_t)B * (L + 1) * 3), U((size_t)B * L * 2);
    std::vector<int> it((size_t)B * cycles), st((size_t)B * cycles), reason((size_t)B * cycles);
    std::vector<altro_track_stats> track((size_t)B * cycles);
    solver.RunTriggered(cycles, shift, w, lo, hi, rule, X.data(), U.data(), it.data(), st.data(), track.data(), reason.data());
    PrintRow("X_cl", X);
    PrintRow("U_cl", U);
    PrintInts("iterations", it);
    PrintInts("status", st);
    PrintInts("reason", reason);
    PrintStats("track", track);
    std::printf("after %d\n", (int)solver.GetStatus());
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
