// The trigger rule (altro-cpp_amd/csrc/altro_common.hpp: trigger_reason) on the host, built with plain g++ by
// tests/test_trigger_rule.py -- the same function k_mpc_trigger calls on the device.
//
//   trigger_rule_driver <rows file> <rows>
// rows file: per row 15 doubles, raw bytes (so NaN and the infinities arrive as they are):
//   max_age dx_tol viol_tol on_unsolved lookahead ahead_tol | age | has_tracked status violation max_dx | status | has_ahead status violation
// Prints the bits FIRST .. AHEAD on the first line, then one reason per row.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "altro_common.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int rows = std::atoi(argv[2]);
  std::vector<double> in((size_t)rows * 15);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
  std::fclose(f);
  using namespace altro_hip;
  std::printf("%d %d %d %d %d %d %d\n", kTrigFirst, kTrigAge, kTrigDeviation, kTrigViolation, kTrigLimit, kTrigUnsolved, kTrigAhead);
  for (int r = 0; r < rows; ++r) {
    const double* v = in.data() + (size_t)r * 15;
    const TriggerRule rule{(int)v[0], v[1], v[2], (int)v[3], (int)v[4], v[5]};
    TrackStats tracked{}, ahead{};
    tracked.status = (int)v[8];
    tracked.violation = v[9];
    tracked.max_dx = v[10];
    ahead.status = (int)v[13];
    ahead.violation = v[14];
    std::printf("%d\n", trigger_reason(rule, (int)v[6], v[7] != 0.0 ? &tracked : nullptr, (int)v[11], v[12] != 0.0 ? &ahead : nullptr));
  }
  return 0;
}
