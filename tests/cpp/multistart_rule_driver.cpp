// The multi-start selection rule (altro-cpp_amd/csrc/altro_common.hpp: ms_class, ms_before, ms_select) on the host, built
// with plain g++ by tests/test_multistart_rule.py -- the same function k_ms_select calls on the device.
//
//   multistart_rule_driver <keys file> <groups> <G>
// keys file: per start three doubles (status, cost, violation), [groups][G][3], raw bytes (so NaN, the infinities and -0.0
// arrive as they are).  Prints one line per group: the winner, then the class of every start.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "altro_common.hpp"

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int groups = std::atoi(argv[2]), G = std::atoi(argv[3]);
  std::vector<double> keys((size_t)groups * G * 3);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(keys.data(), sizeof(double), keys.size(), f) != keys.size()) return 3;
  std::fclose(f);
  std::vector<int> status(G);
  std::vector<double> cost(G), viol(G);
  for (int p = 0; p < groups; ++p) {
    for (int g = 0; g < G; ++g) {
      const double* k = keys.data() + ((size_t)p * G + g) * 3;
      status[g] = (int)k[0];
      cost[g] = k[1];
      viol[g] = k[2];
    }
    std::printf("%d", altro_hip::ms_select(status.data(), cost.data(), viol.data(), G, 1));
    for (int g = 0; g < G; ++g) std::printf(" %d", altro_hip::ms_class(status[g], cost[g], viol[g]));
    std::printf("\n");
  }
  return 0;
}
