// part_offsets_driver.cpp -- prints, as one JSON object, where Parts (altro_common.hpp: host code, no HIP) puts the parts of the
// two device blocks the closed-loop code carves: the block of a tracked run (TrackedRunParts) and the block Engine::MpcTrack
// stages for a host caller (TrackStageParts).  argv: n m B cycles shift.  tests/test_part_offsets.py holds the expectations.
#include <cstddef>
#include <cstdio>
#include <cstdlib>

#include "altro_common.hpp"

using namespace altro_hip;

template <int K>
static void Print(const char* name, const Parts<K>& p, const char* tail) {
  std::printf("\"%s\": {\"cnt\": [", name);
  for (int i = 0; i < K; ++i) std::printf("%s%zu", i ? ", " : "", p.cnt[i]);
  std::printf("], \"off\": [");
  for (int i = 0; i <= K; ++i) std::printf("%s%zu", i ? ", " : "", p.off[i]);
  std::printf("], \"total\": %zu}%s\n", p.total(), tail);
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int n = std::atoi(argv[1]), m = std::atoi(argv[2]);
  const size_t B = (size_t)std::atoi(argv[3]), cycles = (size_t)std::atoi(argv[4]), shift = (size_t)std::atoi(argv[5]);
  std::printf("{\"stats_doubles\": %zu,\n", sizeof(TrackStats) / sizeof(double));
  Print("tracked_run", TrackedRunParts(n, m, B, cycles, shift), ",");
  // one cycle of that run as a host call: B lanes (one sample), `shift` steps, every array present ...
  Print("track_stage", TrackStageParts(n, m, B, shift, true, true, true, true, true, true), ",");
  // ... and with only w and the statistics: an array the caller leaves out takes no room
  Print("track_stage_sparse", TrackStageParts(n, m, B, shift, false, true, false, false, false, true), "}");
  return 0;
}
