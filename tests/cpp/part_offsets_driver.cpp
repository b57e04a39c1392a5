// part_offsets_driver.cpp -- prints, as one JSON object, where Parts (altro_common.hpp: host code, no HIP) puts the parts of the
// two device blocks the closed-loop code carves: the block of a tracked run (TrackedRunParts) and the block Engine::MpcTrack
// stages for a host caller (TrackStageParts), and the named layouts of the other staged calls and of the other runs.
// argv: n m B cycles shift.  tests/test_part_offsets.py holds the expectations.
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
  Print("track_stage_sparse", TrackStageParts(n, m, B, shift, false, true, false, false, false, true), ",");
  // the block of a multi-start run (w, dU [2][N = shift][m]) and of a plain one (neither; no clearances either)
  Print("plain_run", PlainRunParts(n, m, B, cycles, shift, true, 2 * shift * m, 0), ",");
  Print("plain_run_sparse", PlainRunParts(n, m, B, cycles, shift, false, 0, 0), ",");
  // the other staged calls, with `shift` steps (and a horizon of `shift` knots): everything per instance and per knot ...
  double x = 0;  // (only whether a pointer is null matters)
  CovArgs c{};
  c.steps = (int)shift;
  c.sigma0_per_instance = 1;
  c.w_mode = 3;
  c.Sigma0 = c.W = &x;
  c.Sigma = c.sx = c.su = c.rpos = &x;
  Print("cov_stage", CovStageParts(n, m, B, c), ",");
  // ... and one shared W, no Sigma0, of the outputs only sx and rpos
  c.w_mode = 0;
  c.Sigma0 = nullptr;
  c.Sigma = c.su = nullptr;
  Print("cov_stage_sparse", CovStageParts(n, m, B, c), ",");
  Print("inflate_stage", InflateStageParts(B, shift, 3, B, shift + 1), ",");  // one obstacle, a base track per instance
  Print("inflate_stage_shared", InflateStageParts(1, shift, 3, B, shift + 1), ",");
  Print("ms_best_stage", MsBestStageParts(n, m, B, shift, true, true, 7), ",");  // statistics of 7 doubles
  Print("ms_best_stage_sparse", MsBestStageParts(n, m, B, shift, false, true, 0), ",");
  Print("perturb_stage", PerturbStageParts(m, B, shift), ",");
  Print("advance_stage", AdvanceStageParts(n, B, true, true), ",");
  Print("advance_stage_sparse", AdvanceStageParts(n, B, false, true), ",");
  Print("reference_stage", ReferenceStageParts(n, m, B * (shift + 1), true), ",");
  Print("reference_stage_sparse", ReferenceStageParts(n, m, B * (shift + 1), false), ",");
  // the int block of a run, in ints, for the four kinds: plain / tracked, multi-start with 5 starts, team (as plain), triggered
  Print("run_ints", RunIntParts(B, cycles, 0, false), ",");
  Print("run_ints_multistart", RunIntParts(B, cycles, B / 5, false), ",");
  Print("run_ints_team", RunIntParts(B, cycles, 0, false), ",");
  Print("run_ints_triggered", RunIntParts(B, cycles, 0, true), ",");
  // a host caller's trigger evaluation with a lookahead, and a device caller's (only the lookahead's statistics)
  Print("trigger_stage", TriggerStageParts(m, B, true, true, true, true, true, true), ",");
  Print("trigger_stage_sparse", TriggerStageParts(m, B, false, false, false, false, false, true), ",");
  Print("lqr_stage", LqrStageParts(n, m, B, shift, true, true, true), ",");  // a horizon of `shift` knots
  Print("lqr_stage_sparse", LqrStageParts(n, m, B, shift, true, false, true), ",");
  Print("mask_stage", MaskStageParts(B), "}");
  return 0;
}
