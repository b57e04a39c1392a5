// Instantiates the batched AL-iLQR engine for (double, UnicycleM) on gfx950.
#include "altro_engine.hpp"
namespace altro_hip {
EngineBase* MakeEngineUnicycleF64(const altro_desc& d, std::string* err) { return MakeEngineImpl<double, UnicycleM>(d, err); }
}  // namespace altro_hip

// The split policy of the persistent tail as the kernels inline it (TwinCtl, altro_kernels.hpp), on the host, for
// tests/test_tail_endgame_policy.py (here because this translation unit sees the kernels' header; in no public header: not
// part of the interface).  Returns the minimum share in use for `asked_min`.
extern "C" int altro_twin_policy(int R, int lag, int asked_min, int* keep, int* claimable, int* see_claim) {
  const int min_share = altro_hip::tw_min_share(asked_min);
  if (keep) *keep = altro_hip::tw_keep(R, lag);
  if (claimable) *claimable = altro_hip::tw_claimable(R, lag, min_share) ? 1 : 0;
  if (see_claim) *see_claim = altro_hip::kTwinSeeClaim;
  return min_share;
}

// The ticket arithmetic of the persistent tail's worker grid as the kernel and LaunchTail use it, on the host, for
// tests/test_tail_workers_policy.py.  Returns the launch's grid for `asked` (ALTRO_HIP_TAIL_WORKERS; negative: unset);
// *workers: resident workers (0: the one-shot grid); *block: the block of the one-shot grid whose identity ticket `ticket`
// of `kind` (0 primary, 1 pool) carries, -1 past the last one.
extern "C" int altro_tail_tickets(int ninst, int npool, int cus, int per_cu, int asked, int kind, int ticket, int* workers, int* block) {
  const int w = altro_hip::tail_worker_count(ninst, npool, cus, per_cu, asked);
  if (workers) *workers = w;
  if (block) *block = altro_hip::tail_block_of_ticket(kind, ticket, ninst, npool);
  return altro_hip::tail_grid(ninst, npool, w);
}
