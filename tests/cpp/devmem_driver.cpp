// devmem_driver.cpp -- altro_devmem.hpp (the owners of the engine's device memory and the staging helper) against host stubs of
// the HIP entry points the header calls: malloc / free with a book of live blocks, memcpy, an allocation and a copy that can be
// told to fail at their k-th call.  No GPU, no HIP runtime.  Prints one JSON object; tests/test_devmem.py holds the
// expectations.  A staged block is exactly total() doubles of malloc, so a wrong offset is an out-of-bounds access for the
// sanitizer build.  argv: n m B steps cycles shift.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "altro_devmem.hpp"

using namespace altro_hip;

// ---- the stubs -----------------------------------------------------------------------------------------------------
static std::set<void*> g_live;
static int g_mallocs = 0, g_frees = 0, g_bad_frees = 0, g_fail_malloc_at = 0;
static int g_copies = 0, g_h2d = 0, g_d2h = 0, g_fail_copy_at = 0, g_syncs = 0;
static hipError_t g_sync_result = hipSuccess;

static hipError_t StubAlloc(void** p, size_t bytes) {
  *p = nullptr;
  if (++g_mallocs == g_fail_malloc_at) return hipErrorOutOfMemory;
  *p = std::malloc(bytes);
  g_live.insert(*p);
  return hipSuccess;
}
static hipError_t StubFree(void* p) {
  ++g_frees;
  if (!g_live.erase(p)) {
    ++g_bad_frees;  // freed twice, or never handed out
    return hipErrorInvalidValue;
  }
  std::free(p);
  return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return StubAlloc(p, bytes); }
hipError_t hipFree(void* p) { return StubFree(p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return StubAlloc(p, bytes); }
hipError_t hipHostFree(void* p) { return StubFree(p); }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
  if (++g_copies == g_fail_copy_at) return hipErrorInvalidValue;
  (kind == hipMemcpyHostToDevice ? g_h2d : g_d2h)++;
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
  ++g_syncs;
  return g_sync_result;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
}
static int g_unexpected = 0;  // an allocation of the driver's own that failed
static void Must(hipError_t e) { g_unexpected += e != hipSuccess; }
static void ResetCounters() {
  g_mallocs = g_frees = g_bad_frees = g_fail_malloc_at = 0;
  g_copies = g_h2d = g_d2h = g_fail_copy_at = g_syncs = 0;
  g_sync_result = hipSuccess;
}

// ---- owners --------------------------------------------------------------------------------------------------------
static void Owners() {
  ResetCounters();
  int live_after_move = 0, live_after_assign = 0, live_after_realloc = 0;
  bool moved_from_empty = false, pinned_dev_ok = false;
  {
    DevBlock<double> a;
    Must(a.alloc(4));
    DevBlock<double> b(std::move(a));  // a move
    moved_from_empty = !a && a.count() == 0 && b && b.count() == 4;
    live_after_move = (int)g_live.size();
    {
      DevBlock<double> c;
      Must(c.alloc(3));
      c = std::move(b);  // a move-assignment onto a live block: what c held goes with b, at the end of b's scope or before
      live_after_assign = (int)g_live.size();
      Must(c.alloc(7));  // alloc on a live block
      live_after_realloc = (int)g_live.size();
      DevBlock<int> zero;
      Must(zero.alloc(0));  // (at least one element is asked for)
    }
    PinnedBlock<int> h;
    Must(h.alloc(16));
    PinnedBlock<int> h2(std::move(h));
    pinned_dev_ok = h2.get() != nullptr && h2.count() == 16 && h.get() == nullptr;
    h2 = PinnedBlock<int>{};  // a fresh value in place of a live block
  }
  std::printf("\"owners\": {\"moved_from_empty\": %s, \"pinned_ok\": %s, \"live_after_move\": %d, \"live_after_assign\": %d, "
              "\"live_after_realloc\": %d, \"mallocs\": %d, \"frees\": %d, \"bad_frees\": %d, \"live\": %zu},\n",
              moved_from_empty ? "true" : "false", pinned_dev_ok ? "true" : "false", live_after_move, live_after_assign, live_after_realloc,
              g_mallocs, g_frees, g_bad_frees, g_live.size());
}

// the shape of Engine::Uploaded: a pool, a block that grows on its own, blocks inside a vector, raw pointers into the pool
struct Track {
  DevBlock<double> track, spare;
};
struct Upload {
  DevPool pool;
  DevBlock<double> path;
  std::vector<Track> tracks;
  float* f = nullptr;
  int* i = nullptr;
  double* d = nullptr;
  unsigned long long* w = nullptr;
};
static constexpr int kUploadAllocs = 8;
static bool Fill(Upload& u) {  // stops at the first failure, as an upload does
  if (u.pool.alloc(&u.f, 5) != hipSuccess) return false;
  if (u.pool.alloc(&u.i, 3) != hipSuccess) return false;
  if (u.pool.alloc(&u.d, 0) != hipSuccess) return false;
  if (u.pool.alloc(&u.w, 9) != hipSuccess) return false;
  if (u.path.alloc(11) != hipSuccess) return false;
  if (u.path.alloc(22) != hipSuccess) return false;  // (it grows)
  u.tracks.emplace_back();
  if (u.tracks.back().track.alloc(6) != hipSuccess) return false;
  if (u.tracks.back().spare.alloc(6) != hipSuccess) return false;
  return true;
}
static void UploadOwner() {
  ResetCounters();
  Upload u;
  const bool filled = Fill(u);
  const size_t live_full = g_live.size();
  u = Upload{};
  std::printf("\"upload\": {\"filled\": %s, \"live_full\": %zu, \"live_after_drop\": %zu, \"pointers_null\": %s, "
              "\"live_after_failed\": [",
              filled ? "true" : "false", live_full, g_live.size(), !u.f && !u.i && !u.d && !u.w && !u.path ? "true" : "false");
  bool all_failed = true;
  for (int k = 1; k <= kUploadAllocs; ++k) {
    g_mallocs = 0;
    g_fail_malloc_at = k;
    all_failed = !Fill(u) && all_failed;
    u = Upload{};
    std::printf("%s%zu", k > 1 ? ", " : "", g_live.size());
  }
  g_fail_malloc_at = 0;
  std::printf("], \"every_k_failed\": %s, \"bad_frees\": %d},\n", all_failed ? "true" : "false", g_bad_frees);
}

// ---- the staging helper --------------------------------------------------------------------------------------------
// What one part holds: elements of `size` bytes, `count` of them (size 0: doubles, as many as the part has).  The host
// array of a part is a malloc of exactly count * size bytes, so a copy that is one byte too long in either direction is an
// out-of-bounds access for the sanitizer build.
struct Elem {
  size_t size, count;
};
static unsigned char Pattern(int part, size_t j, int salt) { return (unsigned char)(salt + 31 * (part + 1) + 7 * j); }
template <int K>
static const void* In(Staged<K>& sg, int i, const void* host, Elem e, size_t count, size_t first, bool whole) {
  switch (e.size) {
    case sizeof(unsigned char): return sg.in(i, (const unsigned char*)host, first, count);
    case sizeof(int): return sg.in(i, (const int*)host, first, count);
    case sizeof(TrackStats): return sg.in(i, (const TrackStats*)host);
    default: return whole ? sg.in(i, (const double*)host) : sg.in(i, (const double*)host, first, count);
  }
}
template <int K>
static void* Out(Staged<K>& sg, int i, void* host, Elem e) {
  switch (e.size) {
    case sizeof(unsigned char): return sg.out(i, (unsigned char*)host, e.count);
    case sizeof(int): return sg.out(i, (int*)host, e.count);
    case sizeof(TrackStats): return sg.out(i, (TrackStats*)host);
    case sizeof(EnsembleStats): return sg.out(i, (EnsembleStats*)host);
    default: return sg.out(i, (double*)host);
  }
}
// One round trip through a layout.  ins / outs / halves: bit i set = part i is an input / an output / an input that two host
// arrays share half and half (u_lo, u_hi).  present: bit i set = the caller brings that array.  elems: what the parts hold
// (null: doubles throughout).
template <int K>
static void RoundTrip(const char* name, const Parts<K>& p, unsigned ins, unsigned outs, unsigned halves, unsigned present, const char* tail,
                      const Elem* elems = nullptr) {
  static_assert(sizeof(TrackStats) != sizeof(EnsembleStats), "In() and Out() tell the element by its size");
  ResetCounters();
  bool arrived = true, back = true, absent_null = true, absent_no_room = true;
  int n_in = 0, n_out = 0;
  hipError_t e;
  {
    DevBlock<double> block;
    Must(block.alloc(p.total()));
    unsigned char* const dev = reinterpret_cast<unsigned char*>(block.get());
    Elem el[K];
    unsigned char *host[K] = {}, *host2[K] = {};  // (host2: the upper half of a shared part, an array of its own)
    const void* dev_in[K] = {};
    void* dev_out[K] = {};
    Staged<K> sg(false, block.get(), p, nullptr);
    for (int i = 0; i < K; ++i) {
      el[i] = elems && elems[i].size ? elems[i] : Elem{sizeof(double), p.cnt[i]};
      const bool here = (present >> i) & 1u;
      const size_t bytes = el[i].size * el[i].count;
      if (!here) absent_no_room = absent_no_room && p.cnt[i] == 0;
      if ((ins >> i) & 1u) {
        if ((halves >> i) & 1u) {
          const size_t h = el[i].count / 2, hb = h * el[i].size;
          if (here) {
            host[i] = (unsigned char*)std::malloc(hb), host2[i] = (unsigned char*)std::malloc(hb);
            for (size_t j = 0; j < hb; ++j) host[i][j] = Pattern(i, j, 1), host2[i][j] = Pattern(i, hb + j, 1);
          }
          dev_in[i] = In(sg, i, host[i], el[i], h, 0, false);
          const void* hi = In(sg, i, host2[i], el[i], h, h, false);
          if (here) arrived = arrived && hi == (const unsigned char*)dev_in[i] + hb, n_in += 2;
        } else {
          if (here) {
            host[i] = (unsigned char*)std::malloc(bytes);
            for (size_t j = 0; j < bytes; ++j) host[i][j] = Pattern(i, j, 1);
          }
          dev_in[i] = In(sg, i, host[i], el[i], el[i].count, 0, true);
          n_in += here;
        }
        if (!here) absent_null = absent_null && dev_in[i] == nullptr;
        if (here) arrived = arrived && dev_in[i] == block.get() + p.off[i];
      } else if ((outs >> i) & 1u) {
        if (here) {
          host[i] = (unsigned char*)std::malloc(bytes);
          std::memset(host[i], 0xee, bytes);
        }
        dev_out[i] = Out(sg, i, host[i], el[i]);
        n_out += here;
        if (!here) absent_null = absent_null && dev_out[i] == nullptr;
        if (here) back = back && dev_out[i] == block.get() + p.off[i];
      } else if (!here) {
        absent_null = absent_null && sg.part(i) == nullptr;
      }
    }
    // the "launch": every present input is where its part starts, to the byte; every present output part is written whole
    // (its rounding at the end too: that must not reach the caller)
    for (int i = 0; i < K; ++i) {
      const size_t bytes = el[i].size * el[i].count, at = p.off[i] * sizeof(double), half = bytes / 2;
      if (dev_in[i] && host2[i]) arrived = arrived && !std::memcmp(dev + at, host[i], half) && !std::memcmp(dev + at + half, host2[i], half);
      if (dev_in[i] && !host2[i]) arrived = arrived && !std::memcmp(dev + at, host[i], bytes);
      if (dev_out[i])
        for (size_t j = 0; j < p.cnt[i] * sizeof(double); ++j) dev[at + j] = Pattern(i, j, 2);
    }
    e = sg.finish();
    for (int i = 0; i < K; ++i) {
      if (dev_out[i])
        for (size_t j = 0; j < el[i].size * el[i].count; ++j) back = back && host[i][j] == Pattern(i, j, 2);
      std::free(host[i]);
      std::free(host2[i]);
    }
  }
  std::printf("\"%s\": {\"total\": %zu, \"arrived\": %s, \"back\": %s, \"absent_null\": %s, \"absent_no_room\": %s, \"h2d\": %d, \"want_h2d\": %d, "
              "\"d2h\": %d, \"want_d2h\": %d, \"syncs\": %d, \"error\": %d, \"live\": %zu}%s\n",
              name, p.total(), arrived ? "true" : "false", back ? "true" : "false", absent_null ? "true" : "false",
              absent_no_room ? "true" : "false", g_h2d, n_in, g_d2h, n_out, g_syncs, (int)e, g_live.size(), tail);
}

// a part that cannot hold what a call brings is a programming error; it is treated as a part without room: a null pointer,
// no copy in either direction, no error.  A count that fills the part to the byte goes through.
static void ShortPart() {
  ResetCounters();
  const Parts<2> p{1, 1};  // one double each: room for two ints
  int up[3] = {1, 2, 3}, down[3] = {-1, -1, -1};
  bool nulls, fits;
  hipError_t e;
  {
    DevBlock<double> block;
    Must(block.alloc(p.total()));
    Staged<2> sg(false, block.get(), p, nullptr);
    nulls = sg.in(0, up, 0, 3) == nullptr && sg.in(0, up, 2, 1) == nullptr && sg.out(1, down, 3) == nullptr;
    fits = sg.in(0, up, 0, 2) == reinterpret_cast<int*>(block.get()) && sg.in(0, up + 2, 1, 1) == reinterpret_cast<int*>(block.get()) + 1;
    e = sg.finish();
  }
  std::printf("\"short_part\": {\"nulls\": %s, \"fits\": %s, \"h2d\": %d, \"d2h\": %d, \"untouched\": %s, \"error\": %d},\n", nulls ? "true" : "false",
              fits ? "true" : "false", g_h2d, g_d2h, down[0] == -1 && down[1] == -1 && down[2] == -1 ? "true" : "false", (int)e);
}

// a failed upload copy: the launch is skipped by the caller, nothing comes down, the stream is still waited for, and the
// copy's error is reported before the wait's
static void FailedCopy() {
  ResetCounters();
  const Parts<3> p{4, 4, 4};
  double a[4] = {1, 2, 3, 4}, b[4] = {5, 6, 7, 8}, c[4] = {0, 0, 0, 0};
  hipError_t e;
  bool ok_after;
  {
    DevBlock<double> block;
    Must(block.alloc(p.total()));
    Staged<3> sg(false, block.get(), p, nullptr);
    g_fail_copy_at = 1;
    g_sync_result = hipErrorUnknown;
    sg.in(0, a);
    sg.in(1, b);
    sg.out(2, c);
    ok_after = sg.ok();
    e = sg.finish();
  }
  const int syncs_finish = g_syncs, h2d = g_h2d, d2h = g_d2h;
  // ... and a helper that goes without finish() while its uploads are on the stream waits for them; one without, or a
  // direct one, does not touch the stream
  ResetCounters();
  {
    DevBlock<double> block;
    Must(block.alloc(p.total()));
    Staged<3> sg(false, block.get(), p, nullptr);
    sg.in(0, a);
  }
  const int syncs_dropped = g_syncs;
  ResetCounters();
  const double* same;
  {
    Staged<3> idle(false, nullptr, p, nullptr);
    Staged<3> direct(true, nullptr, p, nullptr);
    same = direct.in(0, a);
    (void)direct.out(2, c);
  }
  std::printf("\"failed_copy\": {\"ok_after\": %s, \"error\": %d, \"copy_error\": %d, \"sync_error\": %d, \"syncs\": %d, \"h2d\": %d, \"d2h\": %d, "
              "\"syncs_dropped\": %d, \"syncs_idle\": %d, \"copies_direct\": %d, \"direct_same\": %s, \"live\": %zu, \"unexpected\": %d}}\n",
              ok_after ? "true" : "false", (int)e, (int)hipErrorInvalidValue, (int)hipErrorUnknown, syncs_finish, h2d, d2h, syncs_dropped,
              g_syncs, g_copies, same == a ? "true" : "false", g_live.size(), g_unexpected);
}

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int n = std::atoi(argv[1]), m = std::atoi(argv[2]);
  const size_t B = (size_t)std::atoi(argv[3]), steps = (size_t)std::atoi(argv[4]), cycles = (size_t)std::atoi(argv[5]),
               shift = (size_t)std::atoi(argv[6]);
  std::printf("{");
  Owners();
  UploadOwner();
  double x = 0;  // (only whether a pointer is null matters to the layouts)
  // dx0 | w | u_lo, u_hi | X_cl | U_cl | stats
  RoundTrip("track_stage", TrackStageParts(n, m, B, steps, true, true, true, true, true, true), 0x07, 0x38, 0x04, 0x3f, ",");
  RoundTrip("track_stage_sparse", TrackStageParts(n, m, B, steps, false, true, false, false, false, true), 0x07, 0x38, 0x04, 0x22, ",");
  // X log | U log | one cycle's X, U | its last state | its disturbance | u_lo, u_hi | statistics: only the bounds go up
  RoundTrip("tracked_run", TrackedRunParts(n, m, B, cycles, shift), 0x40, 0x00, 0x40, 0xff, ",");
  RoundTrip("tracked_run_sparse", TrackedRunParts(n, m, B, cycles, shift), 0x40, 0x00, 0x40, 0xbf, ",");
  // X log | U log | w | dU | clearances
  RoundTrip("plain_run", PlainRunParts(n, m, B, cycles, shift, true, 2 * steps * m, B * cycles), 0x0c, 0x00, 0, 0x1f, ",");
  RoundTrip("plain_run_sparse", PlainRunParts(n, m, B, cycles, shift, false, 0, 0), 0x0c, 0x00, 0, 0x03, ",");
  // Sigma0 | W | Sigma | sx | su | rpos
  CovArgs c{};
  c.steps = (int)steps;
  c.sigma0_per_instance = 1;
  c.w_mode = 3;
  c.Sigma0 = c.W = &x;
  c.Sigma = c.sx = c.su = c.rpos = &x;
  RoundTrip("cov_stage", CovStageParts(n, m, B, c), 0x03, 0x3c, 0, 0x3f, ",");
  c.sigma0_per_instance = 0;
  c.w_mode = 0;
  c.Sigma0 = nullptr;
  c.Sigma = c.su = nullptr;
  RoundTrip("cov_stage_sparse", CovStageParts(n, m, B, c), 0x03, 0x3c, 0, 0x2a, ",");
  // base track | rpos (both required: the sparse case is the shared base track)
  RoundTrip("inflate_stage", InflateStageParts(B, steps, 3, B, steps + 1), 0x03, 0, 0, 0x03, ",");
  RoundTrip("inflate_stage_shared", InflateStageParts(1, steps, 3, B, steps + 1), 0x03, 0, 0, 0x03, ",");
  // X | U | statistics of 7 doubles
  RoundTrip("ms_best_stage", MsBestStageParts(n, m, B, steps, true, true, 7), 0, 0x07, 0, 0x07, ",");
  RoundTrip("ms_best_stage_sparse", MsBestStageParts(n, m, B, steps, false, true, 0), 0, 0x07, 0, 0x02, ",");
  RoundTrip("perturb_stage", PerturbStageParts(m, B, steps), 0x01, 0, 0, 0x01, ",");
  // x0 | w
  RoundTrip("advance_stage", AdvanceStageParts(n, B, true, true), 0x03, 0, 0, 0x03, ",");
  RoundTrip("advance_stage_sparse", AdvanceStageParts(n, B, false, true), 0x03, 0, 0, 0x02, ",");
  RoundTrip("advance_stage_empty", AdvanceStageParts(n, B, false, false), 0x03, 0, 0, 0x00, ",");
  // Xref | Uref
  RoundTrip("reference_stage", ReferenceStageParts(n, m, B * (steps + 1), true), 0x03, 0, 0, 0x03, ",");
  RoundTrip("reference_stage_sparse", ReferenceStageParts(n, m, B * (steps + 1), false), 0x03, 0, 0, 0x01, ",");
  // the layouts that hold ints, bytes and statistics structs: every host array exactly as long as its elements
  const Elem stats{sizeof(TrackStats), B}, summ{sizeof(EnsembleStats), B}, intsB{sizeof(int), B}, bytesB{sizeof(unsigned char), B};
  // tracked | age | u_lo, u_hi | mask | reason | the lookahead's statistics (scratch: nobody's array)
  const Elem trig[6] = {stats, intsB, {}, bytesB, intsB, {}};
  RoundTrip("trigger_stage", TriggerStageParts(m, B, true, true, true, true, true, true), 0x07, 0x18, 0x04, 0x3f, ",", trig);
  RoundTrip("trigger_stage_sparse", TriggerStageParts(m, B, false, false, false, false, false, true), 0x07, 0x18, 0x04, 0x20, ",", trig);
  // Sigma0 | W | u_lo, u_hi | dev_mean | dev_mom2 | alive | viol_count | summary | stats, two samples
  EnsembleArgs en{};
  en.steps = (int)steps, en.S = 2, en.sigma0_per_instance = 1, en.w_mode = 3;
  en.Sigma0 = en.W = en.u_lo = en.u_hi = &x;
  en.dev_mean = en.dev_mom2 = en.dx0 = en.w = &x;
  int ix = 0;
  EnsembleStats ex{};
  TrackStats tx{};
  en.alive = en.viol_count = &ix, en.summary = &ex, en.stats = &tx;
  const Elem intsK{sizeof(int), B * (steps + 1)}, lanes{sizeof(TrackStats), B * 2};
  const Elem ens[9] = {{}, {}, {}, {}, {}, intsK, intsK, summ, lanes};
  RoundTrip("ensemble_stage", EnsembleStageParts(n, m, B, en), 0x007, 0x1f8, 0x004, 0x1ff, ",", ens);
  // Sigma0 | W | dx0 | w
  RoundTrip("noise_stage", NoiseStageParts(n, B, en), 0x3, 0xc, 0, 0xf, ",");
  RoundTrip("gauss_stage", GaussStageParts(m), 0x1, 0, 0, 0x1, ",");
  // K | P | fail, a horizon of `steps` knots
  const Elem lqr[3] = {{}, {}, intsB};
  RoundTrip("lqr_stage", LqrStageParts(n, m, B, steps, true, true, true), 0, 0x7, 0, 0x7, ",", lqr);
  RoundTrip("lqr_stage_sparse", LqrStageParts(n, m, B, steps, true, false, true), 0, 0x7, 0, 0x5, ",", lqr);
  RoundTrip("mask_stage", MaskStageParts(B), 0x1, 0, 0, 0x1, ",", &bytesB);
  ShortPart();
  FailedCopy();
  return 0;
}
