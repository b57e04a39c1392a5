// fused_lds_driver.cpp -- prints the LDS layout of the persistent tail kernel (FusedLds, altro_common.hpp: host code, no HIP)
// for a grid of shapes, beside the byte count Engine::PlanForwardLds computed before the struct existed, as one JSON list.
// tests/test_fused_lds.py holds the expectations.
#include <cstddef>
#include <cstdio>

#include "altro_common.hpp"

using namespace altro_hip;

// Rec<T, n, m> (altro_device.hpp needs HIP): records are padded to 16 bytes
template <class T>
struct RecN {
  int V, nP, mP, KP;
  RecN(int n, int m) : V(16 / (int)sizeof(T)), nP(pad(n)), mP(pad(m)), KP(pad(m * n + m)) {}
  int pad(int e) const { return (e + V - 1) / V * V; }
};

// Engine::PlanForwardLds before FusedLds: copied literally (PadV, PaddedBlock and kFwdSlots spelled out beside it)
template <class T>
static size_t ParentFormula(const RecN<T>& R, int nm, int N_, size_t rows, size_t nslots, size_t npool) {
  const size_t kFwdSlots = 4;
  auto PadV = [&](size_t e) { return (e + R.V - 1) / R.V * R.V; };
  auto PaddedBlock = [](size_t bytes) { return bytes + (size_t)(((160 - (long long)bytes % 256) + 256) % 256); };
  const size_t per_inst = PaddedBlock(((size_t)(N_ + 1) * R.nP + (size_t)N_ * R.mP + (size_t)N_ * R.KP +
                                       2 * PadV(rows) + PadV((size_t)nslots)) * sizeof(T));
  const size_t shared_bytes = (PadV((size_t)npool) + kFwdSlots * (size_t)nm * kBlock) * sizeof(T) + 2 * kBlock * sizeof(int) +
                              kBlock * sizeof(double);
  return (shared_bytes + (2 * kSyncFused - kFwdSlots) * (size_t)nm * kBlock * sizeof(T) + per_inst + 15) / 16 * 16 +
         (4 + 2 + kBlock + 2 + 16) * sizeof(double) +
         (size_t)(N_ + 1) * kLineSearchLanes * nm * sizeof(T) +  // + the candidates of one instance
         ((size_t)N_ * R.KP + kBlock) * sizeof(T) + 48 * sizeof(double) +  // + the speculative pass (gains, hand-over), step-length table, sequence words
         ((size_t)N_ + 4) * sizeof(T) +                                    // + the knot costs of the expansion step
         PadV(rows) * sizeof(T);                                           // + the constraint values of the expansions computed ahead
}

static bool g_first = true;
template <class T>
static void Case(const char* type, int n, int m, int N, int rows, int nslots, int npool) {
  const RecN<T> R(n, m);
  const int nm = n + m, e = (int)sizeof(T);
  const FwdLds<T> L{(N + 1) * R.nP, N * R.mP, N * R.KP, rows, nslots, R.V};
  const FusedLds<T> F{L, N, nm, npool};
  // name, offset, bytes the kernel uses there, alignment it relies on (16: 16-byte LDS operations; 8: doubles, and the
  // sequence words; 4: ints and single elements)
  struct Sub { const char* name; int off; long long size; int align; };
  const Sub subs[] = {
      {"block", 0, (long long)L.total() * e, 16},
      {"pool", F.oPool(), (long long)L.padv(npool) * e, 16},
      {"xch", F.oXch(), 2LL * kSyncFused * nm * kBlock * e, 16},
      {"flags", F.oFlags(), 2LL * kBlock * (long long)sizeof(int), 4},
      {"grad", F.oGrad(), (long long)kBlock * 8, 8},
      {"fh", F.oFh(), (long long)kFhWords * 8, 8},
      {"junk", F.oJunk(), (long long)kBlock * 8, 8},
      {"active", F.oActive(), (long long)sizeof(int), 4},
      {"ff", F.oFf(), (long long)kFfWords * 8, 8},
      {"cand", F.oCand(), (long long)(N + 1) * kLineSearchLanes * nm * e, 16},
      {"kd2", F.oKD2(), ((long long)N * R.KP + kBlock) * e, 16},
      {"fh2", F.oFh2(), (long long)kFh2Words * 8, 8},
      {"alpha", F.oAlpha(), (long long)kLineSearchLanes * e, e},
      {"sync", F.oSync(), (long long)kSyWords * (long long)sizeof(int), 8},
      {"cost", F.oCost(), (long long)(N + 1) * e, e},
      {"cval_ahead", F.oCvalAhead(), (long long)rows * e, e},
  };
  printf("%s{\"type\": \"%s\", \"n\": %d, \"m\": %d, \"N\": %d, \"rows\": %d, \"nslots\": %d, \"npool\": %d, \"bytes\": %zu, \"parent\": %zu, "
         "\"used\": %d, \"subs\": [", g_first ? "" : ",\n", type, n, m, N, rows, nslots, npool, F.bytes(),
         ParentFormula<T>(R, nm, N, (size_t)rows, (size_t)nslots, (size_t)npool), F.used());
  g_first = false;
  for (size_t i = 0; i < sizeof(subs) / sizeof(subs[0]); ++i)
    printf("%s[\"%s\", %d, %lld, %d]", i ? ", " : "", subs[i].name, subs[i].off, subs[i].size, subs[i].align);
  printf("]}");
}

int main() {
  // the built-in models (unicycle, triple integrator, quadrotor) and the shapes of tests/models/shape_chain.hpp
  const int shapes[][2] = {{3, 2}, {6, 2}, {12, 4}, {1, 1}, {2, 2}, {1, 2}, {3, 1}, {5, 3}, {7, 3}, {9, 1}, {13, 2}, {6, 5}, {3, 5}};
  printf("[");
  for (const auto& s : shapes)
    for (int N : {1, 2, 100, 126, 127}) {
      Case<double>("double", s[0], s[1], N, 7, 1, 5);
      Case<float>("float", s[0], s[1], N, 7, 1, 5);
    }
  // (3, 2): every combination of the edge cases
  for (int N : {1, 2, 100, 126, 127})
    for (int rows : {0, 1, 7, 303})
      for (int nslots : {0, 1, 5})
        for (int npool : {0, 1, 5}) {
          Case<double>("double", 3, 2, N, rows, nslots, npool);
          Case<float>("float", 3, 2, N, rows, nslots, npool);
        }
  printf("]\n");
  return 0;
}
