// Host-only driver of tests/test_ensemble_abi.py: altro_rng.hpp and the ensemble's helpers of altro_common.hpp, built with
// plain g++ (no HIP) under the address and undefined-behaviour sanitizers and run directly.  Prints one JSON object; doubles
// go out as C99 hex floats (exact).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "altro_common.hpp"
#include "altro_rng.hpp"

using namespace altro_hip;

static void hexlist(const double* v, int count) {
  printf("[");
  for (int i = 0; i < count; ++i) printf("%s\"%a\"", i ? ", " : "", v[i]);
  printf("]");
}
template <int K>
static void parts(const char* name, const Parts<K>& p, bool last = false) {
  printf("\"%s\": {\"cnt\": [", name);
  for (int i = 0; i < K; ++i) printf("%s%zu", i ? ", " : "", p.cnt[i]);
  printf("], \"off\": [");
  for (int i = 0; i <= K; ++i) printf("%s%zu", i ? ", " : "", p.off[i]);
  printf("], \"total\": %zu}%s\n", p.total(), last ? "" : ",");
}

int main() {
  printf("{\n\"philox\": [");
  const uint32_t kat[3][6] = {{0, 0, 0, 0, 0, 0},
                              {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                              {0x243f6a88u, 0x85a308d3u, 0x13198a2e, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
  for (int i = 0; i < 3; ++i) {
    uint32_t out[4];
    altro_rng::philox4x32_10(kat[i], kat[i] + 4, out);
    printf("%s[%u, %u, %u, %u]", i ? ", " : "", out[0], out[1], out[2], out[3]);
  }
  // draws: (seed, k, s, instance, stream, j)
  const unsigned long long draws[][6] = {{0, 0, 0, 0, 0, 0},
                                         {20261020ull, 0xffffffffull, 5, 1, 0, 0},
                                         {20261020ull, 7, 329, 3, 0, 1},
                                         {0x123456789abcdef0ull, 11, 0, 0x1ffffffffull, 1, 65535},
                                         {0xffffffffffffffffull, 99, 4095, 0xfffffffeull, 1, 2},
                                         {42, 3, 64, 2, 0, 5}};
  printf("],\n\"draws\": [");
  for (size_t i = 0; i < sizeof(draws) / sizeof(draws[0]); ++i) {
    const unsigned long long* d = draws[i];
    uint32_t r[4];
    altro_rng::draw_words(d[0], (uint32_t)d[1], (uint32_t)d[2], d[3], (uint32_t)d[4], (uint32_t)d[5], r);
    double z[2], u[2] = {altro_rng::uniform53(r[0], r[1]), altro_rng::uniform53(r[2], r[3])};
    altro_rng::normal_pair(d[0], (uint32_t)d[1], (uint32_t)d[2], d[3], (uint32_t)d[4], (uint32_t)d[5], &z[0], &z[1]);
    printf("%s\n {\"in\": [%llu, %llu, %llu, %llu, %llu, %llu], \"words\": [%u, %u, %u, %u], \"u\": ", i ? "," : "", d[0], d[1], d[2], d[3],
           d[4], d[5], r[0], r[1], r[2], r[3]);
    hexlist(u, 2);
    printf(", \"z\": ");
    hexlist(z, 2);
    printf("}");
  }
  // factors: exactly representable matrices (n, row-major), a singular and an indefinite one among them; garbage above the
  // diagonal of the second must not matter
  struct Case { int n; std::vector<double> W; };
  const std::vector<Case> cases = {
      {1, {4.0}},
      {2, {4.0, 777.0, 2.0, 10.0}},                              // L = [[2, 0], [1, 3]]
      {3, {1.0, 0, 0, 2.0, 4.0, 0, 3.0, 6.0, 9.0}},              // rank one: columns 1, 2 are zero
      {3, {0.25, 0, 0, 0.0, 0.0, 0, 0.5, 0.0, 17.0}},            // a state without noise in the middle
      {3, {4.0, 0, 0, 2.0, 1.0, 0, 0.0, 0.0, 0.0}},              // singular: d_1 = 0 exactly
      {2, {1.0, 0, 2.0, 1.0}},                                   // indefinite
      {2, {-1.0, 0, 0.0, 1.0}},                                  // a negative diagonal
      {3, {0, 0, 0, 0, 0, 0, 0, 0, 0}},                          // zero
      {4, {16.0, 0, 0, 0, 4.0, 5.0, 0, 0, 8.0, 4.0, 9.0, 0, 12.0, 7.0, 12.0, 26.0}}};  // L = [[4],[1,2],[2,1,2],[3,2,2,3]]
  printf("],\n\"factors\": [");
  for (size_t i = 0; i < cases.size(); ++i) {
    const int n = cases[i].n;
    std::vector<double> L((size_t)n * n, -1.0);
    const int refused = altro_rng::psd_factor(cases[i].W.data(), n, L.data());
    printf("%s\n {\"n\": %d, \"refused\": %d, \"W\": ", i ? "," : "", n, refused);
    hexlist(cases[i].W.data(), n * n);
    printf(", \"L\": ");
    hexlist(L.data(), n * n);
    printf("}");
  }
  // L xi of the 4 x 4 factor above with the normals of one draw
  {
    std::vector<double> L(16);
    altro_rng::psd_factor(cases.back().W.data(), 4, L.data());
    double out[4], xi[4];
    altro_rng::normals<4>(20261020ull, 3, 17, 2, altro_rng::kStreamNoise, xi);
    altro_rng::noise<4>(20261020ull, 3, 17, 2, L.data(), out);
    printf("],\n\"noise\": {\"in\": [20261020, 3, 17, 2], \"xi\": ");
    hexlist(xi, 4);
    printf(", \"out\": ");
    hexlist(out, 4);
    printf("},\n");
  }
  printf("\"slabs\": [");
  const long long bs[][2] = {{1, 1}, {1, 64}, {1, 65}, {2, 323}, {3, 70}, {2, 4096}, {64, 64}, {64, 1024}, {100, 1100}, {1023, 130},
                             {1024, 100000}, {4096, 1024}, {5, 1025}, {1, 1088}, {300, 64 * 17}};
  for (size_t i = 0; i < sizeof(bs) / sizeof(bs[0]); ++i)
    printf("%s[%lld, %lld, %d, %d]", i ? ", " : "", bs[i][0], bs[i][1], EnsembleSlabs(bs[i][0], bs[i][1]), EnsembleChunksPerSlab(bs[i][0], bs[i][1]));
  printf("],\n\"values\": [%d, %d, %d],\n\"stats_doubles\": %zu,\n", EnsembleValues(3), EnsembleValues(6), EnsembleValues(12),
         sizeof(EnsembleStats) / sizeof(double));
  // the staged blocks for n = 3, m = 2, B = 5, steps = 2, S = 7
  double dummy = 0;
  int idummy = 0;
  EnsembleStats es{};
  TrackStats ts{};
  EnsembleArgs a{};
  a.steps = 2, a.S = 7, a.sigma0_per_instance = 1, a.w_mode = 3;
  a.Sigma0 = a.W = a.u_lo = a.u_hi = &dummy;
  a.dev_mean = a.dev_mom2 = a.dx0 = a.w = &dummy;
  a.alive = a.viol_count = &idummy;
  a.summary = &es, a.stats = &ts;
  parts("ensemble_stage", EnsembleStageParts(3, 2, 5, a));
  parts("noise_stage", NoiseStageParts(3, 5, a));
  EnsembleArgs s{};
  s.steps = 2, s.S = 7, s.w_mode = 2;
  s.W = &dummy, s.alive = &idummy, s.stats = &ts, s.w = &dummy;
  parts("ensemble_stage_sparse", EnsembleStageParts(3, 2, 5, s));
  parts("noise_stage_sparse", NoiseStageParts(3, 5, s));
  parts("gauss_stage", GaussStageParts(2), true);
  printf("}\n");
  return 0;
}
