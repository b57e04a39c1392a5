// altro_rng.hpp — the counter-based random numbers of the library (include/altro_ensemble.h states the same contract).
// Plain C++: compiles with g++ for the host-side tests and with hipcc, where every function is __host__ __device__.  No HIP
// include, no state: a draw is a pure function of (seed, counter), so any lane of any kernel can make it, in any order.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers 0xD2511F53,
// 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85, ten rounds.
//
// The draw:  key = (seed & 0xffffffff, seed >> 32),  counter = (k, s, (instance_base + b) mod 2^32, (stream << 16) | j), j < 65536.
// One Philox call gives r0..r3 and the normal pair (z_{2j}, z_{2j+1}):
//     u1 = ((r0 >> 5) 2^26 + (r1 >> 6) + 0.5) 2^-53,   u2 the same from r2, r3        (u1 > 0 always)
//     rad = sqrt(-2 ln u1),   z_{2j} = rad cos(2 pi u2),   z_{2j+1} = rad sin(2 pi u2)      all in fp64
// Streams: kStreamNoise with k = knot is the process noise of that knot, with k = kKnotInitial the initial error;
// kStreamControls with k = knot and s = 0 the multi-start control perturbations.
//
// The factor: noise of covariance W is L xi, L the lower factor of lower_sym(W) (only i >= j is read) by a SEMIDEFINITE
// Cholesky, column by column, with t = 4 n 2^-52 max_i |W_ii|:  d_j = W_jj - sum_{k<j} L_jk^2;  |d_j| <= t: column j of L is
// zero (a state that carries no noise);  d_j < -t: refused;  otherwise L_jj = sqrt(d_j), L_ij = (W_ij - sum_k L_ik L_jk) / L_jj.
// (The rounding error of d_j is below (n + 1) 2^-53 W_jj because sum L_jk^2 <= W_jj: t is that bound with a margin of 8.)
//
// Rounding: L xi is a chain of explicit fma from zero, j = 0 .. i, and its result passes through rng_pin() before anything
// is added to it, so that the product rounds the same in every kernel it is inlined into (the library is built with
// -ffp-contract=fast).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ALTRO_RNG_FN __host__ __device__ inline
#define ALTRO_RNG_UNROLL _Pragma("unroll")
#else
#define ALTRO_RNG_UNROLL
#define ALTRO_RNG_FN inline
#endif

namespace altro_rng {

constexpr uint32_t kStreamNoise = 0, kStreamControls = 1;
constexpr uint32_t kKnotInitial = 0xffffffffu;

// keeps a value out of any contraction across this point
ALTRO_RNG_FN void rng_pin(double& x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#else
  asm volatile("" : "+m"(x));
#endif
}

ALTRO_RNG_FN void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
ALTRO_RNG_UNROLL
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// two words -> a uniform on a grid of 2^-53 (every operation but the + 0.5 is exact; that one rounds to nearest even)
ALTRO_RNG_FN double uniform53(uint32_t hi, uint32_t lo) {
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6) + 0.5) * (1.0 / 9007199254740992.0);
}

// the words of draw (k, s, instance, stream, j)
ALTRO_RNG_FN void draw_words(uint64_t seed, uint32_t k, uint32_t s, uint64_t instance, uint32_t stream, uint32_t j, uint32_t r[4]) {
  const uint32_t ctr[4] = {k, s, (uint32_t)instance, (stream << 16) | j}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  philox4x32_10(ctr, key, r);
}

// the normal pair (z_{2j}, z_{2j+1}) of that draw
ALTRO_RNG_FN void normal_pair(uint64_t seed, uint32_t k, uint32_t s, uint64_t instance, uint32_t stream, uint32_t j, double* z0,
                              double* z1) {
  uint32_t r[4];
  draw_words(seed, k, s, instance, stream, j, r);
  const double u1 = uniform53(r[0], r[1]), u2 = uniform53(r[2], r[3]);
  double arg = 6.283185307179586476925 * u2, ln = log(u1);
  rng_pin(arg);
  rng_pin(ln);
  const double rad = sqrt(-2.0 * ln);
  double sn, cs;
#if defined(__HIP_DEVICE_COMPILE__)
  sincos(arg, &sn, &cs);
#else
  sn = sin(arg), cs = cos(arg);
#endif
  rng_pin(sn);
  rng_pin(cs);
  *z0 = rad * cs;
  *z1 = rad * sn;
}

// xi[0 .. n): the first n normals of draws j = 0 .. ceil(n / 2) - 1
template <int n>
ALTRO_RNG_FN void normals(uint64_t seed, uint32_t k, uint32_t s, uint64_t instance, uint32_t stream, double* xi) {
ALTRO_RNG_UNROLL
  for (int j = 0; j < (n + 1) / 2; ++j) {
    double a, b;
    normal_pair(seed, k, s, instance, stream, (uint32_t)j, &a, &b);
    xi[2 * j] = a;
    if (2 * j + 1 < n) xi[2 * j + 1] = b;
  }
}

// out = L xi, L row-major [n][n] of which only i >= j is read; every out[i] is pinned
template <int n>
ALTRO_RNG_FN void mul_lower(const double* L, const double* xi, double* out) {
ALTRO_RNG_UNROLL
  for (int i = 0; i < n; ++i) {
    double acc = 0.0;
ALTRO_RNG_UNROLL
    for (int j = 0; j <= i; ++j) acc = fma(L[i * n + j], xi[j], acc);
    rng_pin(acc);
    out[i] = acc;
  }
}

// out[0 .. n) = L xi with xi the stream-0 normals of (k, s, instance): the noise of one (instance, sample, knot)
template <int n>
ALTRO_RNG_FN void noise(uint64_t seed, uint32_t k, uint32_t s, uint64_t instance, const double* L, double* out) {
  double xi[n];
  normals<n>(seed, k, s, instance, kStreamNoise, xi);
  mul_lower<n>(L, xi, out);
}

// The semidefinite Cholesky factor described above.  W, L row-major [n][n]; all of L is written (zeros above the diagonal).
// Returns 0, or 1 where W is refused (not positive semidefinite, or not finite); L is then unspecified.
ALTRO_RNG_FN int psd_factor(const double* W, int n, double* L) {
  double top = 0.0;
  for (int i = 0; i < n; ++i) top = fabs(W[i * n + i]) > top ? fabs(W[i * n + i]) : top;
  const double t = 4.0 * (double)n * 2.220446049250313e-16 * top;
  if (!(t < (double)INFINITY)) return 1;  // (a NaN fails too)
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    for (int k = 0; k < j; ++k) {
      double p = L[j * n + k] * L[j * n + k];
      rng_pin(p);
      s += p;
    }
    const double d = W[j * n + j] - s;
    if (!(d >= -t)) return 1;
    const bool zero = fabs(d) <= t;
    const double root = zero ? 0.0 : sqrt(d);
    for (int i = 0; i < j; ++i) L[i * n + j] = 0.0;
    L[j * n + j] = root;
    for (int i = j + 1; i < n; ++i) {
      double a = 0.0;
      for (int k = 0; k < j; ++k) {
        double p = L[i * n + k] * L[j * n + k];
        rng_pin(p);
        a += p;
      }
      L[i * n + j] = zero ? 0.0 : (W[i * n + j] - a) / root;
    }
  }
  return 0;
}

}  // namespace altro_rng
