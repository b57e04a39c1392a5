// k_lqr_recur and k_cov_recur driven on their own (tests/test_recur_kernels_gpu.py): the two recursions are templates over
// (n, m) alone and take plain pointers, so the lane groups no model of the suite reaches -- G = 32, n = G, m = 8 -- are
// instantiated here without an engine.  A shared library with two C entry points; each takes host arrays in the kernels' own
// layouts, copies them to the device (the outputs too: what the caller put there is what a lane that stores nothing leaves),
// launches ONE kernel with the grid the engine uses, and copies the outputs back.  Returns the HIP status, or -1 for a shape
// that is not in the list.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "altro_kernels.hpp"

using namespace altro_hip;

// (n, m): n = G = 8; n = G = 16; G = 32 with 15 dead lanes; G = 32, m = 3; both documented maxima; m = 8 > n; G = 2, m > n;
// and one shape a plug-in reaches too
#define RECUR_SHAPES(X) X(8, 1) X(16, 4) X(17, 2) X(24, 3) X(32, 8) X(4, 8) X(2, 6) X(13, 2)

namespace {

// device memory for the length of one call
struct Dev {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t status = hipSuccess;
  Dev(const void* src, size_t count, size_t elem) : bytes(count * elem) {
    if (!src || !bytes) return;
    status = hipMalloc(&p, bytes);
    if (status == hipSuccess) status = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
  }
  ~Dev() {
    if (p) (void)hipFree(p);
  }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  hipError_t back(void* dst) const { return p ? hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

#define RECUR_TRY(expr)                \
  do {                                 \
    const hipError_t e_ = (expr);      \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

hipError_t finish() {
  const hipError_t launched = hipGetLastError();
  const hipError_t done = hipDeviceSynchronize();
  return launched != hipSuccess ? launched : done;
}

template <int n, int m>
int run_lqr(const double* AB, const double* Wt, double* Kt, double* Pt, int* fail, int B, unsigned Bp, int N) {
  const size_t bp = Bp;
  Dev dAB(AB, (size_t)N * n * (n + m) * bp, sizeof(double)), dW(Wt, (size_t)(2 * n * n + m * m), sizeof(double));
  Dev dK(Kt, (size_t)N * m * n * bp, sizeof(double)), dP(Pt, (size_t)(N + 1) * n * n * bp, sizeof(double)), dF(fail, bp, sizeof(int));
  for (const Dev* d : {&dAB, &dW, &dK, &dP, &dF}) RECUR_TRY(d->status);
  constexpr int per_block = kBlock / cov_group(n);
  hipLaunchKernelGGL((k_lqr_recur<n, m>), dim3((B + per_block - 1) / per_block), dim3(kBlock), 0, 0, dAB.as<const double>(),
                     dW.as<const double>(), dK.as<double>(), dP.as<double>(), dF.as<int>(), B, Bp, N);
  RECUR_TRY(finish());
  RECUR_TRY(dK.back(Kt));
  RECUR_TRY(dP.back(Pt));
  RECUR_TRY(dF.back(fail));
  return 0;
}

// `rows` >= B instances are allocated in every instance-major array (the rows behind B are the caller's canaries)
template <int n, int m>
int run_cov(const double* F, const double* Kw, const double* Sigma0, int sigma0_per_instance, const double* W, int w_mode, double* Sigma,
            double* sx, double* su, double* rpos, int B, unsigned Bp, int steps, int rows) {
  const size_t bp = Bp, r = (size_t)rows, nn = (size_t)n * n;
  Dev dF(F, (size_t)steps * nn * bp, sizeof(double)), dKw(Kw, (size_t)steps * m * n * bp, sizeof(double));
  Dev dS0(Sigma0, (sigma0_per_instance ? r : 1) * nn, sizeof(double));
  Dev dWn(W, ((w_mode & 1) ? r : 1) * ((w_mode & 2) ? (size_t)steps : 1) * nn, sizeof(double));
  Dev dSig(Sigma, r * (steps + 1) * nn, sizeof(double)), dsx(sx, r * (steps + 1) * n, sizeof(double));
  Dev dsu(su, r * steps * m, sizeof(double)), drp(rpos, r * (steps + 1), sizeof(double));
  for (const Dev* d : {&dF, &dKw, &dS0, &dWn, &dSig, &dsx, &dsu, &drp}) RECUR_TRY(d->status);
  CovArgs g;
  g.steps = steps, g.sigma0_per_instance = sigma0_per_instance, g.w_mode = w_mode;
  g.Sigma0 = dS0.as<const double>(), g.W = dWn.as<const double>();
  g.Sigma = dSig.as<double>(), g.sx = dsx.as<double>(), g.su = dsu.as<double>(), g.rpos = drp.as<double>();
  constexpr int per_block = kBlock / cov_group(n);
  hipLaunchKernelGGL((k_cov_recur<n, m>), dim3((B + per_block - 1) / per_block), dim3(kBlock), 0, 0, g, dF.as<const double>(),
                     dKw.as<const double>(), B, Bp);
  RECUR_TRY(finish());
  RECUR_TRY(dSig.back(Sigma));
  RECUR_TRY(dsx.back(sx));
  RECUR_TRY(dsu.back(su));
  RECUR_TRY(drp.back(rpos));
  return 0;
}

}  // namespace

// AB [N][n (n + m)][Bp], Wt = Q | R | Qf (full symmetric), Kt [N][m n][Bp], Pt [N + 1][n n][Bp], fail [Bp]
extern "C" int recur_lqr(int n, int m, const double* AB, const double* Wt, double* Kt, double* Pt, int* fail, int B, int Bp, int N) {
  if (B < 1 || Bp < B || N < 1 || !AB || !Wt || !Kt || !Pt || !fail) return -1;
#define X(n_, m_) \
  if (n == n_ && m == m_) return run_lqr<n_, m_>(AB, Wt, Kt, Pt, fail, B, (unsigned)Bp, N);
  RECUR_SHAPES(X)
#undef X
  return -1;
}

// F [steps][n n][Bp] row-major, Kw [steps][m n][Bp]; Sigma0, W as CovArgs says (either may be null) with `rows` instances
// where they are per instance; Sigma, sx, su, rpos instance-major with `rows` instances (any may be null, not all)
extern "C" int recur_cov(int n, int m, const double* F, const double* Kw, const double* Sigma0, int sigma0_per_instance, const double* W,
                         int w_mode, double* Sigma, double* sx, double* su, double* rpos, int B, int Bp, int steps, int rows) {
  if (B < 1 || Bp < B || rows < B || steps < 1 || (w_mode & ~3) || !F || !Kw || (!Sigma && !sx && !su && !rpos)) return -1;
#define X(n_, m_) \
  if (n == n_ && m == m_) return run_cov<n_, m_>(F, Kw, Sigma0, sigma0_per_instance, W, w_mode, Sigma, sx, su, rpos, B, (unsigned)Bp, steps, rows);
  RECUR_SHAPES(X)
#undef X
  return -1;
}
