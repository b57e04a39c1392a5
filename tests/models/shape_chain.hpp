// A nonlinear chain of any shape as a CONTINUOUS user model: n = SHAPE_N states, m = SHAPE_M controls (defines put in front
// of the source by the tests and by oracle/Makefile).  xdot_i = x_{i+1} - 0.1 sin(x_i) (the last state has no successor);
// control j adds (1 + 0.1 j) u_j to state n - 1 - (j mod n).  The RK4 Jacobians are dense for every shape, m > n included,
// so every tile of every backward kernel carries data.  One text serves the whole matrix of tests/test_model_shapes_gpu.py
// (n, m) -- the shapes that pick each branch of the backward dispatch -- and is compiled for the host into
// oracle/_build/liboracle_shape_<n>_<m>.so as well.
#ifndef SHAPE_N
#define SHAPE_N 3
#endif
#ifndef SHAPE_M
#define SHAPE_M 2
#endif
struct UserModel {
  static constexpr int n = SHAPE_N, m = SHAPE_M;
  template <class T>
  ALTRO_MODEL_FN static void f(const T* x, const T* u, T* xd) {
    for (int i = 0; i < n; ++i) xd[i] = (i + 1 < n ? x[i + 1] : T(0)) - T(0.1) * sin(x[i]);
    for (int j = 0; j < m; ++j) xd[n - 1 - j % n] += (T(1) + T(0.1) * T(j)) * u[j];
  }
  template <class T>
  ALTRO_MODEL_FN static void jac(const T* x, const T*, T* J) {  // n x (n + m), column-major
    for (int i = 0; i < n * (n + m); ++i) J[i] = T(0);
    for (int i = 0; i < n; ++i) {
      J[i + i * n] = -T(0.1) * cos(x[i]);
      if (i + 1 < n) J[i + (i + 1) * n] = T(1);
    }
    for (int j = 0; j < m; ++j) J[(n - 1 - j % n) + (n + j) * n] = T(1) + T(0.1) * T(j);
  }
};
