// altro_common.hpp — host-side types shared by the C-ABI front end (altro_capi.cpp) and the
// templated device engines (altro_engine.hpp).  No HIP types in here.
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/altro_hip.h"

namespace altro_hip {

// ---- compile-time limits of the closed registry ---------------------------------------------------
constexpr int kMaxConPerKnot = 4;  // constraints attached to one knot point
constexpr int kMaxClasses = 8;     // distinct (cost, constraint list) combinations over the knots
constexpr int kMaxCostGroups = 8;
#ifndef ALTRO_LS_LANES
#define ALTRO_LS_LANES 20  // (experimental builds: 10 -- six instances per wavefront, only with line_search_max_iterations <= 10)
#endif
constexpr int kLineSearchLanes = ALTRO_LS_LANES;  // speculative line-search trials evaluated side by side
constexpr int kHistFields = 8;
constexpr int kMaxRuns = 16;  // maximal runs of consecutive knots sharing one class
constexpr int kMaxFastCircles = 3;  // circles of one constraint that the specialised cost-wave layouts keep in registers
constexpr int kMaxSharedPool = 128;  // shared parameters that travel to the forward kernel as kernel arguments
// CostGroupDesc::q_pi / r_pi / c_pi of a tracking group (altro_set_lqr_tracking_cost): the term is neither shared (0) nor per
// instance (1) but PER KNOT -- element q_off / r_off / c_off + i of the reference-term record of (knot, instance)
constexpr int kParPerKnot = 2;
// doubles of one reference-term record: q[n] | r[m] | c, rounded up to a pair (16-byte records)
constexpr int RefTermRecord(int n, int m) { return (n + m + 1 + 1) & ~1; }
// doubles of one point of the reference path: x[n] | u[m], rounded up to a pair
constexpr int RefPathRecord(int n, int m) { return (n + m + 1) & ~1; }
// ConDesc::per_instance of a KNOT constraint (include/altro_knot_params.h: altro_add_knot_constraint): its parameters are
// neither shared (0) nor per instance (1) but PER KNOT -- elements param_off + i of the knot-parameter record of (knot,
// instance), DevArrays::kpar, which k_knot_params copies from the constraint's parameter track
constexpr int kParPerKnotCon = 3;
constexpr int kMaxKnotCons = 16;  // knot constraints of one handle (they travel to k_knot_params as one kernel argument)

// ---- dtype-independent problem specification (what the altro::problem::Problem setters record) ---
struct CostSpec {
  int k_begin, k_end;
  std::vector<double> Q, R, xref, uref;
  int per_instance;  // bit0 xref, bit1 uref (user cost: params are per instance)
  int user = 0;      // 0: LQR cost; 1 + t: the t-th user cost type of the model's source (ALTRO_USER_COSTS) instead
  std::vector<double> params;  // user cost: [nparams] or [B][nparams]
  int tracking = 0;  // altro_set_lqr_tracking_cost: xref / uref of knot k are the handle's reference at k (xref, uref stay empty)
};
struct ConSpec {
  int kind, k_begin, k_end, nparams, per_instance;
  std::vector<double> params;
  int user_type = 0;  // ALTRO_CON_USER: index of the constraint type in the model's source (ALTRO_USER_CONSTRAINTS)
  // altro_add_knot_constraint: the parameters of knot k are row min(offset + k, rows - 1) of the constraint's track (params
  // stays empty).  A track set before the device state exists waits here: track[rows][nparams] or [B][rows][nparams].
  int knot = 0;
  std::vector<double> track;
  int track_rows = 0, track_per_instance = 0;
};
struct ProblemSpec {
  altro_desc desc{};
  int model_kind = 0;
  int dof = 0;
  float hstep = 0.0f;
  // Trajectory::SetStep(k, h) / SetTime(k, t) (trajectory.hpp:119-120): per-knot steps hk[N] and times tk[N + 1]; empty =
  // the uniform step above with t_k = float(k) * h, t_N = h * N (trajectory.hpp:122-130)
  std::vector<float> hk, tk;
  // Problem::SetDynamics(model, k) with different models along the horizon (problem.hpp:155-166): knot k uses model
  // knot_model[k] of the user source's ALTRO_USER_MODELS list; empty = model 0 everywhere
  std::vector<int> knot_model;
  std::vector<CostSpec> costs;
  std::vector<ConSpec> cons;
  std::vector<double> x0;  // [n] or [B][n]
  int x0_per_instance = 0;
  std::vector<double> X, U;  // host layout, instance-major
  // after the upload a new trajectory goes from the caller's buffers straight to the device: views for that one call
  const double* X_view = nullptr;
  const double* U_view = nullptr;
  bool has_X = false, has_U = false;
  int traj_per_instance = 0;
  double penalty = -1.0;  // SetPenalty issued before the device state exists
  double phi = -1.0;
  // altro_set_reference before the device state exists: the path Xref[rows][n], Uref[rows][m] ([B][rows][.] per instance;
  // ref_U empty = zeros) and the window offset; the engine owns both after the upload
  std::vector<double> ref_X, ref_U;
  int ref_rows = 0, ref_per_instance = 0, ref_offset = 0;
  int track_offset = 0;  // altro_set_track_offset before the device state exists: the window of every constraint track
};

// ---- receding-horizon advance (include/altro_mpc.h) --------------------------------------------------
// Where every dual / penalty row comes from when the horizon moves forward by `shift` knots: src[r] in [0, rows), or -1 for a
// row that starts afresh.  PER CONSTRAINT, not per knot class: constraint j (the j-th altro_add_constraint call; knots
// [kb[j], ke[j]), p[j] rows, eq[j] != 0 for an equality) keeps its rows wherever it is attached to both the knot and the knot
// the shift reads (min(k + shift, N - 1)).  Rows of a knot: equalities first, then inequalities, each in insertion order
// (al_cost.hpp:267-272).  The terminal knot's rows map to themselves.
inline std::vector<int> MpcRowMap(int N, int shift, const std::vector<int>& kb, const std::vector<int>& ke, const std::vector<int>& p,
                                  const std::vector<int>& eq) {
  const int J = (int)kb.size();
  std::vector<std::vector<int>> row_of(N + 1, std::vector<int>(J, -1));  // first row of constraint j at knot k
  int rows = 0;
  for (int k = 0; k <= N; ++k)
    for (int pass = 0; pass < 2; ++pass)
      for (int j = 0; j < J; ++j)
        if (k >= kb[j] && k < ke[j] && (eq[j] != 0) == (pass == 0)) {
          row_of[k][j] = rows;
          rows += p[j];
        }
  std::vector<int> src(rows, -1);
  for (int k = 0; k <= N; ++k) {
    const int ks = k < N ? std::min(k + shift, N - 1) : N;
    for (int j = 0; j < J; ++j)
      if (row_of[k][j] >= 0 && row_of[ks][j] >= 0)
        for (int i = 0; i < p[j]; ++i) src[row_of[k][j] + i] = row_of[ks][j] + i;
  }
  return src;
}

// ---- closed-loop tracking (include/altro_mpc.h: altro_mpc_track) --------------------------------------
// altro_track_stats as the kernel writes it (the C-ABI translation unit asserts that the two layouts agree; a user-model
// plugin compiles this header without the C header)
struct TrackStats {
  int status, steps_done;
  double cost, violation, max_dx, max_du;
};
// One call of Engine::MpcTrack / one launch of k_mpc_track.  Every pointer may be null; host or device memory as the call says.
struct TrackArgs {
  int steps, S;
  const double *dx0, *w;      // [B][S][n], [B][S][steps][n]
  const double *u_lo, *u_hi;  // [m] each, both or neither
  double *X_cl, *U_cl;        // [B][S][steps + 1][n], [B][S][steps][m]
  double* x_end;              // [B][S][n]: row `steps` of X_cl on its own (what altro_mpc_run_tracked advances from)
  TrackStats* stats;          // [B][S]
  int check_bounds;           // options.check_forwardpass_bounds, state_max, control_max
  double state_max, control_max;
};

// ---- event-triggered re-planning (include/altro_trigger.h) ------------------------------------------------
// altro_trigger_rule as the kernel reads it (the C-ABI translation unit asserts that the two layouts agree) and the bits of
// a reason (ALTRO_TRIGGER_*)
struct TriggerRule {
  int max_age;
  double dx_tol, viol_tol;
  int on_unsolved, lookahead;
  double ahead_tol;
};
enum TriggerBit {
  kTrigFirst = 1,
  kTrigAge = 2,
  kTrigDeviation = 4,
  kTrigViolation = 8,
  kTrigLimit = 16,
  kTrigUnsolved = 32,
  kTrigAhead = 64
};
// One call of Engine::Trigger / one launch of k_mpc_trigger.  Every pointer may be null; host or device memory as the call says.
struct TriggerArgs {
  TriggerRule rule;
  const TrackStats* tracked;  // [B]
  const int* age;             // [B]
  const double *u_lo, *u_hi;  // [m] each, both or neither: the lookahead's
  unsigned char* mask;        // [B]
  int* reason;                // [B]
  TrackArgs track;            // the options of the lookahead's tracking call (check_bounds, state_max, control_max)
};

// One call of Engine::CovPropagate / one launch of k_cov_recur (include/altro_covariance.h).  Every pointer may be null; host
// or device memory as the call says.
struct CovArgs {
  int steps, sigma0_per_instance, w_mode;  // w_mode: bit 0 per instance, bit 1 per knot
  const double *Sigma0, *W;                // [n][n] | [B][n][n];  [n][n] | [B][n][n] | [steps][n][n] | [B][steps][n][n]
  double *Sigma, *sx, *su, *rpos;          // [B][steps + 1][n][n], [B][steps + 1][n], [B][steps][m], [B][steps + 1]
};

// ---- time-varying LQR tracking gains (include/altro_lqr.h) -----------------------------------------------------------------
constexpr int kLqrMaxN = 32;  // states (as kCovMaxN: k_lqr_recur has k_cov_recur's lane groups)
constexpr int kLqrMaxM = 8;   // controls: every lane factors S = R + B^T P B on its own
// One call of Engine::LqrGains.  Q, R (required) and Qf (null: Q) are [n][n], [m][m], [n][n]; K [B][N][m n], P [B][N + 1][n][n]
// and fail [B] may be null; host or device memory as the call says.
struct LqrArgs {
  const double *Q, *R, *Qf;
  int install;
  double *K, *P;
  int* fail;
};
// The weights as k_lqr_recur reads them: Q | R | Qf with every lower triangle mirrored, Qf = Q where it is null.  Refuses a
// lower-triangle entry that is not finite and an R whose lower triangle has no Cholesky factor; `err` gets the text.
inline bool LqrPackWeights(int n, int m, const double* Q, const double* R, const double* Qf, std::vector<double>* out, std::string* err,
                           const char* who) {
  out->assign((size_t)(2 * n * n + m * m), 0.0);
  double *q = out->data(), *r = q + n * n, *qf = r + m * m;
  auto mirror = [&](const double* src, int d, double* dst, const char* name) {
    for (int i = 0; i < d; ++i)
      for (int j = 0; j <= i; ++j) {
        const double v = src[i * d + j];
        if (!std::isfinite(v)) {
          *err = std::string(who) + ": " + name + "[" + std::to_string(i) + "][" + std::to_string(j) + "] is not finite";
          return false;
        }
        dst[i * d + j] = dst[j * d + i] = v;
      }
    return true;
  };
  if (!mirror(Q, n, q, "Q") || !mirror(R, m, r, "R") || !mirror(Qf ? Qf : Q, n, qf, "Qf")) return false;
  std::vector<double> L(r, r + m * m);  // Cholesky of R by rows, in place in the lower triangle
  for (int c = 0; c < m; ++c) {
    double d = L[c * m + c];
    for (int t = 0; t < c; ++t) d -= L[c * m + t] * L[c * m + t];
    if (!(d > 0.0) || !std::isfinite(d)) {
      *err = std::string(who) + ": R is not positive definite (the Cholesky pivot of row " + std::to_string(c) + " is " + std::to_string(d) + ")";
      return false;
    }
    const double root = std::sqrt(d);
    L[c * m + c] = root;
    for (int a = c + 1; a < m; ++a) {
      double v = L[a * m + c];
      for (int t = 0; t < c; ++t) v -= L[a * m + t] * L[c * m + t];
      L[a * m + c] = v / root;
    }
  }
  return true;
}

// ---- Monte-Carlo ensembles (include/altro_ensemble.h) --------------------------------------------------------------------
// altro_ensemble_stats as k_ens_finish writes it (the C-ABI translation unit asserts that the two layouts agree)
struct EnsembleStats {
  int samples, stopped_state, stopped_control, violated;
  double cost_mean, cost_max, violation_max, max_dx, max_du;
};
constexpr int kEnsMaxN = 32;         // states of a model the ensemble accepts (as kCovMaxN)
constexpr int kEnsChunk = 64;        // samples of one chunk: a wavefront
constexpr int kEnsFillWaves = 1024;  // wavefronts that fill the device (256 compute units x 4 SIMDs)
constexpr int kEnsMaxSlabs = 16;     // most partials per instance: bounds the scratch and what k_ens_finish adds
// fp64 sums per (instance, knot): n of e, n (n + 1) / 2 of the lower triangle of e e^T
constexpr int EnsembleValues(int n) { return n * (n + 3) / 2; }
// Slabs of one instance: a wavefront (one per workgroup) takes ONE slab -- `EnsembleChunksPerSlab` consecutive chunks of 64
// samples of ONE instance, one after the other -- and leaves one partial per slab, which k_ens_finish adds in slab order.
// A pure function of (B, S): the order of every sum, and with it every bit of the result, depends on nothing else.  One slab
// once the instances alone fill the device (B >= kEnsFillWaves); otherwise as many as fill it, at most kEnsMaxSlabs and no
// more than there are chunks, then lowered so that no slab is empty.
inline int EnsembleChunksPerSlab(long long B, long long S) {
  const long long chunks = (S + kEnsChunk - 1) / kEnsChunk, fill = (kEnsFillWaves + B - 1) / B;
  const long long want = std::max<long long>(1, std::min<long long>(std::min<long long>(chunks, fill), kEnsMaxSlabs));
  return (int)((chunks + want - 1) / want);
}
inline int EnsembleSlabs(long long B, long long S) {
  const long long chunks = (S + kEnsChunk - 1) / kEnsChunk, per = EnsembleChunksPerSlab(B, S);
  return (int)((chunks + per - 1) / per);
}
// One call of Engine::MpcEnsemble / Engine::NoiseFill.  Every pointer may be null; host or device memory as the call says.
struct EnsembleArgs {
  int steps, S, sigma0_per_instance, w_mode;
  unsigned long long seed, instance_base;
  const double *Sigma0, *W;   // as CovArgs
  const double *u_lo, *u_hi;  // [m] each, both or neither
  double viol_tol;
  double *dev_mean, *dev_mom2;  // [B][steps + 1][n], [B][steps + 1][n][n]
  int *alive, *viol_count;      // [B][steps + 1] each
  EnsembleStats* summary;       // [B]
  TrackStats* stats;            // [B][S]
  double *dx0, *w;              // NoiseFill's outputs: [B][S][n], [B][S][steps][n]
  int check_bounds;             // options.check_forwardpass_bounds, state_max, control_max
  double state_max, control_max;
};

// ---- blocks carved into parts ---------------------------------------------------------------------------------------
// Element counts of the K parts of one block -> the element every part starts at; off[K] is the size of the block.
template <int K>
struct Parts {
  size_t cnt[K], off[K + 1];
  Parts(std::initializer_list<size_t> counts) : cnt{}, off{} {
    int i = 0;
    for (size_t c : counts) {
      cnt[i] = c;
      off[i + 1] = off[i] + c;
      ++i;
    }
  }
  size_t total() const { return off[K]; }
};
// doubles that hold `count` elements of V: how a layout counted in doubles sizes a part of ints, bytes or structs
template <class V>
constexpr size_t DoublesFor(size_t count) {
  return (count * sizeof(V) + sizeof(double) - 1) / sizeof(double);
}
// the block Engine::MpcTrack stages for a host caller, in doubles: dx0 | w | u_lo, u_hi | X_cl | U_cl | stats.  L = B S lanes;
// an array the caller leaves out takes no room.
inline Parts<6> TrackStageParts(int n, int m, size_t L, size_t steps, bool dx0, bool w, bool bounds, bool X_cl, bool U_cl, bool stats) {
  static_assert(sizeof(TrackStats) % sizeof(double) == 0, "the statistics are staged in a block of doubles");
  return {dx0 ? L * n : 0,          w ? L * steps * n : 0,
          bounds ? 2 * (size_t)m : 0, X_cl ? L * (steps + 1) * n : 0,
          U_cl ? L * steps * m : 0, stats ? DoublesFor<TrackStats>(L) : 0};
}
// the block of a tracked closed-loop run, in doubles: X log | U log | one cycle's X, U | its last state | its disturbance |
// u_lo, u_hi | statistics [cycles][B]
inline Parts<8> TrackedRunParts(int n, int m, size_t B, size_t cycles, size_t shift) {
  const size_t Lk = cycles * shift;
  return {B * (Lk + 1) * n, B * Lk * m, B * (shift + 1) * n, B * shift * m, B * n, B * shift * n, 2 * (size_t)m,
          DoublesFor<TrackStats>(cycles * B)};
}
// the block of every other closed-loop run: X log | U log | w [cycles][B][n] | dU (`nd` doubles) | clearances (`nclear`)
inline Parts<5> PlainRunParts(int n, int m, size_t B, size_t cycles, size_t shift, bool w, size_t nd, size_t nclear) {
  return {B * (cycles * shift + 1) * n, B * cycles * shift * m, w ? cycles * B * n : 0, nd, nclear};
}
// The int block of a closed-loop run, counted in INTS: iterations [B][cycles] | statuses | winners [B / G][cycles] (a multi-
// start run: `winners` = B / G, else 0) | reason log [cycles][B] | ages [B] | reasons [B] | next mask (bytes [B], rounded up to
// ints); the last four only for a triggered run.  Winners and reason log are parts of their own: no run has both, so the
// block is as large as when the two shared one place.  (The tracked kinds record iterations and statuses [cycles][B].)
inline Parts<7> RunIntParts(size_t B, size_t cycles, size_t winners, bool triggered) {
  const size_t t = triggered ? 1 : 0;
  return {B * cycles, B * cycles, winners * cycles, t * B * cycles, t * B, t * B, t * ((B + sizeof(int) - 1) / sizeof(int))};
}
// the blocks the other calls stage for a host caller, in doubles; an array the caller leaves out takes no room.
// Engine::CovPropagate: Sigma0 | W | Sigma | sx | su | rpos
inline Parts<6> CovStageParts(int n, int m, size_t B, const CovArgs& c) {
  const size_t st = (size_t)c.steps, nn = (size_t)n * n;
  return {c.Sigma0 ? (c.sigma0_per_instance ? B : 1) * nn : 0,
          c.W ? ((c.w_mode & 1) ? B : 1) * ((c.w_mode & 2) ? st : 1) * nn : 0,
          c.Sigma ? B * (st + 1) * nn : 0,
          c.sx ? B * (st + 1) * n : 0,
          c.su ? B * st * m : 0,
          c.rpos ? B * (st + 1) : 0};
}
// Engine::MpcEnsemble: Sigma0 | W | u_lo, u_hi | dev_mean | dev_mom2 | alive | viol_count | summary | stats (alive and
// viol_count are ints [B][steps + 1]: DoublesFor<int>).  Engine::NoiseFill: Sigma0 | W | dx0 | w
inline Parts<9> EnsembleStageParts(int n, int m, size_t B, const EnsembleArgs& c) {
  static_assert(sizeof(EnsembleStats) % sizeof(double) == 0, "the summaries are staged in a block of doubles");
  const size_t st = (size_t)c.steps, nn = (size_t)n * n, ints = DoublesFor<int>(B * (st + 1));
  return {c.Sigma0 ? (c.sigma0_per_instance ? B : 1) * nn : 0,
          c.W ? ((c.w_mode & 1) ? B : 1) * ((c.w_mode & 2) ? st : 1) * nn : 0,
          c.u_lo ? 2 * (size_t)m : 0,
          c.dev_mean ? B * (st + 1) * n : 0,
          c.dev_mom2 ? B * (st + 1) * nn : 0,
          c.alive ? ints : 0,
          c.viol_count ? ints : 0,
          c.summary ? DoublesFor<EnsembleStats>(B) : 0,
          c.stats ? DoublesFor<TrackStats>(B * (size_t)c.S) : 0};
}
inline Parts<4> NoiseStageParts(int n, size_t B, const EnsembleArgs& c) {
  const size_t st = (size_t)c.steps, nn = (size_t)n * n, L = B * (size_t)c.S;
  return {c.Sigma0 ? (c.sigma0_per_instance ? B : 1) * nn : 0,
          c.W ? ((c.w_mode & 1) ? B : 1) * ((c.w_mode & 2) ? st : 1) * nn : 0,
          c.dx0 ? L * n : 0,
          c.w ? L * st * n : 0};
}
// Engine::CovInflate: the base track [cols][rows][np] | rpos [B][knots];  Engine::MsPerturb: dU [cols][N][m];
// Engine::Advance: x0 [B][n] | w [B][n];  Engine::SetReference: Xref | Uref, `points` = rows x columns of the path
inline Parts<2> InflateStageParts(size_t cols, size_t rows, size_t np, size_t B, size_t knots) { return {cols * rows * np, B * knots}; }
// Engine::MsGetBest: X [P][N + 1][n] | U [P][N][m] | statistics [P] of `stats_doubles` doubles each
inline Parts<3> MsBestStageParts(int n, int m, size_t P, size_t N, bool X, bool U, size_t stats_doubles) {
  return {X ? P * (N + 1) * n : 0, U ? P * N * m : 0, P * stats_doubles};
}
// Engine::Trigger: tracked [B] | age (ints [B]) | u_lo, u_hi | mask (bytes [B]) | reason (ints [B]), a host caller's | the
// lookahead's statistics [B] (every caller's: scratch that lives for the call)
inline Parts<6> TriggerStageParts(int m, size_t B, bool tracked, bool age, bool bounds, bool mask, bool reason, bool ahead) {
  const size_t ts = DoublesFor<TrackStats>(B), ints = DoublesFor<int>(B), bytes = DoublesFor<unsigned char>(B);
  return {tracked ? ts : 0, age ? ints : 0, bounds ? 2 * (size_t)m : 0, mask ? bytes : 0, reason ? ints : 0, ahead ? ts : 0};
}
// Engine::LqrGains: K [B][N][m][n] | P [B][N + 1][n][n] | fail (ints [B]);  Engine::SetSolveMask: the mask (bytes [B])
inline Parts<3> LqrStageParts(int n, int m, size_t B, size_t N, bool K, bool P, bool fail) {
  return {K ? B * N * m * n : 0, P ? B * (N + 1) * n * n : 0, fail ? DoublesFor<int>(B) : 0};
}
inline Parts<1> MaskStageParts(size_t B) { return {DoublesFor<unsigned char>(B)}; }
inline Parts<1> PerturbStageParts(int m, size_t cols, size_t N) { return {cols * N * m}; }
inline Parts<1> GaussStageParts(int m) { return {(size_t)m}; }  // Engine::MsPerturbGaussian: sigma [m]
inline Parts<2> AdvanceStageParts(int n, size_t B, bool x0, bool w) { return {x0 ? B * n : 0, w ? B * n : 0}; }
inline Parts<2> ReferenceStageParts(int n, int m, size_t points, bool U) { return {points * n, U ? points * m : 0}; }

// ---- one closed-loop run (altro_mpc_run, altro_mpc_run_tracked, altro_mpc_run_multistart, altro_mpc_run_team) -----------
// EngineBase::LoopBegin .. LoopEnd: between the two, every LoopCycle (behind the cycle's solve) logs what the loop applies
// and moves the horizon by `shift`.  All pointers are host arrays of the one C call that drives the run; any may be null.
enum LoopKind {
  kLoopPlain = 0,   // advance under w[c]
  kLoopTracked,     // track `shift` knots under the gains and w[c], advance from the tracked state
  kLoopMultiStart,  // select and spread the best of G starts, advance under w[c], perturb by dU
  kLoopTeam,        // log the team's clearance, advance under w[c] (the C API runs the team's rounds as the cycle's solve)
  kLoopTriggered    // kLoopTracked whose solves run under the mask the trigger rule left (include/altro_trigger.h)
};
struct LoopSpec {
  int kind, cycles, shift;
  const double* w;   // the disturbance of cycle c at w + c * w_stride: [B][n], tracked [B][shift][n]
  size_t w_stride;
  int G, dU_per_instance;       // multi-start: starts per problem; dU [G][N][m] or [B][N][m]
  const double* dU;
  int A, index;                 // team: agents per team, the team's knot circle constraint
  const double* radius;         // team: one per instance
  const double *u_lo, *u_hi;    // tracked, triggered: [m] each, both or neither
  TriggerRule rule;             // triggered
};
struct LoopStep {  // what a cycle takes from the handle at the moment it runs
  double reset_pen;  // the penalty of a row that starts afresh
  bool ilqr_mode;    // picks the status as GetStats does
  TrackArgs track;   // the options of a tracking call (check_bounds, state_max, control_max)
};
struct LoopOut {  // [B][cycles shift + 1][n], [B][cycles shift][m], [B][cycles] each; winner [B / G][cycles], clear [B / A][cycles]
  double *X_cl = nullptr, *U_cl = nullptr;
  int *iterations = nullptr, *status = nullptr, *winner = nullptr;
  double* clear = nullptr;
  TrackStats* track = nullptr;
  int* reason = nullptr;  // triggered: [B][cycles]
};

// ---- knot constraints (include/altro_knot_params.h) ----------------------------------------------------
// One launch of k_knot_params: every knot constraint of the handle, its knots, its place in the knot-parameter record and
// its track on the device -- track[(col * rows + row) * np + e], the caller's layout, cols = 1 (shared) or B.  Knot k reads
// row min(max(offset - base, 0) + k, rows - 1): base is 0 for every track a caller set, and the window offset at the
// moment of the fill for a track written by altro_team_fill_tracks (include/altro_team.h), whose row 0 is "now".
struct KnotTrack {
  const double* track;  // nullptr: no track set yet (the record keeps zeros)
  int k_begin, k_end, np, off, rows, cols, base;
};
struct KnotParArgs {
  int ncon, kt, offset, pad;
  KnotTrack c[kMaxKnotCons];
};

// ---- device-visible problem description (lives in global memory, read with scalar loads) ---------
struct ConDesc {
  int kind;          // altro_constraint_kind
  int type;          // 0 equality (dual cone = identity), 1 inequality (negative orthant)
  int p;             // rows
  int per_instance;  // params in the per-instance pool ([slot][Bp]) instead of the shared pool; kParPerKnotCon: per knot
  int param_off;     // first slot / element of this constraint's parameters (per knot: element of the knot's record)
  int row_off;       // row offset inside the knot
  unsigned lo_mask;  // CONTROL_BOUND: controls with a finite lower bound (basic_constraints.hpp:138-145); USER: index of the type
  unsigned hi_mask;  // CONTROL_BOUND: controls with a finite upper bound
};
struct KnotClass {
  int cost_group;
  int ncon;
  int nrows;
  int pad;
  ConDesc con[kMaxConPerKnot];
};
struct CostGroupDesc {
  int Q_off, R_off;          // shared pool, column-major n x n and m x m
  int q_off, r_off, c_off;   // pool element (shared) or slot (per instance)
  int q_pi, r_pi, c_pi;      // 0 shared, 1 per instance, kParPerKnot: from the reference-term record of the knot
  int q_diag, r_diag;        // Q / R are diagonal (every off-diagonal entry is exactly zero)
  int user, u_off, u_pi;     // user cost (altro_set_user_cost): 1 + index of its type; parameters at u_off (pool element / first slot)
};
// A run of consecutive knot points [k_begin, k_end) with the same class: rows of knot k start at
// rowbase + (k - k_begin) * nrows(cls).  Lets the serial kernels keep the class in scalar registers.
// `fast` selects a compile-time-specialised constraint layout for the serial rollout loop.
enum FastKind {
  kFastGeneric = 0,  // anything: table-driven evaluation
  kFastNone = 1,     // no constraint on these knots
  kFastB = 2,        // [CONTROL_BOUND with every lower and upper bound finite]
  kFastCB = 3,       // [CIRCLE, CONTROL_BOUND(full)]
  kFastBC = 4,       // [CONTROL_BOUND(full), CIRCLE]
  kFastC = 5         // [CIRCLE]
};
struct KnotRun {
  int k_begin, k_end, cls, rowbase;
  int fast, pad0, pad1, pad2;
};
struct ProblemDesc {
  int n, m, N, B, Bp;
  int nclass, ngroups, total_rows;
  int nruns, nslots;  // nslots: per-instance parameter slots (ipool rows)
  float hstep;        // uniform step (trajectory.hpp:122-130); the terminal knot's step is unused
  int npool;          // elements in the shared parameter pool
  KnotRun runs[kMaxRuns];
  KnotClass cls[kMaxClasses];
  CostGroupDesc grp[kMaxCostGroups];
};

// Options in the form the kernels consume (copied from altro_options at every launch).
struct DevOpts {
  int max_iterations_total, max_iterations_outer, max_iterations_inner;
  int bp_reg_fail_threshold, check_forwardpass_bounds, line_search_max_iterations, reset_duals;
  int fast_forward_stalls;  // opt-in (ALTRO_HIP_FAST_FORWARD_STALLS): see k_sweep_fused
  double cost_tolerance, gradient_tolerance;
  double bp_reg_increase_factor, bp_reg_initial, bp_reg_max, bp_reg_min;
  double state_max, control_max;
  double line_search_lower_bound, line_search_upper_bound, line_search_decrease_factor;
  double constraint_tolerance, maximum_penalty, initial_penalty;
};

// ---- the persistent tail kernel (k_sweep_fused): its words and its LDS, shared by the kernels and the engine -------------
#if defined(__HIPCC__)
#define ALTRO_HD __host__ __device__ __forceinline__
#else
#define ALTRO_HD inline
#endif
constexpr int kBlock = 64;  // one wavefront per workgroup: instances never share data

// ---- multi-start (include/altro_multistart.h): THE selection rule, host and device -----------------------------------
// The key of a start is the status, cost and violation altro_get_stats reports.  Class 0: solved, both numbers finite --
// ordered by cost; class 1: any other status, both finite -- by violation, then cost; class 2: a NaN or an infinity.  The
// lower class wins, comparisons are fp64 `<`, ties go to the lowest start index: a total order.
ALTRO_HD int ms_class(int status, double cost, double violation) {
  if (!(__builtin_isfinite(cost) && __builtin_isfinite(violation))) return 2;
  return status == ALTRO_SOLVED ? 0 : 1;
}
// start a STRICTLY before start b, whatever their indices (false on a tie)
ALTRO_HD bool ms_before(int status_a, double cost_a, double viol_a, int status_b, double cost_b, double viol_b) {
  const int ca = ms_class(status_a, cost_a, viol_a), cb = ms_class(status_b, cost_b, viol_b);
  if (ca != cb) return ca < cb;
  if (ca == 2) return false;
  if (ca == 1) {
    if (viol_a < viol_b) return true;
    if (viol_b < viol_a) return false;
  }
  return cost_a < cost_b;
}
// the winner among starts 0 .. G-1 (element g of each array at g * stride)
ALTRO_HD int ms_select(const int* status, const double* cost, const double* violation, int G, int stride) {
  int w = 0;
  for (int g = 1; g < G; ++g)
    if (ms_before(status[g * stride], cost[g * stride], violation[g * stride], status[w * stride], cost[w * stride],
                  violation[w * stride]))
      w = g;
  return w;
}

// ---- event-triggered re-planning (include/altro_trigger.h): THE rule, host and device ----------------------------------
// The reason instance b is re-planned, 0 if it is not: the OR of the criteria that hold.  `tracked`: the statistics of the
// segment just tracked, null without any (the three tracked criteria are off); `status`: what altro_get_stats reports for
// the instance; `ahead`: the statistics of the lookahead's track, read only with rule.lookahead > 0.  Every comparison is
// !(v <= tol): a NaN triggers.  kTrigFirst is the run's own, never set here.
ALTRO_HD int trigger_reason(const TriggerRule& rule, int age, const TrackStats* tracked, int status, const TrackStats* ahead) {
  int why = 0;
  if (age >= rule.max_age) why |= kTrigAge;
  if (tracked) {
    if (rule.dx_tol >= 0.0 && !(tracked->max_dx <= rule.dx_tol)) why |= kTrigDeviation;
    if (rule.viol_tol >= 0.0 && !(tracked->violation <= rule.viol_tol)) why |= kTrigViolation;
    if (tracked->status != ALTRO_UNSOLVED) why |= kTrigLimit;
  }
  if (rule.on_unsolved && status != ALTRO_SOLVED) why |= kTrigUnsolved;
  if (rule.lookahead > 0 && ahead && (ahead->status != ALTRO_UNSOLVED || !(ahead->violation <= rule.ahead_tol))) why |= kTrigAhead;
  return why;
}
// knots per synchronisation of the persistent kernel's knot loop (the batched sweeps: 2), see producer_syncs_after.
// Round 2 (hardware barriers only): 4 measured 5.24 -> 5.30 ms on config 2, 5.03 -> 4.74 ms on config 3, the headline kept
// 2.  Round 3: with the forward waves of config 2 synchronised through sequence words (kSpecFree) a meeting costs the
// consumers an LDS round trip, and 4 wins on both (tail iteration 43.8 -> 42.2 us on config 2, 57.1 -> 55.6 us on
// config 3): 4.
#ifndef ALTRO_SYNC_FUSED
#define ALTRO_SYNC_FUSED 4
#endif
constexpr int kSyncFused = ALTRO_SYNC_FUSED;
constexpr int kSyWords = 16;  // sequence words of the forward pass (FwdSyncWord, altro_kernels.hpp)

// What a launch of the persistent kernel reports to the host: the words behind the sweep counters (`sweeps_out` in the
// kernel; Engine::ReadBackCounters reads them back).
enum TailReportWord {
  kRwChainLoops = 0,   // longest chain of iterations of one instance inside this launch
  kRwUnits = 1,        // (instance, iteration) units processed by this launch
  kRwSweeps = 2,       // ... the longest chain counted from the first sweep of the solve
  kRwSyncErr = 3,      // a forward wave gave up waiting for a sequence word
  kRwHandovers = 4,    // confirmed joints between twin workgroups (depends on timing)
  kRwClaims = 5,       // claims of pool workgroups, at every level (depends on timing)
  kRwGroupLoops = 6,   // most iterations any ONE job ran (a primary's or a pool workgroup's share; a worker of the
                       // worker grid runs several jobs, each reports for itself)
  kRwWords = 8
};
// fh (wave 0's backward pass) and fh2 (the fourth wave's speculative one): what a backward pass hands to the forward pass
// of the same kernel.  Both blocks use the same indices; the slots from kFhRegLog on exist in fh2 only.
enum FhSlot {
  kFhJ0 = 0,        // running cost of the expansion step (auxiliary wave -> cost wave, behind barrier A)
  kFhDV0 = 1,       // expected cost change, linear and quadratic term
  kFhDV1 = 2,
  kFhInitCost = 3,  // stats_.initial_cost (auxiliary wave -> cost wave)
  kFhRho = 4,       // regularisation the backward pass leaves (DecreaseRegularization)
  kFhDrho = 5,
  kFhWords = 6,     // size of fh
  kFhRegLog = 6,    // fh2: the regularisation the speculative pass ran with (stats_.Log("reg", rho_))
  kFhSpecOk = 7,    // fh2: the speculative pass went through without a Cholesky failure
  kFhSpecRho = 8,   // fh2: the regularisation the speculative pass assumed phase 3 would set (FwdSpec::inbox)
  kFhSpecDrho = 9,
  kFh2Words = 12    // size of fh2 (two words spare)
};
// ff: what phase 3 of the forward pass leaves for the kernel's bookkeeping, LDS mirrors of per-instance scalars, and the
// words with which thread 0 (or wave 0) tells the workgroup a decision.  Slots 12 - 14 carry one name per purpose: each
// purpose is written by one thread, read behind the next workgroup barrier and dead before the next purpose's writer runs
// -- the claim words before the iteration loop, segment and twin words in separate barrier intervals of the loop's end, the
// commit words behind the loop.
enum FfSlot {
  kFfRejected = 0,      // phase 3: the line search rejected every trial
  kFfRho = 1,           // phase 3: the regularisation entering the next iteration
  kFfDrho = 2,
  kFfInnerDone = 3,     // phase 3: the inner solve ended (or the column left the solve)
  kFfInitCost = 4,      // mirror of initial_cost (auxiliary wave, lane 0 only)
  kFfNeedInitCost = 5,  // mirror of need_init_cost
  kFfItInner = 6,       // phase 3: the counters entering the next iteration
  kFfItTotal = 7,
  kFfClaimItInner = 8,  // pool workgroup: the state its claim enters with (tw_try_claim -> tw_enter_clone)
  kFfClaimItTotal = 9,
  kFfClaimRho = 10,
  kFfClaimDrho = 11,
  kFfClaimOpen = 12,    // pool workgroup, before the loop: the claim was not refused while the clone was made
  kFfSegLeave = 12,     // loop, segment joint: this column retires or was cancelled
  kFfTwinAction = 13,   // loop, twin bookkeeping: 0 go on, 1 this worker's claim was refused, 2 joint reached -- hand over
  kFfHandResult = 13,   // loop, hand-over (behind the action's barrier): 3 handed over, 1 own claim refused, 0 go on alone
  kFfCommitOk = 13,     // behind the loop: the predecessor confirmed -- commit the shadow column
  kFfClaimInst = 14,    // pool workgroup, before the loop: the instance of the claimed streak
  kFfLoopsBefore = 14,  // hand-over and commit: iterations the workers before this one ran
  kFfClaimSource = 15,  // pool workgroup: mailbox of the publisher it claimed from, -1 none
  kFfWords = 16
};

// DISTANCE BETWEEN THE STAGED BLOCKS OF A WORKGROUP'S INSTANCES: see ALTRO_FWD_BLOCK_MOD in altro_kernels.hpp
#ifndef ALTRO_FWD_BLOCK_MOD
#define ALTRO_FWD_BLOCK_MOD 160
#endif
ALTRO_HD constexpr int fwd_block_pad_bytes(long long raw_bytes) {
  return ALTRO_FWD_BLOCK_MOD < 0 ? 0 : (int)(((ALTRO_FWD_BLOCK_MOD - raw_bytes % 256) + 256) % 256);
}
template <class T>
struct FwdLds {  // element counts of one instance's staged block (16-byte aligned sub-blocks)
  int nX, nU, nKD, nR, nS, V;
  ALTRO_HD int padv(int e) const { return (e + V - 1) / V * V; }
  ALTRO_HD int rowsP() const { return padv(nR); }
  ALTRO_HD int raw() const { return nX + nU + nKD + 2 * padv(nR) + padv(nS); }
  ALTRO_HD int total() const { return raw() + fwd_block_pad_bytes((long long)raw() * (long long)sizeof(T)) / (int)sizeof(T); }
};
// LDS of k_sweep_fused: byte offset of every sub-block, in the order the kernel keeps them, and the size the engine asks
// for.  Every count that enters is a multiple of 16 bytes (records and rows are padded to V elements, the block padding keeps
// that, a hand-off slot is kBlock elements wide), so every sub-block up to sCost starts 16-byte aligned without rounding;
// sCand keeps the 128-byte phase of the block before it.  tests/test_fused_lds.py checks all of this against the formula
// Engine::PlanForwardLds used to carry.
template <class T>
struct FusedLds {
  FwdLds<T> blk;  // the forward block of one instance: X | U | KD | lam | pen | ipool
  int N, nm, npool;
  static constexpr int kE = (int)sizeof(T), kD = (int)sizeof(double);
  ALTRO_HD int oPool() const { return blk.total() * kE; }                    // shared parameter pool
  ALTRO_HD int oXch() const { return oPool() + blk.padv(npool) * kE; }       // 2 kSyncFused hand-off slots [nm][kBlock]
  ALTRO_HD int oFlags() const { return oXch() + 2 * kSyncFused * nm * kBlock * kE; }  // 2 kBlock ints: bound checks, statuses
  ALTRO_HD int oGrad() const { return oFlags() + 2 * kBlock * (int)sizeof(int); }     // kBlock gradient slots
  ALTRO_HD int oFh() const { return oGrad() + kBlock * kD; }                 // fh[kFhWords]
  ALTRO_HD int oJunk() const { return oFh() + kFhWords * kD; }               // one junk slot per lane of the backward wave
  ALTRO_HD int oActive() const { return oJunk() + kBlock * kD; }             // active flag (an int in a pair of doubles)
  ALTRO_HD int oFf() const { return oActive() + 2 * kD; }                    // ff[kFfWords]
  ALTRO_HD int oCand() const { return oFf() + kFfWords * kD; }               // [N + 1][kLineSearchLanes][nm] candidates
  ALTRO_HD int oKD2() const { return oCand() + (N + 1) * kLineSearchLanes * nm * kE; }  // the speculative pass's gains + junk
  ALTRO_HD int oFh2() const { return oKD2() + (blk.nKD + kBlock) * kE; }     // fh2[kFh2Words]
  ALTRO_HD int oAlpha() const { return oFh2() + kFh2Words * kD; }            // [kLineSearchLanes] step lengths (8-byte slots)
  ALTRO_HD int oSync() const { return oAlpha() + kLineSearchLanes * kD; }    // [kSyWords] ints
  ALTRO_HD int oCost() const { return oSync() + kSyWords * (int)sizeof(int); }  // [N + 1] knot costs, padded to a pair
  ALTRO_HD int oCvalAhead() const { return oCost() + ((N + 2) & ~1) * kE; }  // [rows] constraint values computed ahead
  ALTRO_HD int used() const { return oCvalAhead() + blk.rowsP() * kE; }
  ALTRO_HD int oTicket() const { return used(); }  // the worker grid's ticket word: the first int of the reserve below
  // the engine has always asked for a little more than the kernel lays out (8 doubles behind the sequence words, N + 4
  // knot costs); the LDS size decides how many workgroups share a CU, so the reserve stays
  ALTRO_HD size_t bytes() const { return (size_t)used() + 8 * kD + (size_t)(N + 4 - ((N + 2) & ~1)) * kE; }
};

// Engines of this process that run their sweeps as chains on streams of their own, PER DEVICE (hardware queues are a
// device's).  The count lives in libaltro_hip.so; a user-model plugin carries its own copy of this header, so the
// library hands every plugin a pointer to ITS counter function at load time (altro_user_set_chain_hook): built-in and
// plugin engines then share one book.  delta = +1 / -1 / 0 (query); returns the count after the change.
inline int ChainClaimLocal(int device, int delta) {
  static std::atomic<int> n[64];
  std::atomic<int>& c = n[device >= 0 && device < 64 ? device : 63];
  if (delta == 0) return c.load();
  return c.fetch_add(delta) + delta;
}
using ChainClaimFn = int (*)(int, int);
inline ChainClaimFn& ChainClaimHook() {
  static ChainClaimFn fn = &ChainClaimLocal;
  return fn;
}
inline int ChainClaim(int device, int delta) { return ChainClaimHook()(device, delta); }

// ---- engine interface ----------------------------------------------------------------------------
class EngineBase {
 public:
  virtual ~EngineBase() {}
  virtual altro_status Upload(const ProblemSpec& spec, std::string* err) = 0;
  virtual altro_status SetInitialState(const ProblemSpec& spec, std::string* err) = 0;
  virtual altro_status SetTrajectory(const ProblemSpec& spec, std::string* err) = 0;
  virtual altro_status SetStep(float hstep) = 0;
  // per-knot steps / times of the spec (or back to the uniform step when both are empty)
  virtual altro_status SetKnotTimes(const ProblemSpec& spec, std::string* err) = 0;
  virtual altro_status ResetTrajectory() = 0;
  virtual altro_status ResetStats() = 0;
  virtual altro_status SetPenalty(double rho) = 0;
  virtual altro_status SetPenaltyScaling(double phi) = 0;
  virtual altro_status SolveAL(const altro_options& o) = 0;
  virtual altro_status SolveILQR(const altro_options& o) = 0;
  virtual altro_status AlInit(const altro_options& o) = 0;
  virtual altro_status SolveSetup(const altro_options& o) = 0;
  virtual altro_status Rollout(const altro_options& o) = 0;
  virtual altro_status Cost(const altro_options& o, double* J) = 0;
  virtual altro_status UpdateExpansions(const altro_options& o) = 0;
  virtual altro_status BackwardPass(const altro_options& o) = 0;
  virtual altro_status ForwardPass(const altro_options& o) = 0;
  virtual altro_status UpdateConvergenceStatistics(const altro_options& o) = 0;
  virtual altro_status UpdateDuals(const altro_options& o) = 0;
  virtual altro_status UpdatePenalties(const altro_options& o) = 0;
  virtual altro_status GetMaxViolation(double* out) = 0;
  virtual altro_status GetMaxPenalty(double* out) = 0;
  virtual altro_status GetTrajectory(double* X, double* U) = 0;
  virtual altro_status GetGains(double* K, double* d) = 0;
  virtual altro_status SetRecordCtg(int enable) = 0;
  virtual altro_status GetCtg(double* P, double* p) = 0;
  virtual altro_status GetExpansion(int k, double* AB, double* lxx, double* lxu, double* luu,
                                    double* lx, double* lu) = 0;
  virtual altro_status GetKnotCosts(double* costs) = 0;
  virtual int NumRows() = 0;
  virtual int NumRowsAt(int k) = 0;
  virtual altro_status GetRows(int which /*0 lam,1 pen,2 cval*/, double* out) = 0;
  virtual altro_status SetDuals(const double* lam) = 0;
  virtual altro_status GetStats(altro_stats* st, bool ilqr_mode) = 0;
  virtual altro_status GetTiming(altro_timing* t) = 0;
  virtual altro_status SetRecordHistory(int capacity) = 0;
  virtual int GetHistory(int instance, int field, double* out, int cap) = 0;
  virtual int GetHistoryAll(int instance, double* out /*[kHistFields][cap]*/, int cap) = 0;
  virtual altro_status PackResultsDevice(void* dst) = 0;
  virtual altro_status PackTrajectoryDevice(double* X, double* U) = 0;
  virtual altro_status DeviceInfo(char* name, int name_len, int* cu_count) = 0;
  // receding-horizon advance (include/altro_mpc.h).  x0, w: fp64 [B][n] or nullptr, host arrays or (on_device) memory of the
  // engine's device; reset_pen: the penalty of a row that starts afresh.
  virtual altro_status MpcAdvance(int shift, const double* x0, const double* w, int on_device, double reset_pen) = 0;
  // closed-loop tracking under the gains on the device (k_mpc_track); changes nothing on the engine
  virtual altro_status MpcTrack(const TrackArgs& call, int on_device) = 0;
  // one closed-loop run (LoopSpec above).  Begin copies to the device what the run keeps there (radii, dU, bounds, w of the
  // multi-start and team kinds) and opens the logs, replacing whatever an earlier run left; End downloads the logs of a run
  // that went through all its cycles and frees the run's blocks, also after a failure
  virtual altro_status LoopBegin(const LoopSpec& spec) = 0;
  virtual altro_status LoopCycle(const LoopStep& step) = 0;
  virtual altro_status LoopEnd(const LoopOut& out) = 0;
  virtual altro_status GetInitialState(double* x0) = 0;
  virtual altro_status SetPenalties(const double* rho) = 0;
  // rows and cone (1: equality) of every registered constraint, in registration order
  virtual void ConShapes(std::vector<int>* p, std::vector<int>* eq) = 0;
  // the reference path of the tracking costs (include/altro_tracking.h: altro_set_reference): host arrays or (on_device) memory
  // of the engine's device; Uref may be null (zeros).  The terms are recomputed on the device behind every change.
  virtual altro_status SetReference(const double* Xref, const double* Uref, int rows, int per_instance, int on_device) = 0;
  virtual altro_status SetReferenceOffset(int offset) = 0;
  virtual int GetReferenceOffset() = 0;
  virtual altro_status GetReferenceTerms(double* q, double* r, double* c) = 0;
  // the parameter tracks of the knot constraints (include/altro_knot_params.h): `index` is the registration index of a knot
  // constraint; P is host memory or (on_device) memory of the engine's device.  The records the kernels read are rewritten on
  // the device behind every change.
  virtual altro_status SetConstraintTrack(int index, const double* P, int rows, int per_instance, int on_device) = 0;
  virtual altro_status SetTrackOffset(int offset) = 0;
  virtual int GetTrackOffset() = 0;
  virtual altro_status GetKnotParams(int index, double* out) = 0;
  // multi-start (include/altro_multistart.h): G adjacent columns are the starts of one problem.  Pointers are host arrays
  // or (on_device) memory of the engine's device; ilqr_mode picks the status as GetStats does.
  virtual altro_status MsSelect(int G, int* winner, int on_device, bool ilqr_mode) = 0;
  virtual altro_status MsSpread(int G, int* winner, int on_device, bool ilqr_mode) = 0;
  virtual altro_status MsPerturb(int G, const double* dU, int per_instance, int on_device) = 0;
  virtual altro_status MsGetBest(int G, double* X, double* U, altro_stats* stats, int* winner, int on_device, bool ilqr_mode) = 0;
  // teams (include/altro_team.h): A adjacent columns are the agents of one team, `index` the registration index of the team's
  // knot circle constraint.  TeamRadius copies the radii (host, one per instance) to the device, where they stay for the
  // fills and clearances that follow; clear is [B / A], host or (on_device) memory of the engine's device.
  virtual altro_status TeamRadius(const double* radius_per_instance) = 0;
  virtual altro_status TeamFill(int A, int index, int mode, double blend) = 0;
  virtual altro_status TeamClearance(int A, int index, double* clear, int on_device) = 0;
  // the solve mask (include/altro_subset.h): a byte per instance, host memory or (on_device) memory of the engine's device;
  // a null host pointer clears it.  GetSolveMask: mask [B] (all ones without a mask), count may be null.  The three below
  // serve a sequential team round: keep the caller's mask aside, set "agent a of every team" on the device, put it back.
  virtual altro_status SetSolveMask(const unsigned char* mask, int on_device) = 0;
  virtual altro_status GetSolveMask(unsigned char* mask, int* count) = 0;
  virtual altro_status SaveSolveMask() = 0;
  virtual altro_status TeamTurnMask(int A, int a) = 0;
  virtual altro_status RestoreSolveMask() = 0;
  // closed-loop covariance (include/altro_covariance.h): CovPropagate changes nothing on the engine; CovInflate writes the
  // per-instance track of knot circle constraint `index` (base [rows][np] or [B][rows][np], rpos [B][N + 1]) and leaves the
  // window offset alone.  Host arrays, or (on_device) memory of the engine's device.
  virtual altro_status CovPropagate(const CovArgs& call, int on_device) = 0;
  virtual altro_status CovInflate(int index, const double* base, int rows, int per_instance, double kappa, const double* rpos,
                                  int on_device) = 0;
  // event-triggered re-planning (include/altro_trigger.h): the rule for every instance (k_mpc_trigger; the lookahead through
  // k_mpc_track); changes nothing on the engine.  The loop kind kLoopTriggered keeps ages, masks and reasons on the device.
  virtual altro_status Trigger(const TriggerArgs& call, int on_device, bool ilqr_mode) = 0;
  // Monte-Carlo ensembles (include/altro_ensemble.h): MpcEnsemble and NoiseFill change nothing on the engine; host arrays, or
  // (on_device) memory of the engine's device.  MsPerturbGaussian: sigma [m] on the host.
  virtual altro_status MpcEnsemble(const EnsembleArgs& call, int on_device) = 0;
  virtual altro_status NoiseFill(const EnsembleArgs& call, int on_device) = 0;
  virtual altro_status MsPerturbGaussian(int G, unsigned long long seed, unsigned long long instance_base, const double* sigma,
                                         int keep_first) = 0;
  // time-varying LQR tracking gains about the plan (include/altro_lqr.h).  LqrGains: host arrays, or (on_device) memory of the
  // engine's device; with `install` the gains replace K of the gain record (d = 0) where the instance did not fail.  The policy
  // (packed weights of LqrPackWeights; empty: off) makes every whole solve end with that pass, installed under the solve's mask.
  virtual altro_status LqrGains(const LqrArgs& call, int on_device) = 0;
  virtual void LqrSetPolicy(const std::vector<double>& packed) = 0;
  virtual const char* LastError() = 0;
};

// One factory per (dtype, model) translation unit (inst_*.hip); returns nullptr if dims mismatch.
EngineBase* MakeEngineUnicycleF64(const altro_desc& d, std::string* err);
EngineBase* MakeEngineUnicycleF32(const altro_desc& d, std::string* err);
EngineBase* MakeEngineTripleInt2F64(const altro_desc& d, std::string* err);
EngineBase* MakeEngineTripleInt2F32(const altro_desc& d, std::string* err);
EngineBase* MakeEngineQuad12F64(const altro_desc& d, std::string* err);
EngineBase* MakeEngineQuad12F32(const altro_desc& d, std::string* err);

}  // namespace altro_hip
