// altro_engine.hpp — host orchestration of the batched AL-iLQR kernels for one (dtype, model).
//
// Owns the device state of one handle (one device, one HIP stream) and drives the sweeps:
//   AL solve  = k_al_init, k_solve_setup, k_rollout, then { k_expansions, k_backward, k_forward }
//               until no instance is active.  The host runs ONE SWEEP AHEAD of the device: sweep
//               i+1 is enqueued before the active-instance counter of sweep i is read back, so the
//               stream never drains (an all-idle sweep costs three empty launches).
// Instantiated once per translation unit (inst_*.hip).
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "altro_devmem.hpp"
#include "altro_kernels.hpp"
#include "altro_problem.hpp"

namespace altro_hip {

#define ALTRO_HIP_CHECK(expr)                                                                  \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      char buf_[512];                                                                          \
      snprintf(buf_, sizeof(buf_), "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,               \
               hipGetErrorString(e_));                                                         \
      err_ = buf_;                                                                             \
      return ALTRO_HIP_ERROR;                                                                  \
    }                                                                                          \
  } while (0)

#define ALTRO_TRY(expr)                  \
  do {                                   \
    altro_status st_ = (expr);           \
    if (st_ != ALTRO_OK) return st_;     \
  } while (0)

// The ALTRO_HIP_* switches of an engine, all read in one place: once, when the engine is constructed
// (the C API creates the engine at the first upload of a handle).
constexpr int kSpecAuto = -1;  // speculation mode of the persistent kernel chosen per problem (see Switches::spec_mode)
enum FwdSrcSwitch { kFwdSrcAuto = -1, kFwdSrcOther = 0, kFwdSrcGlobal = 1 };
struct Switches {
  struct OptInt {  // a number that overrides a computed default
    bool set = false;
    int v = 0;
  };
  // ALTRO_HIP_DEBUG_POISON=<hex pattern>[,mix]: fill LDS, line-search candidates and shadow columns with the pattern
  bool poison_on = false;
  unsigned poison_pattern = 0;
  int poison_mix = 0;
  OptInt persist_at;               // ALTRO_HIP_PERSIST_AT: active instances at which the persistent tail kernel takes over
  bool twin = true;                // ALTRO_HIP_TWIN=0: no twin workgroups, no columns for them
  bool segments = true;            // ALTRO_HIP_SEGMENTS=0: no segments of rejection streaks
  OptInt chains;                   // ALTRO_HIP_CHAINS: chains of batched sweeps, 1 .. kMaxSweepChains (also skips the stream probe)
  OptInt fwd_per_wave;             // ALTRO_HIP_FWD_PER_WAVE: at most this many instances per forward workgroup
  int fwd_src = kFwdSrcAuto;       // ALTRO_HIP_FWD_SRC=global | anything else: where the rollout wave reads its inputs
  int sweep_loop = -1;             // ALTRO_HIP_SWEEP_LOOP: 0 never, any other number always, unset (-1): iff the batch fits the slots
  OptInt loop_per_cu;              // ALTRO_HIP_LOOP_PER_CU: at most this many loop workgroups per CU
  int cand_front = 6;              // ALTRO_HIP_CAND_FRONT: line-search trials that own a candidate slot
  bool twin_debug = false;         // ALTRO_HIP_TWIN_DEBUG: mailbox dump of the twins
  bool twin_debug_all = false;     // ALTRO_HIP_TWIN_DEBUG=all: every segment, every primary and every idle pool workgroup of a large launch too
  int twin_depth = kTwinDefaultDepth;  // ALTRO_HIP_TWIN_DEPTH=n: at most 2^n workers per rejection streak (1: one twin per primary)
  int twin_min = tw_min_share(kTwinDefaultMin);  // ALTRO_HIP_TWIN_MIN=n: iterations both shares of a split must hold (>= kTwinMinFloor)
  int twin_spread = kTwinDefaultSpread;  // ALTRO_HIP_TWIN_SPREAD=s: the pool treats segments within 2^s iterations left of each other as equals (0: the longest first, for all)
  int twin_misclaim = 0;           // ALTRO_HIP_TWIN_MISCLAIM=k (tests): every k-th claim assumes a regularisation one ulp off
  // ALTRO_HIP_TAIL_WORKERS: the persistent launch as a grid of resident workers that take its jobs by ticket.  Unset: as
  // many as the device holds at once; 0: the one-shot grid, a workgroup per job; n: at most n workers (tests)
  int tail_workers = kTailWorkersDefault;
  const char* sweep_log = nullptr; // ALTRO_HIP_SWEEP_LOG[=all]: timeline of the chains of sweeps
  bool loop_log = false;           // ALTRO_HIP_LOOP_LOG: phase log of the device-side loop
  bool force_valu_backward = false, force_coop_backward = false;  // ALTRO_HIP_BACKWARD = valu | coop: a fallback backward kernel (tests)
  bool dense_expansions = true;    // ALTRO_HIP_NO_DENSE_EXPANSIONS
  // speculative backward pass of the persistent kernel: on its fourth wave (default) or not at all (ALTRO_HIP_SPECULATION=off)
  // (default, kSpecAuto: the fourth wave -- free-running beside software-synchronised forward waves where the rollout
  //  wave paces the knot loop, in lock step on problems with circle constraints, whose knot loop is paced by the cost
  //  wave: there the sequence words only add their polls.  Measured per tail iteration: config 2 46.0 -> 42.0 us free,
  //  config 3 54.7 lock step against 57.0 us free.)
  int spec_mode = kSpecAuto;
  bool fast_forward = false;       // ALTRO_HIP_FAST_FORWARD_STALLS
  // the start of a solve as one launch (k_begin_solve); ALTRO_HIP_BEGIN_SOLVE=split restores the seven stream operations
  // (the bit-identity test of the two, tests/test_fused_gpu.py)
  bool begin_merged = true;
  bool no_fused = false;           // ALTRO_HIP_NO_FUSED_SWEEP

  static bool NotZero(const char* e) { return !(e && atoi(e) == 0); }  // "set and equal to 0" switches a feature off
  static bool Is(const char* e, const char* what) { return e && std::strcmp(e, what) == 0; }
  Switches() {
    auto env = [](const char* name) { return std::getenv(name); };
    auto number = [&](const char* name) {
      const char* e = env(name);
      return e ? OptInt{true, atoi(e)} : OptInt{};
    };
    if (const char* e = env("ALTRO_HIP_DEBUG_POISON")) {
      poison_on = true;
      poison_pattern = (unsigned)strtoul(e, nullptr, 16);
      poison_mix = std::strchr(e, ',') != nullptr;
    }
    persist_at = number("ALTRO_HIP_PERSIST_AT");
    twin = NotZero(env("ALTRO_HIP_TWIN"));
    segments = NotZero(env("ALTRO_HIP_SEGMENTS"));
    chains = number("ALTRO_HIP_CHAINS");
    if (chains.set) chains.v = std::max(1, std::min(kMaxSweepChains, chains.v));
    fwd_per_wave = number("ALTRO_HIP_FWD_PER_WAVE");
    if (const char* e = env("ALTRO_HIP_FWD_SRC")) fwd_src = Is(e, "global") ? kFwdSrcGlobal : kFwdSrcOther;
    if (const char* e = env("ALTRO_HIP_SWEEP_LOOP")) sweep_loop = NotZero(e) ? 1 : 0;
    loop_per_cu = number("ALTRO_HIP_LOOP_PER_CU");
    if (const char* e = env("ALTRO_HIP_CAND_FRONT")) cand_front = std::max(0, std::min(kLineSearchLanes - 1, atoi(e)));
    twin_debug = env("ALTRO_HIP_TWIN_DEBUG") != nullptr;
    twin_debug_all = Is(env("ALTRO_HIP_TWIN_DEBUG"), "all");
    if (const char* e = env("ALTRO_HIP_TWIN_DEPTH")) twin_depth = std::max(1, std::min(kTwinMaxDepth, atoi(e)));
    if (const char* e = env("ALTRO_HIP_TWIN_MIN")) twin_min = tw_min_share(atoi(e));
    if (const char* e = env("ALTRO_HIP_TWIN_SPREAD")) twin_spread = std::max(0, std::min(kTwinMaxSpread, atoi(e)));
    if (const char* e = env("ALTRO_HIP_TWIN_MISCLAIM")) twin_misclaim = std::max(0, atoi(e));
    if (const char* e = env("ALTRO_HIP_TAIL_WORKERS")) tail_workers = std::max(0, atoi(e));
    sweep_log = env("ALTRO_HIP_SWEEP_LOG");
    loop_log = env("ALTRO_HIP_LOOP_LOG") != nullptr;
    force_valu_backward = Is(env("ALTRO_HIP_BACKWARD"), "valu");
    force_coop_backward = Is(env("ALTRO_HIP_BACKWARD"), "coop");
    dense_expansions = env("ALTRO_HIP_NO_DENSE_EXPANSIONS") == nullptr;
    const char* spec = env("ALTRO_HIP_SPECULATION");
    spec_mode = Is(spec, "off") ? (int)kSpecOff : Is(spec, "free") ? (int)kSpecFree : Is(spec, "wave") ? (int)kSpecWave : kSpecAuto;
    fast_forward = env("ALTRO_HIP_FAST_FORWARD_STALLS") != nullptr;
    begin_merged = !Is(env("ALTRO_HIP_BEGIN_SOLVE"), "split");
    no_fused = env("ALTRO_HIP_NO_FUSED_SWEEP") != nullptr;
  }
};

inline DevOpts ToDevOpts(const altro_options& o) {
  DevOpts d{};
  d.max_iterations_total = o.max_iterations_total;
  d.max_iterations_outer = o.max_iterations_outer;
  d.max_iterations_inner = o.max_iterations_inner;
  d.bp_reg_fail_threshold = o.bp_reg_fail_threshold;
  d.check_forwardpass_bounds = o.check_forwardpass_bounds;
  d.line_search_max_iterations = o.line_search_max_iterations;
  d.reset_duals = o.reset_duals;
  d.cost_tolerance = o.cost_tolerance;
  d.gradient_tolerance = o.gradient_tolerance;
  d.bp_reg_increase_factor = o.bp_reg_increase_factor;
  d.bp_reg_initial = o.bp_reg_initial;
  d.bp_reg_max = o.bp_reg_max;
  d.bp_reg_min = o.bp_reg_min;
  d.state_max = o.state_max;
  d.control_max = o.control_max;
  d.line_search_lower_bound = o.line_search_lower_bound;
  d.line_search_upper_bound = o.line_search_upper_bound;
  d.line_search_decrease_factor = o.line_search_decrease_factor;
  d.constraint_tolerance = o.constraint_tolerance;
  d.maximum_penalty = o.maximum_penalty;
  d.initial_penalty = o.initial_penalty;
  return d;
}

template <class T, class M>
class Engine final : public EngineBase {
  static constexpr int n = M::n, m = M::m, nm = n + m;
  using R = Rec<T, n, m>;
  using RS = rec_scalar_t<T, M>;  // storage type of the expansion and gain records (float under WithRec32<>)
  using RR = Rec<RS, n, m>;

 public:
  explicit Engine(const altro_desc& d) : desc_(d) {}
  ~Engine() override { Release(); }
  const char* LastError() override { return err_.c_str(); }

  altro_status Init() {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    ALTRO_HIP_CHECK(hipEventCreateWithFlags(&start_ev_, hipEventDisableTiming));
    ALTRO_HIP_CHECK(hipEventCreateWithFlags(&tail_ev_, hipEventDisableTiming | hipEventBlockingSync));
    cur_ = stream_;
    ALTRO_HIP_CHECK(hipDeviceGetAttribute(&num_cus_, hipDeviceAttributeMultiprocessorCount, desc_.device_id));
    // (round 3, tail iteration at 39 us: hand-over at 1x .. 8x the CUs measured, 2x .. 4x best by ~1 %: workgroups beyond
    //  the CUs queue up behind the first round; from 6x on the persistent kernel loses to the batched sweeps)
    persist_at_ = sw_.persist_at.set ? sw_.persist_at.v : 2 * num_cus_;
    fwd_single_at_ = 2 * num_cus_;  // (measured 1x .. 8x the CUs: config 3 -1.2 % at 2x, config 2 indifferent)
    return ReserveCounters(1024);
  }
  // one counter per sweep (device: filled by the forward kernel's atomics; host: pinned + mapped,
  // written by the next sweep's first kernel), so no memset / copy sits between the sweeps
  altro_status ReserveCounters(int count) {
    if ((size_t)count <= hm_.d_counter.count()) return ALTRO_OK;
    hm_.d_counter.reset();
    ALTRO_HIP_CHECK(hm_.h_counter.alloc((size_t)count));
    ALTRO_HIP_CHECK(hipHostGetDevicePointer((void**)&h_counter_dev_, (void*)hm_.h_counter.get(), 0));
    ALTRO_HIP_CHECK(hm_.d_counter.alloc((size_t)count));
    return ALTRO_OK;
  }

  // ---- problem upload -------------------------------------------------------------------------
  altro_status Upload(const ProblemSpec& spec, std::string* err) override {
    altro_status st;
    if (uploaded_) {
      err_ = "problem definition changed after the device state was created; create a new handle";
      st = ALTRO_NOT_READY;
    } else {
      st = UploadImpl(spec);
      // EVERY failed upload -- a rejected argument, a failed allocation, a HIP error half-way -- leaves the engine as it
      // was before it: buffers, chain streams and the chain booking of the partial upload go, so that the retry neither
      // leaks them nor meets its own ChainClaim
      if (st != ALTRO_OK) DropUpload();
    }
    return Report(st, err);
  }
  altro_status Report(altro_status st, std::string* err) const {  // the error text of a failed call into the caller's string
    if (st != ALTRO_OK && err) *err = err_;
    return st;
  }
  altro_status SetInitialState(const ProblemSpec& spec, std::string* err) override {
    ctg_replayable_ = false;  // (what a replayed backward pass would read no longer belongs to the last whole solve: ADVICE r5)
    return Report(SetInitialStateImpl(spec), err);
  }
  altro_status SetTrajectory(const ProblemSpec& spec, std::string* err) override {
    ctg_replayable_ = false;
    return Report(SetTrajectoryImpl(spec), err);
  }

  // The integration step belongs to the trajectory (trajectory.hpp:122-130), which the caller may replace
  // between solves: it can be set at any time, and the calls that integrate refuse to run without it.
  altro_status SetStep(float hstep) override {
    if (!uploaded_) return ALTRO_OK;  // Upload takes it from the spec
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    pd_.hstep = hstep;
    ALTRO_HIP_CHECK(CopySync(up_.d_pd, &pd_, sizeof(pd_), hipMemcpyHostToDevice));
    return ALTRO_OK;
  }
  // Trajectory::SetStep(k, h) / SetTime(k, t) (trajectory.hpp:119-120) and time-varying user models
  // (ContinuousDynamics::Evaluate(x, u, t, xdot), dynamics.hpp:59-95).  The hot kernels are built around one step for the
  // whole horizon (ProblemDesc::hstep: a loop invariant of the rollout wave, of the fused RK4 and of the persistent
  // kernel); a trajectory with its own steps or a model that reads the time takes the general path instead -- the
  // expansions / initial rollout read h[k], t[k] per knot, the forward pass runs on k_forward (one wave per three
  // instances, inputs from global memory) and the persistent tail kernel is not used.  Same schedule, same results as
  // the oracle (tests/test_knot_times_gpu.py); slower per iteration.
  altro_status SetKnotTimes(const ProblemSpec& s, std::string* err) override { return Report(SetKnotTimesImpl(s), err); }
  altro_status SetKnotTimesImpl(const ProblemSpec& s) {
    if (!uploaded_) return ALTRO_OK;  // Upload takes them from the spec
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    const bool per_knot = !s.hk.empty() || kTimeVarying;
    // (a time-varying model whose trajectory has no step yet -- the facade uploads the problem before it hands the
    //  trajectory over -- stays without knot times: StepOk() refuses every integrating call until altro_set_uniform_step /
    //  altro_set_steps come, and both end up here again)
    if (!per_knot || (s.hk.empty() && !(s.hstep > 0.0f))) {
      A_.hk = nullptr;
      A_.tk = nullptr;
      return ALTRO_OK;
    }
    std::vector<float> hk(N_ + 1, 0.0f), tk(N_ + 1, 0.0f);
    for (int k = 0; k < N_; ++k) hk[k] = s.hk.empty() ? s.hstep : s.hk[k];
    if (!s.tk.empty()) {
      for (int k = 0; k <= N_; ++k) tk[k] = s.tk[k];
    } else if (s.hk.empty()) {  // SetUniformStep (trajectory.hpp:122-130)
      for (int k = 0; k < N_; ++k) tk[k] = static_cast<float>(k) * s.hstep;
      tk[N_] = s.hstep * N_;
    }  // (steps without times: the times stay zero, as Trajectory::SetStep leaves them)
    for (int k = 0; k < N_; ++k)
      if (!(hk[k] > 0.0f)) {
        err_ = "the integration step of knot " + std::to_string(k) + " is not set (Trajectory::SetStep / SetUniformStep)";
        return ALTRO_NOT_READY;
      }
    if (!up_.d_hk) {
      ALTRO_TRY(Alloc(&up_.d_hk, (size_t)N_ + 1));
      ALTRO_TRY(Alloc(&up_.d_tk, (size_t)N_ + 1));
    }
    ALTRO_HIP_CHECK(CopySync(up_.d_hk, hk.data(), hk.size() * sizeof(float), hipMemcpyHostToDevice));
    ALTRO_HIP_CHECK(CopySync(up_.d_tk, tk.data(), tk.size() * sizeof(float), hipMemcpyHostToDevice));
    A_.hk = up_.d_hk;
    A_.tk = up_.d_tk;
    return ALTRO_OK;
  }
  altro_status ResetTrajectory() override {
    ctg_replayable_ = false;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_HIP_CHECK(hipMemcpyAsync(A_.X, up_.X_init, (size_t)(N_ + 1) * R::nP * Bp_ * sizeof(T), hipMemcpyDeviceToDevice, stream_));
    ALTRO_HIP_CHECK(hipMemcpyAsync(A_.U, up_.U_init, (size_t)N_ * R::mP * Bp_ * sizeof(T), hipMemcpyDeviceToDevice, stream_));
    return ALTRO_OK;
  }
  altro_status ResetStats() override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    hipLaunchKernelGGL(k_reset_stats<T>, GridB(), dim3(kBlock), 0, stream_, A_);
    return ALTRO_OK;
  }
  altro_status SetPenalty(double rho) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    hipLaunchKernelGGL(k_set_rows<T>, GridB(), dim3(kBlock), 0, stream_, A_, up_.d_pd, 0, 1, T(rho));
    return Sync();
  }
  altro_status SetPenaltyScaling(double phi) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    std::vector<double> v(kMaxClasses * kMaxConPerKnot, phi);
    ALTRO_HIP_CHECK(CopySync(up_.d_phi, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    return ALTRO_OK;
  }

  // ---- solves -----------------------------------------------------------------------------------
  altro_status SolveAL(const altro_options& o) override { return Solve(o, kFwdAL); }
  altro_status SolveILQR(const altro_options& o) override { return Solve(o, kFwdILQR); }

  altro_status AlInit(const altro_options& o) override {
    if (!RefOk()) return ALTRO_NOT_READY;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    const DevOpts d = ToDevOpts(o);
    hipLaunchKernelGGL(k_al_init<T>, GridAlInit(), dim3(kBlock), 0, stream_, A_, up_.d_pd, d);
    LaunchKnotCosts();
    hipLaunchKernelGGL(k_log_viol_pen<T>, GridB(), dim3(kBlock), 0, stream_, A_, up_.d_pd);
    return Sync();
  }
  altro_status SolveSetup(const altro_options& o) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    hipLaunchKernelGGL(k_solve_setup<T>, GridB(), dim3(kBlock), 0, stream_, A_, ToDevOpts(o), 0);
    return Sync();
  }
  altro_status Rollout(const altro_options&) override {
    if (!StepOk()) return ALTRO_NOT_READY;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    hipLaunchKernelGGL((k_rollout<T, M>), GridB(), dim3(kBlock), 0, stream_, A_, up_.d_pd, 1);
    return Sync();
  }
  altro_status Cost(const altro_options&, double* J) override {
    if (!RefOk()) return ALTRO_NOT_READY;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    LaunchKnotCosts();
    hipLaunchKernelGGL(k_sum_costs<T>, GridB(), dim3(kBlock), 0, stream_, A_, up_.d_tmp);
    ALTRO_TRY(Sync());
    if (J) return DownloadVec(up_.d_tmp, J);
    return ALTRO_OK;
  }
  altro_status UpdateExpansions(const altro_options&) override {
    ctg_replayable_ = false;  // (the records a replayed backward pass would read are about to change)
    if (!StepOk() || !RefOk()) return ALTRO_NOT_READY;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    if (KnotRouted(A_))
      hipLaunchKernelGGL((k_expansions_trk<T, M>), GridBK(), dim3(kBlock), 0, stream_, A_, up_.d_pd, 1, (int*)nullptr, (int*)nullptr);
    else
      hipLaunchKernelGGL((k_expansions<T, M>), GridBK(), dim3(kBlock), 0, stream_, A_, up_.d_pd, 1, (int*)nullptr, (int*)nullptr);
    return Sync();
  }
  altro_status BackwardPass(const altro_options& o) override {
    cur_ = stream_;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    LaunchBackward(A_, ToDevOpts(o), 1, B_);
    ctg_fresh_ = A_.record_ctg != 0;
    ctg_replayable_ = false;
    return Sync();
  }
  // the backward pass of the last iteration of a whole solve, once more, with the cost-to-go records on (see GetCtg)
  altro_status ReplayCtg() {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    // the per-instance scalars as the solve left them (both blocks go behind the synchronisation below)
    DevBlock<double> tmpT;
    DevBlock<int> tmpI;
    const size_t nT = (size_t)kNumScalarT * Bp_ * sizeof(double), nI = (size_t)kNumScalarI * Bp_ * sizeof(int);
    ALTRO_HIP_CHECK(tmpT.alloc((size_t)kNumScalarT * Bp_));
    if (tmpI.alloc((size_t)kNumScalarI * Bp_) != hipSuccess) {
      err_ = "ReplayCtg: out of device memory";
      return ALTRO_HIP_ERROR;
    }
    hipError_t e = hipMemcpyAsync(tmpT.get(), up_.d_scalarT, nT, hipMemcpyDeviceToDevice, stream_);
    if (e == hipSuccess) e = hipMemcpyAsync(tmpI.get(), up_.d_scalarI, nI, hipMemcpyDeviceToDevice, stream_);
    // the regularisation the last backward pass used (stats_.Log("reg", rho_)) is what this one starts from
    if (e == hipSuccess) e = hipMemcpyAsync(A_.rho_reg, A_.reg_log, (size_t)Bp_ * sizeof(double), hipMemcpyDeviceToDevice, stream_);
    if (e == hipSuccess) {
      DevArrays<T> A = A_;
      A.record_ctg = 1;
      cur_ = stream_;
      LaunchBackward(A, last_opts_, 1, B_);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(up_.d_scalarT, tmpT.get(), nT, hipMemcpyDeviceToDevice, stream_);
    if (e == hipSuccess) e = hipMemcpyAsync(up_.d_scalarI, tmpI.get(), nI, hipMemcpyDeviceToDevice, stream_);
    const hipError_t es = hipStreamSynchronize(stream_);  // (also after a failure: the blocks must not go under a copy in flight)
    ALTRO_HIP_CHECK(e);
    ALTRO_HIP_CHECK(es);
    ctg_fresh_ = true;
    return ALTRO_OK;
  }
  altro_status ForwardPass(const altro_options& o) override {
    cur_ = stream_;
    ctg_replayable_ = false;  // (a step-level forward pass moves the trajectory)
    if (!StepOk() || !RefOk()) return ALTRO_NOT_READY;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    LaunchForward(A_, ToDevOpts(o), (int)kFwdStepOnly, 1, B_);
    return Sync();
  }
  altro_status UpdateConvergenceStatistics(const altro_options& o) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    hipLaunchKernelGGL((k_conv_stats<T, M>), GridB(), dim3(kBlock), 0, stream_, A_, up_.d_pd, ToDevOpts(o));
    return Sync();
  }
  altro_status UpdateDuals(const altro_options&) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    hipLaunchKernelGGL(k_update_duals<T>, GridB(), dim3(kBlock), 0, stream_, A_, up_.d_pd);
    return Sync();
  }
  altro_status UpdatePenalties(const altro_options&) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    hipLaunchKernelGGL(k_update_penalties<T>, GridB(), dim3(kBlock), 0, stream_, A_, up_.d_pd);
    return Sync();
  }
  altro_status GetMaxViolation(double* out) override { return MaxViolPen(up_.d_tmp, nullptr, out); }
  altro_status GetMaxPenalty(double* out) override { return MaxViolPen(nullptr, up_.d_tmp, out); }
  altro_status MaxViolPen(double* viol, double* pen, double* out) {  // (one of the two is up_.d_tmp, the other null)
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    hipLaunchKernelGGL(k_max_viol_pen<T>, GridB(), dim3(kBlock), 0, stream_, A_, up_.d_pd, viol, pen);
    ALTRO_TRY(Sync());
    return DownloadVec(up_.d_tmp, out);
  }

  // ---- results ----------------------------------------------------------------------------------
  altro_status GetTrajectory(double* X, double* U) override {
    if (X) ALTRO_TRY(DownloadRec(A_.X, N_ + 1, R::nP, 0, n, X));
    if (U) return DownloadRec(A_.U, N_, R::mP, 0, m, U);
    return ALTRO_OK;
  }
  altro_status GetGains(double* K, double* d) override {
    if (K) ALTRO_TRY(DownloadRec((const RS*)A_.KD, N_, RR::KP, RR::oK, m * n, K));
    if (d) return DownloadRec((const RS*)A_.KD, N_, RR::KP, RR::oD, m, d);
    return ALTRO_OK;
  }
  altro_status SetRecordCtg(int enable) override {
    A_.record_ctg = enable ? 1 : 0;
    return ALTRO_OK;
  }
  // KnotPointFunctions::GetCostToGoHessian / Gradient (knot_point_function_type.hpp:243-268): P, p of the LAST backward
  // pass.  The solve itself keeps them in registers unless altro_set_record_ctg asked for the records (the persistent kernel
  // never stores them).  The reference's stay readable after Solve(); here a read behind a solve that did not record runs
  // that backward pass ONCE MORE with the recording on -- the expansions of the last iteration are still in memory, the
  // regularisation it used is logged (reg_log) -- and puts the solver state back (ReplayCtg): same kernels on the same
  // inputs, the same P, p.
  altro_status GetCtg(double* P, double* p) override {
    if (!ctg_fresh_) {
      if (!ctg_replayable_) {
        err_ = "no cost-to-go to read: it belongs to a backward pass -- altro_solve_*, or altro_backward_pass after "
               "altro_set_record_ctg(h, 1) -- and the trajectory or the expansions have changed since the last one";
        return ALTRO_NOT_READY;
      }
      ALTRO_TRY(ReplayCtg());
    }
    if (P) ALTRO_TRY(DownloadRec(A_.CTG, N_ + 1, R::CP, R::oP, n * n, P));
    if (p) return DownloadRec(A_.CTG, N_ + 1, R::CP, R::op, n, p);
    return ALTRO_OK;
  }
  altro_status GetExpansion(int k, double* AB, double* lxx, double* lxu, double* luu, double* lx,
                            double* lu) override {
    if (k < 0 || k > N_) return ALTRO_INVALID_ARG;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    std::vector<RS> h((size_t)RR::EP * Bp_);
    ALTRO_HIP_CHECK(CopySync(h.data(), (const RS*)A_.EXP + (size_t)k * Bp_ * RR::EP, h.size() * sizeof(RS), hipMemcpyDeviceToHost));
    auto take = [&](double* out, int off, int E, bool stage_only) {
      if (!out || (stage_only && k >= N_)) return;
      for (int b = 0; b < B_; ++b)
        for (int e = 0; e < E; ++e) out[(size_t)b * E + e] = (double)h[(size_t)b * RR::EP + off + e];
    };
    take(AB, R::oAB, n * nm, true);
    take(lxx, R::oLxx, n * n, false);
    take(lxu, R::oLxu, n * m, true);
    take(luu, R::oLuu, m * m, true);
    take(lx, R::oLx, n, false);
    take(lu, R::oLu, m, true);
    return ALTRO_OK;
  }
  altro_status GetKnotCosts(double* costs) override { return DownloadRec(A_.costs, N_ + 1, 1, 0, 1, costs); }
  int NumRows() override { return pd_.total_rows; }
  int NumRowsAt(int k) override {
    if (k < 0 || k > N_) return -1;
    return pd_.cls[knot_class_[k]].nrows;
  }
  altro_status GetRows(int which, double* out) override {
    T* src = which == 0 ? A_.lam : (which == 1 ? A_.pen : A_.cval);
    const int R = pd_.total_rows;
    if (R == 0) return ALTRO_OK;
    std::vector<T> h((size_t)R * Bp_);
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    ALTRO_HIP_CHECK(CopySync(h.data(), src, h.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (int b = 0; b < B_; ++b)
      for (int r = 0; r < R; ++r) out[(size_t)b * R + r] = (double)h[(size_t)r * Bp_ + b];
    return ALTRO_OK;
  }
  altro_status SetDuals(const double* lam) override { return UploadRows(A_.lam, lam); }
  altro_status GetStats(altro_stats* st, bool ilqr_mode) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    std::vector<double> f((size_t)kNumScalarT * Bp_);
    std::vector<int> iv((size_t)kNumScalarI * Bp_);
    ALTRO_HIP_CHECK(CopySync(f.data(), up_.d_scalarT, f.size() * sizeof(double), hipMemcpyDeviceToHost));
    ALTRO_HIP_CHECK(CopySync(iv.data(), up_.d_scalarI, iv.size() * sizeof(int), hipMemcpyDeviceToHost));
    auto F = [&](double* p, int b) { return f[(size_t)(p - up_.d_scalarT) + b]; };
    auto I = [&](int* p, int b) { return iv[(size_t)(p - up_.d_scalarI) + b]; };
    for (int b = 0; b < B_; ++b) {
      altro_stats& s = st[b];
      s.status_ilqr = I(A_.status, b);
      s.status = ilqr_mode ? s.status_ilqr : I(A_.status_al, b);
      s.iterations_inner = I(A_.it_inner, b);
      s.iterations_outer = I(A_.it_outer, b);
      s.iterations_total = I(A_.it_total, b);
      s.reserved = 0;
      s.cost = F(A_.cost_cur, b);
      s.initial_cost = F(A_.initial_cost, b);
      s.cost_decrease = F(A_.dJ, b);
      s.gradient = F(A_.grad, b);
      s.violation = F(A_.viol, b);
      s.max_penalty = F(A_.penmax, b);
      s.alpha = F(A_.alpha, b);
      s.regularization = F(A_.reg_log, b);
      s.improvement_ratio = F(A_.z, b);
    }
    return ALTRO_OK;
  }
  altro_status GetTiming(altro_timing* t) override {
    if (timing_.instance_iterations < 0 && uploaded_) {
      ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
      ALTRO_TRY(SumInstanceIterations());
    }
    *t = timing_;
    return ALTRO_OK;
  }
  altro_status SetRecordHistory(int capacity) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    hm_.hist.reset();
    hm_.hist_len.reset();
    A_.hist = nullptr;
    A_.hist_len = nullptr;
    A_.hist_cap = 0;
    if (capacity > 0) {
      ALTRO_HIP_CHECK(hm_.hist.alloc((size_t)kHistFields * capacity * Bp_));
      ALTRO_HIP_CHECK(hm_.hist_len.alloc((size_t)Bp_));
      ALTRO_HIP_CHECK(ZeroSync(hm_.hist_len.get(), 0, (size_t)Bp_ * sizeof(int)));
      A_.hist = hm_.hist.get();
      A_.hist_len = hm_.hist_len.get();
      A_.hist_cap = capacity;
    }
    return ALTRO_OK;
  }
  int GetHistory(int instance, int field, double* out, int cap) override {
    if (!A_.hist || instance < 0 || instance >= B_ || field < 0 || field >= kHistFields) return -1;
    if (hipSetDevice(desc_.device_id) != hipSuccess) return -1;
    if (hipStreamSynchronize(stream_) != hipSuccess) return -1;
    int len = 0;
    if (CopySync(&len, A_.hist_len + instance, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    // the reference's vectors also hold the row opened by the last NewIteration: a copy of the last
    const int cnt = std::min(std::min(len, A_.hist_cap), cap);
    if (cnt <= 0) return 0;
    // column `instance` of the [field][row][Bp] block: one strided copy
    if (hipMemcpy2DAsync(out, sizeof(double), A_.hist + (size_t)field * A_.hist_cap * Bp_ + instance, (size_t)Bp_ * sizeof(double),
                         sizeof(double), (size_t)cnt, hipMemcpyDeviceToHost, stream_) != hipSuccess ||
        hipStreamSynchronize(stream_) != hipSuccess)
      return -1;
    return cnt;
  }
  // every field of one instance's history at once: one synchronisation in front, the eight column copies enqueued back
  // to back, one synchronisation behind (the per-field call costs three per field)
  int GetHistoryAll(int instance, double* out, int cap) override {
    if (!A_.hist || instance < 0 || instance >= B_ || cap <= 0) return -1;
    if (hipSetDevice(desc_.device_id) != hipSuccess) return -1;
    int len = 0;
    if (CopySync(&len, A_.hist_len + instance, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const int cnt = std::min(std::min(len, A_.hist_cap), cap);
    if (cnt <= 0) return 0;
    for (int f = 0; f < kHistFields; ++f)
      if (hipMemcpy2DAsync(out + (size_t)f * cap, sizeof(double), A_.hist + (size_t)f * A_.hist_cap * Bp_ + instance,
                           (size_t)Bp_ * sizeof(double), sizeof(double), (size_t)cnt, hipMemcpyDeviceToHost, stream_) != hipSuccess)
        return -1;
    if (hipStreamSynchronize(stream_) != hipSuccess) return -1;
    return cnt;
  }
  altro_status DeviceInfo(char* name, int name_len, int* cu_count) override {
    hipDeviceProp_t p;
    ALTRO_HIP_CHECK(hipGetDeviceProperties(&p, desc_.device_id));
    if (name && name_len > 0) {
      std::strncpy(name, p.name, name_len - 1);
      name[name_len - 1] = 0;
    }
    if (cu_count) *cu_count = p.multiProcessorCount;
    return ALTRO_OK;
  }
  altro_status PackResultsDevice(void* dst) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    hipLaunchKernelGGL(k_pack_results<T>, GridB(), dim3(kBlock), 0, stream_, A_, (double*)dst, last_mode_ilqr_ ? 1 : 0);
    return Sync();
  }
  // records [knots][Bp][nP] -> the caller's rows [B][knots][n] straight into the caller's DEVICE buffers
  altro_status PackTrajectoryDevice(double* X, double* U) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    if (X)
      hipLaunchKernelGGL((k_rec_to_rows<T>), dim3((B_ + kBlock - 1) / kBlock, N_ + 1), dim3(kBlock), 0, stream_, (const T*)A_.X, X,
                         N_ + 1, R::nP, 0, n, B_, Bp_);
    if (U)
      hipLaunchKernelGGL((k_rec_to_rows<T>), dim3((B_ + kBlock - 1) / kBlock, N_), dim3(kBlock), 0, stream_, (const T*)A_.U, U, N_,
                         R::mP, 0, m, B_, Bp_);
    return Sync();
  }

  // ---- the reference path of the tracking costs (include/altro_tracking.h: altro_set_reference) ---------------------
  // The path lives on the device (Uploaded::refpath, one column or B of them); every change of path or window ends in ONE launch
  // of k_ref_terms on the engine's stream, which rewrites the term records the cost kernels read (DevArrays::ref).  A handle
  // without a tracking cost keeps the path and the offset it is given and launches nothing.
  altro_status SetReference(const double* Xref, const double* Uref, int rows, int per_instance, int on_device) override {
    if (!Xref || rows < 1) {
      err_ = "altro_set_reference: the path needs Xref and at least one row";
      return ALTRO_INVALID_ARG;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    ctg_replayable_ = false;  // (as SetTrajectory: what a replayed backward pass would read belongs to the old reference)
    const int cols = per_instance ? B_ : 1;
    const size_t need = (size_t)rows * cols * kRefPT;
    if (need > up_.refpath.count()) ALTRO_HIP_CHECK(up_.refpath.alloc(need));
    StagedCall<2> c(this, ReferenceStageParts(n, m, (size_t)rows * cols, Uref != nullptr), on_device, "altro_set_reference", kEngineBlock);
    ALTRO_TRY(c.Refused());
    const double *Xd = c.sg.in(0, Xref), *Ud = c.sg.in(1, Uref);
    hipLaunchKernelGGL((k_ref_pack<n, m>), dim3((cols + kBlock - 1) / kBlock, rows), dim3(kBlock), 0, stream_, Xd, Ud, up_.refpath.get(), rows,
                       cols);
    up_.ref_rows = rows;
    up_.ref_cols = cols;
    up_.ref_offset = 0;
    LaunchRefTerms();
    return c.Finish();
  }
  altro_status SetReferenceOffset(int offset) override {
    if (offset < 0) {
      err_ = "altro_set_reference_offset: the offset must not be negative";
      return ALTRO_INVALID_ARG;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ctg_replayable_ = false;
    up_.ref_offset = offset;
    LaunchRefTerms();
    return Sync();
  }
  int GetReferenceOffset() override { return up_.ref_offset; }
  altro_status GetReferenceTerms(double* q, double* r, double* c) override {
    if (!A_.ref) {  // no tracking cost: every knot reads zero
      const size_t BK = (size_t)B_ * (N_ + 1);
      if (q) std::fill(q, q + BK * n, 0.0);
      if (r) std::fill(r, r + BK * m, 0.0);
      if (c) std::fill(c, c + BK, 0.0);
      return ALTRO_OK;
    }
    if (q) ALTRO_TRY(DownloadRec(A_.ref, N_ + 1, kRefRT, 0, n, q));
    if (r) ALTRO_TRY(DownloadRec(A_.ref, N_ + 1, kRefRT, n, m, r));
    if (c) ALTRO_TRY(DownloadRec(A_.ref, N_ + 1, kRefRT, n + m, 1, c));
    return ALTRO_OK;
  }
  // the per-knot costs of the step-level calls (k_knot_costs; its twin on a handle with a tracking cost)
  void LaunchKnotCosts() {
    if (KnotRouted(A_))
      hipLaunchKernelGGL((k_knot_costs_trk<T, M>), GridBK(), dim3(kBlock), 0, stream_, A_, up_.d_pd);
    else
      hipLaunchKernelGGL((k_knot_costs<T, M>), GridBK(), dim3(kBlock), 0, stream_, A_, up_.d_pd);
  }
  // the term records of the current path and window (nothing to do without a tracking cost or without a path)
  void LaunchRefTerms() {
    if (!A_.ref || up_.ref_rows < 1) return;
    hipLaunchKernelGGL((k_ref_terms<T, n, m>), GridBK(), dim3(kBlock), 0, stream_, A_, up_.d_pd, (const double*)up_.refpath.get(), up_.d_ref, up_.ref_rows,
                       up_.ref_cols, up_.ref_offset);
  }
  // a cost evaluation on a handle with a tracking cost needs the path
  bool RefOk() {
    for (const KnotCon& c : up_.kcons)
      if (c.rows < 1) {
        err_ = "constraint " + std::to_string(c.index) + " is a knot constraint but has no parameter track (altro_set_constraint_track)";
        return false;
      }
    if (!A_.ref || up_.ref_rows > 0) return true;
    err_ = "a knot has a tracking cost but no reference path is set (altro_set_reference)";
    return false;
  }
  // a handle whose cost kernels must know their knot: a tracking cost or a knot constraint (either record may be missing).
  // It runs the *_trk twins of the general kernels, and neither the persistent kernel nor segments (FusedOk, PlanRun).
  static bool KnotRouted(const DevArrays<T>& A) { return A.ref != nullptr || A.kpar != nullptr; }

  // ---- the parameter tracks of the knot constraints (include/altro_knot_params.h) -----------------------------------------
  // Every knot constraint owns a track on the device, in the caller's layout ([rows][np], or [B][rows][np]); every change of a
  // track or of the window ends in ONE launch of k_knot_params on the engine's stream, which rewrites the records the cost
  // kernels read (DevArrays::kpar).
  struct KnotCon {
    int index, k_begin, k_end, np, off, kind;  // registration index; knots; parameters; element in the record; kind
    DevBlock<double> track;  // (count(): its capacity; rows x cols x np of it are the track)
    int rows = 0, cols = 0;
    // a track written by altro_team_fill_tracks (include/altro_team.h): row 0 belongs to window offset `base` (0 for every
    // track a caller set), `team` marks it, and the fill writes into the spare buffer and swaps
    int base = 0;
    bool team = false;
    DevBlock<double> spare;
  };
  KnotCon* FindKnotCon(int index, const char* who) {
    for (KnotCon& c : up_.kcons)
      if (c.index == index) return &c;
    err_ = std::string(who) + ": constraint " + std::to_string(index) + " is not a knot constraint (altro_add_knot_constraint)";
    return nullptr;
  }
  altro_status SetConstraintTrack(int index, const double* P, int rows, int per_instance, int on_device) override {
    KnotCon* c = FindKnotCon(index, "altro_set_constraint_track");
    if (!c) return ALTRO_INVALID_ARG;
    if (!P || rows < 1) {
      err_ = "altro_set_constraint_track: the track needs at least one row";
      return ALTRO_INVALID_ARG;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    ctg_replayable_ = false;  // (as SetTrajectory: what a replayed backward pass would read belongs to the old parameters)
    const int cols = per_instance ? B_ : 1;
    const size_t need = (size_t)rows * cols * c->np;
    if (need > c->track.count()) {
      c->rows = 0;
      ALTRO_HIP_CHECK(c->track.alloc(need));
    }
    ALTRO_HIP_CHECK(hipMemcpyAsync(c->track.get(), P, need * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream_));
    c->rows = rows;
    c->cols = cols;
    c->base = 0;
    c->team = false;
    LaunchKnotParams();
    return Sync();
  }
  altro_status SetTrackOffset(int offset) override {
    if (offset < 0) {
      err_ = "altro_set_track_offset: the offset must not be negative";
      return ALTRO_INVALID_ARG;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ctg_replayable_ = false;
    up_.track_offset = offset;
    LaunchKnotParams();
    return Sync();
  }
  int GetTrackOffset() override { return up_.track_offset; }
  altro_status GetKnotParams(int index, double* out) override {
    KnotCon* c = FindKnotCon(index, "altro_get_knot_params");
    if (!c || !out) return ALTRO_INVALID_ARG;
    return DownloadRec(A_.kpar + (size_t)c->k_begin * Bp_ * A_.kpar_kt, c->k_end - c->k_begin, A_.kpar_kt, c->off, c->np, out);
  }
  // the records of the current tracks and window (nothing to do without a knot constraint)
  void LaunchKnotParams() {
    if (!A_.kpar) return;
    KnotParArgs g{};
    g.ncon = (int)up_.kcons.size();
    g.kt = A_.kpar_kt;
    g.offset = up_.track_offset;
    for (int j = 0; j < g.ncon; ++j) {
      const KnotCon& c = up_.kcons[j];
      g.c[j] = KnotTrack{c.rows > 0 ? c.track.get() : nullptr, c.k_begin, c.k_end, c.np, c.off, c.rows, c.cols, c.base};
    }
    hipLaunchKernelGGL((k_knot_params<0>), GridBK(), dim3(kBlock), 0, stream_, g, up_.d_kpar, B_, Bp_);
  }

  // ---- receding-horizon advance (include/altro_mpc.h) ----------------------------------------------
  // One launch (k_mpc_advance) on the engine's stream; the row map of a shift is built once and stays on the device.
  // Model-independent: the kernel never calls the dynamics.  Expansions, knot costs, stored constraint values and cost-to-go
  // records stay where they are -- the next solve recomputes them -- so what a cost-to-go replay would read is gone.
  altro_status MpcAdvance(int shift, const double* x0, const double* w, int on_device, double reset_pen) override {
    return Advance(shift, x0, w, on_device, reset_pen, nullptr);
  }
  // where the advance of one cycle of a closed-loop run logs what the loop applied (LoopRun); a plain advance has none
  struct LogSlot {
    double *X, *U;
    int *it, *st;
    int cycle, cycles;
  };
  altro_status Advance(int shift, const double* x0, const double* w, int on_device, double reset_pen, const LogSlot* log) {
    if (shift < 1 || shift > N_ - 1) {
      err_ = "altro_mpc_advance: the shift must lie in [1, N - 1]";
      return ALTRO_INVALID_ARG;
    }
    if (kTimeVarying || A_.hk || A_.knot_model) {
      err_ = "altro_mpc_advance: per-knot steps, times or models (a time-varying or discrete user model included) do not move "
             "along the horizon yet";
      return ALTRO_UNSUPPORTED;
    }
    constexpr int kdv = RR::KP * (int)sizeof(RS) / 16, xv = R::nP * (int)sizeof(T) / 16, uv = R::mP * (int)sizeof(T) / 16;
    constexpr int widest = kdv > xv ? (kdv > uv ? kdv : uv) : (xv > uv ? xv : uv);
    static_assert(widest <= kMpcThreads * kMpcItems, "one record must fit a chunk of k_mpc_advance");
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ctg_replayable_ = false;
    ctg_fresh_ = false;
    const int* map = nullptr;
    ALTRO_TRY(MpcMap(shift, &map));
    MpcArgs g{};
    g.shift = shift;
    // columns per workgroup: one for a small batch (its knots spread over the lanes), up to 64 for a large one (the lanes
    // run along the records of neighbouring columns); never more than one chunk of the widest record holds
    g.tile = 1;
    while (g.tile < 64 && g.tile * 128 < B_ && 2 * g.tile * widest <= kMpcThreads * kMpcItems) g.tile *= 2;
    g.n = n;
    g.m = m;
    g.kd_vecs = kdv;
    g.rows = pd_.total_rows;
    g.row_src = map;
    g.reset_pen = reset_pen;
    StagedCall<2> c(this, AdvanceStageParts(n, (size_t)B_, x0 != nullptr, w != nullptr), on_device, "altro_mpc_advance", kEngineBlock);
    ALTRO_TRY(c.Refused());
    g.x0 = c.sg.in(0, x0);
    g.w = c.sg.in(1, w);
    if (log) {
      g.Xlog = log->X;
      g.Ulog = log->U;
      g.itlog = log->it;
      g.stlog = log->st;
      g.cycle = log->cycle;
      g.cycles = log->cycles;
    }
    hipLaunchKernelGGL(k_mpc_advance<T>, dim3((B_ + g.tile - 1) / g.tile, 5), dim3(kMpcThreads), 0, stream_, A_, g);
    if (A_.ref) {  // the window of a tracking cost's reference moves with the horizon (the end of the path is held)
      up_.ref_offset = (int)std::min<long long>((long long)up_.ref_offset + shift, 0x7fffffffLL);
      LaunchRefTerms();
    }
    if (A_.kpar) {  // ... and so does the window of the knot constraints' tracks (the last row is held)
      up_.track_offset = (int)std::min<long long>((long long)up_.track_offset + shift, 0x7fffffffLL);
      LaunchKnotParams();
    }
    return c.Finish();
  }
  // ---- multi-start (include/altro_multistart.h) -----------------------------------------------------
  // G adjacent columns are the starts of one problem.  Everything runs on the engine's stream; the winners live in a device
  // array of the engine (hm_.ms_win) unless the caller brings device memory for them.  The C API has checked G against the batch.
  altro_status MsCheck(int G) {
    if (G < 1 || B_ % G != 0) {
      err_ = "multi-start: starts must be at least 1 and divide the batch";
      return ALTRO_INVALID_ARG;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    if (!hm_.ms_win) ALTRO_HIP_CHECK(hm_.ms_win.alloc((size_t)B_));
    return ALTRO_OK;
  }
  // k_ms_select into `win` (device, [P]); log: one more copy at log[p * stride + off]
  void LaunchMsSelect(int G, bool ilqr_mode, int* win, int* log, int stride, int off) {
    const int P = B_ / G;
    hipLaunchKernelGGL(k_ms_select<T>, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, stream_, A_, G, P, ilqr_mode ? 1 : 0, win, log,
                       stride, off);
  }
  // where the winners of this call go on the device, and their way back to a host caller
  int* MsWinDev(int* winner, int on_device) { return winner && on_device ? winner : hm_.ms_win.get(); }
  altro_status MsWinOut(int G, int* winner, int on_device) {
    ALTRO_TRY(Sync());
    if (winner && !on_device) ALTRO_HIP_CHECK(CopySync(winner, hm_.ms_win.get(), (size_t)(B_ / G) * sizeof(int), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  }
  altro_status MsSelect(int G, int* winner, int on_device, bool ilqr_mode) override {
    ALTRO_TRY(MsCheck(G));
    LaunchMsSelect(G, ilqr_mode, MsWinDev(winner, on_device), nullptr, 0, 0);
    return MsWinOut(G, winner, on_device);
  }
  void LaunchMsSpread(int G, const int* win) {
    static_assert(R::nP * sizeof(T) % 16 == 0 && R::mP * sizeof(T) % 16 == 0 && RR::KP * sizeof(RS) % 16 == 0,
                  "records are whole 16-byte units");
    MsSpreadArgs g{};
    g.G = G;
    g.B = B_;
    g.winner = win;
    g.rec[0] = reinterpret_cast<uint4*>(A_.X);
    g.rec[1] = reinterpret_cast<uint4*>(A_.U);
    g.rec[2] = reinterpret_cast<uint4*>(A_.KD);
    g.rec_knots[0] = N_ + 1;
    g.rec_knots[1] = N_;
    g.rec_knots[2] = N_;
    g.rec_vecs[0] = R::nP * (int)sizeof(T) / 16;
    g.rec_vecs[1] = R::mP * (int)sizeof(T) / 16;
    g.rec_vecs[2] = RR::KP * (int)sizeof(RS) / 16;
    g.rows = pd_.total_rows;
    g.knots1 = N_ + 1;
    // lanes for the largest of the seven arrays, capped: the kernel strides over what is left
    size_t most = (size_t)std::max(pd_.total_rows, N_ + 1) * B_;
    for (int j = 0; j < 3; ++j) most = std::max(most, (size_t)g.rec_knots[j] * g.rec_vecs[j] * B_);
    const unsigned gx = (unsigned)std::min<size_t>((most + kMsThreads - 1) / kMsThreads, (size_t)16 * std::max(num_cus_, 1));
    hipLaunchKernelGGL(k_ms_spread<T>, dim3(gx, 7), dim3(kMsThreads), 0, stream_, A_, g);
  }
  altro_status MsSpread(int G, int* winner, int on_device, bool ilqr_mode) override {
    ALTRO_TRY(MsCheck(G));
    ctg_replayable_ = false;  // (as SetTrajectory)
    int* win = MsWinDev(winner, on_device);
    LaunchMsSelect(G, ilqr_mode, win, nullptr, 0, 0);
    if (G > 1) LaunchMsSpread(G, win);
    return MsWinOut(G, winner, on_device);
  }
  void LaunchMsPerturb(int G, const double* dU_dev, int per_instance) {
    const size_t total = (size_t)N_ * B_ * (R::mP / 2);
    hipLaunchKernelGGL(k_ms_perturb<T>, dim3((unsigned)((total + kMsThreads - 1) / kMsThreads)), dim3(kMsThreads), 0, stream_, A_, dU_dev, G,
                       per_instance ? 1 : 0, m, R::mP);
  }
  altro_status MsPerturb(int G, const double* dU, int per_instance, int on_device) override {
    ALTRO_TRY(MsCheck(G));
    if (!dU) {
      err_ = "altro_multistart_perturb: dU is required";
      return ALTRO_INVALID_ARG;
    }
    ctg_replayable_ = false;
    StagedCall<1> c(this, PerturbStageParts(m, (size_t)(per_instance ? B_ : G), (size_t)N_), on_device, "altro_multistart_perturb", kEngineBlock);
    ALTRO_TRY(c.Refused());
    LaunchMsPerturb(G, c.sg.in(0, dU), per_instance);
    return c.Finish();
  }
  // U += sigma z with z drawn on the device (include/altro_ensemble.h): sigma [m] goes through the engine's staging block
  altro_status MsPerturbGaussian(int G, unsigned long long seed, unsigned long long instance_base, const double* sigma,
                                 int keep_first) override {
    ALTRO_TRY(MsCheck(G));
    if (!sigma) {
      err_ = "altro_multistart_perturb_gaussian: sigma is required";
      return ALTRO_INVALID_ARG;
    }
    ctg_replayable_ = false;
    StagedCall<1> c(this, GaussStageParts(m), 0, "altro_multistart_perturb_gaussian", kEngineBlock);
    ALTRO_TRY(c.Refused());
    const double* sd = c.sg.in(0, sigma);
    const size_t total = (size_t)N_ * B_ * (R::mP / 2);
    hipLaunchKernelGGL(k_ms_perturb_gauss<T>, dim3((unsigned)((total + kMsThreads - 1) / kMsThreads)), dim3(kMsThreads), 0, stream_, A_, sd, G,
                       keep_first ? 1 : 0, seed, instance_base, m, R::mP);
    return c.Finish();
  }
  // The winners' trajectories through k_rec_to_rows with the winner as the source column, their statistics through k_ms_stats.
  // A host caller's arrays are staged in ONE device block (X | U | stats) and come back with one copy each.
  altro_status MsGetBest(int G, double* X, double* U, altro_stats* stats, int* winner, int on_device, bool ilqr_mode) override {
    ALTRO_TRY(MsCheck(G));
    const int P = B_ / G;
    static_assert(sizeof(altro_stats) % sizeof(double) == 0, "altro_stats is a whole number of doubles");
    StagedCall<3> c(this, MsBestStageParts(n, m, (size_t)P, (size_t)N_, X != nullptr, U != nullptr, stats ? DoublesFor<altro_stats>(1) : 0),
                    on_device, "altro_multistart_get_best", kEngineBlock);
    ALTRO_TRY(c.Refused());
    double *dX = c.sg.out(0, X), *dU = c.sg.out(1, U);
    altro_stats* dS = c.sg.out(2, stats);
    int* win = MsWinDev(winner, on_device);
    LaunchMsSelect(G, ilqr_mode, win, nullptr, 0, 0);
    const dim3 gp((P + kBlock - 1) / kBlock);
    if (X)
      hipLaunchKernelGGL((k_rec_to_rows<T>), dim3(gp.x, N_ + 1), dim3(kBlock), 0, stream_, (const T*)A_.X, dX, N_ + 1, R::nP, 0, n, P, Bp_,
                         (const int*)win, G);
    if (U)
      hipLaunchKernelGGL((k_rec_to_rows<T>), dim3(gp.x, N_), dim3(kBlock), 0, stream_, (const T*)A_.U, dU, N_, R::mP, 0, m, P, Bp_,
                         (const int*)win, G);
    if (stats) hipLaunchKernelGGL(k_ms_stats<T>, gp, dim3(kBlock), 0, stream_, A_, (const int*)win, G, P, ilqr_mode ? 1 : 0, dS);
    ALTRO_TRY(c.Finish());  // (the one wait that MsWinOut would start with)
    if (winner && !on_device) ALTRO_HIP_CHECK(CopySync(winner, hm_.ms_win.get(), (size_t)P * sizeof(int), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  }

  // ---- teams (include/altro_team.h) -----------------------------------------------------------------
  // A adjacent columns are the agents of one team; the team's knot circle constraint gets its per-instance track from the
  // plans in X (k_team_tracks, into the constraint's spare buffer, then the two swap).  The radii live on the device, one per
  // instance, from TeamRadius on.  Everything runs on the engine's stream.  The C API has checked every argument it can.
  KnotCon* TeamCheck(int A, int index, const char* who) {
    if (A < 2 || B_ % A != 0) {
      err_ = std::string(who) + ": agents must be at least 2 and divide the batch";
      return nullptr;
    }
    KnotCon* c = FindKnotCon(index, who);
    if (!c) return nullptr;
    if (c->kind != ALTRO_CON_CIRCLE || c->np != 3 * (A - 1) || n < 2) {
      err_ = std::string(who) + ": constraint " + std::to_string(index) + " must be a knot circle constraint with 3 (agents - 1) parameters";
      return nullptr;
    }
    return c;
  }
  altro_status TeamRadius(const double* radius) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    if (!hm_.team_rad) ALTRO_HIP_CHECK(hm_.team_rad.alloc(2 * (size_t)B_));  // radii | clearances
    ALTRO_HIP_CHECK(CopySync(hm_.team_rad.get(), radius, (size_t)B_ * sizeof(double), hipMemcpyHostToDevice));
    return ALTRO_OK;
  }
  altro_status TeamFill(int A, int index, int mode, double blend) override {
    KnotCon* c = TeamCheck(A, index, "altro_team_fill_tracks");
    if (!c) return ALTRO_INVALID_ARG;
    if (!hm_.team_rad) {
      err_ = "altro_team_fill_tracks: no radii on the device yet";
      return ALTRO_NOT_READY;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    ctg_replayable_ = false;  // (as SetConstraintTrack)
    const int rows = N_ + 1;
    const size_t need = (size_t)B_ * rows * c->np;
    if (need > c->spare.count()) ALTRO_HIP_CHECK(c->spare.alloc(need));
    TeamFillArgs g{};
    g.out = c->spare.get();
    // a track last written by a team fill has this very shape; any other is replaced, not blended
    g.old = c->team && c->rows == rows && c->cols == B_ && blend != 1.0 ? c->track.get() : nullptr;
    g.radius = hm_.team_rad.get();
    g.A = A;
    g.B = B_;
    g.rows = rows;
    g.priority = mode == 1 ? 1 : 0;
    g.ahead = up_.track_offset > c->base ? up_.track_offset - c->base : 0;
    g.blend = blend;
    const size_t total = (size_t)B_ * rows * (A - 1);
    hipLaunchKernelGGL(k_team_tracks<T>, dim3((unsigned)((total + kTeamThreads - 1) / kTeamThreads)), dim3(kTeamThreads), 0, stream_,
                       (const T*)A_.X, R::nP, Bp_, g);
    AdoptSpare(c, rows, up_.track_offset, true);
    return Sync();
  }
  void LaunchTeamClearance(int A, const KnotCon& c, double* clear, int stride, int off) {
    const int teams = B_ / A, per_block = kTeamThreads / 64;
    hipLaunchKernelGGL(k_team_clearance<T>, dim3((teams + per_block - 1) / per_block), dim3(kTeamThreads), 0, stream_, (const T*)A_.X,
                       R::nP, Bp_, (const double*)hm_.team_rad.get(), A, teams, c.k_begin, c.k_end, clear, stride, off);
  }
  altro_status TeamClearance(int A, int index, double* clear, int on_device) override {
    KnotCon* c = TeamCheck(A, index, "altro_team_clearance");
    if (!c || !hm_.team_rad || !clear) return ALTRO_INVALID_ARG;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    double* dst = on_device ? clear : hm_.team_rad.get() + B_;
    LaunchTeamClearance(A, *c, dst, 1, 0);
    ALTRO_TRY(Sync());
    if (!on_device) ALTRO_HIP_CHECK(CopySync(clear, dst, (size_t)(B_ / A) * sizeof(double), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  }

  // ---- the solve mask (include/altro_subset.h) ------------------------------------------------------
  // A byte per instance in hm_.mask; k_mask_compact turns it into one ascending list per chain slice (the slices StartChains
  // cuts), which the first sweep of a chain, or the persistent tail kernel, takes where an unmasked solve takes "everyone".
  // The host keeps the slices' counts: it sizes grids with them and decides with them whether the solve fits the tail at once.
  MaskSlices MaskSlicesNow() const {
    MaskSlices s{};
    s.n = chains_;
    for (int c = 0; c < chains_; ++c) {
      s.lo[c] = chains_ > 1 ? std::min(B_, c * chain_size_) : 0;
      s.hi[c] = chains_ > 1 ? std::min(B_, (c + 1) * chain_size_) : B_;
    }
    return s;
  }
  int* MaskCounts() const { return hm_.mask_list.get() + B_; }
  altro_status MaskBlocks() {
    if (!hm_.mask) ALTRO_HIP_CHECK(hm_.mask.alloc((size_t)B_));
    if (!hm_.mask_list) ALTRO_HIP_CHECK(hm_.mask_list.alloc((size_t)B_ + kMaxSweepChains + 1));
    return ALTRO_OK;
  }
  // `src` (device bytes, possibly hm_.mask itself) -> hm_.mask, the lists and their counts.  `known`: the counts per slice
  // where the host can tell them without looking (a host mask, a team's turn); otherwise s.n + 1 words come back, once.
  altro_status CompactMask(const unsigned char* src, const MaskSlices& s, const int* known) {
    ALTRO_HIP_CHECK(hipMemsetAsync(MaskCounts() + s.n, 0, sizeof(int), stream_));
    hipLaunchKernelGGL((k_mask_compact<0>), dim3(s.n), dim3(kMaskThreads), 0, stream_, src, hm_.mask.get(), s, hm_.mask_list.get(),
                       MaskCounts());
    ALTRO_HIP_CHECK(hipGetLastError());
    int words[kMaxSweepChains + 1] = {};
    if (known) {
      for (int c = 0; c < s.n; ++c) words[s.n] += (words[c] = known[c]);
    } else {
      ALTRO_HIP_CHECK(CopySync(words, MaskCounts(), (size_t)(s.n + 1) * sizeof(int), hipMemcpyDeviceToHost));
    }
    mask_.chains = chains_;
    mask_.chain_size = chain_size_;
    for (int c = 0; c < kMaxSweepChains; ++c) mask_.count[c] = c < s.n ? words[c] : 0;
    mask_.total = words[s.n];
    mask_.on = true;
    return ALTRO_OK;
  }
  altro_status SetSolveMask(const unsigned char* mask, int on_device) override {
    if (!uploaded_) {
      err_ = "altro_set_solve_mask: no problem on the device";
      return ALTRO_NOT_READY;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(SumInstanceIterations());  // (of the last solve, under the mask it ran with)
    if (!mask) {
      mask_.on = false;
      return ALTRO_OK;
    }
    ALTRO_TRY(Sync());
    ALTRO_TRY(MaskBlocks());
    const MaskSlices s = MaskSlicesNow();
    if (on_device) {
      ALTRO_TRY(CompactMask(mask, s, nullptr));
      return Sync();
    }
    // a host mask: staged as the other host arrays are (k_mask_compact reads bytes 0 .. B - 1 and no further), its counts known here
    int known[kMaxSweepChains] = {};
    for (int c = 0; c < s.n; ++c)
      for (int b = s.lo[c]; b < s.hi[c]; ++b) known[c] += mask[b] != 0;
    StagedCall<1> c(this, MaskStageParts((size_t)B_), 0, "altro_set_solve_mask", kEngineBlock);
    ALTRO_TRY(c.Refused());
    const unsigned char* src = c.sg.in(0, mask, 0, (size_t)B_);
    return c.Finish(c.sg.ok() ? CompactMask(src, s, known) : ALTRO_OK);
  }
  altro_status GetSolveMask(unsigned char* mask, int* count) override {
    if (!mask_.on) {  // no mask: everyone
      std::memset(mask, 1, (size_t)B_);
      if (count) *count = B_;
      return ALTRO_OK;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_HIP_CHECK(CopySync(mask, hm_.mask.get(), (size_t)B_, hipMemcpyDeviceToHost));
    if (count) *count = mask_.total;
    return ALTRO_OK;
  }
  // the lists belong to the chain slices they were cut for: should the slices have moved since, compact again
  altro_status Recompact() {
    if (!mask_.on || (mask_.chains == chains_ && mask_.chain_size == chain_size_)) return ALTRO_OK;
    return CompactMask(hm_.mask.get(), MaskSlicesNow(), nullptr);
  }
  // one turn of a sequential team round: the mask "agent a of every team", written and compacted on the device; the
  // counts follow from A and the slices
  altro_status TeamTurnMask(int A, int a) override {
    if (!uploaded_ || A < 1 || a < 0 || a >= A) return ALTRO_INVALID_ARG;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(SumInstanceIterations());
    ALTRO_TRY(MaskBlocks());
    hipLaunchKernelGGL((k_team_turn_mask<0>), dim3((B_ + kMaskThreads - 1) / kMaskThreads), dim3(kMaskThreads), 0, stream_, hm_.mask.get(),
                       B_, A, a);
    const MaskSlices s = MaskSlicesNow();
    int known[kMaxSweepChains] = {};
    // (instances b in [lo, hi) with b % A == a: those below hi less those below lo)
    auto below = [&](int x) { return x <= a ? 0 : (x - a - 1) / A + 1; };
    for (int c = 0; c < s.n; ++c) known[c] = below(s.hi[c]) - below(s.lo[c]);
    return CompactMask(hm_.mask.get(), s, known);
  }
  // what a sequential team round puts back when it is over: the mask bytes the handle had, kept on the device meanwhile
  altro_status SaveSolveMask() override {
    mask_saved_on_ = mask_.on;
    if (!mask_.on) return ALTRO_OK;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    if (!hm_.mask_saved) ALTRO_HIP_CHECK(hm_.mask_saved.alloc((size_t)B_));
    ALTRO_HIP_CHECK(CopySync(hm_.mask_saved.get(), hm_.mask.get(), (size_t)B_, hipMemcpyDeviceToDevice));
    mask_saved_ = mask_;
    return ALTRO_OK;
  }
  altro_status RestoreSolveMask() override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(SumInstanceIterations());
    if (!mask_saved_on_) {
      mask_.on = false;
      return ALTRO_OK;
    }
    ALTRO_TRY(CompactMask(hm_.mask_saved.get(), MaskSlicesNow(), mask_saved_.chains == chains_ && mask_saved_.chain_size == chain_size_ ? mask_saved_.count : nullptr));
    return Sync();
  }
  // timing_.instance_iterations of the last solve, if nobody has asked yet: the iterations of the instances it ran
  altro_status SumInstanceIterations() {
    if (!(timing_.instance_iterations < 0) || !uploaded_) return ALTRO_OK;
    ALTRO_TRY(Sync());
    std::vector<int> it(Bp_);
    ALTRO_HIP_CHECK(CopySync(it.data(), A_.it_total, (size_t)Bp_ * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<unsigned char> in;
    if (last_solve_masked_) {
      in.resize((size_t)B_);
      ALTRO_HIP_CHECK(CopySync(in.data(), hm_.mask.get(), (size_t)B_, hipMemcpyDeviceToHost));
    }
    long long tot = 0;
    for (int b = 0; b < B_; ++b) tot += in.empty() || in[b] ? it[b] : 0;
    timing_.instance_iterations = tot;
    return ALTRO_OK;
  }

  // ---- closed-loop covariance (include/altro_covariance.h) ------------------------------------------
  // k_cov_linearise over (instance, knot) into the engine's scratch F | Kw ([steps][n n][Bp], [steps][m n][Bp]), then
  // k_cov_recur along the knots.  Host arrays are staged through ONE device block that lives for the call, as MpcTrack does;
  // device arrays are used where they are.  Reads the engine's arrays only: no flag of the engine changes.
  altro_status LaunchCov(const CovArgs& g) {
    const size_t nf = (size_t)g.steps * n * n * Bp_, nk = (size_t)g.steps * m * n * Bp_;
    if (nf + nk > hm_.cov_f.count() && hm_.cov_f.alloc(nf + nk) != hipSuccess) {
      err_ = "altro_cov_propagate: out of device memory for " + std::to_string((nf + nk) * sizeof(double)) + " bytes of linearisations";
      return ALTRO_HIP_ERROR;
    }
    double *F = hm_.cov_f.get(), *Kw = F + nf;
    hipLaunchKernelGGL((k_cov_linearise<T, M>), dim3((B_ + kBlock - 1) / kBlock, g.steps), dim3(kBlock), 0, stream_, A_, up_.d_pd, F, Kw);
    constexpr int per_block = n <= kCovMaxN ? kBlock / cov_group(n <= kCovMaxN ? n : 1) : 1;
    hipLaunchKernelGGL((k_cov_recur<n, m>), dim3((B_ + per_block - 1) / per_block), dim3(kBlock), 0, stream_, g, (const double*)F,
                       (const double*)Kw, B_, (unsigned)Bp_);
    return ALTRO_OK;
  }
  altro_status CovPropagate(const CovArgs& call, int on_device) override {
    if (call.steps < 1 || call.steps > N_ || (call.w_mode & ~3) || (!call.Sigma && !call.sx && !call.su && !call.rpos) ||
        (call.rpos && n < 2)) {
      err_ = "altro_cov_propagate: steps must lie in [1, N], w_mode in 0..3, an output is required, and rpos needs two states";
      return ALTRO_INVALID_ARG;
    }
    if (n > kCovMaxN) {
      err_ = "altro_cov_propagate: models of more than " + std::to_string(kCovMaxN) + " states are not supported";
      return ALTRO_UNSUPPORTED;
    }
    if (!StepOk()) return ALTRO_NOT_READY;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    // the staged block of a host caller (CovStageParts); it goes when this call returns, behind the wait of finish()
    StagedCall<6> c(this, CovStageParts(n, m, (size_t)B_, call), on_device, "altro_cov_propagate", kCallBlock);
    ALTRO_TRY(c.Refused());
    Staged<6>& sg = c.sg;
    CovArgs g = call;
    g.Sigma0 = sg.in(0, call.Sigma0);
    g.W = sg.in(1, call.W);
    g.Sigma = sg.out(2, call.Sigma);
    g.sx = sg.out(3, call.sx);
    g.su = sg.out(4, call.su);
    g.rpos = sg.out(5, call.rpos);
    return c.Finish(sg.ok() ? LaunchCov(g) : ALTRO_OK);
  }
  // the spare buffer a kernel has just been launched to write becomes the constraint's track, one column per instance
  void AdoptSpare(KnotCon* c, int rows, int base, bool team) {
    std::swap(c->track, c->spare);
    c->rows = rows, c->cols = B_, c->base = base, c->team = team;
    LaunchKnotParams();
  }
  // the routine of TeamFill: write the constraint's spare buffer, then swap; the track is an ordinary one afterwards (base 0)
  altro_status CovInflate(int index, const double* base, int rows, int per_instance, double kappa, const double* rpos,
                          int on_device) override {
    KnotCon* c = FindKnotCon(index, "altro_cov_inflate_circles");
    if (!c) return ALTRO_INVALID_ARG;
    if (c->kind != ALTRO_CON_CIRCLE || c->np % 3 != 0 || !base || !rpos || rows < 1 || !(kappa >= 0.0) || !std::isfinite(kappa)) {
      err_ = "altro_cov_inflate_circles: a knot circle constraint, a base track of at least one row, rpos and a finite kappa >= 0";
      return ALTRO_INVALID_ARG;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    const size_t need = (size_t)B_ * rows * c->np;
    StagedCall<2> sc(this, InflateStageParts((size_t)(per_instance ? B_ : 1), (size_t)rows, (size_t)c->np, (size_t)B_, (size_t)N_ + 1),
                     on_device, "altro_cov_inflate_circles", kCallBlock);
    ALTRO_TRY(sc.Refused());
    base = sc.sg.in(0, base);
    rpos = sc.sg.in(1, rpos);
    if (need > c->spare.count()) ALTRO_HIP_CHECK(c->spare.alloc(need));
    ctg_replayable_ = false;  // (as SetConstraintTrack)
    const int nobs = c->np / 3;
    const size_t total = (size_t)B_ * rows * nobs;
    hipLaunchKernelGGL((k_cov_inflate<0>), dim3((unsigned)((total + kTeamThreads - 1) / kTeamThreads)), dim3(kTeamThreads), 0, stream_,
                       c->spare.get(), base, rpos, B_, rows, nobs, per_instance ? B_ : 1, up_.track_offset, N_, kappa);
    AdoptSpare(c, rows, 0, false);
    return sc.Finish();
  }

  // ---- time-varying LQR tracking gains (include/altro_lqr.h) -----------------------------------------
  // k_lqr_linearise over (instance, knot), k_lqr_recur along the knots, k_lqr_install over (instance, knot), all on the
  // engine's stream, through the covariance's scratch block grown to [A | B] | K | P | weights | fail (the two users follow
  // each other on one stream).  `w` (LqrPackWeights) must live until the stream is done.  K, P, fail: device memory or null.
  altro_status LqrUnsupported() {
    err_ = "altro_lqr_gains: 1 .. " + std::to_string(kLqrMaxM) + " controls and at most " + std::to_string(kLqrMaxN) + " states are supported";
    return ALTRO_UNSUPPORTED;
  }
  altro_status LaunchLqr(const std::vector<double>& w, int install, const unsigned char* mask, double* K, double* P, int* fail) {
    if constexpr (!lqr_supported(n, m)) {
      return LqrUnsupported();
    } else {
      const size_t nab = (size_t)N_ * n * nm * Bp_, nk = (size_t)N_ * m * n * Bp_, np = (size_t)(N_ + 1) * n * n * Bp_;
      const size_t nw = ((size_t)(2 * n * n + m * m) + 1) & ~(size_t)1, nfail = ((size_t)Bp_ + 1) / 2, need = nab + nk + np + nw + nfail;
      if (need > hm_.cov_f.count() && hm_.cov_f.alloc(need) != hipSuccess) {
        err_ = "altro_lqr_gains: out of device memory for " + std::to_string(need * sizeof(double)) + " bytes of linearisations and gains";
        return ALTRO_HIP_ERROR;
      }
      double *AB = hm_.cov_f.get(), *Kt = AB + nab, *Pt = Kt + nk, *Wt = Pt + np;
      int* const failS = reinterpret_cast<int*>(Wt + nw);
      ALTRO_HIP_CHECK(hipMemcpyAsync(Wt, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
      hipLaunchKernelGGL((k_lqr_linearise<T, M>), dim3((B_ + kBlock - 1) / kBlock, N_), dim3(kBlock), 0, stream_, A_, up_.d_pd, AB);
      constexpr int per_block = kBlock / cov_group(n);
      hipLaunchKernelGGL((k_lqr_recur<n, m>), dim3((B_ + per_block - 1) / per_block), dim3(kBlock), 0, stream_, (const double*)AB,
                         (const double*)Wt, Kt, Pt, failS, B_, (unsigned)Bp_, N_);
      if (install) ctg_replayable_ = false;  // (a replayed backward pass would write the solver's gains back over these)
      hipLaunchKernelGGL((k_lqr_install<RS, n, m>), dim3((B_ + kBlock - 1) / kBlock, N_ + 1), dim3(kBlock), 0, stream_, A_.KD,
                         (const double*)Kt, (const double*)Pt, (const int*)failS, mask, install, K, P, fail, B_, (unsigned)Bp_, N_);
      return ALTRO_OK;
    }
  }
  altro_status LqrGains(const LqrArgs& call, int on_device) override {
    const char* who = on_device ? "altro_lqr_gains_device" : "altro_lqr_gains";
    if (!call.Q || !call.R || (!call.install && !call.K && !call.P)) {
      err_ = std::string(who) + ": Q and R are required, and K or P unless the gains are installed";
      return ALTRO_INVALID_ARG;
    }
    if (!lqr_supported(n, m)) return LqrUnsupported();
    if (!StepOk()) return ALTRO_NOT_READY;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    // the weights of a device caller come to the host to be checked and mirrored, like a host caller's
    std::vector<double> hq, hr, hf;
    const double *Q = call.Q, *Rw = call.R, *Qf = call.Qf;
    if (on_device) {
      hq.resize(n * n), hr.resize(m * m), hf.resize(n * n);
      ALTRO_HIP_CHECK(CopySync(hq.data(), call.Q, hq.size() * sizeof(double), hipMemcpyDeviceToHost));
      ALTRO_HIP_CHECK(CopySync(hr.data(), call.R, hr.size() * sizeof(double), hipMemcpyDeviceToHost));
      if (call.Qf) ALTRO_HIP_CHECK(CopySync(hf.data(), call.Qf, hf.size() * sizeof(double), hipMemcpyDeviceToHost));
      Q = hq.data(), Rw = hr.data(), Qf = call.Qf ? hf.data() : nullptr;
    }
    if (!LqrPackWeights(n, m, Q, Rw, Qf, &lqr_w_, &err_, who)) return ALTRO_INVALID_ARG;
    // the staged block of a host caller (LqrStageParts)
    StagedCall<3> c(this, LqrStageParts(n, m, (size_t)B_, (size_t)N_, call.K, call.P, call.fail), on_device, who, kCallBlock);
    ALTRO_TRY(c.Refused());
    double* const K = c.sg.out(0, call.K);
    double* const P = c.sg.out(1, call.P);
    int* const fail = c.sg.out(2, call.fail, (size_t)B_);
    return c.Finish(LaunchLqr(lqr_w_, call.install, nullptr, K, P, fail));
  }
  void LqrSetPolicy(const std::vector<double>& packed) override { lqr_policy_ = packed; }

  // ---- closed-loop tracking (include/altro_mpc.h) ---------------------------------------------------
  // One launch of k_mpc_track, one lane per (instance, sample).  Host arrays are staged through ONE device block that lives
  // for the call; device arrays are used where they are.  Reads the engine's arrays only: no flag of the engine changes.
  altro_status MpcTrack(const TrackArgs& call, int on_device) override {
    if (call.steps < 1 || call.steps > N_ || call.S < 1 || (call.u_lo == nullptr) != (call.u_hi == nullptr)) {
      err_ = "altro_mpc_track: steps must lie in [1, N], samples must be positive, and u_lo / u_hi come together";
      return ALTRO_INVALID_ARG;
    }
    if (!StepOk() || !RefOk()) return ALTRO_NOT_READY;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    // the staged block of a host caller (TrackStageParts); it goes when this call returns, behind the wait of finish()
    StagedCall<6> c(this, TrackStageParts(n, m, (size_t)B_ * (size_t)call.S, (size_t)call.steps, call.dx0, call.w, call.u_lo, call.X_cl,
                                          call.U_cl, call.stats), on_device, "altro_mpc_track", kCallBlock);
    ALTRO_TRY(c.Refused());
    Staged<6>& sg = c.sg;
    TrackArgs g = call;
    g.dx0 = sg.in(0, call.dx0);
    g.w = sg.in(1, call.w);
    g.u_lo = sg.in(2, call.u_lo, 0, m);
    g.u_hi = sg.in(2, call.u_hi, m, m);
    g.X_cl = sg.out(3, call.X_cl);
    g.U_cl = sg.out(4, call.U_cl);
    g.stats = sg.out(5, call.stats);
    if (!on_device) g.x_end = nullptr;  // (a device caller's only: what altro_mpc_run_tracked advances from)
    return c.Finish(sg.ok() ? LaunchTrack(g) : ALTRO_OK);
  }

  // ---- Monte-Carlo ensembles (include/altro_ensemble.h) --------------------------------------------
  // The factors of the call's Sigma0 and W (device arrays) into `fac`, L0 | Lw, by k_ens_factor; the two status words come
  // back before anything else is launched, and a refused matrix ends the call with its instance and knot in the text.
  altro_status EnsFactors(const char* who, const EnsembleArgs& g, DevBlock<double>* fac, DevBlock<int>* word, const double** L0,
                          const double** Lw) {
    const size_t nn = (size_t)n * n;
    const size_t c0 = g.Sigma0 ? (g.sigma0_per_instance ? (size_t)B_ : 1) : 0;
    const size_t cw = g.W ? ((g.w_mode & 1) ? (size_t)B_ : 1) * ((g.w_mode & 2) ? (size_t)g.steps : 1) : 0;
    *L0 = *Lw = nullptr;
    if (c0 + cw == 0) return ALTRO_OK;
    if (c0 > 0x7fffffffull || cw > 0x7fffffffull) {
      err_ = std::string(who) + ": more than 2^31 - 1 covariance matrices";
      return ALTRO_INVALID_ARG;
    }
    if (fac->alloc((c0 + cw) * nn) != hipSuccess || word->alloc(2) != hipSuccess) {
      err_ = std::string(who) + ": out of device memory for " + std::to_string((c0 + cw) * nn * sizeof(double)) + " bytes of factors";
      return ALTRO_HIP_ERROR;
    }
    ALTRO_HIP_CHECK(hipMemsetAsync(word->get(), 0, 2 * sizeof(int), stream_));
    if (c0) {
      *L0 = fac->get();
      hipLaunchKernelGGL((k_ens_factor<0>), dim3((unsigned)((c0 + kEnsThreads - 1) / kEnsThreads)), dim3(kEnsThreads), 0, stream_, g.Sigma0,
                         fac->get(), n, (int)c0, word->get());
    }
    if (cw) {
      *Lw = fac->get() + c0 * nn;
      hipLaunchKernelGGL((k_ens_factor<0>), dim3((unsigned)((cw + kEnsThreads - 1) / kEnsThreads)), dim3(kEnsThreads), 0, stream_, g.W,
                         fac->get() + c0 * nn, n, (int)cw, word->get() + 1);
    }
    ALTRO_HIP_CHECK(hipGetLastError());
    int bad[2] = {0, 0};
    ALTRO_HIP_CHECK(CopySync(bad, word->get(), sizeof(bad), hipMemcpyDeviceToHost));
    if (bad[0]) {
      const size_t i = c0 - (size_t)bad[0];
      err_ = std::string(who) + ": Sigma0 is not positive semidefinite" + (g.sigma0_per_instance ? " (instance " + std::to_string(i) + ")" : "");
      return ALTRO_INVALID_ARG;
    }
    if (bad[1]) {
      const size_t i = cw - (size_t)bad[1], per = (g.w_mode & 2) ? (size_t)g.steps : 1;
      err_ = std::string(who) + ": W is not positive semidefinite (" + ((g.w_mode & 1) ? "instance " + std::to_string(i / per) : "every instance") +
             ", " + ((g.w_mode & 2) ? "knot " + std::to_string(i % per) : "every knot") + ")";
      return ALTRO_INVALID_ARG;
    }
    return ALTRO_OK;
  }
  bool EnsShapeOk(const char* who, const EnsembleArgs& c) {
    if (c.steps < 1 || c.steps > N_ || c.S < 1 || (c.w_mode & ~3)) {
      err_ = std::string(who) + ": steps must lie in [1, N], samples must be positive and w_mode lie in 0..3";
      return false;
    }
    return true;
  }
  // Factors, one launch of k_mpc_ensemble over (instance, slab), k_ens_finish.  Host arrays are staged through ONE device block
  // (EnsembleStageParts) that lives for the call, as do the factors and the slabs' partials; device arrays are used where
  // they are.  Reads the engine's arrays only: no flag of the engine changes.
  altro_status MpcEnsemble(const EnsembleArgs& call, int on_device) override {
    const char* who = "altro_mpc_ensemble";
    if (!EnsShapeOk(who, call)) return ALTRO_INVALID_ARG;
    if ((call.u_lo == nullptr) != (call.u_hi == nullptr) || !(call.viol_tol >= 0.0) || !std::isfinite(call.viol_tol) ||
        (!call.dev_mean && !call.dev_mom2 && !call.alive && !call.viol_count && !call.summary && !call.stats)) {
      err_ = std::string(who) + ": u_lo / u_hi come together, viol_tol is finite and not negative, and an output is required";
      return ALTRO_INVALID_ARG;
    }
    if (n > kEnsMaxN) {
      err_ = std::string(who) + ": models of more than " + std::to_string(kEnsMaxN) + " states are not supported";
      return ALTRO_UNSUPPORTED;
    }
    if (!StepOk() || !RefOk()) return ALTRO_NOT_READY;
    const int slabs = EnsembleSlabs(B_, call.S);
    if ((size_t)B_ * (size_t)slabs > 0x7fffffffull) {
      err_ = std::string(who) + ": instances x slabs exceed one launch (2^31 - 1 wavefronts)";
      return ALTRO_INVALID_ARG;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    const size_t K1 = (size_t)call.steps + 1, waves = (size_t)B_ * slabs, V = (size_t)EnsembleValues(n);
    DevBlock<double> fac, part;
    DevBlock<int> word, cnt;
    DevBlock<EnsSlabSum> sums;
    if (part.alloc(waves * K1 * V) != hipSuccess || cnt.alloc(waves * K1 * 2) != hipSuccess || sums.alloc(waves) != hipSuccess) {
      err_ = std::string(who) + ": out of device memory for " + std::to_string(waves * K1 * (V + 1) * sizeof(double)) + " bytes of partial sums";
      return ALTRO_HIP_ERROR;
    }
    StagedCall<9> c(this, EnsembleStageParts(n, m, (size_t)B_, call), on_device, who, kCallBlock);
    ALTRO_TRY(c.Refused());
    Staged<9>& sg = c.sg;
    EnsLaunch q{};
    q.g = call;
    q.g.Sigma0 = sg.in(0, call.Sigma0);
    q.g.W = sg.in(1, call.W);
    q.g.u_lo = sg.in(2, call.u_lo, 0, m);
    q.g.u_hi = sg.in(2, call.u_hi, m, m);
    EnsFinishArgs f{};
    f.dev_mean = sg.out(3, call.dev_mean);
    f.dev_mom2 = sg.out(4, call.dev_mom2);
    f.alive = sg.out(5, call.alive, (size_t)B_ * K1);
    f.viol_count = sg.out(6, call.viol_count, (size_t)B_ * K1);
    f.summary = sg.out(7, call.summary);
    q.g.stats = sg.out(8, call.stats);
    const altro_status st = sg.ok() ? EnsFactors(who, q.g, &fac, &word, &q.L0, &q.Lw) : ALTRO_OK;
    if (st == ALTRO_OK && sg.ok()) {
      q.part = part.get(), q.cnt = cnt.get(), q.sums = sums.get();
      q.slabs = slabs, q.per_slab = EnsembleChunksPerSlab(B_, call.S);
      if (KnotRouted(A_))
        hipLaunchKernelGGL((k_mpc_ensemble_trk<T, M>), dim3((unsigned)waves), dim3(kEnsChunk), 0, stream_, A_, up_.d_pd, q);
      else
        hipLaunchKernelGGL((k_mpc_ensemble<T, M>), dim3((unsigned)waves), dim3(kEnsChunk), 0, stream_, A_, up_.d_pd, q);
      f.part = part.get(), f.cnt = cnt.get(), f.sums = sums.get();
      f.B = B_, f.steps = call.steps, f.slabs = slabs, f.n = n, f.S = call.S;
      const size_t total = (size_t)B_ * K1 * V;
      hipLaunchKernelGGL((k_ens_finish<0>), dim3((unsigned)((total + kEnsThreads - 1) / kEnsThreads)), dim3(kEnsThreads), 0, stream_, f);
    }
    return c.Finish(st);
  }
  altro_status NoiseFill(const EnsembleArgs& call, int on_device) override {
    const char* who = "altro_noise_fill";
    if (!EnsShapeOk(who, call)) return ALTRO_INVALID_ARG;
    if (!call.dx0 && !call.w) {
      err_ = std::string(who) + ": at least one of dx0 and w is required";
      return ALTRO_INVALID_ARG;
    }
    if (n > kEnsMaxN) {
      err_ = std::string(who) + ": models of more than " + std::to_string(kEnsMaxN) + " states are not supported";
      return ALTRO_UNSUPPORTED;
    }
    const size_t blocks = ((size_t)B_ * (size_t)call.S + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffull) {
      err_ = std::string(who) + ": instances x samples exceed one launch (2^31 - 1 wavefronts)";
      return ALTRO_INVALID_ARG;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    DevBlock<double> fac;  // (the factors outlive the frame's wait: declared ahead of it)
    DevBlock<int> word;
    StagedCall<4> c(this, NoiseStageParts(n, (size_t)B_, call), on_device, who, kCallBlock);
    ALTRO_TRY(c.Refused());
    Staged<4>& sg = c.sg;
    EnsembleArgs g = call;
    g.Sigma0 = sg.in(0, call.Sigma0);
    g.W = sg.in(1, call.W);
    g.dx0 = sg.out(2, call.dx0);
    g.w = sg.out(3, call.w);
    const double *L0 = nullptr, *Lw = nullptr;
    const altro_status st = sg.ok() ? EnsFactors(who, g, &fac, &word, &L0, &Lw) : ALTRO_OK;
    if (st == ALTRO_OK && sg.ok()) hipLaunchKernelGGL((k_noise_fill<n>), dim3((unsigned)blocks), dim3(kBlock), 0, stream_, g, L0, Lw, B_);
    return c.Finish(st);
  }

  // ---- event-triggered re-planning (include/altro_trigger.h) ----------------------------------------
  // What the trigger calls refuse once the device state exists, before any device work: what Advance refuses (the rule
  // decides over a plan that moves along the horizon) and the cost-to-go records that a masked solve refuses.
  altro_status TriggerCheck(const char* who) {
    if (kTimeVarying || A_.hk || A_.knot_model) {
      err_ = std::string(who) + ": per-knot steps, times or models (a time-varying or discrete user model included) do not move "
             "along the horizon yet";
      return ALTRO_UNSUPPORTED;
    }
    if (A_.record_ctg) {
      err_ = std::string(who) + ": a masked solve does not record the cost-to-go (altro_set_record_ctg): switch the records off";
      return ALTRO_UNSUPPORTED;
    }
    return ALTRO_OK;
  }
  // The lookahead's track -- one sample, no disturbance, statistics only, into `ahead` -- and k_mpc_trigger, on the engine's
  // stream (every array of `g` in device memory).  Reads the engine's arrays only.
  altro_status LaunchTrigger(const TriggerArgs& g, TrackStats* ahead, bool ilqr_mode) {
    const bool look = g.rule.lookahead > 0;
    if (look) {
      TrackArgs t = g.track;
      t.steps = g.rule.lookahead;
      t.S = 1;
      t.dx0 = t.w = nullptr;
      t.u_lo = g.u_lo;
      t.u_hi = g.u_hi;
      t.X_cl = t.U_cl = t.x_end = nullptr;
      t.stats = ahead;
      ALTRO_TRY(LaunchTrack(t));
    }
    hipLaunchKernelGGL((k_mpc_trigger<0>), GridB(), dim3(kBlock), 0, stream_, g.rule, g.tracked, g.age,
                       (const int*)(ilqr_mode ? A_.status : A_.status_al), (const TrackStats*)(look ? ahead : nullptr), g.mask, g.reason, B_);
    return ALTRO_OK;
  }
  // Host arrays are staged through ONE device block that lives for the call (TriggerStageParts); device arrays are used where
  // they are.  The lookahead's statistics live in that block for either caller.  No flag of the engine changes.
  altro_status Trigger(const TriggerArgs& call, int on_device, bool ilqr_mode) override {
    const TriggerRule& r = call.rule;
    if (r.max_age < 1 || r.lookahead < 0 || r.lookahead > N_ || (call.u_lo == nullptr) != (call.u_hi == nullptr)) {
      err_ = "altro_mpc_trigger: max_age must be positive, lookahead must lie in [0, N], and u_lo / u_hi come together";
      return ALTRO_INVALID_ARG;
    }
    ALTRO_TRY(TriggerCheck("altro_mpc_trigger"));
    if (r.lookahead > 0 && (!StepOk() || !RefOk())) return ALTRO_NOT_READY;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    const bool host = !on_device;
    const size_t B = (size_t)B_;
    StagedCall<6> c(this, TriggerStageParts(m, B, host && call.tracked, host && call.age, host && call.u_lo, host && call.mask,
                                            host && call.reason, r.lookahead > 0), on_device, "altro_mpc_trigger", kCallBlock, true);
    ALTRO_TRY(c.Refused());
    Staged<6>& sg = c.sg;
    TriggerArgs g = call;
    g.tracked = sg.in(0, call.tracked);
    g.age = sg.in(1, call.age, 0, B);
    g.u_lo = sg.in(2, call.u_lo, 0, m);
    g.u_hi = sg.in(2, call.u_hi, m, m);
    g.mask = sg.out(3, call.mask, B);
    g.reason = sg.out(4, call.reason, B);
    return c.Finish(sg.ok() ? LaunchTrigger(g, reinterpret_cast<TrackStats*>(sg.part(5)), ilqr_mode) : ALTRO_OK);
  }

  // ---- one closed-loop run (LoopSpec, altro_common.hpp) ----------------------------------------------
  // What lives on the device between LoopBegin and LoopEnd: one block of doubles, one of ints, one cycle counter.  The plain,
  // multi-start and team kinds log through k_mpc_advance (LogSlot): rows of X, U per instance, iterations and statuses
  // [B][cycles].  The closed-loop states of the tracked kind are the TRACKED ones, so it does not use that log: k_mpc_track
  // writes one cycle's rows, two strided copies append them, and iterations, statuses and TrackStats are recorded cycle-major
  // [cycles][B] (one contiguous row per cycle) and transposed on the host in LoopEnd.  One layout for both takes a kernel
  // change.  The triggered kind is the tracked kind with three more things on the device: the age of every plan, the mask
  // and the reasons the cycle's rule evaluation (LaunchTrigger) leaves for the next cycle's solve, and the log of the
  // reasons.  Its cycle log is written by k_trigger_log, under the mask the cycle's solve ran with.
  struct LoopRun {
    LoopSpec spec{};  // (its host pointers belong to the C call that drives the run)
    int cycle = 0;    // cycles that went through
    DevBlock<double> d;
    DevBlock<int> i;
    double *Xlog = nullptr, *Ulog = nullptr;  // [B][cycles shift + 1][n], [B][cycles shift][m]
    int *it = nullptr, *win = nullptr;        // iterations | statuses; multi-start: winners [B / G][cycles]
    double *w = nullptr, *dU = nullptr, *clear = nullptr;  // multi-start, team: w and dU on the device; team: [B / A][cycles]
    double *Xc = nullptr, *Uc = nullptr, *xend = nullptr, *wc = nullptr, *ulo = nullptr, *uhi = nullptr;  // tracked: one cycle's
    TrackStats* stats = nullptr;                                                                          // arrays; [cycles][B]
    // triggered: reasons [cycles][B]; ages [B]; the reasons [B] and the mask bytes [B] of the solve to come
    int *why_log = nullptr, *age = nullptr, *why = nullptr;
    unsigned char* next_mask = nullptr;
    DevBlock<double> ahead;  // triggered, with a lookahead: its statistics [B]
    bool masked = false;     // triggered: the run has put its mask on the handle
  };
  altro_status LoopBegin(const LoopSpec& s) override {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    hm_.run = LoopRun{};
    const bool ms = s.kind == kLoopMultiStart, team = s.kind == kLoopTeam;
    if (ms) ALTRO_TRY(MsCheck(s.G));
    if (team) {
      if (s.A < 2 || B_ % s.A != 0 || !s.radius) {
        err_ = "altro_mpc_run_team: agents must be at least 2 and divide the batch, with one radius per instance";
        return ALTRO_INVALID_ARG;
      }
      ALTRO_TRY(TeamRadius(s.radius));
    }
    const bool trig = s.kind == kLoopTriggered;
    if (trig) {
      ALTRO_TRY(TriggerCheck("altro_mpc_run_triggered"));
      if (mask_.on) {
        err_ = "altro_mpc_run_triggered: the handle carries a solve mask; the run sets its own (clear it with altro_set_solve_mask(h, NULL))";
        return ALTRO_UNSUPPORTED;
      }
    }
    LoopRun r;
    r.spec = s;
    const size_t B = (size_t)B_, cycles = (size_t)s.cycles;
    const bool tracked = s.kind == kLoopTracked || trig;
    const Parts<8> pt = TrackedRunParts(n, m, B, cycles, (size_t)s.shift);
    const Parts<5> pp = PlainRunParts(n, m, B, cycles, (size_t)s.shift, s.w && (ms || team),
                                      ms && s.dU ? (size_t)(s.dU_per_instance ? B_ : s.G) * N_ * m : 0, team ? (size_t)(B_ / s.A) * cycles : 0);
    const Parts<7> pi = RunIntParts(B, cycles, ms ? (size_t)(B_ / s.G) : 0, trig);
    if (r.i.alloc(pi.total()) != hipSuccess ||
        r.d.alloc(tracked ? pt.total() : pp.total()) != hipSuccess ||
        (trig && s.rule.lookahead > 0 && r.ahead.alloc(DoublesFor<TrackStats>(B)) != hipSuccess)) {
      err_ = "closed-loop run: out of device memory for the logs";
      return ALTRO_HIP_ERROR;
    }
    // iterations | statuses | winners | reason log | ages | reasons | next mask (a part the run's kind lacks has no room)
    r.it = r.i.get();
    r.win = r.it + pi.off[2];
    r.why_log = r.it + pi.off[3];
    r.age = r.it + pi.off[4];
    r.why = r.it + pi.off[5];
    r.next_mask = reinterpret_cast<unsigned char*>(r.it + pi.off[6]);
    // the run's host inputs go up with the block carved (one wait for all of them, none without any; a block that goes on
    // a failure has no copy in flight)
    if (tracked) {
      Staged<8> sg(false, r.d.get(), pt, stream_);
      r.Xlog = sg.part(0);
      r.Ulog = sg.part(1);
      r.Xc = sg.part(2);
      r.Uc = sg.part(3);
      r.xend = sg.part(4);
      r.wc = sg.part(5);
      r.ulo = const_cast<double*>(sg.in(6, s.u_lo, 0, m));
      r.uhi = const_cast<double*>(sg.in(6, s.u_hi, m, m));
      r.stats = reinterpret_cast<TrackStats*>(sg.part(7));
      if (sg.copies() > 0) ALTRO_HIP_CHECK(sg.finish());
    } else {
      Staged<5> sg(false, r.d.get(), pp, stream_);
      r.Xlog = sg.part(0);
      r.Ulog = sg.part(1);
      r.w = const_cast<double*>(sg.in(2, s.w));
      r.dU = const_cast<double*>(sg.in(3, s.dU));
      r.clear = sg.part(4);
      if (sg.copies() > 0) ALTRO_HIP_CHECK(sg.finish());
    }
    if (trig) {
      // cycle 0: everyone, reason kTrigFirst, age 0; the counts per slice are the slices' sizes
      ALTRO_TRY(MaskBlocks());
      ALTRO_HIP_CHECK(hipMemsetAsync(r.age, 0, B * sizeof(int), stream_));
      ALTRO_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r.why), kTrigFirst, B, stream_));
      ALTRO_HIP_CHECK(hipMemsetAsync(r.next_mask, 1, B, stream_));
      const MaskSlices sl = MaskSlicesNow();
      int known[kMaxSweepChains] = {};
      for (int c = 0; c < sl.n; ++c) known[c] = sl.hi[c] - sl.lo[c];
      r.masked = true;  // (from here on LoopEnd takes the mask off again)
      hm_.run = std::move(r);
      ALTRO_TRY(SumInstanceIterations());  // (of the last solve before the run, as SetSolveMask)
      ALTRO_TRY(CompactMask(hm_.run.next_mask, sl, known));
      return Sync();
    }
    hm_.run = std::move(r);
    return ALTRO_OK;
  }
  altro_status LoopCycle(const LoopStep& step) override {
    LoopRun& r = hm_.run;
    const LoopSpec& s = r.spec;
    if (!r.i || r.cycle >= s.cycles) {
      err_ = "closed-loop run: no cycle left";
      return ALTRO_NOT_READY;
    }
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    const size_t B = (size_t)B_, c = (size_t)r.cycle, cb = (size_t)s.cycles * B;
    // this cycle's disturbance: the run's device copy, or the caller's array (the plain advance and the tracking stage it)
    const double* const w = s.w ? (r.w ? r.w : s.w) + c * s.w_stride : nullptr;
    const LogSlot log{r.Xlog, r.Ulog, r.it, r.it + cb, r.cycle, s.cycles};
    if (s.kind == kLoopPlain) {
      ALTRO_TRY(Advance(s.shift, nullptr, w, 0, step.reset_pen, &log));
    } else if (s.kind == kLoopTracked || s.kind == kLoopTriggered) {
      const bool trig = s.kind == kLoopTriggered;
      const size_t sh = (size_t)s.shift, Lk = (size_t)s.cycles * sh;
      // the statistics of the solve behind this cycle
      if (trig) {  // (of the instances it ran; their ages start again, and every age counts the cycle being followed)
        hipLaunchKernelGGL((k_trigger_log<0>), GridB(), dim3(kBlock), 0, stream_, (const unsigned char*)hm_.mask.get(), (const int*)A_.it_total,
                           (const int*)(step.ilqr_mode ? A_.status : A_.status_al), (const int*)r.why, r.age, r.it + c * B, r.it + cb + c * B,
                           r.why_log + c * B, B_);
      } else {
        ALTRO_HIP_CHECK(hipMemcpyAsync(r.it + c * B, A_.it_total, B * sizeof(int), hipMemcpyDeviceToDevice, stream_));
        ALTRO_HIP_CHECK(hipMemcpyAsync(r.it + cb + c * B, A_.status_al, B * sizeof(int), hipMemcpyDeviceToDevice, stream_));
      }
      if (w) ALTRO_HIP_CHECK(hipMemcpyAsync(r.wc, w, B * sh * n * sizeof(double), hipMemcpyHostToDevice, stream_));
      TrackArgs g = step.track;
      g.steps = s.shift;
      g.S = 1;
      g.dx0 = nullptr;
      g.w = w ? r.wc : nullptr;
      g.u_lo = r.ulo;
      g.u_hi = r.uhi;
      g.X_cl = r.Xc;
      g.U_cl = r.Uc;
      g.x_end = r.xend;
      g.stats = r.stats + c * B;
      ALTRO_TRY(LaunchTrack(g));
      // rows c s .. c s + s of every instance's log (the last of them is the next cycle's first, and the log's last row)
      ALTRO_HIP_CHECK(hipMemcpy2DAsync(r.Xlog + c * sh * n, (Lk + 1) * n * sizeof(double), r.Xc, (sh + 1) * n * sizeof(double),
                                       (sh + 1) * n * sizeof(double), B, hipMemcpyDeviceToDevice, stream_));
      ALTRO_HIP_CHECK(hipMemcpy2DAsync(r.Ulog + c * sh * m, Lk * m * sizeof(double), r.Uc, sh * m * sizeof(double), sh * m * sizeof(double), B,
                                       hipMemcpyDeviceToDevice, stream_));
      ALTRO_TRY(Advance(s.shift, r.xend, nullptr, 1, step.reset_pen, nullptr));
      if (trig && r.cycle + 1 < s.cycles) {
        // the rule over what this cycle tracked, for the next cycle's solve; of the mask only the slices' counts come back
        TriggerArgs g{};
        g.rule = s.rule;
        g.tracked = r.stats + c * B;
        g.age = r.age;
        g.u_lo = r.ulo;
        g.u_hi = r.uhi;
        g.mask = r.next_mask;
        g.reason = r.why;
        g.track = step.track;
        ALTRO_TRY(LaunchTrigger(g, reinterpret_cast<TrackStats*>(r.ahead.get()), step.ilqr_mode));
        ALTRO_TRY(CompactMask(r.next_mask, MaskSlicesNow(), nullptr));
      }
    } else if (s.kind == kLoopMultiStart) {
      ctg_replayable_ = false;
      LaunchMsSelect(s.G, step.ilqr_mode, hm_.ms_win.get(), r.win, s.cycles, r.cycle);
      if (s.G > 1) LaunchMsSpread(s.G, hm_.ms_win.get());
      ALTRO_TRY(Advance(s.shift, nullptr, w, 1, step.reset_pen, &log));
      if (r.dU) {
        LaunchMsPerturb(s.G, r.dU, s.dU_per_instance);
        ALTRO_TRY(Sync());
      }
    } else {
      KnotCon* kc = TeamCheck(s.A, s.index, "altro_mpc_run_team");
      if (!kc || !hm_.team_rad) return ALTRO_INVALID_ARG;
      LaunchTeamClearance(s.A, *kc, r.clear, s.cycles, r.cycle);
      ALTRO_TRY(Advance(s.shift, nullptr, w, 1, step.reset_pen, &log));
    }
    ++r.cycle;
    return ALTRO_OK;
  }
  altro_status LoopEnd(const LoopOut& o) override {
    LoopRun r;  // the run goes with this call, whatever happens: behind the synchronisation no copy touches its blocks
    std::swap(r, hm_.run);
    const LoopSpec& s = r.spec;
    hipError_t e = hipSetDevice(desc_.device_id);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    if (r.masked) {  // a triggered run leaves the handle without a mask, whatever happened (as SetSolveMask clears one)
      if (e == hipSuccess && r.cycle == s.cycles) {
        (void)SumInstanceIterations();  // (hm_.mask is still the last solve's)
      } else if (e == hipSuccess && r.cycle > 0 && timing_.instance_iterations < 0) {
        // a run that broke off: hm_.mask is the NEXT solve's already, so the sum of the last solve that went through comes
        // from its row of the log, which holds 0 for the instances it skipped
        std::vector<int> it((size_t)B_);
        if (CopySync(it.data(), r.it + (size_t)(r.cycle - 1) * B_, it.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess) {
          long long tot = 0;
          for (int v : it) tot += v;
          timing_.instance_iterations = tot;
        }
      }
      mask_.on = false;
    }
    const bool tracked = s.kind == kLoopTracked || s.kind == kLoopTriggered;
    auto down = [&](void* dst, const void* src, size_t bytes) {
      if (e == hipSuccess && dst) e = CopySync(dst, src, bytes, hipMemcpyDeviceToHost);
    };
    if (r.i && r.cycle == s.cycles) {
      const size_t B = (size_t)B_, cycles = (size_t)s.cycles, Lk = cycles * s.shift, cb = cycles * B;
      down(o.X_cl, r.Xlog, B * (Lk + 1) * n * sizeof(double));
      down(o.U_cl, r.Ulog, B * Lk * m * sizeof(double));
      if (!tracked) {
        down(o.iterations, r.it, cb * sizeof(int));
        down(o.status, r.it + cb, cb * sizeof(int));
      } else {  // recorded [cycles][B], handed out [B][cycles]
        if (o.iterations || o.status) {  // (neighbours in the block: one copy for the two)
          std::vector<int> h(2 * cb);
          down(h.data(), r.it, h.size() * sizeof(int));
          if (e == hipSuccess) CyclesToColumns(h.data(), o.iterations, B, cycles), CyclesToColumns(h.data() + cb, o.status, B, cycles);
        }
        if (s.kind == kLoopTriggered) DownCycleMajor(r.why_log, o.reason, B, cycles, &e);
        DownCycleMajor(r.stats, o.track, B, cycles, &e);
      }
      if (s.kind == kLoopMultiStart) down(o.winner, r.win, (size_t)(B_ / s.G) * cycles * sizeof(int));
      if (s.kind == kLoopTeam) down(o.clear, r.clear, (size_t)(B_ / s.A) * cycles * sizeof(double));
    }
    ALTRO_HIP_CHECK(e);
    return ALTRO_OK;
  }
  // a log recorded [cycles][B] on the host -> the caller's [B][cycles] (null: not asked for)
  template <class V>
  static void CyclesToColumns(const V* rows, V* out, size_t B, size_t cycles) {
    for (size_t c = 0; out && c < cycles; ++c)
      for (size_t b = 0; b < B; ++b) out[b * cycles + c] = rows[c * B + b];
  }
  // ... and the same from the device: one copy and its wait, unless an earlier copy failed (*e) or the log is not asked for
  template <class V>
  void DownCycleMajor(const V* dev, V* out, size_t B, size_t cycles, hipError_t* e) {
    if (!out || *e != hipSuccess) return;
    std::vector<V> h(B * cycles);
    *e = CopySync(h.data(), dev, h.size() * sizeof(V), hipMemcpyDeviceToHost);
    if (*e == hipSuccess) CyclesToColumns(h.data(), out, B, cycles);
  }
  altro_status GetInitialState(double* x0) override { return DownloadRec(A_.x0, 1, R::nP, 0, n, x0); }
  altro_status SetPenalties(const double* rho) override { return UploadRows(A_.pen, rho); }
  void ConShapes(std::vector<int>* p, std::vector<int>* eq) override {
    *p = con_p_;
    *eq = con_eq_;
  }

 private:
  // the device copy of MpcRowMap(shift), built at the first advance by that shift
  altro_status MpcMap(int shift, const int** out) {
    auto it = up_.mpc_maps.find(shift);
    if (it == up_.mpc_maps.end()) {
      const std::vector<int> src = MpcRowMap(N_, shift, con_kb_, con_ke_, con_p_, con_eq_);
      if ((int)src.size() != pd_.total_rows) {
        err_ = "altro_mpc_advance: the row map does not match the rows on the device";
        return ALTRO_HIP_ERROR;
      }
      int* d = nullptr;
      ALTRO_TRY(Alloc(&d, src.size()));
      if (!src.empty()) ALTRO_HIP_CHECK(CopySync(d, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice));
      it = up_.mpc_maps.emplace(shift, d).first;
    }
    *out = it->second;
    return ALTRO_OK;
  }
  // the caller's rows [B][total_rows] into a device row array (duals, penalties)
  altro_status UploadRows(T* dst, const double* src) {
    ctg_replayable_ = false;
    const int R = pd_.total_rows;
    if (R == 0) return ALTRO_OK;
    std::vector<T> h((size_t)R * Bp_, T(0));
    for (int b = 0; b < B_; ++b)
      for (int r = 0; r < R; ++r) h[(size_t)r * Bp_ + b] = T(src[(size_t)b * R + r]);
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    ALTRO_HIP_CHECK(CopySync(dst, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return ALTRO_OK;
  }
  // the launch of k_mpc_track on the engine's stream (every array of `g` in device memory)
  altro_status LaunchTrack(const TrackArgs& g) {
    const size_t blocks = ((size_t)B_ * (size_t)g.S + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffull) {
      err_ = "altro_mpc_track: instances x samples exceed one launch (2^31 - 1 wavefronts)";
      return ALTRO_INVALID_ARG;
    }
    if (KnotRouted(A_))  // (a tracking cost or a knot constraint: the twin that reads the per-knot records, CtxTrackK)
      hipLaunchKernelGGL((k_mpc_track_trk<T, M>), dim3((unsigned)blocks), dim3(kBlock), 0, stream_, A_, up_.d_pd, g);
    else
      hipLaunchKernelGGL((k_mpc_track<T, M>), dim3((unsigned)blocks), dim3(kBlock), 0, stream_, A_, up_.d_pd, g);
    return ALTRO_OK;
  }
  // ---- helpers ----------------------------------------------------------------------------------
  dim3 GridB() const { return dim3((B_ + kBlock - 1) / kBlock); }
  dim3 GridBK() const { return dim3((B_ + kBlock - 1) / kBlock, N_ + 1); }
  dim3 GridAlInit() const { return dim3((B_ + kBlock - 1) / kBlock, std::max(1, (pd_.total_rows + kAlInitRows - 1) / kAlInitRows)); }
  // Backward pass launch: fp64 unicycle-sized problems run on the matrix cores (4 instances per
  // wavefront), everything else on the one-lane-per-instance VALU kernel.
  // The MFMA backward pass computes in fp64 whatever the storage type of the engine is
  static constexpr bool kMfmaBackward = n <= 3 && m <= 2;  // (round 4: every model that fits the 4 x 4 tiles, not only the unicycle's shape)
  // larger models: one instance per wavefront -- on the 16x16x4 fp64 matrix cores (k_backward_mfma16), or with
  // the matrices in LDS and the products on the vector ALUs (k_backward_coop: ALTRO_HIP_BACKWARD=coop)
  // (n = 4 -- the cart-pole class of user models -- takes the 16x16 tile too while the launch has few instances: one
  //  instance per wavefront at ~0.4 us per knot against ~1.5 us for the one-lane-per-instance kernel, which only wins on
  //  throughput once the instances outnumber the SIMDs several times: kMfma16SmallMax.  Decided by the handle's batch,
  //  not by the instances still active, so that an instance sees the same arithmetic in every sweep of every solve)
  static constexpr bool kMfma16Backward = n >= 4 && n <= 12 && m <= 4;
  static constexpr int kMfma16SmallMax = 4096;
  // gain records big enough (m n + m >= 14 elements) that reading K from global memory can pay: see kdg_
  static constexpr bool kKdgEligible = n * m >= 12;
  // rollout inputs from global memory, two knots ahead in three register sets: small records only
  // (round 6: ... and the large models, for which it competes with kSrcKdg -- see the LDS plan in UploadImpl)
  static constexpr bool kRgEligible = (!kKdgEligible && R::KP + R::nP + R::mP <= 16) || kKdgEligible;
  static constexpr bool kCoopBackward = !kMfmaBackward && n >= 6;
  // ALTRO_HIP_DEBUG_POISON=<hex pattern>[,mix]: before every kernel of a solve, fill the LDS of every CU with the pattern
  // (and the line-search candidates once, at upload), to flush out reads of memory the solve has not written.
  void PoisonLds() {
    if (!sw_.poison_on) return;
    hipFuncSetAttribute(reinterpret_cast<const void*>(&k_poison_lds<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL((k_poison_lds<0>), dim3(num_cus_ * 8), dim3(256), 160 * 1024, cur_, sw_.poison_pattern, 160 * 1024 / 4,
                       sw_.poison_mix, (int*)nullptr);
  }
  void LaunchBackward(const DevArrays<T>& A, const DevOpts& d, int all, int ninst) {
    PoisonLds();
    if constexpr (kMfmaBackward) {
      if (!sw_.force_valu_backward && mfma_offsets_ok_) {
        if (A.record_ctg)
          hipLaunchKernelGGL((k_backward_mfma<T, M, true>), dim3((ninst + 3) / 4), dim3(kBlock), 0, cur_, A, d, all);
        else
          hipLaunchKernelGGL((k_backward_mfma<T, M, false>), dim3((ninst + 3) / 4), dim3(kBlock), 0, cur_, A, d, all);
        return;
      }
    }
    if constexpr (kMfma16Backward) {
      if (!sw_.force_valu_backward && !sw_.force_coop_backward && mfma_offsets_ok_ && (n > 4 || B_ <= kMfma16SmallMax)) {
        if (A.record_ctg)
          hipLaunchKernelGGL((k_backward_mfma16<T, M, true>), dim3(ninst), dim3(kBlock), 0, cur_, A, d, all);
        else
          hipLaunchKernelGGL((k_backward_mfma16<T, M, false>), dim3(ninst), dim3(kBlock), 0, cur_, A, d, all);
        return;
      }
    }
    if constexpr (kCoopBackward) {
      if (!sw_.force_valu_backward) {
        hipLaunchKernelGGL((k_backward_coop<T, M>), dim3(ninst), dim3(kBlock), 0, cur_, A, d, all);
        return;
      }
    }
    hipLaunchKernelGGL((k_backward<T, M>), dim3((ninst + kBlock - 1) / kBlock), dim3(kBlock), 0, cur_, A, d, all);
  }
  // The fused sweep kernel needs the MFMA backward pass, the LDS-staged forward pass with one instance
  // per workgroup, no cost-to-go recording and 1 .. 20 line-search trials (with none the forward pass hands on the status
  // the backward pass left, which the batched forward kernels read back from memory).
  bool FusedOk(const DevOpts& d) const {
    if constexpr (!kMfmaBackward) return false;
    return !sw_.force_valu_backward && !sw_.no_fused && mfma_offsets_ok_ && fwd_lds_bytes_ > 0 && !A_.record_ctg && !A_.hk &&
           !KnotRouted(A_) &&  // (a tracking cost's term records and a knot constraint's parameter records are global
                               //  memory: the general kernels, as for per-knot steps)
           d.line_search_max_iterations >= 1 && d.line_search_max_iterations <= kLineSearchLanes && fused_lds_bytes_ <= 160 * 1024;
  }
  // Forward pass launch: instances per wavefront and the LDS-staged variant are chosen from the size
  // of one instance's read-only block (X, U, K, d, lambda, rho); see k_forward.
  void LaunchForward(const DevArrays<T>& A, const DevOpts& d, int mode, int all, int ninst, int ninst_all_chains = -1) {
    PoisonLds();
    // (per-knot steps / times / models: the three-wave kernel takes them for every model without a hand-fused RK4 --
    //  user models, the triple integrator, the 12-state model; the unicycle's fused rollout keeps ONE step as a loop
    //  invariant and goes to k_forward)
    // (a tracking cost: k_forward for EVERY model -- its terms are per-knot records in global memory, which the staged
    //  contexts of k_forward2 do not carry)
    if (fwd_lds_bytes_ > 0 && d.line_search_max_iterations <= kLineSearchLanes && (!A.hk || !M::kHasFusedRk4) && !KnotRouted(A)) {
      // two-wave pipeline (rollout wave + cost wave), inputs staged in LDS.  When the instances left
      // would not even fill the CUs one by one, each gets a workgroup of its own: the prologue and the
      // epilogue of the kernel (staging, winner copy) shrink with the instances per workgroup.
      const int per_wave = (std::max(ninst, ninst_all_chains) <= fwd_single_at_) ? 1 : fwd_per_wave_;
      const size_t lds = fwd_shared_bytes_ + (size_t)per_wave * fwd_per_inst_bytes_;
      const dim3 grid2((ninst + per_wave - 1) / per_wave);
      WithForwardSrc([&](auto src) {
        hipLaunchKernelGGL((k_forward2<T, M, decltype(src)::value>), grid2, dim3(kFwdWaves * kBlock), lds, cur_, A, up_.d_pd, pd_, d, mode,
                           all, per_wave);
      });
      return;
    }
    const dim3 grid((ninst + fwd_per_wave_ - 1) / fwd_per_wave_);
    {
      // fallback: single wave, reads from HBM (staged block larger than LDS, > 20 line-search trials, per-knot
      // steps / times: SetKnotTimes, or a tracking cost)
      if (KnotRouted(A))
        hipLaunchKernelGGL((k_forward_trk<T, M>), grid, dim3(kBlock), 0, cur_, A, up_.d_pd, d, mode, all, fwd_per_wave_);
      else
        hipLaunchKernelGGL((k_forward<T, M>), grid, dim3(kBlock), 0, cur_, A, up_.d_pd, d, mode, all, fwd_per_wave_);
    }
  }
  static void CpuRelax() {  // one spin-wait hint, whatever the host CPU
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield");
#else
    std::this_thread::yield();
#endif
  }
  bool StepOk() {
    if (pd_.hstep > 0.0f || A_.hk) return true;
    err_ = "the integration step is not set (altro_set_uniform_step / Trajectory::SetUniformStep)";
    return false;
  }
  altro_status Sync() {
    ALTRO_HIP_CHECK(hipGetLastError());
    ALTRO_HIP_CHECK(hipStreamSynchronize(stream_));
    return ALTRO_OK;
  }
  // Every copy and fill of the engine runs on the engine's own stream and is waited for: that stream is non-blocking, so
  // work on the null stream (where a plain hipMemcpy / hipMemset goes -- and a device-to-device hipMemcpy or a hipMemset
  // may return before it has run) would not be ordered against the kernels and the asynchronous copies of the solves.
  hipError_t CopySync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, stream_);
    return e != hipSuccess ? e : hipStreamSynchronize(stream_);
  }
  hipError_t ZeroSync(void* dst, int value, size_t bytes) {
    const hipError_t e = hipMemsetAsync(dst, value, bytes, stream_);
    return e != hipSuccess ? e : hipStreamSynchronize(stream_);
  }
  // an upload-lifetime array (Uploaded::pool): at least one element, zero-filled on the engine's stream and waited for
  template <class U>
  altro_status Alloc(U** p, size_t count) {
    ALTRO_HIP_CHECK(up_.pool.alloc(p, count));
    ALTRO_HIP_CHECK(ZeroSync(*p, 0, std::max<size_t>(count, 1) * sizeof(U)));
    return ALTRO_OK;
  }
  // back to one chain: the chains' streams, their events and the booking of this engine go
  void DropChains() {
    if (counted_chained_) ChainClaim(desc_.device_id, -1);
    counted_chained_ = false;
    for (int c = 1; c < kMaxChains; ++c) {
      if (chain_stream_[c]) hipStreamDestroy(chain_stream_[c]);
      if (chain_ev_[c]) hipEventDestroy(chain_ev_[c]);
      chain_stream_[c] = nullptr;
      chain_ev_[c] = nullptr;
    }
    chains_ = 1;
  }
  // A_ with nothing of an upload in it: what belongs to the handle -- the history buffers and the recording switches -- stays
  DevArrays<T> HandleView() const {
    DevArrays<T> A{};
    A.hist = hm_.hist.get();
    A.hist_len = hm_.hist_len.get();
    A.hist_cap = A_.hist_cap;
    A.record_ctg = A_.record_ctg;
    return A;
  }
  // undo a (partial) UploadImpl: device buffers, chain streams and the chain booking go; the engine's own stream stays
  void DropUpload() {
    uploaded_ = false;
    if (hipSetDevice(desc_.device_id) != hipSuccess) return;
    hipStreamSynchronize(stream_);
    up_ = Uploaded{};
    A_ = HandleView();
    DropChains();
  }
  // every block is freed HERE, with the engine's device current and before its stream goes (the members' destructors find nothing)
  void Release() {
    if (hipSetDevice(desc_.device_id) != hipSuccess) return;
    up_ = Uploaded{};
    hm_ = HandleMem{};
    for (auto& e : prof_ev_) hipEventDestroy(e);
    DropChains();
    if (start_ev_) hipEventDestroy(start_ev_);
    if (tail_ev_) hipEventDestroy(tail_ev_);
    if (stream_) hipStreamDestroy(stream_);
  }
  altro_status DownloadVec(const double* dev, double* out) {
    ALTRO_HIP_CHECK(CopySync(out, dev, (size_t)B_ * sizeof(double), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  }
  // Staging buffer of the host boundary: the caller's row layout on the device (see k_rec_to_rows / k_rows_to_rec).
  altro_status EnsureStage(size_t doubles) {
    if (doubles > hm_.stage.count()) ALTRO_HIP_CHECK(hm_.stage.alloc(doubles));
    return ALTRO_OK;
  }
  // The frame of one staged call (Staged, altro_devmem.hpp): the block of the layout `p`, then `sg`, then Finish().  The block
  // is the call's own (kCallBlock: it goes with the frame, behind the wait of Finish) or the engine's staging block, grown to
  // fit (kEngineBlock).  A device caller (`on_device`) has no block unless the layout holds scratch parts (`scratch`), which
  // every caller needs.  Refused() is to be asked before `sg` is used: the block could not be had, and the text is set.
  enum StageBlock { kCallBlock, kEngineBlock };
  template <int K>
  class StagedCall {
   public:
    StagedCall(Engine* e, const Parts<K>& p, int on_device, const char* who, StageBlock which, bool scratch = false)
        : e_(e),
          st_(Block(p.total(), !on_device || scratch, who, which == kCallBlock)),
          sg(on_device != 0, which == kCallBlock ? own_.get() : e->hm_.stage.get(), p, e->stream_) {}
    altro_status Refused() const { return st_; }
    // the tail of every staged call, behind its launches (`launched`: their status; a refused launch leaves nothing to
    // download): the downloads, the one wait -- also after a failure -- and the first error
    altro_status Finish(altro_status launched = ALTRO_OK) {
      const hipError_t e = sg.finish(launched == ALTRO_OK);
      if (launched != ALTRO_OK) return launched;
      return e_->HipStatus(e);
    }

   private:
    altro_status Block(size_t doubles, bool needed, const char* who, bool own) {
      if (!needed || doubles == 0) return ALTRO_OK;
      if (!own) return e_->EnsureStage(doubles);
      if (own_.alloc(doubles) == hipSuccess) return ALTRO_OK;
      e_->err_ = std::string(who) + ": out of device memory for " + std::to_string(doubles * sizeof(double)) + " bytes of staged arrays";
      return ALTRO_HIP_ERROR;
    }
    Engine* const e_;
    DevBlock<double> own_;
    const altro_status st_;

   public:
    Staged<K> sg;
  };
  altro_status HipStatus(hipError_t e) {
    ALTRO_HIP_CHECK(e);
    return ALTRO_OK;
  }
  // device records [knots][Bp][EP] (fields at off..off+E) -> host [B][knots][E]: converted on the device, one contiguous
  // copy straight into the caller's buffer
  template <class E_>
  altro_status DownloadRec(const E_* dev, int knots, int EP, int off, int E, double* out) {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    const size_t count = (size_t)B_ * knots * E;
    ALTRO_TRY(EnsureStage(count));
    hipLaunchKernelGGL((k_rec_to_rows<E_>), dim3((B_ + kBlock - 1) / kBlock, knots), dim3(kBlock), 0, stream_, dev, hm_.stage.get(), knots,
                       EP, off, E, B_, Bp_);
    ALTRO_HIP_CHECK(hipGetLastError());
    ALTRO_HIP_CHECK(CopySync(out, hm_.stage.get(), count * sizeof(double), hipMemcpyDeviceToHost));
    return ALTRO_OK;
  }
  // host [B][knots][E] (or shared [knots][E]; nullptr: zeros) -> device records [knots][Bp][EP] (padding zeroed)
  altro_status UploadRec(T* dev, int knots, int EP, int E, const double* src, bool per_instance) {
    const size_t count = (size_t)(per_instance ? B_ : 1) * knots * E;
    if (src) {
      ALTRO_TRY(EnsureStage(count));
      ALTRO_HIP_CHECK(hipMemcpyAsync(hm_.stage.get(), src, count * sizeof(double), hipMemcpyHostToDevice, stream_));
    }
    hipLaunchKernelGGL((k_rows_to_rec<T>), dim3(Bp_ / kBlock, knots), dim3(kBlock), 0, stream_, src ? (const double*)hm_.stage.get() : nullptr,
                       dev, knots, EP, E, B_, Bp_, per_instance ? 1 : 0);
    ALTRO_HIP_CHECK(hipGetLastError());
    return Sync();
  }

  altro_status SetInitialStateImpl(const ProblemSpec& s) {
    if (!uploaded_) return ALTRO_OK;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());
    // x0 records [b][nP]: one "knot" with Bp instances
    if (s.x0.empty()) return UploadRec(A_.x0, 1, R::nP, n, nullptr, false);
    return UploadRec(A_.x0, 1, R::nP, n, s.x0.data(), s.x0_per_instance != 0);
  }
  altro_status SetTrajectoryImpl(const ProblemSpec& s) {
    if (!uploaded_) return ALTRO_OK;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(Sync());  // ResetTrajectory may still be copying on the (non-blocking) stream
    const double* Xh = !s.has_X ? nullptr : (s.X_view ? s.X_view : s.X.data());
    const double* Uh = !s.has_U ? nullptr : (s.U_view ? s.U_view : s.U.data());
    ALTRO_TRY(UploadRec(A_.X, N_ + 1, R::nP, n, Xh, s.traj_per_instance != 0));
    ALTRO_TRY(UploadRec(A_.U, N_, R::mP, m, Uh, s.traj_per_instance != 0));
    ALTRO_HIP_CHECK(CopySync(up_.X_init, A_.X, (size_t)(N_ + 1) * R::nP * Bp_ * sizeof(T), hipMemcpyDeviceToDevice));
    ALTRO_HIP_CHECK(CopySync(up_.U_init, A_.U, (size_t)N_ * R::mP * Bp_ * sizeof(T), hipMemcpyDeviceToDevice));
    return ALTRO_OK;
  }

  // ---- problem upload: the steps of UploadImpl, in the order it runs them -----------------------------------
  // per-knot models (Problem::SetDynamics(model, k), problem.hpp:155-166): indices into the source's ALTRO_USER_MODELS,
  // checked before anything is allocated
  altro_status CheckKnotModels(const ProblemSpec& s) {
    for (size_t k = 0; k < s.knot_model.size() && (int)k < desc_.N; ++k) {
      const int w = s.knot_model[k];
      if (w < 0 || w >= kModelCount) {
        err_ = "altro_set_knot_models: knot " + std::to_string(k) + " asks for model " + std::to_string(w) + ", this handle's model " +
               (kModelCount > 1 ? "source lists " + std::to_string(kModelCount) + " models (ALTRO_USER_MODELS)"
                                : std::string("is a single model (a user source with #define ALTRO_USER_MODELS A, B, ... holds several)"));
        return ALTRO_INVALID_ARG;
      }
    }
    return ALTRO_OK;
  }
  // bytes of the expansion records with `columns` instances: the MFMA backward pass addresses them with 32-bit byte offsets
  size_t ExpBytes(size_t columns) const { return ((size_t)kBwdFrontPad + (size_t)N_ + 2) * RR::EP * columns * sizeof(RS); }
  // batch sizes, and the shadow columns behind the batch: the twins' columns, then the segments'
  void SizeShadowColumns() {
    B_ = desc_.batch;
    N_ = desc_.N;
    Bp_ = ((B_ + kBlock - 1) / kBlock) * kBlock;
    // Twin workgroups of the persistent kernel (TwinCtl, altro_kernels.hpp) clone an instance into a SHADOW COLUMN of the
    // per-instance arrays: every array is allocated up_.twin_cap instances wider (the stride of all of them is Bp_), one column
    // per slot of a persistent launch.  ALTRO_HIP_TWIN=0: no columns, no twins.
    up_.twin_cap = 0;
    if constexpr (kMfmaBackward) {
      if (sw_.twin && !sw_.fast_forward && !sw_.no_fused) {
        // (a solve that has split rejection streaks hands over at 3/2 of persist_at_, see Solve)
        // (at most 16384: the pool's scan packs a mailbox's position into 16 bits)
        // (at least a column per CU: a pool workgroup serves one claim and is gone, and with shares of 4 iterations the
        //  streaks of a small batch use far more claims than the batch has instances -- batch 48 / 64 with obstacles ran its
        //  pool of 64 dry half-way and walked its late streaks alone: 2.7 -> 5.9 ms warm; profiles/tail_endgame_experiments.txt)
        const int per_cu = ((num_cus_ + kBlock - 1) / kBlock) * kBlock;
        const int want = std::min({std::max(Bp_, per_cu), 16384, ((persist_at_ * 3 / 2 + 8 + kBlock - 1) / kBlock) * kBlock});
        // (only widen while the 32-bit byte offsets hold)
        if (ExpBytes((size_t)(Bp_ + want)) < (size_t)0xffffffffu) up_.twin_cap = want;
      }
    }
    // Segments of rejection streaks in the batched sweeps (DevArrays::seg_*): shadow columns [Bpad, Bpad + up_.seg_total),
    // one slice per chain of sweeps, then the twin columns.  Only for batches that run batched sweeps at all; ALTRO_HIP_SEGMENTS=0 switches it off.
    up_.seg_total = 0;
    seg_col0_ = Bp_;
    if constexpr (kMfmaBackward) {
      if (sw_.segments && !sw_.fast_forward && B_ > persist_at_) {
        // (5/8 of the batch: most of the plateau of config 3 -- a quarter of its instances, three clones each -- fits, and
        //  what the wider arrays cost a batch that never splits stays around 0.5 %: config 2 runs 0.3 % / 1 % / 2 % slower
        //  with 2048 / 3520 / 4096 unused columns behind its 4672; config 3 is as fast with 2560 as with 4096;
        //  profiles/r05_experiments.txt #3)
        const int want = (Bp_ * 5 / 8) / kBlock * kBlock;
        if (ExpBytes((size_t)(Bp_ + want + up_.twin_cap)) < (size_t)0xffffffffu) up_.seg_total = want;
      }
    }
    seg_parts_ = 4;
    Bp_ += up_.seg_total + up_.twin_cap;
  }
  // what the problem compiler needs to know of the model's user types (altro_device.hpp)
  static UserTypeTable UserTypes() {
    UserTypeTable t;
    for (int i = 0; i < UserCostList::size; ++i) t.cost_nparams.push_back(UserCostParams(i));
    for (int i = 0; i < UserConList::size; ++i) {
      int np = -1, p = -1, eq = -1;
      UserConInfo(i, &np, &p, &eq);
      t.con_nparams.push_back(np);
      t.con_p.push_back(p);
      t.con_eq.push_back(eq);
    }
    return t;
  }
  // take the compiled problem over, then the 32-bit index guard: it drops the segments' columns first, then the twins'
  altro_status AdoptProblem(const CompiledProblem<T>& cp) {
    if (cp.status != ALTRO_OK) {
      err_ = cp.err;
      return cp.status;
    }
    pd_ = cp.pd;
    knot_class_ = cp.knot_class;
    knot_rowbase_ = cp.knot_rowbase;
    con_kb_ = cp.con_kb;
    con_ke_ = cp.con_ke;
    con_p_ = cp.con_p;
    con_eq_ = cp.con_eq;
    con_knot_off_ = cp.con_knot_off;
    knot_record_ = cp.knot_record;
    const double lim = 2147483647.0;
    auto biggest = [&]() {
      return std::max({(double)(N_ + 1) * RR::EP * Bp_, (double)(N_ + 1) * nm * kLineSearchLanes * Bp_, (double)std::max(pd_.total_rows, 1) * Bp_,
                       (double)(N_ + 1) * knot_record_ * Bp_});  // (knot_par indexes the knot-parameter records with 32 bits)
    };
    // (the shadow columns widen every array; a batch that fits 32-bit indexing without them must not be refused
    //  because of them)
    if (biggest() > lim && up_.seg_total > 0) {
      Bp_ -= up_.seg_total;
      up_.seg_total = 0;
    }
    if (biggest() > lim && up_.twin_cap > 0) {
      Bp_ -= up_.twin_cap;
      up_.twin_cap = 0;
    }
    pd_.Bp = Bp_;
    if (biggest() > lim) {
      err_ = "problem too large for 32-bit device indexing (split the batch over several handles)";
      return ALTRO_UNSUPPORTED;
    }
    return ALTRO_OK;
  }
  // the per-instance device arrays, every one Bp_ columns wide
  altro_status AllocArrays() {
    A_ = HandleView();
    A_.B = B_;
    A_.Bp = Bp_;
    A_.N = N_;
    const size_t bp = Bp_, rows = pd_.total_rows;
    ALTRO_TRY(Alloc(&A_.x0, (size_t)R::nP * bp));
    ALTRO_TRY(Alloc(&A_.X, (size_t)(N_ + 1) * R::nP * bp));
    ALTRO_TRY(Alloc(&A_.U, (size_t)N_ * R::mP * bp));
    {
      // k_backward_mfma reads a zeroed pad record behind the last knot and lets its prefetch run up to
      // kBwdFrontPad records below knot 0
      const size_t front = (size_t)kBwdFrontPad * RR::EP * bp;
      RS* exp = nullptr;
      ALTRO_TRY(Alloc(&exp, front + (size_t)(N_ + 1) * RR::EP * bp + RR::EP));
      A_.EXP = exp + front;
      mfma_offsets_ok_ = (front + (size_t)(N_ + 2) * RR::EP * bp) * sizeof(RS) < (size_t)0xffffffffu;
    }
    ALTRO_TRY(Alloc(&A_.costs, (size_t)(N_ + 1) * bp));
    {
      RS* kd = nullptr;
      ALTRO_TRY(Alloc(&kd, (size_t)N_ * RR::KP * bp));
      A_.KD = kd;
    }
    ALTRO_TRY(Alloc(&A_.CTG, (size_t)(N_ + 1) * R::CP * bp + kBlock));  // (+ the junk sink of the recording backward pass)
    ALTRO_HIP_CHECK(up_.pool.alloc(&A_.trial, (size_t)(N_ + 1) * nm * kLineSearchLanes * bp));  // (the one array Alloc()'s zero fill is not spent on)
    if (sw_.poison_on) {
      std::vector<unsigned> junk((size_t)(N_ + 1) * nm * kLineSearchLanes * bp * sizeof(T) / 4);
      for (size_t i = 0; i < junk.size(); ++i) junk[i] = sw_.poison_mix ? (sw_.poison_pattern ^ ((unsigned)i * 2654435761u)) : sw_.poison_pattern;
      ALTRO_HIP_CHECK(CopySync(A_.trial, junk.data(), junk.size() * 4, hipMemcpyHostToDevice));
    }
    ALTRO_TRY(Alloc(&A_.lam, rows * bp));
    ALTRO_TRY(Alloc(&A_.pen, rows * bp));
    ALTRO_TRY(Alloc(&A_.cval, rows * bp));
    ALTRO_TRY(Alloc(&up_.d_tmp, bp));
    // mailboxes of the workers (up_.twin_cap primaries, then up_.twin_cap pool workgroups), then their state words
    if (up_.twin_cap > 0) ALTRO_TRY(Alloc(&up_.d_twin_box, TwinBoxWords()));
    if (up_.seg_total > 0) {
      // (kept out of A_: only the launches of Solve that take part in the scheme see them, SegArrays)
      ALTRO_TRY(Alloc(&up_.seg.end, bp));
      ALTRO_TRY(Alloc(&up_.seg.next, bp));
      ALTRO_TRY(Alloc(&up_.seg.flag, bp));
      ALTRO_TRY(Alloc(&up_.seg.streak, bp));
      ALTRO_TRY(Alloc(&up_.seg.tot0, bp));
      ALTRO_TRY(Alloc(&up_.seg.rho0, bp));
      ALTRO_TRY(Alloc(&up_.seg.drho0, bp));
      ALTRO_TRY(Alloc(&up_.d_seg_cursor, kMaxChains));
    }
    ALTRO_TRY(Alloc(&up_.d_list[0], bp));
    ALTRO_TRY(Alloc(&up_.d_list[1], bp));
    // the reference-term records, only for a problem with a tracking cost (a group marked kParPerKnot)
    bool tracking = false;
    for (int k = 0; k <= N_; ++k) tracking = tracking || pd_.grp[pd_.cls[knot_class_[k]].cost_group].q_pi == kParPerKnot;
    if (tracking) {
      ALTRO_TRY(Alloc(&up_.d_ref, (size_t)(N_ + 1) * kRefRT * bp));
      A_.ref = up_.d_ref;
      A_.ref_rt = kRefRT;
    }
    // the knot-parameter records, only for a problem with a knot constraint (a ConDesc marked kParPerKnotCon)
    if (knot_record_ > 0) {
      ALTRO_TRY(Alloc(&up_.d_kpar, (size_t)(N_ + 1) * knot_record_ * bp));
      A_.kpar = up_.d_kpar;
      A_.kpar_kt = knot_record_;
    }
    return ALTRO_OK;
  }
  // the chains of batched sweeps: how many, their streams, and whether those run side by side
  altro_status SetUpChains() {
    const size_t bp = Bp_;
    // four for a batch that fills the GPU several times over (measured on 4096 instances:
    // config 2 -5 %, config 3 -14 %; a quarter of a 1024-instance batch no longer fills the CUs)
    chains_ = B_ >= 2048 ? kDefaultChains : 1;
    // (the streams of a process share four hardware queues: a second engine with chains of its own would queue up
    //  behind this one's persistent kernel -- only the first large engine of a process gets them)
    if (chains_ > 1 && ChainClaim(desc_.device_id, 0) > 0) chains_ = 1;
    if (sw_.chains.set) chains_ = sw_.chains.v;
    for (;;) {
      chain_size_ = ((B_ + chains_ - 1) / chains_ + kBlock - 1) / kBlock * kBlock;
      if (chains_ == 1 || chain_size_ * (chains_ - 1) < B_) break;
      chains_--;  // (the last chain would be empty)
    }
    if (chains_ > 1) {
      ChainClaim(desc_.device_id, +1);
      counted_chained_ = true;
      ALTRO_TRY(Alloc(&up_.d_iota, bp));
      ALTRO_TRY(Alloc(&up_.d_merged, bp));
      std::vector<int> iota(bp);
      for (int i = 0; i < (int)bp; ++i) iota[i] = i;
      ALTRO_HIP_CHECK(CopySync(up_.d_iota, iota.data(), (size_t)bp * sizeof(int), hipMemcpyHostToDevice));
      for (int c = 1; c < chains_; ++c) {
        ALTRO_HIP_CHECK(hipStreamCreateWithFlags(&chain_stream_[c], hipStreamNonBlocking));
        ALTRO_HIP_CHECK(hipEventCreateWithFlags(&chain_ev_[c], hipEventDisableTiming));
      }
    }
    if (chains_ > 1 && !sw_.chains.set) return ProbeChainStreams();
    return ALTRO_OK;
  }
  // Do the chains' streams run side by side?  The streams of a process share a few hardware queues (four unless
  // GPU_MAX_HW_QUEUES says otherwise), handed out in order of creation: with other streams around (another
  // handle, a framework's stream pool, RCCL) two chains can land on one queue and take turns -- slower than one
  // chain.  One wavefront spinning for 200 us on every chain stream: side by side they take 200 us together.
  // Timed ON THE DEVICE: every spin kernel stamps its start and its end with the constant 100 MHz clock, and the
  // chains run side by side iff the intervals overlap (the latest start lies well before the earliest end).  Host
  // wall time around launches and synchronisations would also count launch latency and host jitter -- eight ranks
  // starting at once could silently lose their chains that way.
  altro_status ProbeChainStreams() {
    const long long ticks = 20000;  // of the 100 MHz constant clock: 200 us
    ALTRO_HIP_CHECK(hipStreamSynchronize(stream_));
    DevBlock<long long> stamps;  // (goes on every return, the early ones included)
    ALTRO_HIP_CHECK(stamps.alloc(2 * kMaxChains));
    long long h_stamps[2 * kMaxChains] = {0};
    long long best_overlap = -(1ll << 60);
    for (int rep = 0; rep < 2; ++rep) {  // (the first round also loads the kernel)
      for (int c = 0; c < chains_; ++c)
        hipLaunchKernelGGL((k_spin<0>), dim3(1), dim3(kBlock), 0, c == 0 ? stream_ : chain_stream_[c], ticks, stamps.get() + 2 * c);
      for (int c = 0; c < chains_; ++c) ALTRO_HIP_CHECK(hipStreamSynchronize(c == 0 ? stream_ : chain_stream_[c]));
      ALTRO_HIP_CHECK(CopySync(h_stamps, stamps.get(), sizeof(h_stamps), hipMemcpyDeviceToHost));
      long long last_start = h_stamps[0], first_end = h_stamps[1];
      for (int c = 1; c < chains_; ++c) {
        last_start = std::max(last_start, h_stamps[2 * c]);
        first_end = std::min(first_end, h_stamps[2 * c + 1]);
      }
      best_overlap = std::max(best_overlap, first_end - last_start);
    }
    chain_overlap_ticks_ = best_overlap;
    if (best_overlap < ticks / 2) {  // two of them ran (mostly) one after the other
      DropChains();
      chain_size_ = Bp_;
    }
    return ALTRO_OK;
  }
  // the problem's data on the device: parameter pools, knot tables, penalty scaling, description, per-instance scalars
  altro_status UploadProblemData(const ProblemSpec& s, const CompiledProblem<T>& cp) {
    const size_t bp = Bp_;
    const std::vector<T>& pool = cp.pool;
    const std::vector<std::vector<T>>& ip = cp.ip;
    ALTRO_TRY(Alloc(&up_.X_init, (size_t)(N_ + 1) * R::nP * bp));
    ALTRO_TRY(Alloc(&up_.U_init, (size_t)N_ * R::mP * bp));
    T* dpool = nullptr;
    T* dipool = nullptr;
    ALTRO_TRY(Alloc(&dpool, pool.size()));
    ALTRO_TRY(Alloc(&dipool, ip.size() * bp));
    if (!pool.empty())
      ALTRO_HIP_CHECK(CopySync(dpool, pool.data(), pool.size() * sizeof(T), hipMemcpyHostToDevice));
    if (!ip.empty()) {
      std::vector<T> flat(ip.size() * bp, T(0));
      for (size_t sl = 0; sl < ip.size(); ++sl)
        for (int b = 0; b < B_; ++b) flat[sl * bp + b] = ip[sl][b];
      ALTRO_HIP_CHECK(CopySync(dipool, flat.data(), flat.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    A_.pool = dpool;
    A_.ipool = dipool;
    int *dkc = nullptr, *dkr = nullptr;
    ALTRO_TRY(Alloc(&dkc, N_ + 1));
    ALTRO_TRY(Alloc(&dkr, N_ + 1));
    ALTRO_HIP_CHECK(CopySync(dkc, knot_class_.data(), (N_ + 1) * sizeof(int), hipMemcpyHostToDevice));
    ALTRO_HIP_CHECK(CopySync(dkr, knot_rowbase_.data(), (N_ + 1) * sizeof(int), hipMemcpyHostToDevice));
    A_.knot_class = dkc;
    A_.knot_rowbase = dkr;
    ALTRO_TRY(Alloc(&up_.d_phi, kMaxClasses * kMaxConPerKnot));
    {
      std::vector<double> v(kMaxClasses * kMaxConPerKnot, s.phi >= 1.0 ? s.phi : 10.0);  // constraint_values.hpp:30
      ALTRO_HIP_CHECK(CopySync(up_.d_phi, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    A_.phi = up_.d_phi;
    ALTRO_TRY(Alloc(&up_.d_pd, 1));
    ALTRO_HIP_CHECK(CopySync(up_.d_pd, &pd_, sizeof(pd_), hipMemcpyHostToDevice));
    // per-instance scalar state, one slab each so GetStats is two copies
    ALTRO_TRY(Alloc(&up_.d_scalarT, (size_t)kNumScalarT * bp));
    ALTRO_TRY(Alloc(&up_.d_scalarI, (size_t)kNumScalarI * bp));
    double** tp[kNumScalarT] = {&A_.rho_reg, &A_.drho,     &A_.dV0,  &A_.dV1,  &A_.J0,
                           &A_.initial_cost, &A_.cost_cur, &A_.cost_prev, &A_.dJ, &A_.grad,
                           &A_.viol,    &A_.penmax,   &A_.alpha, &A_.z,   &A_.reg_log};
    for (int i = 0; i < kNumScalarT; ++i) *tp[i] = up_.d_scalarT + (size_t)i * bp;
    int** ipn[kNumScalarI] = {&A_.status, &A_.status_al, &A_.it_inner, &A_.it_outer,
                              &A_.it_total, &A_.phase,   &A_.need_init_cost};
    for (int i = 0; i < kNumScalarI; ++i) *ipn[i] = up_.d_scalarI + (size_t)i * bp;
    std::vector<int> ones(bp, ALTRO_UNSOLVED);
    ALTRO_HIP_CHECK(CopySync(A_.status, ones.data(), bp * sizeof(int), hipMemcpyHostToDevice));
    ALTRO_HIP_CHECK(CopySync(A_.status_al, ones.data(), bp * sizeof(int), hipMemcpyHostToDevice));
    return ALTRO_OK;
  }
  // ---- LDS plan of the forward pass ---------------------------------------------------------------------------
  static size_t PadV(size_t e) { return (e + R::V - 1) / R::V * R::V; }
  // (+ the optional padding between the instances' blocks of a workgroup: FwdLds::total)
  static size_t PaddedBlock(size_t bytes) { return bytes + (size_t)fwd_block_pad_bytes((long long)bytes); }
  // LDS of one instance that keeps only the multipliers and the per-instance parameters (k_forward2<.., kSrcGlb>)
  size_t PerInstGlbBytes() const { return PaddedBlock((2 * PadV((size_t)pd_.total_rows) + PadV((size_t)pd_.nslots)) * sizeof(T)); }
  // workgroups of kernel fn (kFwdWaves waves, lds_wg bytes of LDS each) that a CU holds at once: the minimum of the
  // register limit -- waves per SIMD of the kernel * 4 SIMDs / kFwdWaves -- and the LDS limit; 0 if the kernel is unknown
  static int WorkgroupsPerCu(const void* fn, size_t lds_wg) {
    hipFuncAttributes at{};
    if (hipFuncGetAttributes(&at, fn) != hipSuccess || at.numRegs <= 0) return 0;
    const int waves = std::min(8, 512 / ((at.numRegs + 7) / 8 * 8));  // per SIMD
    return std::min(waves * 4 / kFwdWaves, (int)(160 * 1024 / lds_wg));
  }
  // The k_forward2 variant of this upload's plan (kdg_, rg_), named once: f gets the source as a compile-time constant.
  template <class F>
  void WithForwardSrc(F&& f) const {
    if (kdg_) {
      if constexpr (kKdgEligible) f(std::integral_constant<int, kSrcKdg>{});
    } else if (rg_) {
      if constexpr (kRgEligible) f(std::integral_constant<int, kSrcGlb>{});
    } else {
      f(std::integral_constant<int, kSrcLds>{});
    }
  }
  // Every instantiated k_sweep_fused variant, listed once: f(FusedVariant<circles, speculation, segments>) for each.
  // (the two variants that know the segments of rejection streaks: default speculation modes only, see LaunchTail)
  template <bool CC, int S, bool SEG = false>
  struct FusedVariant {
    static constexpr bool circles = CC, segments = SEG;
    static constexpr int spec = S;
    static const void* Fn() { return reinterpret_cast<const void*>(&k_sweep_fused<T, M, CC, S, SEG>); }
  };
  template <class F>
  static void ForEachFusedVariant(F&& f) {
    f(FusedVariant<false, kSpecFree, true>{});
    f(FusedVariant<true, kSpecWave, true>{});
    f(FusedVariant<false, kSpecOff>{});
    f(FusedVariant<true, kSpecOff>{});
    f(FusedVariant<false, kSpecWave>{});
    f(FusedVariant<true, kSpecWave>{});
    f(FusedVariant<false, kSpecFree>{});
    f(FusedVariant<true, kSpecFree>{});
  }
  // Up to 3 instances per wavefront, at most 80 KiB per workgroup (two workgroups per CU); if even one instance does not
  // fit in 160 KiB, read from HBM instead.  Then the variants that keep less in LDS, and the kernels' LDS attributes.
  altro_status PlanForwardLds() {
    const size_t rows = pd_.total_rows;
    const size_t per_inst = PaddedBlock(((size_t)(N_ + 1) * R::nP + (size_t)N_ * R::mP + (size_t)N_ * R::KP +
                                         2 * PadV(rows) + PadV((size_t)pd_.nslots)) * sizeof(T));
    const int lanes_max = lanes_per_wave();
    fwd_per_wave_ = lanes_max;
    while (fwd_per_wave_ > 1 && fwd_per_wave_ * per_inst > 80 * 1024) fwd_per_wave_--;
    const size_t shared_bytes = (PadV((size_t)pd_.npool) + kFwdSlots * (size_t)nm * kBlock) * sizeof(T) + 2 * kBlock * sizeof(int) +
                                kBlock * sizeof(double);
    while (fwd_per_wave_ > 1 && shared_bytes + fwd_per_wave_ * per_inst > 80 * 1024) fwd_per_wave_--;
    if (sw_.fwd_per_wave.set) fwd_per_wave_ = std::max(1, std::min(fwd_per_wave_, sw_.fwd_per_wave.v));
    fwd_lds_bytes_ = shared_bytes + fwd_per_wave_ * per_inst;
    fwd_shared_bytes_ = shared_bytes;
    fwd_per_inst_bytes_ = per_inst;
    // the persistent kernel takes its pointers from the same struct (FusedLds, altro_common.hpp)
    fused_lds_bytes_ = FusedLds<T>{FwdLds<T>{(N_ + 1) * R::nP, N_ * R::mP, N_ * R::KP, pd_.total_rows, pd_.nslots, R::V}, N_, nm, pd_.npool}.bytes();
    kdg_ = false;
    rg_ = false;
    if constexpr (kRgEligible && !kKdgEligible) PlanForwardGlbSmall(shared_bytes, per_inst);
    if constexpr (kKdgEligible) PlanForwardLarge(shared_bytes, per_inst);
    if (fwd_lds_bytes_ > 160 * 1024) {
      fwd_lds_bytes_ = 0;
      fwd_per_wave_ = lanes_max;
    } else if (fwd_lds_bytes_ > 64 * 1024) {
      hipError_t e = hipSuccess;
      WithForwardSrc([&](auto src) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_forward2<T, M, decltype(src)::value>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)fwd_lds_bytes_);
      });
      ALTRO_HIP_CHECK(e);
    }
    if constexpr (kMfmaBackward) {
      if (fused_lds_bytes_ > 64 * 1024 && fused_lds_bytes_ <= 160 * 1024) {
        hipError_t e = hipSuccess;
        ForEachFusedVariant([&](auto v) {
          if (e == hipSuccess) e = hipFuncSetAttribute(decltype(v)::Fn(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fused_lds_bytes_);
        });
        ALTRO_HIP_CHECK(e);
      }
    }
    return ALTRO_OK;
  }
  // Small models: the rollout wave reads (xbar, ubar, K, d) from global memory two knots ahead; LDS keeps only the
  // multipliers and the parameters, so that four workgroups (the register limit) instead of two share a CU.
  // Needs the winner-only gradient measure of phase 2, whose terms live in the hand-off slots.
  void PlanForwardGlbSmall(size_t shared_bytes, size_t per_inst) {
    const int lanes_max = lanes_per_wave();
    const size_t per_inst_g = PerInstGlbBytes();
    // Taken when it lets more instances be resident on a CU than the fully staged variant (WorkgroupsPerCu).  Config 3
    // (fp32 records: 152 VGPRs, three waves per SIMD): 6 -> 9 instances, -7 % per forward sweep; config 2 (fp64 records in
    // flight: 171 VGPRs, two waves per SIMD): 6 -> 6, and the staged variant is 2 % faster.  ALTRO_HIP_FWD_SRC=lds / global
    // override the choice.
    bool want = false;
    if (sw_.fwd_src != kFwdSrcAuto) {
      want = sw_.fwd_src == kFwdSrcGlobal;
    } else if (fwd_per_wave_ == lanes_max) {
      want = WorkgroupsPerCu(reinterpret_cast<const void*>(&k_forward2<T, M, kSrcGlb>), shared_bytes + lanes_max * per_inst_g) >
             WorkgroupsPerCu(reinterpret_cast<const void*>(&k_forward2<T, M, kSrcLds>), shared_bytes + lanes_max * per_inst);
    } else {
      want = true;  // the staged block does not even allow three instances per workgroup
    }
    if (want && 16 + lanes_max * N_ <= kFwdSlots * nm * kBlock && shared_bytes + lanes_max * per_inst_g <= 80 * 1024) {
      rg_ = true;
      fwd_per_wave_ = lanes_max;
      if (sw_.fwd_per_wave.set) fwd_per_wave_ = std::max(1, std::min(fwd_per_wave_, sw_.fwd_per_wave.v));
      fwd_per_inst_bytes_ = per_inst_g;
      fwd_lds_bytes_ = shared_bytes + fwd_per_wave_ * per_inst_g;
    }
  }
  // Models whose gain records fill the LDS (12-state model: 83 of 134 KB per instance -> one instance per CU):
  // keep only d in LDS, let the rollout wave read K from global memory one knot ahead, and put up to three
  // instances into one workgroup (one workgroup per CU, 160 KiB)
  void PlanForwardLarge(size_t shared_bytes, size_t per_inst) {
    const int lanes_max = lanes_per_wave();
    const size_t per_inst_b = PaddedBlock(((size_t)(N_ + 1) * R::nP + (size_t)N_ * R::mP + (size_t)N_ * R::mP +
                                           2 * PadV((size_t)pd_.total_rows) + PadV((size_t)pd_.nslots)) * sizeof(T));
    int pw_b = lanes_max;
    while (pw_b > 1 && shared_bytes + pw_b * per_inst_b > 160 * 1024) pw_b--;
    if (shared_bytes + per_inst > 80 * 1024 && pw_b > 1) {
      kdg_ = true;
      fwd_per_wave_ = pw_b;
      fwd_per_inst_bytes_ = per_inst_b;
      fwd_lds_bytes_ = shared_bytes + pw_b * per_inst_b;
    }
    // Round 6: ... or NOTHING of the trajectory and the gains in LDS (k_forward2<.., kSrcGlb> for the large
    // models: the rollout wave reads xbar, ubar, K, d from global memory one knot ahead, the gain record in its storage
    // type; one barrier per knot, so two hand-off slots instead of four).  What is left -- the multipliers and the slots --
    // lets TWO workgroups share a CU's LDS, and the variant is compiled for two waves per SIMD (256 registers): config 4
    // keeps 4 instances on a CU instead of 2, its 512 forward workgroups run in ONE round instead of two.  Taken when it
    // raises the instances resident on a CU (ALTRO_HIP_FWD_SRC=kdg | global overrides).
    const size_t shared_g = (PadV((size_t)pd_.npool) + 2 * (size_t)fwd_sync_batched<M, kSrcGlb>() * nm * kBlock) * sizeof(T) +
                            2 * kBlock * sizeof(int) + kBlock * sizeof(double);
    const size_t per_inst_g = PerInstGlbBytes();
    int pw_g = lanes_max;
    while (pw_g > 1 && shared_g + pw_g * per_inst_g > 80 * 1024) pw_g--;
    // (0 workgroups: the kernel is unknown, or its block does not fit a CU's 160 KiB)
    const int wgs_g = WorkgroupsPerCu(reinterpret_cast<const void*>(&k_forward2<T, M, kSrcGlb>), shared_g + pw_g * per_inst_g);
    const int resident_g = wgs_g * pw_g, resident_now = kdg_ ? fwd_per_wave_ : (int)std::max<size_t>(1, 160 * 1024 / std::max<size_t>(1, fwd_lds_bytes_)) * fwd_per_wave_;
    const bool want = sw_.fwd_src != kFwdSrcAuto ? sw_.fwd_src == kFwdSrcGlobal : resident_g > resident_now;
    if (want && wgs_g > 0 && 16 + pw_g * N_ <= 2 * fwd_sync_batched<M, kSrcGlb>() * nm * kBlock) {
      kdg_ = false;
      rg_ = true;
      fwd_per_wave_ = pw_g;
      fwd_shared_bytes_ = shared_g;
      fwd_per_inst_bytes_ = per_inst_g;
      fwd_lds_bytes_ = shared_g + pw_g * per_inst_g;
    }
  }
  // The device-side sweep loop (k_sweep_loop, round 6): persistent workgroups of the forward pass's shape that run
  // E -> B -> F for the instances in their slots; as many workgroups as the GPU holds at once (registers: two waves per
  // SIMD; LDS: the forward block, which the gain buffer of the backward pass shares), never more than the batch fills.
  altro_status PlanSweepLoop() {
    up_.loop_groups = 0;
    if constexpr (kMfmaBackward) {
      if (sw_.sweep_loop != 0 && fwd_lds_bytes_ > 0 && !kdg_ && fwd_per_wave_ == lanes_per_wave() && B_ > persist_at_) {
        const size_t bwd_bytes = ((size_t)kBwdChunk * 4 * RR::KP + kBlock) * sizeof(double);  // (backward_mfma_body's sKD)
        loop_lds_bytes_ = std::max(fwd_lds_bytes_, bwd_bytes);
        const void* fn = rg_ ? LoopKernel<kSrcGlb>() : LoopKernel<kSrcLds>();
        if (fn && loop_lds_bytes_ <= 160 * 1024) {
          if (loop_lds_bytes_ > 64 * 1024)
            ALTRO_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)loop_lds_bytes_));
          int per_cu = 0;
          ALTRO_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kFwdWaves * kBlock, loop_lds_bytes_));
          if (sw_.loop_per_cu.set) per_cu = std::max(1, std::min(per_cu, sw_.loop_per_cu.v));
          const int slots = lanes_per_wave();
          up_.loop_groups = std::max(0, std::min(per_cu * num_cus_, (B_ + slots - 1) / slots));
          loop_per_cu_ = per_cu;
          // WHEN it takes the bulk phase (measured, profiles/r06_experiments.txt #1): a batch that fits the slots of the
          // resident workgroups (two per CU, three slots each: 1536 instances on an MI355X) runs as fast (kTurn90) or up to
          // 23 % faster (obstacles, 1024 instances) than the host-paced sweeps, with no host in the loop; a larger batch is
          // worked off in generations -- slots refilled as instances finish -- at 1536 instances in flight against the
          // sweeps' whole batch over four chains, and is 15 - 25 % slower (4096 kTurn90: 7.5 against 6.3 ms).  So: the
          // loop by default iff the batch fits the slots; ALTRO_HIP_SWEEP_LOOP=1 forces it for any batch, =0 never.
          if (sw_.sweep_loop != 1 && B_ > per_cu * num_cus_ * slots) up_.loop_groups = 0;
        }
        if (up_.loop_groups > 0) {
          ALTRO_TRY(Alloc(&up_.d_loop_win, (size_t)up_.loop_groups * 4));
          ALTRO_TRY(Alloc(&up_.d_loop_ctl, (size_t)kLwWords + kRwWords));  // (+ the words the persistent tail kernel reports)
          ALTRO_TRY(Alloc(&up_.d_loop_tail, (size_t)B_ + 16));
        }
      }
    }
    return ALTRO_OK;
  }
  // the list of per-knot models, if any knot asks for another than model 0
  altro_status UploadKnotModels(const ProblemSpec& s) {
    if (s.knot_model.empty()) return ALTRO_OK;
    bool any = false;
    for (int k = 0; k < N_; ++k) any = any || s.knot_model[k] != 0;
    if (!any) return ALTRO_OK;
    int* dkm = nullptr;
    ALTRO_TRY(Alloc(&dkm, (size_t)N_ + 1));
    std::vector<int> km(s.knot_model.begin(), s.knot_model.begin() + N_);
    km.push_back(0);
    ALTRO_HIP_CHECK(CopySync(dkm, km.data(), km.size() * sizeof(int), hipMemcpyHostToDevice));
    A_.knot_model = dkm;
    return ALTRO_OK;
  }
  // Build the device state of the problem from the recorded setter calls.
  altro_status UploadImpl(const ProblemSpec& s) {
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    ALTRO_TRY(CheckKnotModels(s));
    SizeShadowColumns();
    const CompiledProblem<T> cp = CompileProblem<T>(s, n, m, N_, B_, UserTypes());
    ALTRO_TRY(AdoptProblem(cp));
    ALTRO_TRY(AllocArrays());
    ALTRO_TRY(SetUpChains());
    ALTRO_TRY(UploadProblemData(s, cp));
    ALTRO_TRY(PlanForwardLds());
    ALTRO_TRY(PlanSweepLoop());
    // candidates of the batched line search: the first 6 trials and the last live one own a slot, deeper winners are
    // replayed (CandLayout); ALTRO_HIP_CAND_FRONT=19 stores every trial (round 3), 0 replays every accepted trial (tests).
    // Measured (ms per solve, configs 2 / 3 / 4): front 19: 8.31 / 39.9 / 5.78; 12: 8.15 / 39.5 / 5.75; 8: 8.04 / 38.8 / 5.70;
    // 6: 7.91 / 38.7 / 5.65; 4: 7.96 / 38.8 / 5.62 (profiles/r04_experiments.txt)
    A_.cand_front = sw_.cand_front;
    A_.xcd_remap = 1;  // (0: workgroup i takes slot block i, round 3)
    ALTRO_TRY(UploadKnotModels(s));
    uploaded_ = true;
    // penalties start at one (constraint_values.hpp:44); an earlier SetPenalty overrides
    hipLaunchKernelGGL(k_set_rows<T>, GridB(), dim3(kBlock), 0, stream_, A_, up_.d_pd, 0, 1,
                       T(s.penalty >= 0 ? s.penalty : 1.0));
    altro_status st = Sync();
    if (st == ALTRO_OK) st = SetInitialStateImpl(s);
    if (st == ALTRO_OK) st = SetKnotTimesImpl(s);
    if (st == ALTRO_OK) st = SetTrajectoryImpl(s);
    if (st == ALTRO_OK && s.ref_rows > 0) {  // altro_set_reference / altro_set_reference_offset issued before the upload
      st = SetReference(s.ref_X.data(), s.ref_U.empty() ? nullptr : s.ref_U.data(), s.ref_rows, s.ref_per_instance, 0);
      if (st == ALTRO_OK && s.ref_offset > 0) st = SetReferenceOffset(s.ref_offset);
    } else if (st == ALTRO_OK) {
      up_.ref_offset = s.ref_offset;
    }
    // the knot constraints, and whatever altro_set_constraint_track / altro_set_track_offset recorded before the upload
    up_.kcons.clear();
    for (size_t i = 0; i < s.cons.size() && st == ALTRO_OK; ++i) {
      if (con_knot_off_[i] < 0) continue;
      KnotCon c;
      c.index = (int)i;
      c.k_begin = s.cons[i].k_begin;
      c.k_end = s.cons[i].k_end;
      c.np = s.cons[i].nparams;
      c.off = con_knot_off_[i];
      c.kind = s.cons[i].kind;
      up_.kcons.push_back(std::move(c));
    }
    if (st == ALTRO_OK) up_.track_offset = s.track_offset;
    for (size_t i = 0; i < s.cons.size() && st == ALTRO_OK; ++i)
      if (con_knot_off_[i] >= 0 && s.cons[i].track_rows > 0)
        st = SetConstraintTrack((int)i, s.cons[i].track.data(), s.cons[i].track_rows, s.cons[i].track_per_instance, 0);
    // (a failed upload leaves the engine as it was before it -- Upload() drops whatever a failed UploadImpl built: the
    //  C-ABI keeps the handle "not uploaded" and the next call uploads again instead of meeting "problem definition changed")
    return st;
  }
  // ALTRO_HIP_DEBUG_POISON: shadow columns (segments of the batched sweeps, twins of the persistent kernel) start every
  // solve full of NaN words (k_poison_columns)
  void PoisonShadowColumns() {
    if (!sw_.poison_on || up_.seg_total + up_.twin_cap <= 0) return;
    const unsigned col0 = (unsigned)(Bp_ - up_.seg_total - up_.twin_cap), ncols = (unsigned)(up_.seg_total + up_.twin_cap);
    auto fill = [&](void* arr, size_t rows, size_t bytes_per_column_row) {
      if (!arr || rows == 0) return;
      hipLaunchKernelGGL((k_poison_columns<0>), dim3(1024), dim3(256), 0, stream_, (unsigned*)arr, (unsigned)rows, (unsigned)Bp_, col0, ncols,
                         (unsigned)(bytes_per_column_row / 4), sw_.poison_pattern, sw_.poison_mix);
    };
    fill(A_.X, N_ + 1, R::nP * sizeof(T));
    fill(A_.U, N_, R::mP * sizeof(T));
    fill(A_.x0, 1, R::nP * sizeof(T));
    fill(A_.costs, N_ + 1, sizeof(T));
    fill(A_.lam, pd_.total_rows, sizeof(T));
    fill(A_.pen, pd_.total_rows, sizeof(T));
    fill(A_.cval, pd_.total_rows, sizeof(T));
    fill((void*)A_.EXP, N_ + 1, RR::EP * sizeof(RS));
    fill((void*)A_.KD, N_, RR::KP * sizeof(RS));
  }
  // ---- the sweep loop -----------------------------------------------------------------------------
  hipEvent_t ProfEvent(size_t i) {
    while (prof_ev_.size() <= i) {
      hipEvent_t e;
      hipEventCreate(&e);
      prof_ev_.push_back(e);
    }
    return prof_ev_[i];
  }
  // One chain of batched sweeps: the instances [lo, hi) of the batch, swept on a stream of their own.  A large batch runs
  // as up to four chains (chains_): the three kernels of a sweep follow each other on one stream -- a latency-bound
  // backward launch, as long as its unluckiest instance, between two throughput-bound ones, and a forward launch whose
  // last round of workgroups leaves most CUs idle -- and chains that drift out of phase fill each other's gaps.  The
  // persistent tail kernel takes the lists all chains leave behind in ONE launch.
  struct Chain {
    int lo = 0, hi = 0;
    hipStream_t st = nullptr;
    int* d_cnt = nullptr;            // this chain's block of device counters (one per sweep; cursors of the list rebuilds)
    volatile int* h_cnt = nullptr;   // ... of host-mapped words (the counts the sweeps publish)
    int* h_cnt_dev = nullptr;
    int sweeps = 0;                  // sweeps enqueued
    int known = 0;                   // newest count the host knows (an upper bound of what the next sweep works on)
    bool waiting = false, done = false, tail = false;
    bool last_split = false;         // the sweep enqueued last was allowed to split rejection streaks (its list may outgrow `known`)
    bool split_seen = false;         // ... some sweep of this chain was: its slice of shadow columns may hold instances
    std::vector<size_t> ev;          // profiler events: chain start, then three per sweep
  };

  // What one call of Solve knows: its options, the launch policy it settled on, the chains, and what has been launched.
  struct SolveRun {
    std::chrono::steady_clock::time_point t0;
    DevOpts d{};
    int mode = 0;
    bool prof = false;
    size_t nev = 0;          // profiler events used so far
    int max_sweeps = 0;      // upper bound on the sweeps of a chain
    int C = 1, cstride = 0;  // chains, and the counter words of each
    bool fused_ok = false;   // the persistent tail kernel can run (FusedOk)
    bool loop_on = false;    // the device-side sweep loop takes the bulk phase
    bool seg_on = false;     // rejection streaks may split into segments
    int seg_capc = 0;        // shadow columns per chain
    int seg_below = 0, seg_above = 0;  // streaks split while the instances left lie in (seg_above, seg_below]
    int seg_persist_at = 0;            // hand-over to the persistent kernel once a chain has split
    Chain chain[kMaxSweepChains];
    bool tail_mode = false;  // the persistent kernel takes over: every chain stops at its next sweep boundary
    bool loop_launched = false, persistent_launched = false;
    size_t loop_ev = 0, fused_ev = 0;  // first profiler event of the two launches
    int loop_handover = 0;
    bool nap_ok = false, nap = false;  // the host may nap while it waits / has begun to
    unsigned spins = 0, naps = 0;      // polls / naps of the scheduler since a chain last made progress
  };
  // (the kernels only see the segments' arrays -- and pay for the bookkeeping of streaks, a few dependent words per instance
  //  and sweep -- from sweep kSegFrom of a chain on: a batch whose sweeps are over by then, config 2, never does)
  static constexpr int kSegFrom = 24;

  // One solve: the steps below, in this order.
  altro_status Solve(const altro_options& o, int mode) {
    if (!StepOk() || !RefOk()) return ALTRO_NOT_READY;
    ALTRO_HIP_CHECK(hipSetDevice(desc_.device_id));
    if (mask_.on) {
      // a solve mask (include/altro_subset.h): the start of the solve, the first sweep of every chain and a tail that
      // starts at once take the compacted lists instead of "everyone"; everything behind them runs on lists anyway
      if (A_.record_ctg) {
        // (ReplayCtg and the batched backward kernels' records cover whole batches: a masked-out instance's records
        //  would not stay what they were)
        err_ = "a masked solve does not record the cost-to-go (altro_set_record_ctg): clear the mask or switch the records off";
        return ALTRO_UNSUPPORTED;
      }
      // (not inside a triggered run: hm_.mask is the coming solve's there, and the sum would bring every instance's count to
      //  the host between two cycles; LoopEnd sums what the run's last solve ran)
      if (!hm_.run.masked) ALTRO_TRY(SumInstanceIterations());
      ALTRO_TRY(Recompact());
      if (mask_.total == 0) {  // nobody takes part: nothing is launched, nothing changes
        std::memset(&timing_, 0, sizeof(timing_));
        return ALTRO_OK;
      }
    }
    SolveRun r;
    ALTRO_TRY(StartRun(r, o, mode));
    ALTRO_TRY(BeginSolve(r));
    ALTRO_TRY(PlanRun(r));
    StartChains(r);
    ALTRO_TRY(LaunchSweepLoop(r));
    ALTRO_TRY(RunChains(r));
    ALTRO_TRY(LaunchTail(r));
    ALTRO_TRY(WaitForDevice(r));
    ALTRO_TRY(SegFixup(r));
    ALTRO_TRY(ReadBackCounters(r));
    if (r.prof) AccountProfile(r);
    timing_.instance_iterations = -1;  // summed on demand (GetTiming): keeps a copy out of every solve
    timing_.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r.t0).count();
    if (!lqr_policy_.empty()) {
      // the gain policy (include/altro_lqr.h): the tracking gains of the plan this solve left replace the solver's, for the
      // instances it ran
      ALTRO_TRY(LaunchLqr(lqr_policy_, 1, mask_.on ? hm_.mask.get() : nullptr, nullptr, nullptr, nullptr));
      ALTRO_TRY(Sync());
    }
    return ALTRO_OK;
  }
  // host state of a solve: options, flags of the results, the bound on the sweeps and the counters that go with it
  altro_status StartRun(SolveRun& r, const altro_options& o, int mode) {
    r.t0 = std::chrono::steady_clock::now();
    r.d = ToDevOpts(o);
    r.d.fast_forward_stalls = sw_.fast_forward ? 1 : 0;
    r.mode = mode;
    r.prof = o.profiler_enable != 0;
    last_mode_ilqr_ = (mode == kFwdILQR);
    last_opts_ = r.d;
    ctg_fresh_ = A_.record_ctg != 0;  // (recorded by the batched backward kernels of this solve, or readable through ReplayCtg)
    ctg_replayable_ = !mask_.on;  // (a replay recomputes every instance's records from what it finds)
    last_solve_masked_ = mask_.on;
    std::memset(&timing_, 0, sizeof(timing_));
    cur_ = stream_;
    PoisonShadowColumns();
    // upper bound on sweeps: every sweep advances every active instance by one inner iteration
    // (64-bit product, clamped: the counters of the sweeps live in a pinned array of this length)
    const long long inner_outer = (long long)std::max(1, o.max_iterations_inner) *
                                  (long long)std::max(1, (mode == kFwdAL) ? o.max_iterations_outer : 1);
    r.max_sweeps =
        (int)std::max<long long>(1, std::min<long long>({(long long)o.max_iterations_total, inner_outer, 1LL << 20})) + 2;
    // Sweep i of a chain works on the instances that its sweep i-1 left active: a dense list built by the forward
    // kernel (two list buffers, one counter per sweep).  Sweep i+1's first kernel publishes the
    // length of its list (= what sweep i left) to pinned host memory; the host polls that word,
    // stays one sweep ahead of the device, and sizes each grid with the newest count it knows --
    // counts only shrink, so it is an upper bound -- so tail sweeps launch a handful of workgroups.
    r.C = chains_;
    r.cstride = 2 * (r.max_sweeps + 12);  // per chain: counts [0, max_sweeps + 2), results of the persistent kernel
                                          // [max_sweeps + 2, + 10), cursors of the list rebuilds (dense sweeps) in the second half
    return ReserveCounters(r.C * r.cstride + 16);
  }
  // the start of a solve on the engine's stream: one merged launch, or (ALTRO_HIP_BEGIN_SOLVE=split) its seven stream operations
  altro_status BeginSolve(SolveRun& r) {
    const DevOpts& d = r.d;
    const int mode = r.mode;
    const size_t counter_words = (size_t)(r.C * r.cstride + 16);
    if (r.prof) hipEventRecord(ProfEvent(r.nev++), stream_);
    twin_box_clean_ = false;
    if (sw_.begin_merged) {
      // ONE launch (k_begin_solve): AL Init, SolveSetup, activation, the open-loop rollout, and the clearing of the shadow
      // columns' flags (no shadow column starts a solve as an active instance, whatever the last solve left in it: the
      // dense expansion launches rebuild their lists from these flags), of the sweep counters and of the twins' mailboxes
      DevArrays<T> As = A_;
      if (up_.seg_total > 0) SegArrays(As);  // (resets the bookkeeping of the segments, DevArrays::seg_*)
      ZeroJobs z{};
      int nz = 0;
      auto zero = [&](void* ptr, size_t words) {
        if (nz >= kZeroJobs || !ptr || words == 0 || words > 0xffffffffull) return false;  // (the caller falls back to a memset)
        z.p[nz] = reinterpret_cast<unsigned*>(ptr);
        z.n[nz++] = (unsigned)words;
        return true;
      };
      if (up_.seg_total + up_.twin_cap > 0 && !zero(A_.phase + (Bp_ - up_.seg_total - up_.twin_cap), (size_t)(up_.seg_total + up_.twin_cap)))
        ALTRO_HIP_CHECK(hipMemsetAsync(A_.phase + (Bp_ - up_.seg_total - up_.twin_cap), 0, (size_t)(up_.seg_total + up_.twin_cap) * sizeof(int), stream_));
      if (!zero(hm_.d_counter.get(), counter_words))
        ALTRO_HIP_CHECK(hipMemsetAsync(hm_.d_counter.get(), 0, counter_words * sizeof(int), stream_));
      if (up_.twin_cap > 0) twin_box_clean_ = zero(up_.d_twin_box, TwinBoxWords() * 2);  // (else: cleared at the launch)
      size_t words = 0;
      for (int j = 0; j < nz; ++j) words += z.n[j];
      const int gx = (B_ + kBlock - 1) / kBlock;
      const int rows_y = (mode == kFwdAL) ? std::max(1, (pd_.total_rows + kAlInitRows - 1) / kAlInitRows) : 0;
      const int zero_y = (int)std::min<size_t>(32, std::max<size_t>(1, words / ((size_t)gx * kBlock * 16)));
      if (mask_.on)
        hipLaunchKernelGGL((k_begin_solve_masked<T, M>), dim3(gx, 1 + rows_y + zero_y), dim3(kBlock), 0, stream_, As, up_.d_pd, d,
                           mode == kFwdAL ? 1 : 0, rows_y, z, (const unsigned char*)hm_.mask.get());
      else
        hipLaunchKernelGGL((k_begin_solve<T, M>), dim3(gx, 1 + rows_y + zero_y), dim3(kBlock), 0, stream_, As, up_.d_pd, d,
                           mode == kFwdAL ? 1 : 0, rows_y, z);
      timing_.launches += 1;
    } else {
      const unsigned char* const mk = hm_.mask.get();
      if (mode == kFwdAL) {
        if (mask_.on)
          hipLaunchKernelGGL(k_al_init_masked<T>, GridAlInit(), dim3(kBlock), 0, stream_, A_, up_.d_pd, d, mk);
        else
          hipLaunchKernelGGL(k_al_init<T>, GridAlInit(), dim3(kBlock), 0, stream_, A_, up_.d_pd, d);
      }
      if (up_.seg_total + up_.twin_cap > 0)
        ALTRO_HIP_CHECK(hipMemsetAsync(A_.phase + (Bp_ - up_.seg_total - up_.twin_cap), 0, (size_t)(up_.seg_total + up_.twin_cap) * sizeof(int), stream_));
      {
        DevArrays<T> As = A_;
        if (up_.seg_total > 0) SegArrays(As);
        if (mask_.on)
          hipLaunchKernelGGL(k_solve_setup_masked<T>, GridB(), dim3(kBlock), 0, stream_, As, d, 1, mk);
        else
          hipLaunchKernelGGL(k_solve_setup<T>, GridB(), dim3(kBlock), 0, stream_, As, d, 1);
      }
      if (mask_.on)
        hipLaunchKernelGGL((k_rollout_masked<T, M>), GridB(), dim3(kBlock), 0, stream_, A_, up_.d_pd, 1, mk);
      else
        hipLaunchKernelGGL((k_rollout<T, M>), GridB(), dim3(kBlock), 0, stream_, A_, up_.d_pd, 1);
      timing_.launches += (mode == kFwdAL) ? 3 : 2;
      ALTRO_HIP_CHECK(hipMemsetAsync(hm_.d_counter.get(), 0, counter_words * sizeof(int), stream_));
    }
    if (r.prof) hipEventRecord(ProfEvent(r.nev++), stream_);
    ALTRO_HIP_CHECK(hipGetLastError());
    return ALTRO_OK;
  }
  // the launch policy of this solve: device-side loop or host-paced chains, segments of rejection streaks, host naps
  altro_status PlanRun(SolveRun& r) {
    r.fused_ok = FusedOk(r.d);
    // the device-side sweep loop takes the bulk phase whenever the persistent tail kernel can follow it (FusedOk: MFMA
    // backward pass, staged forward pass, uniform step, <= 20 line-search trials, no cost-to-go records)
    // ... and no solve mask is set: its workgroups pull index ranges of the batch, not a list
    r.loop_on = up_.loop_groups > 0 && r.fused_ok && !mask_.on;
    r.loop_handover = std::min(B_, persist_at_);
    // segments of rejection streaks: not with a recorded history (its rows are appended in iteration order)
    // ... nor with cost-to-go records: every shadow column writes P, p into its own CTG column, and neither
    // k_seg_fixup nor the twins' commit copy those back -- altro_get_ctg would return the records of the backward pass at which
    // the instance's OWN column retired
    // ... nor with a tracking cost or a knot constraint: a shadow column would need the reference-term records / the
    // knot-parameter records of its instance (copy_column)
    r.seg_on = up_.seg_total > 0 && !A_.hist && !A_.record_ctg && !r.d.fast_forward_stalls && r.C * kBlock <= up_.seg_total && !r.loop_on &&
               !KnotRouted(A_) && sw_.spec_mode == kSpecAuto;  // (the persistent kernel's variants that know the segments: default modes only)
    r.seg_capc = r.seg_on ? (up_.seg_total / r.C) / kBlock * kBlock : 0;
    if (r.seg_on) ALTRO_HIP_CHECK(hipMemsetAsync(up_.d_seg_cursor, 0, kMaxChains * sizeof(int), stream_));
    // may a sweep of a chain split streaks (SplitsIn)?  Only while the batch has room: a streak split while most of the batch
    // is still iterating only makes sweeps longer that the GPU already fills (the gain is in packing the plateau of the
    // long inner solves into fewer sweeps)
    r.seg_below = (int)((long long)B_ * seg_below_pct_ / 100);
    // ... and not any more once the hand-over to the persistent kernel is near (3 x persist_at_ instances left): the
    // launch takes whatever the lists hold by then, and a list that has just grown fourfold means rounds of workgroups
    // instead of one (config 3: 32.2 - 32.6 ms with this bound, 33 - 35 ms with 1.5 x).  Once a chain has split, the
    // hand-over itself moves to 1.5 x persist_at_: what is left when the segments retire are the long runners, whose
    // iterations the persistent kernel runs at a fifth of a batched sweep's latency.
    r.seg_above = std::min(3 * persist_at_, B_ * 3 / 8);  // (a batch of 2048 keeps a window below its 65 %)
    r.seg_persist_at = persist_at_ * 3 / 2;
    r.nap_ok = host_wait_backoff_ && B_ >= kHostNapMinBatch;
    return ALTRO_OK;
  }
  // the chains' slices of the batch and of the counters; the other chains start behind the engine's stream
  void StartChains(SolveRun& r) {
    const int C = r.C;
    for (int c = 0; c < C; ++c) {
      Chain& ch = r.chain[c];
      ch.lo = C > 1 ? std::min(B_, c * chain_size_) : 0;
      ch.hi = C > 1 ? std::min(B_, (c + 1) * chain_size_) : B_;
      ch.st = c == 0 ? stream_ : chain_stream_[c];
      ch.d_cnt = hm_.d_counter.get() + (size_t)c * r.cstride;
      ch.h_cnt = hm_.h_counter.get() + (size_t)c * r.cstride;
      ch.h_cnt_dev = h_counter_dev_ + (size_t)c * r.cstride;
      ch.known = mask_.on ? mask_.count[c] : ch.hi - ch.lo;
      ch.done = mask_.on && ch.known == 0;  // (a slice the mask leaves empty: this chain launches nothing)
      for (int i = 0; i < r.max_sweeps + 2; ++i) ch.h_cnt[i] = -1;
    }
    if (C > 1) {
      // the other chains start behind the initialisation (and the counter reset) on the engine's stream
      hipEventRecord(start_ev_, stream_);
      for (int c = 1; c < C; ++c) hipStreamWaitEvent(r.chain[c].st, start_ev_, 0);
    }
    for (int c = 0; c < C; ++c) {
      if (!r.prof) break;
      if (c == 0) {
        r.chain[c].ev.push_back(r.nev - 1);
      } else {
        hipEventRecord(ProfEvent(r.nev), r.chain[c].st);
        r.chain[c].ev.push_back(r.nev++);
      }
    }
  }
  // ---- what the chains of a run know ------------------------------------------------------------------------
  int TotalKnown(const SolveRun& r) const {
    long long t = 0;
    for (int c = 0; c < r.C; ++c) t += r.chain[c].done ? 0 : r.chain[c].known;
    return (int)std::min<long long>(t, B_);
  }
  void RecordEvent(SolveRun& r, Chain& ch) {
    if (!r.prof) return;
    hipEventRecord(ProfEvent(r.nev), ch.st);
    ch.ev.push_back(r.nev++);
  }
  // a chain's slice of the two list buffers: its instances and its shadow columns -- every column is listed at most once
  // (a chain never holds more than hi - lo instances of its own)
  int* ListOf(const SolveRun& r, int which, const Chain& ch) const { return up_.d_list[which] + ch.lo + (int)(&ch - r.chain) * r.seg_capc; }
  // the segments' arrays and this chain's slice of shadow columns into the launch arguments of its sweep i
  void SegFields(const SolveRun& r, DevArrays<T>& A, const Chain& ch, int i) const {
    if (!r.seg_on || i < kSegFrom) {
      A.seg_end = nullptr;
      return;
    }
    const int c = (int)(&ch - r.chain);
    SegArrays(A);
    A.seg_cursor = up_.d_seg_cursor + c;
    A.seg_lo = seg_col0_ + c * r.seg_capc;
    A.seg_hi = A.seg_lo + r.seg_capc;
    A.seg_parts = seg_parts_;
  }
  // may sweep i of a chain split streaks?  Only every kSegSplitEvery-th does: the host sizes the grids of sweep i + 1 from
  // the count sweep i - 1 left, and a sweep that splits is the only thing that can make a list longer than that
  // (and only inside the window of PlanRun)
  bool SplitsIn(const SolveRun& r, int i) const {
    return r.seg_on && i >= kSegFrom + 2 && (i % kSegSplitEvery) == 0 && TotalKnown(r) <= r.seg_below && TotalKnown(r) > r.seg_above;
  }
  // upper bound of the instances the sweep about to be enqueued may meet, given the newest count the host knows (what the
  // sweep before it left): a streak that splits adds seg_parts - 1 columns per instance between that count and this sweep
  int BoundOf(const SolveRun& r, const Chain& ch) const {
    const int known = std::max(1, ch.known);
    if (!ch.last_split) return known;
    return (int)std::min<long long>((long long)(ch.hi - ch.lo) + r.seg_capc, (long long)known * seg_parts_);
  }
  bool AnySplit(const SolveRun& r) const {
    bool any = false;
    for (int c = 0; c < r.C; ++c) any = any || r.chain[c].split_seen;
    return r.seg_on && any;
  }
  // sweep i of a chain: expansions, backward pass, forward pass on the chain's stream -- or the chain's turn to the tail
  altro_status EnqueueSweep(SolveRun& r, Chain& ch, int i) {
    const int C = r.C;
    DevArrays<T> A = A_;
    A.chain_lo = ch.lo;
    A.chain_hi = (C > 1 || r.seg_on) ? ch.hi : 0;
    SegFields(r, A, ch, i);
    if (i == 0 && mask_.on) {  // the masked-in instances of the chain's slice, in order (k_mask_compact)
      A.act_list = hm_.mask_list.get() + ch.lo;
      A.act_count = MaskCounts() + (int)(&ch - r.chain);
      A.host_count = nullptr;
    } else if (i == 0) {
      A.act_list = C > 1 ? up_.d_iota + ch.lo : nullptr;
      A.act_count = nullptr;
      A.act_count_const = ch.hi - ch.lo;
      A.host_count = nullptr;
    } else {
      A.act_list = ListOf(r, i % 2, ch);
      A.act_count = ch.d_cnt + (i - 1);
      A.host_count = ch.h_cnt_dev + (i - 1);
    }
    A.next_list = ListOf(r, (i + 1) % 2, ch);
    A.next_count = ch.d_cnt + i;
    const int ninst = i == 0 ? std::max(1, ch.known) : BoundOf(r, ch);
    const bool may_split = SplitsIn(r, i);
    if (!may_split) A.seg_parts = 1;
    // (a batch that fits the CUs from the start -- the MPC case, one or a few dozen instances -- goes to the persistent
    //  kernel at once: its first sweep as three launches and a host round trip would only add latency)
    // (under a solve mask the chains of a large batch too: what counts is how many instances take part)
    if (r.fused_ok && (i > 0 || ((C == 1 || mask_.on) && !no_fused_first_)) &&
        (r.tail_mode || TotalKnown(r) <= (AnySplit(r) ? r.seg_persist_at : persist_at_))) {
      // the tail: every instance left gets a workgroup that runs whole iterations (k_sweep_fused, launched by LaunchTail
      // for all chains together); this chain's list is the one sweep i would have worked on
      r.tail_mode = true;
      ch.tail = true;
      return ALTRO_OK;
    }
    cur_ = ch.st;
    const int span = ch.hi - ch.lo;
    const dim3 gridB((ninst + kBlock - 1) / kBlock);
    PoisonLds();
    // (small models only: their expansions are HBM-bound; the 12-state model's are compute-bound and pay for the idle
    //  lanes of a dense launch: config 4 +13 %)
    // (a handle with a tracking cost: the twin kernel that reads the reference-term records, same launches)
    auto expansions = [&](dim3 grid, int all, int* order_list, int* order_count) {
      if (KnotRouted(A))
        hipLaunchKernelGGL((k_expansions_trk<T, M>), grid, dim3(kBlock), 0, ch.st, A, up_.d_pd, all, order_list, order_count);
      else
        hipLaunchKernelGGL((k_expansions<T, M>), grid, dim3(kBlock), 0, ch.st, A, up_.d_pd, all, order_list, order_count);
    };
    if (i > 0 && sw_.dense_expansions && !kKdgEligible && 4 * (long long)std::max(1, ch.known) >= span) {  // (thresholds 1/2 ... 1/16 measured: 1/4 ... 1/8 best)
      // a good part of the chain is still iterating: lane = instance (coalesced rows and records), and the list is
      // rebuilt in runs of neighbouring instances for the two kernels that follow (see k_expansions); the launch also
      // covers the chain's slice of shadow columns (instance_of_slot)
      expansions(dim3((span + (ch.split_seen ? r.seg_capc : 0) + kBlock - 1) / kBlock, N_ + 1), 2, ListOf(r, i % 2, ch),
                 ch.d_cnt + (r.max_sweeps + 12) + i);
    } else {
      expansions(dim3(gridB.x, N_ + 1), 0, nullptr, nullptr);
    }
    RecordEvent(r, ch);
    LaunchBackward(A, r.d, 0, ninst);
    RecordEvent(r, ch);
    LaunchForward(A, r.d, r.mode, 0, ninst, TotalKnown(r));
    RecordEvent(r, ch);
    cur_ = stream_;
    ch.last_split = may_split;
    ch.split_seen = ch.split_seen || may_split;
    timing_.launches += 3;
    timing_.sweep_launches += 1;
    return ALTRO_OK;
  }
  // ONE launch instead of the chains of sweeps: persistent workgroups pull instances, run E -> B -> F for them until
  // they finish, and leave what is unfinished when `loop_handover` instances are left to the persistent tail kernel,
  // which is enqueued right behind (the host never looks in between)
  altro_status LaunchSweepLoop(SolveRun& r) {
    if (!r.loop_on) return ALTRO_OK;
    if constexpr (kMfmaBackward) {
      ALTRO_HIP_CHECK(hipMemsetAsync(up_.d_loop_ctl, 0, (size_t)(kLwWords + kRwWords) * sizeof(int), stream_));
      const int per_xcd = ((B_ + kLoopXcds - 1) / kLoopXcds + 15) / 16 * 16;
      const LoopCtl lc{up_.d_loop_win, up_.d_loop_ctl, up_.d_loop_tail, r.loop_handover, per_xcd};
      PoisonLds();
      if (r.prof) {
        r.loop_ev = r.nev;
        hipEventRecord(ProfEvent(r.nev++), stream_);
      }
      const dim3 gl(up_.loop_groups), bl(kFwdWaves * kBlock);
      WithForwardSrc([&](auto src) {
        hipLaunchKernelGGL((k_sweep_loop<T, M, decltype(src)::value>), gl, bl, loop_lds_bytes_, stream_, A_, up_.d_pd, pd_, r.d, r.mode, lc);
      });
      if (r.prof) hipEventRecord(ProfEvent(r.nev++), stream_);
      timing_.launches += 1;
      timing_.sweep_launches += 1;
      for (int c = 0; c < r.C; ++c) r.chain[c].done = true;
      r.tail_mode = true;
      r.loop_launched = true;
    }
    return ALTRO_OK;
  }
  // The host waits for words the device writes into pinned memory.  It is ONE SWEEP AHEAD -- the sweep it is about to
  // enqueue only has to be in the queue before the one in flight ends, a hundred microseconds or more away -- so it
  // need not burn a core on the poll: a short spin (the word usually lands within microseconds of a neighbouring
  // chain's), then naps of ~50 us (eight ranks of a node, or the worker threads of libaltro_group.so, share the
  // container's CPU quota with RCCL's proxy threads).  A small batch -- the latency path -- keeps spinning.
  // One wait of a scheduler round that made no progress; returns whether the streams are due for a look.
  bool SpinOrNap(SolveRun& r, bool progressed) {
    // (naps only once the solve has run for kHostNapAfterUs: a 0.3 ms solve of 1024 small problems keeps the spin)
    if (r.nap_ok && !r.nap && (r.spins & 0xff) == 0)
      r.nap = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - r.t0).count() > kHostNapAfterUs;
    if (progressed) {
      r.spins = 0;
      r.naps = 0;
      return false;
    }
    if (r.nap && r.spins >= kHostSpinsBeforeNap) {
      std::this_thread::sleep_for(std::chrono::microseconds(20));  // (timer slack makes it ~70 us)
      timing_.host_naps += 1;
      return (++r.naps & 0xf) == 0;
    }
    CpuRelax();
    return (++r.spins & 0x3ff) == 0 && !r.nap;
  }
  // a chain whose stream has drained must have published the count it is waited for: otherwise its launch failed
  altro_status CheckChainStreams(SolveRun& r) {
    for (int c = 0; c < r.C; ++c) {
      Chain& ch = r.chain[c];
      if (ch.done || ch.tail || !ch.waiting) continue;
      const hipError_t q = hipStreamQuery(ch.st);
      if (q == hipSuccess) {  // stream drained: the word must be there, or the launch failed
        if (__atomic_load_n(&ch.h_cnt[ch.sweeps - 2], __ATOMIC_ACQUIRE) >= 0) continue;
        ALTRO_HIP_CHECK(hipGetLastError());
        err_ = "sweep counter was never published";
        return ALTRO_HIP_ERROR;
      }
      if (q != hipErrorNotReady) ALTRO_HIP_CHECK(q);
    }
    return ALTRO_OK;
  }
  // The host-paced scheduler.  Every chain: enqueue sweep s, then wait for the count sweep s-1 left (published by sweep s,
  // which is already enqueued), then enqueue sweep s+1 ... -- the chains polled in turn, none of them ever blocking the
  // others -- until every chain has run dry, met its cap or turned to the tail.
  altro_status RunChains(SolveRun& r) {
    for (int c = 0; c < r.C && !r.loop_launched; ++c) {
      if (r.chain[c].done) continue;  // (a chain whose slice the solve mask leaves empty)
      ALTRO_TRY(EnqueueSweep(r, r.chain[c], 0));
      if (!r.chain[c].tail) r.chain[c].sweeps = 1;  // (tail already: the persistent kernel takes the batch from its first sweep)
    }
    for (;;) {
      bool any = false, progressed = false;
      for (int c = 0; c < r.C; ++c) {
        Chain& ch = r.chain[c];
        if (ch.done || ch.tail) continue;
        any = true;
        if (ch.waiting) {
          const int v = __atomic_load_n(&ch.h_cnt[ch.sweeps - 2], __ATOMIC_ACQUIRE);
          if (v < 0) continue;
          ch.known = v;
          ch.waiting = false;
          progressed = true;
          if (v == 0) {
            ch.done = true;
            continue;
          }
        }
        if (ch.sweeps >= r.max_sweeps) {  // the iteration caps bound the sweeps; nothing left to learn
          ch.done = true;
          progressed = true;
          continue;
        }
        ALTRO_TRY(EnqueueSweep(r, ch, ch.sweeps));  // publishes the count left by sweep (sweeps - 1)
        progressed = true;
        if (ch.tail) continue;  // (not enqueued: the persistent kernel comes instead)
        ch.sweeps++;
        ch.waiting = true;
      }
      if (!any) break;
      if (SpinOrNap(r, progressed)) ALTRO_TRY(CheckChainStreams(r));
    }
    return ALTRO_OK;
  }
  // the persistent tail kernel (k_sweep_fused): ONE launch on the engine's stream for what all chains, or the loop, left
  altro_status LaunchTail(SolveRun& r) {
    if (!r.tail_mode) return ALTRO_OK;
    if constexpr (kMfmaBackward) {
      const int C = r.C;
      DevArrays<T> A = A_;
      ChainLists lists{};
      long long ninst_l = 0;
      bool whole_batch = false;
      A.chain_size = C > 1 ? chain_size_ : 0;
      for (int c = 0; c < C; ++c) {
        Chain& ch = r.chain[c];
        A.chain_base[c] = ch.sweeps;  // batched sweeps this chain ran (0 .. sweeps-1)
        if (!ch.tail) continue;
        if (ch.sweeps == 0 && mask_.on) {  // (no batched sweep ran: the masked-in instances of the chain's slice, in order)
          lists.list[lists.n] = hm_.mask_list.get() + ch.lo;
          lists.count[lists.n] = MaskCounts() + c;
          lists.n++;
          ninst_l += ch.known;
          continue;
        }
        if (ch.sweeps == 0) {  // (single chain, no batched sweep ran: every instance, in order)
          whole_batch = true;
          ninst_l += B_;
          continue;
        }
        lists.list[lists.n] = ListOf(r, ch.sweeps % 2, ch);
        lists.count[lists.n] = ch.d_cnt + (ch.sweeps - 1);
        lists.n++;
        ninst_l += BoundOf(r, ch);
        if (ch.st != stream_) {  // the engine's stream continues behind this chain's last sweep
          hipEventRecord(chain_ev_[c], ch.st);
          hipStreamWaitEvent(stream_, chain_ev_[c], 0);
        }
      }
      if (r.loop_launched) {
        ninst_l = r.loop_handover;  // (an upper bound: the list's length stays on the device)
        A.chain_size = 0;
      }
      const int ninst = (int)std::min<long long>(std::max<long long>(ninst_l, 1), (long long)B_ + (r.seg_on ? up_.seg_total : 0));
      const bool any_split = AnySplit(r);
      if (any_split) {
        SegArrays(A);
        A.seg_lo = seg_col0_;  // (this launch: first shadow column / columns per chain, for the report of a handed-over column)
        A.seg_hi = r.seg_capc;
      }
      if (r.loop_launched) {
        A.act_list = up_.d_loop_tail;
        A.act_count = up_.d_loop_ctl + kLwTail;
      } else if (whole_batch) {
        A.act_list = nullptr;
        A.act_count = nullptr;
        A.act_count_const = B_;
      } else if (lists.n == 1) {
        A.act_list = lists.list[0];
        A.act_count = lists.count[0];
      } else {
        int* const merged_count = hm_.d_counter.get() + (size_t)C * r.cstride;
        hipLaunchKernelGGL((k_merge_lists<0>), dim3(1), dim3(256), 0, stream_, lists, up_.d_merged, merged_count);
        A.act_list = up_.d_merged;
        A.act_count = merged_count;
        timing_.launches += 1;
      }
      A.host_count = nullptr;
      A.next_list = nullptr;  // nobody comes after this launch
      A.next_count = nullptr;
      PoisonLds();
      if (r.prof) {
        r.fused_ev = r.nev;
        hipEventRecord(ProfEvent(r.nev++), stream_);
      }
      // (the variant without the circle layouts for problems that have no circle constraint: see forward2_body)
      bool circles = false;
      for (int k = 0; k < pd_.nruns; ++k)
        circles = circles || pd_.runs[k].fast == kFastC || pd_.runs[k].fast == kFastCB || pd_.runs[k].fast == kFastBC;
      // (with a fourth wave that runs the next iteration's backward pass beside the forward pass: see the kernel)
      int* const out = r.loop_launched ? up_.d_loop_ctl + kLwWords : hm_.d_counter.get() + r.max_sweeps + 2;
      const int spec = sw_.spec_mode == kSpecAuto ? (circles ? (int)kSpecWave : (int)kSpecFree) : sw_.spec_mode;
      // twin workgroups (TwinCtl): one behind every primary, dispatched after all of them (same launch, higher block
      // indices); not with a recorded history (its rows are appended in iteration order)
      TwinCtl tw{};
      if (up_.twin_cap > 0 && !A.hist && !r.d.fast_forward_stalls) {
        if (!twin_box_clean_)  // (cleared by k_begin_solve otherwise: nothing touches the mailboxes before this launch)
          hipMemsetAsync(up_.d_twin_box, 0, TwinBoxWords() * sizeof(unsigned long long), stream_);
        // the pool: a workgroup per primary, or -- a small batch -- what the device has CUs left for, one shadow column each.
        // (The variants that carry segments of the batched sweeps keep one twin per primary: their bookkeeping step is full.)
        // (They also keep the former minimum share: their launch has a straggler for every CU, and a claimer's start-up --
        //  a first iteration of 75 us -- is paid for with a CU another straggler waits for.  Config 3, alternating runs:
        //  32.2 - 32.4 ms at 12 against 32.6 - 32.7 at 4, inside a spread of 0.8; profiles/tail_endgame_experiments.txt.)
        const int min_share = any_split ? std::max(sw_.twin_min, kTwinSegMin) : sw_.twin_min;
        const int pool = std::min(up_.twin_cap, std::max(ninst, num_cus_ - ninst));
        unsigned long long* const state = up_.d_twin_box + (size_t)2 * up_.twin_cap * kTwWords;
        tw = TwinCtl{up_.d_twin_box, state, ninst, up_.twin_cap, Bp_ - up_.twin_cap, kTwinLag, sw_.twin_debug ? 1 : 0,
                     pool, any_split ? 1 : sw_.twin_depth, min_share, sw_.twin_spread, sw_.twin_misclaim,
                     0, reinterpret_cast<int*>(state + (size_t)2 * up_.twin_cap)};
      }
      const int npool = tw.base > 0 ? tw.npool : 0;
      const dim3 b3(kFwdWaves * kBlock), b4((kFwdWaves + 1) * kBlock);
      timing_.twin_workgroups = npool;  // pool jobs of this launch (the one-shot grid: its pool workgroups)
      // The variant of (circles, speculation, segments).  Columns of split streaks may be in the lists once a chain has
      // split: then the variants that verify / retire / cancel them in the loop's bookkeeping step (seg_on holds only
      // under the default speculation modes); every other launch runs the kernels as they were before the segments existed.
      ForEachFusedVariant([&](auto v) {
        using V = decltype(v);
        if (V::circles == circles && V::spec == spec && V::segments == any_split) {
          const dim3 blk = V::spec == kSpecOff ? b3 : b4;
          // The WORKER grid (TwinCtl::workers, k_sweep_fused): as many workgroups as the device holds at once, by the
          // occupancy query for this variant and its LDS (1 per CU today), each taking the launch's jobs by ticket.
          // ALTRO_HIP_TAIL_WORKERS=0: the one-shot grid, a workgroup per job; =n: at most n workers (tests).  A launch
          // without twins has no pool to keep fed and keeps the one-shot grid.
          if (tw.base > 0 && sw_.tail_workers != 0)
            tw.workers = tail_worker_count(ninst, npool, num_cus_, FusedPerCu(V::Fn(), (int)blk.x), sw_.tail_workers);
          const dim3 g(tail_grid(ninst, npool, tw.workers));
          hipLaunchKernelGGL((k_sweep_fused<T, M, V::circles, V::spec, V::segments>), g, blk, fused_lds_bytes_, stream_, A, up_.d_pd, pd_,
                             r.d, r.mode, 1, out, tw);
        }
      });
      if (r.prof) hipEventRecord(ProfEvent(r.nev++), stream_);
      r.persistent_launched = true;
      timing_.launches += 1;
    }
    return ALTRO_OK;
  }
  // wait until everything the solve enqueued has run: without a core where the wait is long, with one on the latency path
  altro_status WaitForDevice(SolveRun& r) {
    if (r.nap_ok && !r.nap)
      r.nap = r.loop_launched || std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - r.t0).count() > kHostNapAfterUs;
    if (r.nap && tail_ev_) {
      // the persistent launch (or the device-side loop) runs for milliseconds: wait for it WITHOUT a core.  Round 4 waited in
      // hipEventSynchronize on a blocking-sync event; measured in round 6 (bench.py's device_loop key: one launch per solve, the
      // host does nothing else) that wait still costs a whole core -- the runtime spins on the signal.  So: query the event
      // and nap (~70 us with the timer slack: < 2 % of the solves that get here -- large batches only; the latency path
      // below kHostNapMinBatch instances keeps hipStreamSynchronize).
      ALTRO_HIP_CHECK(hipEventRecord(tail_ev_, stream_));
      for (;;) {
        const hipError_t q = hipEventQuery(tail_ev_);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) ALTRO_HIP_CHECK(q);
        std::this_thread::sleep_for(std::chrono::microseconds(20));
        timing_.host_naps += 1;
      }
    }
    for (int c = 1; c < r.C; ++c) ALTRO_HIP_CHECK(hipStreamSynchronize(r.chain[c].st));
    ALTRO_HIP_CHECK(hipStreamSynchronize(stream_));
    ALTRO_HIP_CHECK(hipGetLastError());
    return ALTRO_OK;
  }
  // chains of segments: the last valid column of each over the instance's own (k_seg_fixup; a workgroup per instance,
  // all but the split ones leave at once)
  altro_status SegFixup(SolveRun& r) {
    if (!AnySplit(r)) return ALTRO_OK;
    if constexpr (kMfmaBackward) {
      DevArrays<T> As = A_;
      SegArrays(As);
      hipLaunchKernelGGL((k_seg_fixup<T, M>), dim3(B_), dim3(kBlock), 0, stream_, As, up_.d_pd);
      timing_.launches += 1;
      int cur[kMaxChains] = {0};
      ALTRO_HIP_CHECK(CopySync(cur, up_.d_seg_cursor, sizeof(cur), hipMemcpyDeviceToHost));  // (synchronises the stream)
      for (int c = 0; c < r.C; ++c) timing_.segment_columns += std::min(cur[c], r.seg_capc);
    }
    return ALTRO_OK;
  }
  // what the device counted: the words of the loop and of the persistent kernel into timing_; a forward wave that gave up
  altro_status ReadBackCounters(SolveRun& r) {
    int sweeps = 0;  // longest chain of iterations, the look-ahead sweep of a chain that ran dry included
    for (int c = 0; c < r.C; ++c) sweeps = std::max(sweeps, r.chain[c].sweeps);
    if (r.persistent_launched) {
      int extra[kRwWords] = {0};  // TailReportWord
      if (r.loop_launched) {
        int words[kLwWords + kRwWords];
        ALTRO_HIP_CHECK(CopySync(words, up_.d_loop_ctl, sizeof(words), hipMemcpyDeviceToHost));
        std::memcpy(extra, words + kLwWords, sizeof(extra));
        timing_.loop_workgroups = words[kLwGroups];
        timing_.loop_instance_iterations = words[kLwUnits];
        timing_.loop_handover = words[kLwTail];
        timing_.loop_iterations = words[kLwMaxLoops];
        sweeps = words[kLwMaxLoops];
        extra[kRwSweeps] += words[kLwMaxLoops];
        if (sw_.loop_log) {
          const double per = words[kLwGroups] > 0 ? 0.01 / words[kLwGroups] : 0.0;  // 100 MHz ticks -> us per workgroup
          fprintf(stderr, "LOOPLOG %d workgroups (%d per CU), %d units, longest %d iterations, handed over %d | us per workgroup: slots %.1f E %.1f B %.1f F %.1f\n",
                  words[kLwGroups], loop_per_cu_, words[kLwUnits], words[kLwMaxLoops], words[kLwTail], per * words[kLwTicks],
                  per * words[kLwTicks + 1], per * words[kLwTicks + 2], per * words[kLwTicks + 3]);
        }
      } else {
        ALTRO_HIP_CHECK(CopySync(extra, hm_.d_counter.get() + r.max_sweeps + 2, sizeof(extra), hipMemcpyDeviceToHost));
      }
      timing_.twin_handovers = extra[kRwHandovers];
      timing_.twin_claims = extra[kRwClaims];
      timing_.fused_workgroup_iterations = extra[kRwGroupLoops];
      if (r.seg_on && sw_.twin_debug) {
        int cur[kMaxChains] = {0};
        ALTRO_HIP_CHECK(CopySync(cur, up_.d_seg_cursor, sizeof(cur), hipMemcpyDeviceToHost));
        fprintf(stderr, "segments: shadow columns used per chain %d %d %d %d (of %d each), persistent launch over <= %d slots, longest own chain %d, longest workgroup %d\n",
                cur[0], cur[1], cur[2], cur[3], r.seg_capc, (int)timing_.twin_workgroups, extra[kRwChainLoops], extra[kRwGroupLoops]);
      }
      if (up_.twin_cap > 0 && sw_.twin_debug) ALTRO_TRY(DumpTwinMailboxes());
      if (extra[kRwSyncErr] != 0) {
        err_ = "k_sweep_fused: a forward wave gave up waiting for its sequence word (software synchronisation)";
        return ALTRO_HIP_ERROR;
      }
      timing_.fused_sweeps = extra[kRwChainLoops];
      timing_.fused_instance_iterations = extra[kRwUnits];
      sweeps = std::max(sweeps, extra[kRwSweeps]);
    }
    timing_.sweeps = sweeps;
    return ALTRO_OK;
  }
  // (mailboxes, state words, and the two ticket counters of the worker grid in one more word: cleared together)
  size_t TwinBoxWords() const { return (size_t)2 * up_.twin_cap * (kTwWords + 1) + 1; }
  // workgroups of a k_sweep_fused variant that share a CU at the upload's LDS size (the runtime's answer, asked once)
  int FusedPerCu(const void* fn, int threads) {
    if (fn != fused_per_cu_fn_ || fused_lds_bytes_ != fused_per_cu_lds_) {
      int n = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, fused_lds_bytes_) != hipSuccess) n = 0;
      fused_per_cu_ = n;
      fused_per_cu_fn_ = fn;
      fused_per_cu_lds_ = fused_lds_bytes_;
    }
    return fused_per_cu_;
  }
  // ALTRO_HIP_TWIN_DEBUG: the twins' mailboxes after the persistent launch, slot by slot (debug print only)
  altro_status DumpTwinMailboxes() {
    const int nbox = 2 * up_.twin_cap;
    std::vector<unsigned long long> box((size_t)nbox * kTwWords);
    ALTRO_HIP_CHECK(CopySync(box.data(), up_.d_twin_box, box.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    int hist[4] = {0, 0, 0, 0}, why[8] = {0}, by_depth[kTwinMaxDepth + 2] = {0};
    unsigned long long t0 = ~0ull;
    for (int s = 0; s < up_.twin_cap; ++s)
      if (box[(size_t)s * kTwWords + kTwStamp + kTsPStart]) t0 = std::min(t0, box[(size_t)s * kTwWords + kTwStamp + kTsPStart]);
    auto us_of = [&](const unsigned long long* ts, int i) { return ts[i] ? (double)(long long)(ts[i] - t0) * 0.01 : -1.0; };
    // one line per segment that a pool workgroup took: who it claimed from, its depth, its iterations and its timeline
    int shown = 0;
    double last_commit = 0, last_pend = 0, last_tstart = 0, last_leave = 0;
    int s_commit = -1, s_pend = -1;
    for (int s = 0; s < nbox; ++s) {
      const unsigned long long* w = &box[(size_t)s * kTwWords];
      const unsigned long long* ts = w + kTwStamp;
      auto us = [&](int i) { return us_of(ts, i); };
      if (s >= up_.twin_cap && w[kTwClaim] != 0) {
        hist[w[kTwHand] & 3]++;
        by_depth[std::min<unsigned long long>(w[kTwGen], kTwinMaxDepth + 1)]++;
        const int limit = timing_.twin_claims <= 48 || sw_.twin_debug_all ? 1 : 8;  // (every segment of a small launch, every eighth otherwise)
        if ((shown++ % limit) == 0)
          fprintf(stderr, "  segment %4d depth %d inst %d from %d: it %d..%d hand %d | start %.0f go %.0f cloned %.0f first %.0f snap %.0f claimed %.0f "
                  "done %.0f (loops %llu) verdict %.0f handed %.0f commit %.0f | xcd %d worker %d\n", s, (int)w[kTwGen], (int)w[kTwInst] - 1, (int)w[kTwPred] - 1,
                  (int)(w[kTwClaim] >> 32), (int)w[kTwEnd], (int)(w[kTwHand] & 3), us(kTsTStart), us(kTsTGo), us(kTsTCloned), us(kTsTFirst), us(kTsPSnap),
                  us(kTsPClaim), us(kTsTDone), ts[kTsTLoops], us(kTsTVerdict), us(kTsPHand), us(kTsTCommit), (int)ts[kTsXcd] - 1, (int)ts[kTsWorker] - 1);
      }
      if (sw_.twin_debug_all && s < up_.twin_cap && ts[kTsPStart] != 0)
        fprintf(stderr, "  primary %4d: start %.0f snap %.0f claimed %.0f handed %.0f end %.0f | xcd %d worker %d\n", s, us(kTsPStart), us(kTsPSnap), us(kTsPClaim),
                us(kTsPHand), us(kTsPEnd), (int)ts[kTsXcd] - 1, (int)ts[kTsWorker] - 1);
      if (sw_.twin_debug_all && s >= up_.twin_cap && w[kTwClaim] == 0 && ts[kTsTIdleEnd] != 0)
        fprintf(stderr, "  idle %4d: start %.0f left %.0f | xcd %d worker %d\n", s, us(kTsTStart), us(kTsTIdleEnd), (int)ts[kTsXcd] - 1, (int)ts[kTsWorker] - 1);
      if (w[kTwWhy] != 0) {
        why[w[kTwWhy] & 7]++;
        if (why[w[kTwWhy] & 7] <= 3)
          fprintf(stderr, "  worker %d refused its successor: why %d at it_inner %d (claim start %d)\n", s, (int)(w[kTwWhy] & 7),
                  (int)((w[kTwWhy] >> 8) & 0xffff), (int)((w[kTwWhy] >> 24) & 0xffff));
      }
      if (us(kTsTCommit) > last_commit) { last_commit = us(kTsTCommit); s_commit = s; }
      if (us(kTsPEnd) > last_pend) { last_pend = us(kTsPEnd); s_pend = s; }
      last_leave = std::max(last_leave, us(kTsPHand));
      last_tstart = std::max(last_tstart, us(kTsTStart));
    }
    fprintf(stderr, "twin timeline: last commit %.0f us (mailbox %d), last primary that finished by itself %.0f us (slot %d), last hand-over %.0f us, "
            "last pool start %.0f us\n", last_commit, s_commit, last_pend, s_pend, last_leave, last_tstart);
    fprintf(stderr, "twin mailboxes: pool %d claims %d confirmed joints %d | segments by depth: 1: %d 2: %d 3: %d 4: %d 5: %d | hand word: open %d ok %d refused %d "
            "revoked %d | refusals: streak broke %d, passed %d, counters %d, rho %d, drho %d, break since snapshot %d\n", (int)timing_.twin_workgroups,
            (int)timing_.twin_claims, (int)timing_.twin_handovers, by_depth[1], by_depth[2], by_depth[3], by_depth[4], by_depth[5], hist[0], hist[1], hist[2],
            hist[3], why[1], why[2], why[3], why[4], why[5], why[6]);
    return ALTRO_OK;
  }
  // profiler-event arithmetic of a solve (altro_options::profiler_enable), and the ALTRO_HIP_SWEEP_LOG timeline
  void AccountProfile(SolveRun& r) {
    float ms = 0, fused_ms = 0;
    hipEventElapsedTime(&ms, prof_ev_[0], prof_ev_[1]);
    timing_.init_ms = ms;
    for (int c = 0; c < r.C; ++c) {
      const std::vector<size_t>& ev = r.chain[c].ev;
      for (size_t e0 = 0; e0 + 3 < ev.size(); e0 += 3) {
        hipEventElapsedTime(&ms, prof_ev_[ev[e0]], prof_ev_[ev[e0 + 1]]);
        timing_.expansions_ms += ms;
        hipEventElapsedTime(&ms, prof_ev_[ev[e0 + 1]], prof_ev_[ev[e0 + 2]]);
        timing_.backward_pass_ms += ms;
        hipEventElapsedTime(&ms, prof_ev_[ev[e0 + 2]], prof_ev_[ev[e0 + 3]]);
        timing_.forward_pass_ms += ms;
      }
    }
    if (r.persistent_launched) {
      hipEventElapsedTime(&fused_ms, prof_ev_[r.fused_ev], prof_ev_[r.fused_ev + 1]);
      timing_.fused_ms += fused_ms;
    }
    if (r.loop_launched) {
      float lms = 0;
      hipEventElapsedTime(&lms, prof_ev_[r.loop_ev], prof_ev_[r.loop_ev + 1]);
      timing_.loop_ms = lms;
    }
    if (!sw_.sweep_log) return;
    // timeline of the chains of sweeps (diagnostics): per sweep its start since the solve began, the length of the list it
    // worked on (what the sweep before it left) and the durations of its three kernels
    for (int c = 0; c < r.C; ++c) {
      const std::vector<size_t>& ev = r.chain[c].ev;
      int idx = 0;
      for (size_t e0 = 0; e0 + 3 < ev.size(); e0 += 3, ++idx) {
        float t = 0, e = 0, b = 0, f = 0;
        hipEventElapsedTime(&t, prof_ev_[0], prof_ev_[ev[e0]]);
        hipEventElapsedTime(&e, prof_ev_[ev[e0]], prof_ev_[ev[e0 + 1]]);
        hipEventElapsedTime(&b, prof_ev_[ev[e0 + 1]], prof_ev_[ev[e0 + 2]]);
        hipEventElapsedTime(&f, prof_ev_[ev[e0 + 2]], prof_ev_[ev[e0 + 3]]);
        if (idx % 4 == 0 || e0 + 6 >= ev.size() || std::string(sw_.sweep_log) == "all")
          fprintf(stderr, "SWEEPLOG chain %d sweep %3d t %7.3f ms list %5d E %6.1f B %6.1f F %6.1f us\n", c, idx, t,
                  idx == 0 ? r.chain[c].hi - r.chain[c].lo : (int)r.chain[c].h_cnt[idx - 1], 1e3 * e, 1e3 * b, 1e3 * f);
      }
    }
    if (r.persistent_launched) {
      float t = 0;
      hipEventElapsedTime(&t, prof_ev_[0], prof_ev_[r.fused_ev]);
      fprintf(stderr, "SWEEPLOG persistent launch t %7.3f ms, %.3f ms, slots <= %d\n", t, fused_ms, (int)timing_.twin_workgroups);
    }
  }

  static constexpr int kNumScalarT = 15, kNumScalarI = 7;
  // (time-varying dynamics, user discrete dynamics and per-knot model lists: every knot has its own (step, time, model))
  static constexpr bool kTimeVarying = model_knot_path<M>::value;
  static constexpr int kModelCount = model_list<M>::type::size;
  static constexpr int kRefPT = RefPathRecord(n, m), kRefRT = RefTermRecord(n, m);
  struct SegPtrs {
    int *end = nullptr, *next = nullptr, *flag = nullptr, *streak = nullptr, *tot0 = nullptr;
    double *rho0 = nullptr, *drho0 = nullptr;
  };
  // Everything that lives as long as ONE problem upload: the pool behind Alloc(), the blocks that grow on their own, every
  // pointer into them and number that goes with them.  DropUpload() assigns a fresh one.  (A_: the view the kernels get.)
  struct Uploaded {
    DevPool pool;
    float *d_hk = nullptr, *d_tk = nullptr;  // per-knot steps / times (SetKnotTimes)
    // the reference of the tracking costs, ALWAYS fp64: path points [row][cols][kRefPT] (cols = 1 shared, B per instance; a
    // block of its own, it grows with the path) and term records [k][Bp][kRefRT] (= A_.ref)
    DevBlock<double> refpath;
    double* d_ref = nullptr;
    int ref_rows = 0, ref_cols = 0, ref_offset = 0;
    // the knot constraints and their tracks (each track a block of its own, it grows with the track), the window offset they
    // share, and the records [k][Bp][knot_record_] (= A_.kpar), ALWAYS fp64
    std::vector<KnotCon> kcons;
    int track_offset = 0;
    double* d_kpar = nullptr;
    ProblemDesc* d_pd = nullptr;
    double* d_tmp = nullptr;
    SegPtrs seg;
    int seg_total = 0;            // shadow columns of the batched sweeps' segments (DevArrays::seg_*)
    int* d_seg_cursor = nullptr;  // next free column of each chain's slice
    int twin_cap = 0;                          // shadow columns behind the batch (twin workgroups of the persistent kernel)
    unsigned long long* d_twin_box = nullptr;  // their mailboxes, [twin_cap][kTwWords]
    int* d_list[2] = {nullptr, nullptr};
    // the device-side sweep loop (k_sweep_loop): persistent workgroups, their windows, the control words, the tail list
    int loop_groups = 0;
    int *d_loop_win = nullptr, *d_loop_ctl = nullptr, *d_loop_tail = nullptr;
    int* d_iota = nullptr;    // 0, 1, 2, ...: the active list of a chain's first sweep
    int* d_merged = nullptr;  // the lists of all chains, concatenated for the persistent kernel
    T *X_init = nullptr, *U_init = nullptr;
    double *d_scalarT = nullptr, *d_phi = nullptr;
    int* d_scalarI = nullptr;
    std::map<int, int*> mpc_maps;  // shift -> device row map of the advance
  };
  // The memory that belongs to the handle and survives a dropped upload.  Release() assigns a fresh one.
  struct HandleMem {
    DevBlock<double> stage;     // staging buffer of the host boundary, grow-only (EnsureStage)
    DevBlock<double> hist;      // the iteration history (SetRecordHistory; = A_.hist, A_.hist_len)
    DevBlock<int> hist_len;
    PinnedBlock<int> h_counter;  // one word per sweep, pinned + mapped ...
    DevBlock<int> d_counter;     // ... and its device twin (ReserveCounters)
    LoopRun run;                 // the closed-loop run in progress (LoopBegin .. LoopEnd)
    DevBlock<int> ms_win;        // winners of the last multi-start call, [B] (MsCheck)
    DevBlock<double> cov_f;      // covariance: F | Kw of the last propagation, [steps][n n + m n][Bp] (LaunchCov); grown by
                                 // LaunchLqr to [A | B] | K | P | weights | fail of the last LQR pass (one stream: never both)
    DevBlock<double> team_rad;   // teams: radius per instance [B] | clearances of a host call [B] (TeamRadius)
    // the solve mask (SetSolveMask): a byte per instance [B]; the masked-in instances of every chain slice, ascending, at the
    // slice's own place [B], then the slices' counts and their sum [kMaxSweepChains + 1] (k_mask_compact)
    DevBlock<unsigned char> mask;
    DevBlock<int> mask_list;
    DevBlock<unsigned char> mask_saved;  // the caller's mask while a sequential team round runs under its turns' masks
  };
  // the host's side of the solve mask: is one set, the chain slices it was compacted for, how many instances each holds
  struct MaskState {
    bool on = false;
    int chains = 0, chain_size = 0;
    int count[kMaxSweepChains] = {};
    int total = 0;
  };
  MaskState mask_, mask_saved_;
  bool mask_saved_on_ = false;
  bool last_solve_masked_ = false;  // (GetTiming sums the iterations of the instances the last solve ran)
  Uploaded up_;
  HandleMem hm_;
  std::vector<int> con_knot_off_;
  int knot_record_ = 0;
  altro_desc desc_;
  int B_ = 0, Bp_ = 0, N_ = 0;
  bool uploaded_ = false;
  bool last_mode_ilqr_ = false;
  DevOpts last_opts_{};          // options of the last whole solve (ReplayCtg)
  bool ctg_fresh_ = false;       // the cost-to-go records are those of the last backward pass
  bool ctg_replayable_ = false;  // ... or can be recomputed from what the last whole solve left in memory
  std::vector<double> lqr_w_;       // packed weights of the LQR pass on the stream (LqrPackWeights); they outlive their copy
  std::vector<double> lqr_policy_;  // ... of the gain policy (include/altro_lqr.h); empty: off
  ProblemDesc pd_{};
  DevArrays<T> A_{};
  void SegArrays(DevArrays<T>& A) const {  // the bookkeeping arrays of the segments into a launch's copy of A_
    A.seg_end = up_.seg.end; A.seg_next = up_.seg.next; A.seg_flag = up_.seg.flag; A.seg_streak = up_.seg.streak;
    A.seg_tot0 = up_.seg.tot0; A.seg_rho0 = up_.seg.rho0; A.seg_drho0 = up_.seg.drho0;
  }
  int seg_col0_ = 0, seg_parts_ = 4;
  const Switches sw_;  // the ALTRO_HIP_* switches, read once when the engine is constructed (no getenv on the solve path)
  int seg_below_pct_ = 65;  // split only below this share of the batch
  bool mfma_offsets_ok_ = false;
  bool kdg_ = false;  // forward pass reads the feedback gains from global memory (k_forward2<.., kSrcKdg>)
  bool rg_ = false;   // ... all of the rollout wave's per-knot inputs (k_forward2<.., kSrcGlb>)
  int fwd_per_wave_ = kBlock / kLineSearchLanes;
  size_t fwd_lds_bytes_ = 0, fwd_shared_bytes_ = 0, fwd_per_inst_bytes_ = 0;
  int num_cus_ = 256;
  bool twin_box_clean_ = false;  // this solve's k_begin_solve has cleared the twins' mailboxes
  const void* fused_per_cu_fn_ = nullptr;  // FusedPerCu(): the variant and LDS size the answer below belongs to
  size_t fused_per_cu_lds_ = 0;
  int fused_per_cu_ = 0;
  static constexpr int kMaxChains = kMaxSweepChains;
  static constexpr int kDefaultChains = 4;
  bool counted_chained_ = false;
  long long chain_overlap_ticks_ = 0;  // result of the side-by-side check of the chain streams (100 MHz ticks)
  int chains_ = 1;      // chains of batched sweeps (see Chain); ALTRO_HIP_CHAINS overrides
  int chain_size_ = 0;  // instances per chain (a multiple of the wavefront size)
  hipStream_t chain_stream_[kMaxChains] = {};
  hipEvent_t chain_ev_[kMaxChains] = {};
  hipEvent_t start_ev_ = nullptr;
  hipEvent_t tail_ev_ = nullptr;  // blocking-sync event behind the last launch of a large batch's solve
  // host side of the sweep loop: spin briefly, then nap (see Solve)
  static constexpr int kHostNapMinBatch = 256;
  static constexpr unsigned kHostSpinsBeforeNap = 400;  // ~10 us of pause instructions
  static constexpr double kHostNapAfterUs = 500.0;      // a solve shorter than this never naps
  bool host_wait_backoff_ = true;
  int loop_per_cu_ = 0;  // the device-side sweep loop (k_sweep_loop; Uploaded::loop_groups)
  size_t loop_lds_bytes_ = 0;
  static constexpr int lanes_per_wave() { return kBlock / kLineSearchLanes; }
  template <int SRC>
  static const void* LoopKernel() {
    if constexpr (kMfmaBackward && (SRC != kSrcGlb || kRgEligible))
      return reinterpret_cast<const void*>(&k_sweep_loop<T, M, SRC>);
    else
      return nullptr;
  }
  hipStream_t cur_ = nullptr;  // the stream the launch helpers enqueue on (a chain's, otherwise the engine's)
  int fwd_single_at_ = 512;  // active instances (all chains) below which every instance gets a forward workgroup of its own
  int persist_at_ = 256;  // active instances at which the persistent tail kernel takes over
  size_t fused_lds_bytes_ = 0;
  bool no_fused_first_ = false;  // (A/B builds: first sweep of a small batch as three launches)
  std::vector<int> knot_class_, knot_rowbase_;
  std::vector<int> con_kb_, con_ke_, con_p_, con_eq_;  // knots, rows and cone of every registered constraint
  hipStream_t stream_ = nullptr;
  int* h_counter_dev_ = nullptr;  // hm_.h_counter as the device sees it (ReserveCounters)
  std::vector<hipEvent_t> prof_ev_;
  altro_timing timing_{};
  std::string err_;
};

template <class T, class M>
EngineBase* MakeEngineImpl(const altro_desc& d, std::string* err) {
  if (d.n != M::n || d.m != M::m) {
    if (err) *err = "state/control dimensions do not match the model";
    return nullptr;
  }
  auto* e = new Engine<T, M>(d);
  if (e->Init() != ALTRO_OK) {
    if (err) *err = e->LastError();
    delete e;
    return nullptr;
  }
  return e;
}

}  // namespace altro_hip
