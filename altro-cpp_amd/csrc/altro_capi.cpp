// altro_capi.cpp — extern "C" front end of libaltro_hip.so (see include/altro_hip.h).
//
// Records the problem definition exactly as the reference's altro::problem::Problem setters do,
// creates the device engine lazily on the first compute call, and forwards every entry point.
// No exception crosses the boundary; there is NO CPU fallback.
#include <dlfcn.h>
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "altro_common.hpp"
#include "../../include/altro_mpc.h"
#include "../../include/altro_tracking.h"
#include "../../include/altro_knot_params.h"
#include "../../include/altro_multistart.h"
#include "../../include/altro_team.h"
#include "../../include/altro_covariance.h"
#include "../../include/altro_subset.h"
#include "../../include/altro_trigger.h"
#include "../../include/altro_ensemble.h"
#include "../../include/altro_lqr.h"

using namespace altro_hip;

extern "C" int altro_chain_claim(int device, int delta);

#define ALTRO_USER_PLUGIN_ABI_HOST 17  // must equal ALTRO_USER_PLUGIN_ABI of altro_user_model.hpp

struct altro_solver_s {
  ProblemSpec spec;
  altro_options opts;
  std::unique_ptr<EngineBase> engine;
  bool uploaded = false;
  bool ilqr_mode = false;
  bool has_gains = false;  // a backward pass (a solve, altro_backward_pass) has left gains on the device: altro_mpc_track
  bool record_ctg = false;  // altro_set_record_ctg(h, 1) went through: masked solves, and so the trigger calls, refuse the handle
  bool has_solved = false;  // a whole solve (altro_solve_al, altro_solve_ilqr, altro_wait) has finished: altro_multistart_select
  std::vector<double> lqr_policy;  // the gain policy (include/altro_lqr.h): packed weights (LqrPackWeights); empty: off
  std::string err;
  // Asynchronous solve (altro_solve_al_async): ONE worker thread per handle, created on first use and
  // parked on a condition variable between solves.  While a solve is pending the handle only answers
  // altro_solve_poll / altro_wait / altro_last_error: everything else returns ALTRO_NOT_READY, so a caller
  // cannot change options, inputs or device buffers under the solve in flight.
  std::thread worker;
  std::mutex mu;
  std::condition_variable cv, cv_done;
  bool job_posted = false, worker_exit = false;
  std::atomic<int> async_done{1};
  bool async_pending = false;
  altro_status async_status = ALTRO_OK;
  std::string async_err;  // the worker's own error text, copied to err by altro_wait
  ~altro_solver_s() {
    if (worker.joinable()) {
      {
        std::lock_guard<std::mutex> lk(mu);
        worker_exit = true;
      }
      cv.notify_all();
      worker.join();
    }
  }
};

static thread_local std::string g_create_error;

// ---- user-model plugins (altro_register_model_source; see altro_user_model.hpp) ---------------------------------
namespace {
struct UserModelEntry {
  std::string name, so_path;
  void* dl = nullptr;
  int n = 0, m = 0;
  EngineBase* (*make)(const altro_desc*, std::string*) = nullptr;
  int (*check)(int, const double*, int, double, double*) = nullptr;
  int (*check_functors)(int, const double*, int, double, double*, int*) = nullptr;
  int functors = 0;  // bit 0: the source defines cost types, bit 1: constraint types
  int cost_types = 0, con_types = 0;
  bool checked = false;
  uint64_t hash = 0;
};
std::mutex g_models_mu;
std::vector<UserModelEntry> g_models;  // kind = ALTRO_MODEL_USER_BASE + index

uint64_t Fnv1a(const std::string& s, uint64_t h = 1469598103934665603ULL) {
  for (unsigned char ch : s) {
    h ^= ch;
    h *= 1099511628211ULL;
  }
  return h;
}
bool ReadFile(const std::string& path, std::string* out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::ostringstream ss;
  ss << f.rdbuf();
  *out = ss.str();
  return true;
}
std::string Tail(const std::string& s, size_t n) { return s.size() > n ? s.substr(s.size() - n) : s; }

// Runs argv[0] with the given arguments, stdout and stderr into `log`: posix_spawn with an argument vector -- no shell,
// so no quoting of paths, and independent of the host application's SIGCHLD disposition as far as waitpid allows
// (std::system() returns -1 when SIGCHLD is ignored).  Returns the exit code, or -1.
extern "C" char** environ;
int RunTool(const std::vector<std::string>& args, const std::string& log) {
  posix_spawn_file_actions_t fa;
  if (posix_spawn_file_actions_init(&fa) != 0) return -1;
  posix_spawn_file_actions_addopen(&fa, 1, log.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
  posix_spawn_file_actions_adddup2(&fa, 1, 2);
  std::vector<char*> argv;
  for (const std::string& a : args) argv.push_back(const_cast<char*>(a.c_str()));
  argv.push_back(nullptr);
  pid_t pid = 0;
  const int rc = posix_spawn(&pid, argv[0], &fa, nullptr, argv.data(), environ);
  posix_spawn_file_actions_destroy(&fa);
  if (rc != 0) return -1;
  int status = 0;
  for (;;) {
    const pid_t w = waitpid(pid, &status, 0);
    if (w == pid) break;
    if (w < 0 && errno != EINTR) return -1;  // (ECHILD: the host reaps children itself -- the result file decides)
  }
  return WIFEXITED(status) ? WEXITSTATUS(status) : -1;
}
// [A-Za-z0-9_] only: the name goes into the generated source (a comment and a #line directive)
std::string SafeName(const char* name) {
  std::string out;
  for (const char* p = name; *p && out.size() < 64; ++p)
    out += (std::isalnum(static_cast<unsigned char>(*p)) || *p == '_') ? *p : '_';
  return out.empty() ? std::string("model") : out;
}

// FunctionBase::CheckJacobian (functionbase.cpp:35-73) on the device: 64 points uniform in [-1, 1]^(n+m)
// (VectorXd::Random), central differences with 1e-6, tolerance kDefaultTolerance = 1e-4 (functionbase.hpp:86) on every
// ENTRY's error relative to max(1, |J_ij|): the reference's forward-difference helper is an opt-in test utility, this
// check gates registration and must not reject a correct Jacobian of a model with large second derivatives -- nor let a
// wrong entry of order one hide behind a large norm of the whole matrix
altro_status CheckUserJacobian(UserModelEntry& e, int device, std::string* err) {
  if (e.checked) return ALTRO_OK;
  const int samples = 64, nm = e.n + e.m;
  std::mt19937_64 gen(e.hash);
  std::vector<double> z((size_t)samples * nm);
  for (double& v : z) v = -1.0 + 2.0 * (static_cast<double>(gen() >> 11) * 0x1p-53);
  double max_err = 0.0;
  const int rc = e.check(device, z.data(), samples, 1e-6, &max_err);
  if (rc != 0) {
    *err = "user model '" + e.name + "': the Jacobian check could not run on the device (code " + std::to_string(rc) + ")";
    return ALTRO_HIP_ERROR;
  }
  if (!(max_err < 1e-4)) {
    char buf[256];
    snprintf(buf, sizeof(buf), "user model '%s': jac() does not match finite differences of f(): max_ij |J_fd - J|_ij / max(1, |J_ij|) = %.3g >= 1e-4 "
             "(FunctionBase::CheckJacobian)", e.name.c_str(), max_err);
    *err = buf;
    return ALTRO_INVALID_ARG;
  }
  if (e.functors) {
    // ScalarFunction::CheckGradient, FunctionBase::CheckHessian / CheckJacobian (functionbase.cpp:42-125) for the
    // user's cost and constraint, at the same points
    double errs[3] = {0, 0, 0};
    int worst[3] = {0, 0, 0};
    const int rc2 = e.check_functors(device, z.data(), samples, 1e-6, errs, worst);
    if (rc2 != 0) {
      *err = "user model '" + e.name + "': the cost / constraint derivative check could not run on the device (code " +
             std::to_string(rc2) + ")";
      return ALTRO_HIP_ERROR;
    }
    const char* what[3] = {"UserCost::gradient() does not match finite differences of eval()",
                           "UserCost::hessian() does not match finite differences of gradient()",
                           "UserConstraint::jacobian() does not match finite differences of eval()"};
    for (int q = 0; q < 3; ++q)
      if (!(errs[q] < 1e-4)) {
        char buf[360];
        snprintf(buf, sizeof(buf), "user model '%s': %s (%s type %d): error %.3g >= 1e-4 (FunctionBase::Check%s)", e.name.c_str(),
                 what[q], q < 2 ? "cost" : "constraint", worst[q], errs[q], q == 0 ? "Gradient" : q == 1 ? "Hessian" : "Jacobian");
        *err = buf;
        return ALTRO_INVALID_ARG;
      }
  }
  e.checked = true;
  return ALTRO_OK;
}
}  // namespace

extern "C" {

void altro_default_options(altro_options* o) {  // altro/common/solver_options.hpp:23-56
  std::memset(o, 0, sizeof(*o));
  o->max_iterations_total = 300;
  o->max_iterations_outer = 30;
  o->max_iterations_inner = 100;
  o->cost_tolerance = 1e-4;
  o->gradient_tolerance = 1e-2;
  o->bp_reg_increase_factor = 1.6;
  o->bp_reg_enable = 1;
  o->bp_reg_initial = 0.0;
  o->bp_reg_max = 1e8;
  o->bp_reg_min = 1e-8;
  o->bp_reg_fail_threshold = 100;
  o->check_forwardpass_bounds = 1;
  o->state_max = 1e8;
  o->control_max = 1e8;
  o->line_search_max_iterations = kLineSearchLanes < 20 ? kLineSearchLanes : 20;  // (20; fewer only in experimental ALTRO_LS_LANES builds)
  o->line_search_lower_bound = 1e-8;
  o->line_search_upper_bound = 10.0;
  o->line_search_decrease_factor = 2;
  o->constraint_tolerance = 1e-4;
  o->maximum_penalty = 1e8;
  o->initial_penalty = 1.0;
  o->reset_duals = 1;
  o->profiler_enable = 0;
}

altro_status altro_create(const altro_desc* desc, altro_handle* out) {
  if (!desc || !out) return ALTRO_INVALID_ARG;
  if (desc->n <= 0 || desc->m <= 0 || desc->N <= 0 || desc->batch <= 0 ||
      (desc->dtype != ALTRO_F64 && desc->dtype != ALTRO_F32)) {
    g_create_error = "invalid altro_desc";
    return ALTRO_INVALID_ARG;
  }
  altro_solver_s* h = new (std::nothrow) altro_solver_s();
  if (!h) return ALTRO_INVALID_ARG;
  h->spec.desc = *desc;
  altro_default_options(&h->opts);
  *out = h;
  return ALTRO_OK;
}

void altro_destroy(altro_handle h) { delete h; }

altro_status altro_get_desc(altro_handle h, altro_desc* out) {
  if (!h || !out) return ALTRO_INVALID_ARG;
  *out = h->spec.desc;
  return ALTRO_OK;
}

const char* altro_last_error(altro_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

}  // extern "C"

namespace {

// Create the engine (needs the model) and upload the recorded problem.
altro_status Ensure(altro_handle h) {
  if (!h) return ALTRO_INVALID_ARG;
  if (h->uploaded) return ALTRO_OK;
  const altro_desc& d = h->spec.desc;
  if (!h->engine) {
    EngineBase* e = nullptr;
    std::string err = "unsupported (model, n, m, dtype) combination";
    const bool f64 = d.dtype == ALTRO_F64;
    switch (h->spec.model_kind) {
      case ALTRO_MODEL_UNICYCLE:
        e = f64 ? MakeEngineUnicycleF64(d, &err) : MakeEngineUnicycleF32(d, &err);
        break;
      case ALTRO_MODEL_TRIPLE_INTEGRATOR:
        if (h->spec.dof == 2) e = f64 ? MakeEngineTripleInt2F64(d, &err) : MakeEngineTripleInt2F32(d, &err);
        break;
      case ALTRO_MODEL_QUADROTOR12:
        e = f64 ? MakeEngineQuad12F64(d, &err) : MakeEngineQuad12F32(d, &err);
        break;
      default:
        if (h->spec.model_kind >= ALTRO_MODEL_USER_BASE) {
          std::lock_guard<std::mutex> lk(g_models_mu);
          const size_t idx = (size_t)(h->spec.model_kind - ALTRO_MODEL_USER_BASE);
          if (idx >= g_models.size()) {
            err = "unknown user model kind (altro_register_model_source returns the kind)";
            break;
          }
          UserModelEntry& um = g_models[idx];
          if (um.n != d.n || um.m != d.m) {
            err = "state/control dimensions do not match the user model";
            break;
          }
          // the Jacobian check runs once per model, at registration or -- registered without a device -- here
          if (CheckUserJacobian(um, d.device_id, &err) != ALTRO_OK) break;
          e = um.make(&d, &err);
        } else {
          err = "altro_set_model has not been called";
        }
        break;
    }
    if (!e) {
      h->err = err;
      return (err.find("hip") != std::string::npos || err.find(".hpp:") != std::string::npos) ? ALTRO_HIP_ERROR
                                                                                                : ALTRO_UNSUPPORTED;
    }
    h->engine.reset(e);
  }
  altro_status st = h->engine->Upload(h->spec, &h->err);
  if (st == ALTRO_OK) {
    h->uploaded = true;
    h->engine->LqrSetPolicy(h->lqr_policy);  // (a policy set before the device state existed)
  }
  return st;
}

// true (and the error text set) while an asynchronous solve owns the handle
bool Busy(altro_handle h) {
  if (!h->async_pending) return false;
  h->err = "an asynchronous solve is pending on this handle (call altro_wait first)";
  return true;
}

template <class F>
altro_status Forward(altro_handle h, F f) {
  if (h && Busy(h)) return ALTRO_NOT_READY;
  altro_status st = Ensure(h);
  if (st != ALTRO_OK) return st;
  st = f(*h->engine);
  if (st != ALTRO_OK) h->err = h->engine->LastError();
  return st;
}

// A knot whose cost is a tracking cost, and no reference path yet: the calls that evaluate costs answer ALTRO_NOT_READY
// here, before any device work.  (After the upload the engine knows: the path may have come through
// altro_set_reference_device.)
bool ReferenceMissing(altro_handle h) {
  if (h->uploaded) return false;
  // ... and likewise a knot constraint without a parameter track (include/altro_knot_params.h)
  for (size_t i = 0; i < h->spec.cons.size(); ++i)
    if (h->spec.cons[i].knot && h->spec.cons[i].track_rows < 1) {
      h->err = "constraint " + std::to_string(i) + " is a knot constraint but has no parameter track (altro_set_constraint_track)";
      return true;
    }
  if (h->spec.ref_rows > 0) return false;
  const int N = h->spec.desc.N;
  std::vector<int> tracking(N + 1, 0);
  for (const CostSpec& c : h->spec.costs)  // the last cost set on a knot wins
    for (int k = std::max(c.k_begin, 0); k < std::min(c.k_end, N + 1); ++k) tracking[k] = c.tracking;
  for (int k = 0; k <= N; ++k)
    if (tracking[k]) {
      h->err = "knot " + std::to_string(k) + " has a tracking cost but no reference path is set (altro_set_reference)";
      return true;
    }
  return false;
}
template <class F>
altro_status ForwardCost(altro_handle h, F f) {
  if (h && !h->async_pending && ReferenceMissing(h)) return ALTRO_NOT_READY;
  return Forward(h, f);
}

// behind a call that ran a backward pass: from now on the device holds gains (altro_mpc_track asks)
altro_status GainsAfter(altro_handle h, altro_status st) {
  if (h && st == ALTRO_OK) h->has_gains = true;
  return st;
}

// behind a whole solve: the statistics the multi-start selection reads exist (include/altro_multistart.h)
altro_status SolvedAfter(altro_handle h, altro_status st) {
  if (h && st == ALTRO_OK) h->has_solved = true;
  return GainsAfter(h, st);
}

// The refusals several entry points share, one text each: true, and the error text set, for an argument that is refused.
bool StepsRefused(altro_handle h, int steps, const char* who) {
  const int N = h->spec.desc.N;
  if (steps >= 1 && steps <= N) return false;
  h->err = std::string(who) + ": steps must lie in [1, N] = [1, " + std::to_string(N) + "], got " + std::to_string(steps);
  return true;
}
bool WModeRefused(altro_handle h, int w_mode, const char* who) {
  if (w_mode >= 0 && w_mode <= (ALTRO_COV_W_PER_INSTANCE | ALTRO_COV_W_PER_KNOT)) return false;
  h->err = std::string(who) + ": w_mode is a combination of ALTRO_COV_W_PER_INSTANCE and ALTRO_COV_W_PER_KNOT, got " + std::to_string(w_mode);
  return true;
}
bool BoundsRefused(altro_handle h, const double* u_lo, const double* u_hi, const char* who) {
  if ((u_lo == nullptr) == (u_hi == nullptr)) return false;
  h->err = std::string(who) + ": u_lo and u_hi come together (both or neither)";
  return true;
}
bool NegativeRefused(altro_handle h, double v, const std::string& what, const char* who) {
  if (v >= 0.0 && v < std::numeric_limits<double>::infinity()) return false;  // (a NaN fails the first)
  h->err = std::string(who) + ": " + what + " must be finite and not negative";
  return true;
}
// `lookahead`: the trigger's wording, whose lookahead is what needs the gains
bool GainsMissing(altro_handle h, const char* who, bool lookahead = false) {
  if (h->has_gains) return false;
  h->err = std::string(who) + (lookahead ? ": the lookahead needs gains, and " : ": ") + "no backward pass has produced " +
           (lookahead ? "any" : "gains") + " on this handle yet (altro_solve_al, altro_solve_ilqr, altro_backward_pass)";
  return true;
}
bool NotKnotConstraint(altro_handle h, int index, const char* who) {
  if (index >= 0 && index < (int)h->spec.cons.size() && h->spec.cons[index].knot) return false;
  h->err = std::string(who) + ": constraint " + std::to_string(index) + " is not a knot constraint (altro_add_knot_constraint)";
  return true;
}

altro_status DefChanged(altro_handle h) {
  if (h->uploaded) {
    h->err = "the problem definition cannot change after the first compute call; create a new handle";
    return ALTRO_NOT_READY;
  }
  return ALTRO_OK;
}

}  // namespace

extern "C" {

altro_status altro_register_model_source(const char* name, const char* source, int check_jacobian, int* kind_out) {
  if (!name || !source || !kind_out) return ALTRO_INVALID_ARG;
  std::string& err = g_create_error;
  // the engine headers live next to the library (in-tree: altro-cpp_amd/csrc); ALTRO_HIP_INCLUDE_DIR overrides
  std::string inc;
  if (const char* e = std::getenv("ALTRO_HIP_INCLUDE_DIR")) {
    inc = e;
  } else {
    Dl_info info;
    if (!dladdr(reinterpret_cast<void*>(&altro_create), &info) || !info.dli_fname) {
      err = "cannot locate libaltro_hip.so (dladdr)";
      return ALTRO_HIP_ERROR;
    }
    inc = info.dli_fname;
    const size_t slash = inc.find_last_of('/');
    inc = slash == std::string::npos ? "." : inc.substr(0, slash);
  }
  std::string hdrs;
  for (const char* f : {"altro_common.hpp", "altro_devmem.hpp", "altro_problem.hpp", "altro_device.hpp", "altro_rng.hpp", "altro_kernels.hpp", "altro_engine.hpp",
                        "altro_user_model.hpp", "../../include/altro_hip.h"}) {
    std::string txt;
    if (!ReadFile(inc + "/" + f, &txt)) {
      err = std::string("engine header ") + f + " not found in " + inc + " (set ALTRO_HIP_INCLUDE_DIR)";
      return ALTRO_NOT_READY;
    }
    hdrs += txt;
  }
  std::string arch = "gfx950";
  if (const char* e = std::getenv("ALTRO_HIP_ARCH")) {
    arch = e;
  } else {
    hipDeviceProp_t p;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && hipGetDeviceProperties(&p, 0) == hipSuccess) {
      arch = p.gcnArchName;
      arch = arch.substr(0, arch.find(':'));
    }
  }
  const std::vector<std::string> flagv = {"-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast", "-mllvm",
                                          "-amdgpu-mfma-vgpr-form=1", "-Wno-unused-value", "-Wno-unused-result",
                                          "--offload-arch=" + arch};
  std::string flags;
  for (const std::string& f : flagv) flags += f + " ";
  const uint64_t hash = Fnv1a(flags, Fnv1a(hdrs, Fnv1a(source)));
  std::lock_guard<std::mutex> lk(g_models_mu);
  for (size_t i = 0; i < g_models.size(); ++i)
    if (g_models[i].hash == hash) {  // same source, same library: already loaded
      *kind_out = ALTRO_MODEL_USER_BASE + (int)i;
      return ALTRO_OK;
    }
  std::string cache = inc + "/_user_cache";
  if (const char* e = std::getenv("ALTRO_HIP_CACHE_DIR")) cache = e;
  mkdir(cache.c_str(), 0700);  // (plugins are code: private to the user.  Stale entries -- every header edit changes the
                               //  hash -- are the deployment's to prune: altro_user_model_path names the live ones)
  const std::string safe = SafeName(name);
  char hx[32];
  snprintf(hx, sizeof(hx), "%016llx", (unsigned long long)hash);
  const std::string stem = cache + "/altro_user_" + hx;
  const std::string so = stem + ".so";
  // A cached plugin is trusted only if it says itself that it was built from this very (source, headers, flags): the
  // generated translation unit embeds the hash, checked after dlopen.  A file that merely carries the right name is
  // recompiled.
  auto embedded_hash_ok = [&](void* dl) {
    auto fn = reinterpret_cast<unsigned long long (*)()>(dlsym(dl, "altro_user_source_hash"));
    return fn && fn() == (unsigned long long)hash;
  };
  void* dl = nullptr;
  if (access(so.c_str(), R_OK) == 0) {
    dl = dlopen(so.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (dl && !embedded_hash_ok(dl)) {
      dlclose(dl);
      dl = nullptr;
    }
    if (!dl) unlink(so.c_str());
  }
  if (!dl) {
    const std::string src = stem + ".hip", log = stem + ".log", tmp = stem + "." + std::to_string((long)getpid()) + ".tmp.so";
    {
      std::ofstream f(src);
      f << "// generated by altro_register_model_source for the user model '" << safe << "'\n"
        << "#include <hip/hip_runtime.h>\n#define ALTRO_MODEL_FN __device__ __forceinline__\n"
        // (the user's functions under the language-level contraction rule, like the generic integrators that call them:
        //  altro_device.hpp, "CONTRACTION MODE OF THE GENERIC DYNAMICS CODE")
        << "#pragma clang fp contract(on)\n"
        << "namespace altro_user {\n#line 1 \"user model " << safe << "\"\n" << source << "\n}  // namespace altro_user\n"
        << "#pragma clang fp contract(fast)\n"
        << "#include \"altro_user_model.hpp\"  // (the engine headers see ALTRO_USER_COST / ALTRO_USER_CONSTRAINT)\n"
        << "extern \"C\" unsigned long long altro_user_source_hash() { return 0x" << hx << "ULL; }\n";
      if (!f) {
        err = "cannot write " + src + " (set ALTRO_HIP_CACHE_DIR to a writable directory)";
        return ALTRO_NOT_READY;
      }
    }
    std::string hipcc = "/opt/rocm/bin/hipcc";
    if (const char* e = std::getenv("HIPCC")) hipcc = e;
    std::vector<std::string> args = {hipcc};
    args.insert(args.end(), flagv.begin(), flagv.end());
    args.push_back("-I" + inc);
    args.push_back("-o");
    args.push_back(tmp);
    args.push_back(src);
    const int rc = RunTool(args, log);
    // (rc == -1 with a result file: waitpid failed because the host application reaps its children itself -- the exit
    //  code is unknown, so the file must prove itself before it gets the cached name: it loads and carries this hash)
    bool tmp_ok = rc == 0;
    if (rc == -1 && access(tmp.c_str(), R_OK) == 0) {
      if (void* probe = dlopen(tmp.c_str(), RTLD_NOW | RTLD_LOCAL)) {
        tmp_ok = embedded_hash_ok(probe);
        dlclose(probe);
      }
    }
    if (!tmp_ok || rename(tmp.c_str(), so.c_str()) != 0) {
      std::string out;
      ReadFile(log, &out);
      err = "compiling the user model '" + safe + "' failed:\n" + Tail(out, 1500);
      unlink(tmp.c_str());
      return ALTRO_INVALID_ARG;
    }
    dl = dlopen(so.c_str(), RTLD_NOW | RTLD_LOCAL);
  }
  UserModelEntry e;
  e.name = safe;
  e.so_path = so;
  e.hash = hash;
  e.dl = dl;
  if (!e.dl) {
    err = std::string("dlopen of the user-model plugin failed: ") + dlerror();
    return ALTRO_HIP_ERROR;
  }
  auto abi = reinterpret_cast<int (*)()>(dlsym(e.dl, "altro_user_abi"));
  auto dims = reinterpret_cast<void (*)(int*, int*)>(dlsym(e.dl, "altro_user_dims"));
  e.make = reinterpret_cast<EngineBase* (*)(const altro_desc*, std::string*)>(dlsym(e.dl, "altro_user_make_engine"));
  e.check = reinterpret_cast<int (*)(int, const double*, int, double, double*)>(dlsym(e.dl, "altro_user_check_jacobian"));
  auto finfo = reinterpret_cast<int (*)(int*, int*)>(dlsym(e.dl, "altro_user_functor_info"));
  e.check_functors =
      reinterpret_cast<int (*)(int, const double*, int, double, double*, int*)>(dlsym(e.dl, "altro_user_check_functors"));
  if (!abi || !dims || !e.make || !e.check || !finfo || !e.check_functors || abi() != ALTRO_USER_PLUGIN_ABI_HOST ||
      !embedded_hash_ok(e.dl)) {
    err = "the cached user-model plugin " + so + " does not match this library; delete it";
    dlclose(e.dl);
    return ALTRO_HIP_ERROR;
  }
  // one book of chained engines for built-in and plugin engines (altro_engine.hpp: ChainClaim)
  if (auto hook = reinterpret_cast<void (*)(int (*)(int, int))>(dlsym(e.dl, "altro_user_set_chain_hook"))) hook(&altro_chain_claim);
  dims(&e.n, &e.m);
  e.functors = finfo(&e.cost_types, &e.con_types);
  if (check_jacobian) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {  // without a device the check runs at first use
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess) dev = 0;  // clear a sticky "no device selected" state; device 0 is fine
      altro_status st = CheckUserJacobian(e, dev, &err);
      if (st != ALTRO_OK) {
        dlclose(e.dl);
        return st;
      }
    }
  } else {
    e.checked = true;  // the caller vouches for the Jacobian
  }
  g_models.push_back(e);
  *kind_out = ALTRO_MODEL_USER_BASE + (int)g_models.size() - 1;
  return ALTRO_OK;
}

// Engines with chains of sweeps per device: the counter every engine of the process books in -- the built-in ones through
// this library's copy of the counter (altro_common.hpp: ChainClaimLocal), plugins through the hook they are handed at load.
int altro_chain_claim(int device, int delta) { return altro_hip::ChainClaimLocal(device, delta); }

int altro_user_model_path(int kind, char* buf, int len) {
  std::lock_guard<std::mutex> lk(g_models_mu);
  const int idx = kind - ALTRO_MODEL_USER_BASE;
  if (idx < 0 || idx >= (int)g_models.size() || !buf || len <= 0) return -1;
  std::snprintf(buf, (size_t)len, "%s", g_models[idx].so_path.c_str());
  return (int)g_models[idx].so_path.size();
}

altro_status altro_set_model(altro_handle h, int kind, const double* params, int nparams) {
  if (!h) return ALTRO_INVALID_ARG;
  if (DefChanged(h) != ALTRO_OK) return ALTRO_NOT_READY;
  h->spec.model_kind = kind;
  h->spec.dof = (kind == ALTRO_MODEL_TRIPLE_INTEGRATOR && params && nparams > 0) ? (int)params[0] : 0;
  return ALTRO_OK;
}
altro_status altro_set_knot_models(altro_handle h, const int* model_of_knot, int count) {
  if (!h || !model_of_knot) return ALTRO_INVALID_ARG;
  if (DefChanged(h) != ALTRO_OK) return ALTRO_NOT_READY;
  if (count != h->spec.desc.N) {
    h->err = "altro_set_knot_models: expected N = " + std::to_string(h->spec.desc.N) + " indices (the terminal knot has no dynamics)";
    return ALTRO_INVALID_ARG;
  }
  for (int k = 0; k < count; ++k)
    if (model_of_knot[k] < 0) {
      h->err = "altro_set_knot_models: index " + std::to_string(k) + " is negative";
      return ALTRO_INVALID_ARG;
    }
  h->spec.knot_model.assign(model_of_knot, model_of_knot + count);  // (checked against the model's list at the upload)
  return ALTRO_OK;
}
altro_status altro_set_uniform_step(altro_handle h, float hstep) {
  if (!h || !(hstep > 0.0f)) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  // the step belongs to the trajectory (trajectory.hpp:122-130), not to the problem definition: it may
  // change between solves, also after the device state exists
  h->spec.hstep = hstep;
  h->spec.hk.clear();  // SetUniformStep overwrites every knot's step and time (trajectory.hpp:122-130)
  h->spec.tk.clear();
  if (h->uploaded) {
    altro_status st = h->engine->SetStep(hstep);
    if (st == ALTRO_OK) st = h->engine->SetKnotTimes(h->spec, &h->err);
    else h->err = h->engine->LastError();
    return st;
  }
  return ALTRO_OK;
}
altro_status altro_set_steps(altro_handle h, const float* hk, int count) {
  if (!h || !hk) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (count != h->spec.desc.N) {
    h->err = "altro_set_steps: expected N = " + std::to_string(h->spec.desc.N) + " steps (the terminal knot has none)";
    return ALTRO_INVALID_ARG;
  }
  for (int k = 0; k < count; ++k)
    if (!(hk[k] > 0.0f)) {
      h->err = "altro_set_steps: step " + std::to_string(k) + " is not positive";
      return ALTRO_INVALID_ARG;
    }
  if (h->spec.tk.empty() && h->spec.hk.empty() && h->spec.hstep > 0.0f) {
    // the times an earlier SetUniformStep left stay (Trajectory::SetStep does not touch them)
    const int N = h->spec.desc.N;
    h->spec.tk.resize(N + 1);
    for (int k = 0; k < N; ++k) h->spec.tk[k] = static_cast<float>(k) * h->spec.hstep;
    h->spec.tk[N] = h->spec.hstep * N;
  }
  h->spec.hk.assign(hk, hk + count);
  if (h->uploaded) return h->engine->SetKnotTimes(h->spec, &h->err);
  return ALTRO_OK;
}
altro_status altro_set_times(altro_handle h, const float* tk, int count) {
  if (!h || !tk) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (count != h->spec.desc.N + 1) {
    h->err = "altro_set_times: expected N + 1 = " + std::to_string(h->spec.desc.N + 1) + " times";
    return ALTRO_INVALID_ARG;
  }
  h->spec.tk.assign(tk, tk + count);  // (only a time-varying model reads them; the steps decide which kernels run)
  if (h->uploaded) return h->engine->SetKnotTimes(h->spec, &h->err);
  return ALTRO_OK;
}
altro_status altro_get_steps(altro_handle h, float* hk, float* tk) {
  if (!h) return ALTRO_INVALID_ARG;
  const int N = h->spec.desc.N;
  for (int k = 0; k < N && hk; ++k) hk[k] = h->spec.hk.empty() ? h->spec.hstep : h->spec.hk[k];
  for (int k = 0; k <= N && tk; ++k)
    tk[k] = !h->spec.tk.empty() ? h->spec.tk[k]
                                : (!h->spec.hk.empty() ? 0.0f : (k < N ? static_cast<float>(k) * h->spec.hstep : h->spec.hstep * N));
  return ALTRO_OK;
}
altro_status altro_set_lqr_cost(altro_handle h, int k_begin, int k_end, const double* Q, const double* R,
                                const double* xref, const double* uref, int per_instance) {
  if (!h || !Q || !R || !xref || !uref) return ALTRO_INVALID_ARG;
  if (DefChanged(h) != ALTRO_OK) return ALTRO_NOT_READY;
  const altro_desc& d = h->spec.desc;
  if (k_begin < 0 || k_end > d.N + 1 || k_begin >= k_end) {
    h->err = "knot range out of bounds";
    return ALTRO_INVALID_ARG;
  }
  CostSpec c;
  c.k_begin = k_begin;
  c.k_end = k_end;
  c.per_instance = per_instance;
  c.Q.assign(Q, Q + d.n * d.n);
  c.R.assign(R, R + d.m * d.m);
  c.xref.assign(xref, xref + (size_t)d.n * ((per_instance & 1) ? d.batch : 1));
  c.uref.assign(uref, uref + (size_t)d.m * ((per_instance & 2) ? d.batch : 1));
  h->spec.costs.push_back(std::move(c));
  return ALTRO_OK;
}
altro_status altro_set_lqr_tracking_cost(altro_handle h, int k_begin, int k_end, const double* Q, const double* R) {
  if (!h || !Q || !R) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (DefChanged(h) != ALTRO_OK) return ALTRO_NOT_READY;
  const altro_desc& d = h->spec.desc;
  if (k_begin < 0 || k_end > d.N + 1 || k_begin >= k_end) {
    h->err = "knot range out of bounds";
    return ALTRO_INVALID_ARG;
  }
  CostSpec c;
  c.k_begin = k_begin;
  c.k_end = k_end;
  c.per_instance = 0;
  c.tracking = 1;
  c.Q.assign(Q, Q + d.n * d.n);
  c.R.assign(R, R + d.m * d.m);
  h->spec.costs.push_back(std::move(c));
  return ALTRO_OK;
}
altro_status altro_set_reference(altro_handle h, const double* Xref, const double* Uref, int rows, int per_instance) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (!Xref || rows < 1) {
    h->err = "altro_set_reference: the path needs Xref and at least one row";
    return ALTRO_INVALID_ARG;
  }
  if (h->uploaded) {  // (no copy into the recorded definition: the path lives on the device)
    const altro_status st = h->engine->SetReference(Xref, Uref, rows, per_instance, 0);
    if (st != ALTRO_OK) h->err = h->engine->LastError();
    return st;
  }
  const altro_desc& d = h->spec.desc;
  const size_t cnt = (size_t)rows * (per_instance ? d.batch : 1);
  h->spec.ref_X.assign(Xref, Xref + cnt * d.n);
  if (Uref) h->spec.ref_U.assign(Uref, Uref + cnt * d.m);
  else h->spec.ref_U.clear();
  h->spec.ref_rows = rows;
  h->spec.ref_per_instance = per_instance ? 1 : 0;
  h->spec.ref_offset = 0;
  return ALTRO_OK;
}
altro_status altro_set_reference_device(altro_handle h, const void* Xref_device, const void* Uref_device, int rows,
                                        int per_instance) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (!Xref_device || rows < 1) {
    h->err = "altro_set_reference_device: the path needs Xref and at least one row";
    return ALTRO_INVALID_ARG;
  }
  return Forward(h, [&](EngineBase& e) {
    return e.SetReference((const double*)Xref_device, (const double*)Uref_device, rows, per_instance, 1);
  });
}
altro_status altro_set_reference_offset(altro_handle h, int offset) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (offset < 0) {
    h->err = "altro_set_reference_offset: the offset must not be negative";
    return ALTRO_INVALID_ARG;
  }
  if (h->uploaded) {
    const altro_status st = h->engine->SetReferenceOffset(offset);
    if (st != ALTRO_OK) h->err = h->engine->LastError();
    return st;
  }
  h->spec.ref_offset = offset;
  return ALTRO_OK;
}
altro_status altro_get_reference_offset(altro_handle h, int* offset) {
  if (!h || !offset) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  *offset = h->uploaded ? h->engine->GetReferenceOffset() : h->spec.ref_offset;
  return ALTRO_OK;
}
altro_status altro_get_reference_terms(altro_handle h, double* q, double* r, double* c) {
  return Forward(h, [&](EngineBase& e) { return e.GetReferenceTerms(q, r, c); });
}
altro_status altro_set_user_cost(altro_handle h, int k_begin, int k_end, const double* params, int nparams,
                                 int per_instance) {
  return altro_set_user_cost_type(h, 0, k_begin, k_end, params, nparams, per_instance);
}
altro_status altro_set_user_cost_type(altro_handle h, int type, int k_begin, int k_end, const double* params, int nparams,
                                      int per_instance) {
  if (!h || type < 0 || nparams < 0 || (nparams > 0 && !params)) return ALTRO_INVALID_ARG;
  if (DefChanged(h) != ALTRO_OK) return ALTRO_NOT_READY;
  const altro_desc& d = h->spec.desc;
  if (k_begin < 0 || k_end > d.N + 1 || k_begin >= k_end) {
    h->err = "knot range out of bounds";
    return ALTRO_INVALID_ARG;
  }
  CostSpec c;
  c.k_begin = k_begin;
  c.k_end = k_end;
  c.per_instance = per_instance ? 1 : 0;
  c.user = 1 + type;
  if (nparams > 0) c.params.assign(params, params + (size_t)nparams * (per_instance ? d.batch : 1));
  h->spec.costs.push_back(std::move(c));  // the type's nparams is checked when the engine of the model exists
  return ALTRO_OK;
}
altro_status altro_add_user_constraint_type(altro_handle h, int type, int k_begin, int k_end, const double* params, int nparams,
                                            int per_instance) {
  if (!h || type < 0) return ALTRO_INVALID_ARG;
  const altro_status st = altro_add_constraint(h, ALTRO_CON_USER, k_begin, k_end, params, nparams, per_instance);
  if (st == ALTRO_OK) h->spec.cons.back().user_type = type;
  return st;
}
altro_status altro_add_constraint(altro_handle h, int kind, int k_begin, int k_end, const double* params,
                                  int nparams, int per_instance) {
  if (!h || nparams < 0 || (nparams > 0 && !params) || (nparams == 0 && kind != ALTRO_CON_USER)) return ALTRO_INVALID_ARG;
  if (DefChanged(h) != ALTRO_OK) return ALTRO_NOT_READY;
  const altro_desc& d = h->spec.desc;
  if (k_begin < 0 || k_end > d.N + 1 || k_begin >= k_end) {
    h->err = "knot range out of bounds";
    return ALTRO_INVALID_ARG;
  }
  if (kind == ALTRO_CON_CONTROL_BOUND) {
    // ControlBound::ValidateBounds, examples/basic_constraints.hpp:131-136
    if (nparams != 2 * d.m) {
      h->err = "control bound needs lb[m], ub[m]";
      return ALTRO_INVALID_ARG;
    }
    for (int j = 0; j < d.m; ++j)
      if (!(params[j] <= params[d.m + j])) {
        h->err = "Lower bound isn't less than the upper bound.";
        return ALTRO_INVALID_ARG;
      }
  }
  ConSpec c;
  c.kind = kind;
  c.k_begin = k_begin;
  c.k_end = k_end;
  c.nparams = nparams;
  c.per_instance = per_instance;
  if (nparams > 0) c.params.assign(params, params + (size_t)nparams * (per_instance ? d.batch : 1));
  h->spec.cons.push_back(std::move(c));
  return ALTRO_OK;
}
// ---- knot constraints (include/altro_knot_params.h) ----------------------------------------------------------------------
altro_status altro_add_knot_constraint(altro_handle h, int kind, int user_type, int k_begin, int k_end, int nparams, int* index) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (DefChanged(h) != ALTRO_OK) return ALTRO_NOT_READY;
  const altro_desc& d = h->spec.desc;
  if (k_begin < 0 || k_end > d.N + 1 || k_begin >= k_end) {
    h->err = "altro_add_knot_constraint: knot range out of bounds";
    return ALTRO_INVALID_ARG;
  }
  bool fits = false;
  if (kind == ALTRO_CON_GOAL) fits = nparams == d.n;
  else if (kind == ALTRO_CON_CONTROL_BOUND) fits = nparams == 2 * d.m;
  else if (kind == ALTRO_CON_CIRCLE) fits = nparams > 0 && nparams % 3 == 0;
  else if (kind == ALTRO_CON_USER) fits = nparams >= 1 && user_type >= 0;  // (the type's own count: checked with the model's source)
  else {
    h->err = "altro_add_knot_constraint: unknown constraint kind";
    return ALTRO_INVALID_ARG;
  }
  if (!fits) {
    h->err = "altro_add_knot_constraint: nparams does not fit the kind (goal: n, control bound: 2m, circle: 3 per circle, "
             "user: the type's nparams, at least one)";
    return ALTRO_INVALID_ARG;
  }
  int knots = 0;
  for (const ConSpec& c : h->spec.cons) knots += c.knot;
  if (knots >= kMaxKnotCons) {
    h->err = "altro_add_knot_constraint: too many knot constraints";
    return ALTRO_UNSUPPORTED;
  }
  ConSpec c;
  c.kind = kind;
  c.k_begin = k_begin;
  c.k_end = k_end;
  c.nparams = nparams;
  c.per_instance = 0;
  c.user_type = kind == ALTRO_CON_USER ? user_type : 0;
  c.knot = 1;
  h->spec.cons.push_back(std::move(c));
  if (index) *index = (int)h->spec.cons.size() - 1;
  return ALTRO_OK;
}
namespace {
// what both track setters refuse before any device work; the ConSpec of the constraint through *out
altro_status TrackCheck(altro_handle h, int index, const void* P, int rows, const char* who, ConSpec** out) {
  if (NotKnotConstraint(h, index, who)) return ALTRO_INVALID_ARG;
  if (!P || rows < 1) {
    h->err = std::string(who) + ": the track needs at least one row";
    return ALTRO_INVALID_ARG;
  }
  *out = &h->spec.cons[index];
  return ALTRO_OK;
}
}  // namespace
altro_status altro_set_constraint_track(altro_handle h, int index, const double* P, int rows, int per_instance) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  ConSpec* c = nullptr;
  altro_status st = TrackCheck(h, index, P, rows, "altro_set_constraint_track", &c);
  if (st != ALTRO_OK) return st;
  const altro_desc& d = h->spec.desc;
  const size_t cnt = (size_t)rows * (per_instance ? d.batch : 1) * c->nparams;
  if (c->kind == ALTRO_CON_CONTROL_BOUND) {
    // the rows of a bound are chosen from its finite entries at problem definition (basic_constraints.hpp:138-145): a knot
    // bound has all 2m rows on every knot, so every entry of its track is finite; ValidateBounds (:131-136) row by row
    for (size_t e = 0; e < cnt; ++e)
      if (!(std::abs(P[e]) < std::numeric_limits<double>::max())) {
        h->err = "altro_set_constraint_track: every entry of a control bound's track must be finite";
        return ALTRO_INVALID_ARG;
      }
    for (size_t r = 0; r < cnt / c->nparams; ++r)
      for (int j = 0; j < d.m; ++j)
        if (!(P[r * c->nparams + j] <= P[r * c->nparams + d.m + j])) {
          h->err = "Lower bound isn't less than the upper bound.";
          return ALTRO_INVALID_ARG;
        }
  }
  if (h->uploaded) {  // (no copy into the recorded definition: the track lives on the device)
    st = h->engine->SetConstraintTrack(index, P, rows, per_instance, 0);
    if (st != ALTRO_OK) h->err = h->engine->LastError();
    return st;
  }
  c->track.assign(P, P + cnt);
  c->track_rows = rows;
  c->track_per_instance = per_instance ? 1 : 0;
  return ALTRO_OK;
}
altro_status altro_set_constraint_track_device(altro_handle h, int index, const void* P_device, int rows, int per_instance) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  ConSpec* c = nullptr;
  const altro_status st = TrackCheck(h, index, P_device, rows, "altro_set_constraint_track_device", &c);
  if (st != ALTRO_OK) return st;
  return Forward(h, [&](EngineBase& e) { return e.SetConstraintTrack(index, (const double*)P_device, rows, per_instance, 1); });
}
altro_status altro_set_track_offset(altro_handle h, int offset) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (offset < 0) {
    h->err = "altro_set_track_offset: the offset must not be negative";
    return ALTRO_INVALID_ARG;
  }
  if (h->uploaded) {
    const altro_status st = h->engine->SetTrackOffset(offset);
    if (st != ALTRO_OK) h->err = h->engine->LastError();
    return st;
  }
  h->spec.track_offset = offset;
  return ALTRO_OK;
}
altro_status altro_get_track_offset(altro_handle h, int* offset) {
  if (!h || !offset) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  *offset = h->uploaded ? h->engine->GetTrackOffset() : h->spec.track_offset;
  return ALTRO_OK;
}
altro_status altro_get_knot_params(altro_handle h, int index, double* out) {
  if (!h || !out) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (NotKnotConstraint(h, index, "altro_get_knot_params")) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.GetKnotParams(index, out); });
}
altro_status altro_set_initial_state(altro_handle h, const double* x0, int per_instance) {
  if (!h || !x0) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  const altro_desc& d = h->spec.desc;
  h->spec.x0.assign(x0, x0 + (size_t)d.n * (per_instance ? d.batch : 1));
  h->spec.x0_per_instance = per_instance;
  if (h->uploaded) return h->engine->SetInitialState(h->spec, &h->err);
  return ALTRO_OK;
}
altro_status altro_set_trajectory(altro_handle h, const double* X, const double* U, int per_instance) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  const altro_desc& d = h->spec.desc;
  const size_t mult = per_instance ? d.batch : 1;
  h->spec.has_X = X != nullptr;
  h->spec.has_U = U != nullptr;
  h->spec.traj_per_instance = per_instance;
  if (h->uploaded) {  // (no copy into the recorded definition: nothing reads it after the upload)
    h->spec.X_view = X;
    h->spec.U_view = U;
    const altro_status st = h->engine->SetTrajectory(h->spec, &h->err);
    h->spec.X_view = nullptr;
    h->spec.U_view = nullptr;
    return st;
  }
  if (X) h->spec.X.assign(X, X + mult * (d.N + 1) * d.n);
  if (U) h->spec.U.assign(U, U + mult * d.N * d.m);
  return ALTRO_OK;
}
altro_status altro_reset_trajectory(altro_handle h) {
  return Forward(h, [&](EngineBase& e) { return e.ResetTrajectory(); });
}
altro_status altro_reset_stats(altro_handle h) {
  return Forward(h, [&](EngineBase& e) { return e.ResetStats(); });
}
altro_status altro_set_options(altro_handle h, const altro_options* o) {
  if (!h || !o) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  h->opts = *o;
  return ALTRO_OK;
}
altro_status altro_get_options(altro_handle h, altro_options* o) {
  if (!h || !o) return ALTRO_INVALID_ARG;
  *o = h->opts;
  return ALTRO_OK;
}
altro_status altro_set_penalty(altro_handle h, double rho) {
  if (!h || !(rho >= 0)) return ALTRO_INVALID_ARG;  // ALTRO_ASSERT(rho >= 0), constraint_values.hpp:80
  if (Busy(h)) return ALTRO_NOT_READY;
  h->spec.penalty = rho;
  if (h->uploaded) return Forward(h, [&](EngineBase& e) { return e.SetPenalty(rho); });
  return ALTRO_OK;
}
altro_status altro_set_penalty_scaling(altro_handle h, double phi) {
  if (!h || !(phi >= 1)) return ALTRO_INVALID_ARG;  // ALTRO_ASSERT(phi >= 1), constraint_values.hpp:85
  if (Busy(h)) return ALTRO_NOT_READY;
  h->spec.phi = phi;
  if (h->uploaded) return Forward(h, [&](EngineBase& e) { return e.SetPenaltyScaling(phi); });
  return ALTRO_OK;
}

altro_status altro_solve_al(altro_handle h) {
  if (h) h->ilqr_mode = false;
  return SolvedAfter(h, ForwardCost(h, [&](EngineBase& e) { return e.SolveAL(h->opts); }));
}
altro_status altro_solve_ilqr(altro_handle h) {
  if (h) h->ilqr_mode = true;
  return SolvedAfter(h, ForwardCost(h, [&](EngineBase& e) { return e.SolveILQR(h->opts); }));
}
altro_status altro_solve_al_async(altro_handle h) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (ReferenceMissing(h)) return ALTRO_NOT_READY;
  // create the device state on the caller's thread: definition errors are reported here, synchronously
  altro_status st = Ensure(h);
  if (st != ALTRO_OK) return st;
  h->ilqr_mode = false;
  if (!h->worker.joinable()) {
    h->worker = std::thread([h]() {
      for (;;) {
        {
          std::unique_lock<std::mutex> lk(h->mu);
          h->cv.wait(lk, [h]() { return h->job_posted || h->worker_exit; });
          if (h->worker_exit) return;
          h->job_posted = false;
        }
        // the engine and the options are frozen while async_pending is set (Busy() guards every setter)
        h->async_status = h->engine->SolveAL(h->opts);
        if (h->async_status != ALTRO_OK) h->async_err = h->engine->LastError();
        {
          std::lock_guard<std::mutex> lk(h->mu);  // (the flag changes under the mutex: altro_wait cannot miss the wake-up)
          h->async_done.store(1, std::memory_order_release);
        }
        h->cv_done.notify_all();
      }
    });
  }
  h->async_pending = true;
  h->async_done.store(0);
  {
    std::lock_guard<std::mutex> lk(h->mu);
    h->job_posted = true;
  }
  h->cv.notify_one();
  return ALTRO_OK;
}
altro_status altro_solve_poll(altro_handle h, int* done) {
  if (!h || !done) return ALTRO_INVALID_ARG;
  *done = h->async_done.load(std::memory_order_acquire);
  return ALTRO_OK;
}
altro_status altro_wait(altro_handle h) {
  if (!h) return ALTRO_INVALID_ARG;
  if (!h->async_pending) {
    h->err = "no asynchronous solve is pending";
    return ALTRO_NOT_READY;
  }
  {
    // blocks on a condition variable (the atomic alone serves altro_solve_poll): a waiting caller costs no core
    std::unique_lock<std::mutex> lk(h->mu);
    h->cv_done.wait(lk, [h]() { return h->async_done.load(std::memory_order_acquire) != 0; });
  }
  h->async_pending = false;
  if (h->async_status != ALTRO_OK) h->err = h->async_err;
  return SolvedAfter(h, h->async_status);
}
altro_status altro_al_init(altro_handle h) { return ForwardCost(h, [&](EngineBase& e) { return e.AlInit(h->opts); }); }
altro_status altro_solve_setup(altro_handle h) { return Forward(h, [&](EngineBase& e) { return e.SolveSetup(h->opts); }); }
altro_status altro_rollout(altro_handle h) { return Forward(h, [&](EngineBase& e) { return e.Rollout(h->opts); }); }
altro_status altro_cost(altro_handle h, double* J) { return ForwardCost(h, [&](EngineBase& e) { return e.Cost(h->opts, J); }); }
altro_status altro_update_expansions(altro_handle h) { return ForwardCost(h, [&](EngineBase& e) { return e.UpdateExpansions(h->opts); }); }
altro_status altro_backward_pass(altro_handle h) {
  return GainsAfter(h, Forward(h, [&](EngineBase& e) { return e.BackwardPass(h->opts); }));
}
altro_status altro_forward_pass(altro_handle h) { return ForwardCost(h, [&](EngineBase& e) { return e.ForwardPass(h->opts); }); }
altro_status altro_update_convergence_statistics(altro_handle h) {
  return Forward(h, [&](EngineBase& e) { return e.UpdateConvergenceStatistics(h->opts); });
}
altro_status altro_update_duals(altro_handle h) { return Forward(h, [&](EngineBase& e) { return e.UpdateDuals(h->opts); }); }
altro_status altro_update_penalties(altro_handle h) { return Forward(h, [&](EngineBase& e) { return e.UpdatePenalties(h->opts); }); }
altro_status altro_get_max_violation(altro_handle h, double* out) {
  if (!out) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.GetMaxViolation(out); });
}
altro_status altro_max_violation(altro_handle h, double* out) {
  if (!out) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) {
    altro_status st = e.Cost(h->opts, nullptr);
    return st != ALTRO_OK ? st : e.GetMaxViolation(out);
  });
}
altro_status altro_get_max_penalty(altro_handle h, double* out) {
  if (!out) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.GetMaxPenalty(out); });
}

altro_status altro_get_trajectory(altro_handle h, double* X, double* U) {
  return Forward(h, [&](EngineBase& e) { return e.GetTrajectory(X, U); });
}
altro_status altro_get_gains(altro_handle h, double* K, double* d) {
  return Forward(h, [&](EngineBase& e) { return e.GetGains(K, d); });
}
altro_status altro_set_record_ctg(altro_handle h, int enable) {
  const altro_status st = Forward(h, [&](EngineBase& e) { return e.SetRecordCtg(enable); });
  if (h && st == ALTRO_OK) h->record_ctg = enable != 0;
  return st;
}
altro_status altro_get_ctg(altro_handle h, double* P, double* p) {
  return Forward(h, [&](EngineBase& e) { return e.GetCtg(P, p); });
}
altro_status altro_get_expansion(altro_handle h, int k, double* AB, double* lxx, double* lxu, double* luu,
                                 double* lx, double* lu) {
  return Forward(h, [&](EngineBase& e) { return e.GetExpansion(k, AB, lxx, lxu, luu, lx, lu); });
}
altro_status altro_get_knot_costs(altro_handle h, double* costs) {
  if (!costs) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.GetKnotCosts(costs); });
}
int altro_num_constraints(altro_handle h) {
  if (!h || Busy(h) || Ensure(h) != ALTRO_OK) return -1;
  return h->engine->NumRows();
}
int altro_num_constraints_at(altro_handle h, int k) {
  if (!h || Busy(h) || Ensure(h) != ALTRO_OK) return -1;
  return h->engine->NumRowsAt(k);
}
altro_status altro_get_duals(altro_handle h, double* lam) {
  if (!lam) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.GetRows(0, lam); });
}
altro_status altro_set_duals(altro_handle h, const double* lam) {
  if (!lam) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.SetDuals(lam); });
}
altro_status altro_get_penalties(altro_handle h, double* rho) {
  if (!rho) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.GetRows(1, rho); });
}
altro_status altro_get_constraint_values(altro_handle h, double* c) {
  if (!c) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.GetRows(2, c); });
}
altro_status altro_get_stats(altro_handle h, altro_stats* stats) {
  if (!stats) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.GetStats(stats, h->ilqr_mode); });
}
altro_status altro_get_timing(altro_handle h, altro_timing* t) {
  if (!t) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.GetTiming(t); });
}
altro_status altro_set_record_history(altro_handle h, int capacity) {
  return Forward(h, [&](EngineBase& e) { return e.SetRecordHistory(capacity); });
}
int altro_get_history(altro_handle h, int instance, int field, double* out, int cap) {
  if (!h || !out || Busy(h) || Ensure(h) != ALTRO_OK) return -1;
  return h->engine->GetHistory(instance, field, out, cap);
}
int altro_get_history_all(altro_handle h, int instance, double* out, int cap) {
  if (!h || !out || Busy(h) || Ensure(h) != ALTRO_OK) return -1;
  return h->engine->GetHistoryAll(instance, out, cap);
}
altro_status altro_device_info(altro_handle h, char* name, int name_len, int* cu_count) {
  if (!h) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.DeviceInfo(name, name_len, cu_count); });
}
altro_status altro_pack_results_device(altro_handle h, void* dst_device) {
  if (!dst_device) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.PackResultsDevice(dst_device); });
}
altro_status altro_pack_trajectory_device(altro_handle h, void* X_device, void* U_device) {
  if (!X_device && !U_device) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.PackTrajectoryDevice((double*)X_device, (double*)U_device); });
}

}  // extern "C"

// ---- receding-horizon loops (include/altro_mpc.h) -------------------------------------------------------------------
namespace {

// what can be said about an advance without a device: the range of the shift, and the handles whose per-knot data would
// have to move along the horizon too
altro_status MpcCheck(altro_handle h, int shift, const char* who) {
  const int N = h->spec.desc.N;
  if (shift < 1 || shift > N - 1) {
    h->err = std::string(who) + ": the shift must lie in [1, N - 1] = [1, " + std::to_string(N - 1) + "], got " + std::to_string(shift);
    return ALTRO_INVALID_ARG;
  }
  if (!h->spec.hk.empty() || !h->spec.tk.empty() || !h->spec.knot_model.empty()) {
    h->err = std::string(who) + ": per-knot steps, times or models (altro_set_steps, altro_set_times, altro_set_knot_models) do "
             "not move along the horizon yet";
    return ALTRO_UNSUPPORTED;
  }
  return ALTRO_OK;
}
// rows and cone of every registered constraint: the built-in kinds from the recorded calls, user types from the engine
altro_status MpcConShapes(altro_handle h, std::vector<int>* p, std::vector<int>* eq) {
  if (!h->uploaded) {
    bool user = false;
    for (const ConSpec& c : h->spec.cons) user = user || c.kind == ALTRO_CON_USER;
    if (!user) {
      const int m = h->spec.desc.m;
      for (const ConSpec& c : h->spec.cons) {
        int rows = 0;
        if (c.kind == ALTRO_CON_GOAL) {
          rows = h->spec.desc.n;
        } else if (c.kind == ALTRO_CON_CIRCLE) {
          rows = c.nparams / 3;
        } else if (c.kind == ALTRO_CON_CONTROL_BOUND && c.knot) {  // (a knot bound: every entry of its track is finite)
          rows = 2 * m;
        } else if (c.kind == ALTRO_CON_CONTROL_BOUND) {  // (the finite bounds: GetFiniteIndices, basic_constraints.hpp:138-145)
          for (int j = 0; j < 2 * m && j < c.nparams; ++j) rows += std::abs(c.params[j]) < std::numeric_limits<double>::max() ? 1 : 0;
        } else {
          h->err = "unknown constraint kind";
          return ALTRO_INVALID_ARG;
        }
        p->push_back(rows);
        eq->push_back(c.kind == ALTRO_CON_GOAL ? 1 : 0);
      }
      return ALTRO_OK;
    }
    const altro_status st = Ensure(h);  // (rows and cone of a user type are the model source's)
    if (st != ALTRO_OK) return st;
  }
  h->engine->ConShapes(p, eq);
  return ALTRO_OK;
}
altro_status MpcRowMapOf(altro_handle h, int shift, std::vector<int>* out) {
  std::vector<int> kb, ke, p, eq;
  const altro_status st = MpcConShapes(h, &p, &eq);
  if (st != ALTRO_OK) return st;
  for (const ConSpec& c : h->spec.cons) {
    kb.push_back(c.k_begin);
    ke.push_back(c.k_end);
  }
  *out = MpcRowMap(h->spec.desc.N, shift, kb, ke, p, eq);
  return ALTRO_OK;
}
// the penalty of a row that starts afresh behind an advance
double ResetPenalty(altro_handle h) { return h->opts.initial_penalty > 0 ? h->opts.initial_penalty : 1.0; }
// behind an advance the initial state lives on the device alone (altro_get_initial_state reads it): the recorded one is out of date
void ForgetX0(altro_handle h) {
  h->spec.x0.clear();
  h->spec.x0_per_instance = 0;
}
// the advance behind both entry points; x0 is [B][n] here
altro_status MpcAdvanceImpl(altro_handle h, int shift, const double* x0, const double* w, int on_device) {
  const altro_status st = Forward(h, [&](EngineBase& e) { return e.MpcAdvance(shift, x0, w, on_device, ResetPenalty(h)); });
  if (st == ALTRO_OK) ForgetX0(h);
  return st;
}

static_assert(sizeof(altro_track_stats) == sizeof(TrackStats) && sizeof(altro_track_stats) == 40 &&
                  offsetof(altro_track_stats, steps_done) == offsetof(TrackStats, steps_done) &&
                  offsetof(altro_track_stats, cost) == offsetof(TrackStats, cost) &&
                  offsetof(altro_track_stats, violation) == offsetof(TrackStats, violation) &&
                  offsetof(altro_track_stats, max_dx) == offsetof(TrackStats, max_dx) &&
                  offsetof(altro_track_stats, max_du) == offsetof(TrackStats, max_du),
              "altro_track_stats (include/altro_mpc.h) and TrackStats (altro_common.hpp) are one layout");
// the options a tracking call takes from the handle
TrackArgs TrackOpts(altro_handle h) {
  TrackArgs g{};
  g.check_bounds = h->opts.check_forwardpass_bounds;
  g.state_max = h->opts.state_max;
  g.control_max = h->opts.control_max;
  return g;
}
// both tracking entry points: everything that can be refused without a device first
altro_status MpcTrackImpl(altro_handle h, int steps, int samples, const double* dx0, const double* w, const double* u_lo,
                          const double* u_hi, double* X_cl, double* U_cl, altro_track_stats* stats, int on_device, const char* who) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (StepsRefused(h, steps, who)) return ALTRO_INVALID_ARG;
  if (samples < 1) {
    h->err = std::string(who) + ": at least one sample per instance, got " + std::to_string(samples);
    return ALTRO_INVALID_ARG;
  }
  if (BoundsRefused(h, u_lo, u_hi, who)) return ALTRO_INVALID_ARG;
  if (GainsMissing(h, who)) return ALTRO_NOT_READY;
  TrackArgs g = TrackOpts(h);
  g.steps = steps;
  g.S = samples;
  g.dx0 = dx0;
  g.w = w;
  g.u_lo = u_lo;
  g.u_hi = u_hi;
  g.X_cl = X_cl;
  g.U_cl = U_cl;
  g.stats = reinterpret_cast<TrackStats*>(stats);
  return Forward(h, [&](EngineBase& e) { return e.MpcTrack(g, on_device); });
}

// One closed-loop run, the skeleton of every altro_mpc_run*: the checks every kind shares, LoopBegin, `cycles` x (solve;
// LoopCycle; forget the recorded x0), and LoopEnd -- also after a failure, it frees the run's device blocks -- with the FIRST
// error's text kept.  The entry points check their own arguments first and bring what differs: the LoopSpec, the cycle's
// solve (altro_solve_al; the team's rounds) and where the logs go.  h is not null and not busy here.
template <class Solve>
altro_status RunClosedLoop(altro_handle h, const char* who, const LoopSpec& spec, Solve solve, const LoopOut& out) {
  if (spec.cycles < 1) {
    h->err = std::string(who) + ": at least one cycle";
    return ALTRO_INVALID_ARG;
  }
  altro_status st = MpcCheck(h, spec.shift, who);
  if (st != ALTRO_OK) return st;
  // (a team run writes the track of its knot constraint itself, in its first fill)
  if (spec.kind != kLoopTeam && ReferenceMissing(h)) return ALTRO_NOT_READY;
  st = Forward(h, [&](EngineBase& e) { return e.LoopBegin(spec); });
  for (int c = 0; c < spec.cycles && st == ALTRO_OK; ++c) {
    st = solve();
    if (st != ALTRO_OK) break;
    const LoopStep step{ResetPenalty(h), h->ilqr_mode, TrackOpts(h)};
    st = Forward(h, [&](EngineBase& e) { return e.LoopCycle(step); });
    if (st == ALTRO_OK) ForgetX0(h);
  }
  if (h->uploaded) {
    const std::string err = h->err;
    const altro_status es = h->engine->LoopEnd(out);
    if (st == ALTRO_OK && es != ALTRO_OK) {
      h->err = h->engine->LastError();
      st = es;
    } else {
      h->err = err;
    }
  }
  return st;
}
// w: [cycles][B][n] -- or [cycles][B][shift][n] under tracking
LoopSpec MakeLoopSpec(altro_handle h, LoopKind kind, int cycles, int shift, const double* w) {
  LoopSpec s{};
  s.kind = kind;
  s.cycles = cycles;
  s.shift = shift;
  s.w = w;
  s.w_stride = (size_t)h->spec.desc.batch * (size_t)h->spec.desc.n * (kind == kLoopTracked || kind == kLoopTriggered ? (size_t)std::max(shift, 0) : 1);
  return s;
}

}  // namespace

extern "C" {

int altro_mpc_num_rows(altro_handle h) {
  if (!h || Busy(h)) return -1;
  std::vector<int> map;
  if (MpcRowMapOf(h, 1, &map) != ALTRO_OK) return -1;
  return (int)map.size();
}
altro_status altro_mpc_row_map(altro_handle h, int shift, int* src_row) {
  if (!h || !src_row) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  altro_status st = MpcCheck(h, shift, "altro_mpc_row_map");
  if (st != ALTRO_OK) return st;
  std::vector<int> map;
  st = MpcRowMapOf(h, shift, &map);
  if (st != ALTRO_OK) return st;
  std::copy(map.begin(), map.end(), src_row);
  return ALTRO_OK;
}
altro_status altro_mpc_advance(altro_handle h, int shift, const double* x0, int x0_per_instance, const double* w) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  const altro_status st = MpcCheck(h, shift, "altro_mpc_advance");
  if (st != ALTRO_OK) return st;
  std::vector<double> all;
  if (x0 && !x0_per_instance) {  // one state for the whole batch
    const int n = h->spec.desc.n, B = h->spec.desc.batch;
    all.resize((size_t)B * n);
    for (int b = 0; b < B; ++b) std::copy(x0, x0 + n, all.begin() + (size_t)b * n);
    x0 = all.data();
  }
  return MpcAdvanceImpl(h, shift, x0, w, 0);
}
altro_status altro_mpc_advance_device(altro_handle h, int shift, const void* x0_device, const void* w_device) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  const altro_status st = MpcCheck(h, shift, "altro_mpc_advance_device");
  if (st != ALTRO_OK) return st;
  return MpcAdvanceImpl(h, shift, (const double*)x0_device, (const double*)w_device, 1);
}
altro_status altro_mpc_run(altro_handle h, int cycles, int shift, const double* w, double* X_cl, double* U_cl, int* iterations,
                           int* status) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  return RunClosedLoop(h, "altro_mpc_run", MakeLoopSpec(h, kLoopPlain, cycles, shift, w), [&] { return altro_solve_al(h); },
                       LoopOut{X_cl, U_cl, iterations, status, nullptr, nullptr, nullptr});
}
altro_status altro_mpc_track(altro_handle h, int steps, int samples, const double* dx0, const double* w, const double* u_lo,
                             const double* u_hi, double* X_cl, double* U_cl, altro_track_stats* stats) {
  return MpcTrackImpl(h, steps, samples, dx0, w, u_lo, u_hi, X_cl, U_cl, stats, 0, "altro_mpc_track");
}
altro_status altro_mpc_track_device(altro_handle h, int steps, int samples, const void* dx0_device, const void* w_device,
                                    const void* u_lo_device, const void* u_hi_device, void* X_cl_device, void* U_cl_device,
                                    void* stats_device) {
  return MpcTrackImpl(h, steps, samples, (const double*)dx0_device, (const double*)w_device, (const double*)u_lo_device,
                      (const double*)u_hi_device, (double*)X_cl_device, (double*)U_cl_device, (altro_track_stats*)stats_device, 1,
                      "altro_mpc_track_device");
}
altro_status altro_mpc_run_tracked(altro_handle h, int cycles, int shift, const double* w, const double* u_lo, const double* u_hi,
                                   double* X_cl, double* U_cl, int* iterations, int* status, altro_track_stats* track) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (cycles < 1) {  // (the driver's check, ahead of the bounds: a call with both wrong has always heard of the cycles)
    h->err = "altro_mpc_run_tracked: at least one cycle";
    return ALTRO_INVALID_ARG;
  }
  if (BoundsRefused(h, u_lo, u_hi, "altro_mpc_run_tracked")) return ALTRO_INVALID_ARG;
  LoopSpec spec = MakeLoopSpec(h, kLoopTracked, cycles, shift, w);
  spec.u_lo = u_lo;
  spec.u_hi = u_hi;
  return RunClosedLoop(h, "altro_mpc_run_tracked", spec, [&] { return altro_solve_al(h); },
                       LoopOut{X_cl, U_cl, iterations, status, nullptr, nullptr, reinterpret_cast<TrackStats*>(track)});
}
altro_status altro_get_initial_state(altro_handle h, double* x0) {
  if (!x0) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.GetInitialState(x0); });
}
altro_status altro_set_penalties(altro_handle h, const double* rho) {
  if (!rho) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.SetPenalties(rho); });
}

}  // extern "C"

// ---- multi-start (include/altro_multistart.h) -------------------------------------------------------------------------
namespace {

// everything that can be refused without a device; need_solve: the call reads the statistics of a finished solve
altro_status MsCheck(altro_handle h, int starts, bool need_solve, const char* who) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  const int B = h->spec.desc.batch;
  if (starts < 1 || B % starts != 0) {
    h->err = std::string(who) + ": starts must be at least 1 and divide the batch of " + std::to_string(B) + ", got " +
             std::to_string(starts);
    return ALTRO_INVALID_ARG;
  }
  if (need_solve && !h->has_solved) {
    h->err = std::string(who) + ": no solve has finished on this handle yet (altro_solve_al, altro_solve_ilqr, altro_wait)";
    return ALTRO_NOT_READY;
  }
  return ALTRO_OK;
}
altro_status MsSelectImpl(altro_handle h, int starts, int* winner, int on_device, const char* who) {
  const altro_status st = MsCheck(h, starts, true, who);
  if (st != ALTRO_OK) return st;
  if (!winner) {
    h->err = std::string(who) + ": winner is required";
    return ALTRO_INVALID_ARG;
  }
  return Forward(h, [&](EngineBase& e) { return e.MsSelect(starts, winner, on_device, h->ilqr_mode); });
}
altro_status MsSpreadImpl(altro_handle h, int starts, int* winner, int on_device, const char* who) {
  const altro_status st = MsCheck(h, starts, true, who);
  if (st != ALTRO_OK) return st;
  return Forward(h, [&](EngineBase& e) { return e.MsSpread(starts, winner, on_device, h->ilqr_mode); });
}
altro_status MsPerturbImpl(altro_handle h, int starts, const double* dU, int per_instance, int on_device, const char* who) {
  const altro_status st = MsCheck(h, starts, false, who);
  if (st != ALTRO_OK) return st;
  if (!dU) {
    h->err = std::string(who) + ": dU is required";
    return ALTRO_INVALID_ARG;
  }
  return Forward(h, [&](EngineBase& e) { return e.MsPerturb(starts, dU, per_instance, on_device); });
}
altro_status MsGetBestImpl(altro_handle h, int starts, double* X, double* U, altro_stats* stats, int* winner, int on_device,
                           const char* who) {
  const altro_status st = MsCheck(h, starts, true, who);
  if (st != ALTRO_OK) return st;
  if (!X && !U && !stats && !winner) {
    h->err = std::string(who) + ": at least one of X, U, stats, winner is required";
    return ALTRO_INVALID_ARG;
  }
  return Forward(h, [&](EngineBase& e) { return e.MsGetBest(starts, X, U, stats, winner, on_device, h->ilqr_mode); });
}

}  // namespace

extern "C" {

altro_status altro_multistart_select(altro_handle h, int starts, int* winner) {
  return MsSelectImpl(h, starts, winner, 0, "altro_multistart_select");
}
altro_status altro_multistart_select_device(altro_handle h, int starts, void* winner_device) {
  return MsSelectImpl(h, starts, (int*)winner_device, 1, "altro_multistart_select_device");
}
altro_status altro_multistart_spread(altro_handle h, int starts, int* winner) {
  return MsSpreadImpl(h, starts, winner, 0, "altro_multistart_spread");
}
altro_status altro_multistart_spread_device(altro_handle h, int starts, void* winner_device) {
  return MsSpreadImpl(h, starts, (int*)winner_device, 1, "altro_multistart_spread_device");
}
altro_status altro_multistart_perturb(altro_handle h, int starts, const double* dU, int per_instance) {
  return MsPerturbImpl(h, starts, dU, per_instance, 0, "altro_multistart_perturb");
}
altro_status altro_multistart_perturb_device(altro_handle h, int starts, const void* dU_device, int per_instance) {
  return MsPerturbImpl(h, starts, (const double*)dU_device, per_instance, 1, "altro_multistart_perturb_device");
}
altro_status altro_multistart_get_best(altro_handle h, int starts, double* X, double* U, altro_stats* stats, int* winner) {
  return MsGetBestImpl(h, starts, X, U, stats, winner, 0, "altro_multistart_get_best");
}
altro_status altro_multistart_get_best_device(altro_handle h, int starts, void* X_device, void* U_device, void* stats_device,
                                              void* winner_device) {
  return MsGetBestImpl(h, starts, (double*)X_device, (double*)U_device, (altro_stats*)stats_device, (int*)winner_device, 1,
                       "altro_multistart_get_best_device");
}
altro_status altro_mpc_run_multistart(altro_handle h, int starts, int cycles, int shift, const double* w, const double* dU,
                                      int dU_per_instance, double* X_cl, double* U_cl, int* iterations, int* status, int* winner) {
  altro_status st = MsCheck(h, starts, false, "altro_mpc_run_multistart");
  if (st != ALTRO_OK) return st;
  LoopSpec spec = MakeLoopSpec(h, kLoopMultiStart, cycles, shift, w);
  spec.G = starts;
  spec.dU = dU;
  spec.dU_per_instance = dU_per_instance;
  return RunClosedLoop(h, "altro_mpc_run_multistart", spec, [&] { return altro_solve_al(h); },
                       LoopOut{X_cl, U_cl, iterations, status, winner, nullptr, nullptr});
}

}  // extern "C"

// ---- teams (include/altro_team.h) ---------------------------------------------------------------------------------------
namespace {

// everything that can be refused without a device; the radii come back one per instance
altro_status TeamCheck(altro_handle h, int agents, int index, const double* radius, int radius_per_instance, const char* who,
                       std::vector<double>* rad) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  const int B = h->spec.desc.batch;
  if (agents < 2 || B % agents != 0) {
    h->err = std::string(who) + ": agents must be at least 2 and divide the batch of " + std::to_string(B) + ", got " +
             std::to_string(agents);
    return ALTRO_INVALID_ARG;
  }
  if (NotKnotConstraint(h, index, who)) return ALTRO_INVALID_ARG;
  const ConSpec& c = h->spec.cons[index];
  if (c.kind != ALTRO_CON_CIRCLE || c.nparams != 3 * (agents - 1)) {
    h->err = std::string(who) + ": constraint " + std::to_string(index) + " must be an ALTRO_CON_CIRCLE with nparams = 3 (agents - 1) = " +
             std::to_string(3 * (agents - 1));
    return ALTRO_INVALID_ARG;
  }
  if (!radius) {
    h->err = std::string(who) + ": radius is required";
    return ALTRO_INVALID_ARG;
  }
  rad->resize((size_t)B);
  for (int b = 0; b < B; ++b) {
    const double r = radius[radius_per_instance ? b : b % agents];
    if (NegativeRefused(h, r, "every radius", who)) return ALTRO_INVALID_ARG;
    (*rad)[(size_t)b] = r;
  }
  return ALTRO_OK;
}
altro_status TeamModeCheck(altro_handle h, int mode, double blend, const char* who) {
  if (mode != ALTRO_TEAM_ALL && mode != ALTRO_TEAM_PRIORITY) {
    h->err = std::string(who) + ": the mode is ALTRO_TEAM_ALL or ALTRO_TEAM_PRIORITY";
    return ALTRO_INVALID_ARG;
  }
  if (!(blend > 0.0) || !(blend <= 1.0)) {  // (a NaN fails both)
    h->err = std::string(who) + ": blend must lie in (0, 1]";
    return ALTRO_INVALID_ARG;
  }
  return ALTRO_OK;
}
altro_status TeamClearanceImpl(altro_handle h, int agents, int index, const double* radius, int radius_per_instance, double* clear,
                               int on_device, const char* who) {
  std::vector<double> rad;
  const altro_status st = TeamCheck(h, agents, index, radius, radius_per_instance, who, &rad);
  if (st != ALTRO_OK) return st;
  if (!clear) {
    h->err = std::string(who) + ": clear is required";
    return ALTRO_INVALID_ARG;
  }
  return Forward(h, [&](EngineBase& e) {
    const altro_status s = e.TeamRadius(rad.data());
    return s != ALTRO_OK ? s : e.TeamClearance(agents, index, clear, on_device);
  });
}
// rounds x (fill; solve) with the radii already on the device
altro_status TeamRounds(altro_handle h, int agents, int index, int mode, double blend, int rounds) {
  altro_status st = ALTRO_OK;
  for (int r = 0; r < rounds && st == ALTRO_OK; ++r) {
    st = Forward(h, [&](EngineBase& e) { return e.TeamFill(agents, index, mode, blend); });
    if (st == ALTRO_OK) st = altro_solve_al(h);
  }
  return st;
}

}  // namespace

extern "C" {

altro_status altro_team_fill_tracks(altro_handle h, int agents, int index, const double* radius, int radius_per_instance, int mode,
                                    double blend) {
  std::vector<double> rad;
  altro_status st = TeamCheck(h, agents, index, radius, radius_per_instance, "altro_team_fill_tracks", &rad);
  if (st == ALTRO_OK) st = TeamModeCheck(h, mode, blend, "altro_team_fill_tracks");
  if (st != ALTRO_OK) return st;
  return Forward(h, [&](EngineBase& e) {
    const altro_status s = e.TeamRadius(rad.data());
    return s != ALTRO_OK ? s : e.TeamFill(agents, index, mode, blend);
  });
}
altro_status altro_team_clearance(altro_handle h, int agents, int index, const double* radius, int radius_per_instance, double* clear) {
  return TeamClearanceImpl(h, agents, index, radius, radius_per_instance, clear, 0, "altro_team_clearance");
}
altro_status altro_team_clearance_device(altro_handle h, int agents, int index, const double* radius, int radius_per_instance,
                                         void* clear_device) {
  return TeamClearanceImpl(h, agents, index, radius, radius_per_instance, (double*)clear_device, 1, "altro_team_clearance_device");
}
altro_status altro_team_solve(altro_handle h, int agents, int index, const double* radius, int radius_per_instance, int mode,
                              double blend, int rounds) {
  std::vector<double> rad;
  altro_status st = TeamCheck(h, agents, index, radius, radius_per_instance, "altro_team_solve", &rad);
  if (st == ALTRO_OK) st = TeamModeCheck(h, mode, blend, "altro_team_solve");
  if (st != ALTRO_OK) return st;
  if (rounds < 1) {
    h->err = "altro_team_solve: at least one round";
    return ALTRO_INVALID_ARG;
  }
  st = Forward(h, [&](EngineBase& e) { return e.TeamRadius(rad.data()); });
  if (st == ALTRO_OK) st = TeamRounds(h, agents, index, mode, blend, rounds);
  return st;
}
altro_status altro_mpc_run_team(altro_handle h, int agents, int index, const double* radius, int radius_per_instance, int mode,
                                double blend, int rounds, int cycles, int shift, const double* w, double* X_cl, double* U_cl,
                                int* iterations, int* status, double* clear) {
  std::vector<double> rad;
  altro_status st = TeamCheck(h, agents, index, radius, radius_per_instance, "altro_mpc_run_team", &rad);
  if (st == ALTRO_OK) st = TeamModeCheck(h, mode, blend, "altro_mpc_run_team");
  if (st != ALTRO_OK) return st;
  if (rounds < 1 || cycles < 1) {
    h->err = "altro_mpc_run_team: at least one round and one cycle";
    return ALTRO_INVALID_ARG;
  }
  LoopSpec spec = MakeLoopSpec(h, kLoopTeam, cycles, shift, w);
  spec.A = agents;
  spec.index = index;
  spec.radius = rad.data();
  return RunClosedLoop(h, "altro_mpc_run_team", spec, [&] { return TeamRounds(h, agents, index, mode, blend, rounds); },
                       LoopOut{X_cl, U_cl, iterations, status, nullptr, clear, nullptr});
}

}  // extern "C"

// ---- the solve mask and sequential team rounds (include/altro_subset.h) ---------------------------------------------------
extern "C" {

altro_status altro_set_solve_mask(altro_handle h, const unsigned char* mask) {
  if (!h) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.SetSolveMask(mask, 0); });
}
altro_status altro_set_solve_mask_device(altro_handle h, const void* mask_device) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (!mask_device) {
    h->err = "altro_set_solve_mask_device: mask_device is required (altro_set_solve_mask(h, NULL) clears the mask)";
    return ALTRO_INVALID_ARG;
  }
  return Forward(h, [&](EngineBase& e) { return e.SetSolveMask((const unsigned char*)mask_device, 1); });
}
altro_status altro_get_solve_mask(altro_handle h, unsigned char* mask, int* count) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (!mask) {
    h->err = "altro_get_solve_mask: mask is required";
    return ALTRO_INVALID_ARG;
  }
  return Forward(h, [&](EngineBase& e) { return e.GetSolveMask(mask, count); });
}
altro_status altro_team_solve_sequential(altro_handle h, int agents, int index, const double* radius, int radius_per_instance,
                                         int sweeps) {
  std::vector<double> rad;
  altro_status st = TeamCheck(h, agents, index, radius, radius_per_instance, "altro_team_solve_sequential", &rad);
  if (st != ALTRO_OK) return st;
  if (sweeps < 1) {
    h->err = "altro_team_solve_sequential: at least one sweep";
    return ALTRO_INVALID_ARG;
  }
  st = Forward(h, [&](EngineBase& e) {
    const altro_status s = e.TeamRadius(rad.data());
    return s != ALTRO_OK ? s : e.SaveSolveMask();
  });
  if (st != ALTRO_OK) return st;
  for (int s = 0; s < sweeps && st == ALTRO_OK; ++s)
    for (int a = 0; a < agents && st == ALTRO_OK; ++a) {
      st = Forward(h, [&](EngineBase& e) {
        const altro_status f = e.TeamFill(agents, index, ALTRO_TEAM_ALL, 1.0);
        return f != ALTRO_OK ? f : e.TeamTurnMask(agents, a);
      });
      if (st == ALTRO_OK) st = altro_solve_al(h);
    }
  // the caller's mask comes back whatever happened; the first failure keeps its text
  const std::string err = h->err;
  const altro_status back = Forward(h, [&](EngineBase& e) { return e.RestoreSolveMask(); });
  if (st != ALTRO_OK) h->err = err;
  return st != ALTRO_OK ? st : back;
}

}  // extern "C"

// ---- event-triggered re-planning (include/altro_trigger.h) ------------------------------------------------------------------
namespace {

static_assert(sizeof(altro_trigger_rule) == sizeof(TriggerRule) && sizeof(altro_trigger_rule) == 40 &&
                  offsetof(altro_trigger_rule, max_age) == offsetof(TriggerRule, max_age) &&
                  offsetof(altro_trigger_rule, dx_tol) == offsetof(TriggerRule, dx_tol) &&
                  offsetof(altro_trigger_rule, viol_tol) == offsetof(TriggerRule, viol_tol) &&
                  offsetof(altro_trigger_rule, on_unsolved) == offsetof(TriggerRule, on_unsolved) &&
                  offsetof(altro_trigger_rule, lookahead) == offsetof(TriggerRule, lookahead) &&
                  offsetof(altro_trigger_rule, ahead_tol) == offsetof(TriggerRule, ahead_tol),
              "altro_trigger_rule (include/altro_trigger.h) and TriggerRule (altro_common.hpp) are one layout");
static_assert(ALTRO_TRIGGER_FIRST == kTrigFirst && ALTRO_TRIGGER_AGE == kTrigAge && ALTRO_TRIGGER_DEVIATION == kTrigDeviation &&
                  ALTRO_TRIGGER_VIOLATION == kTrigViolation && ALTRO_TRIGGER_LIMIT == kTrigLimit &&
                  ALTRO_TRIGGER_UNSOLVED == kTrigUnsolved && ALTRO_TRIGGER_AHEAD == kTrigAhead,
              "ALTRO_TRIGGER_* (include/altro_trigger.h) and TriggerBit (altro_common.hpp) are the same bits");

TriggerRule RuleOf(const altro_trigger_rule& r) {
  return TriggerRule{r.max_age, r.dx_tol, r.viol_tol, r.on_unsolved, r.lookahead, r.ahead_tol};
}
// what can be said about a rule and the bounds without a device
altro_status TriggerRuleCheck(altro_handle h, const altro_trigger_rule* rule, const double* u_lo, const double* u_hi, const char* who) {
  const std::string w(who);
  const int N = h->spec.desc.N;
  if (!rule) {
    h->err = w + ": rule is required";
    return ALTRO_INVALID_ARG;
  }
  if (rule->max_age < 1) {
    h->err = w + ": max_age must be at least 1, got " + std::to_string(rule->max_age);
    return ALTRO_INVALID_ARG;
  }
  if (rule->dx_tol != rule->dx_tol || rule->viol_tol != rule->viol_tol || (rule->lookahead > 0 && rule->ahead_tol != rule->ahead_tol)) {
    h->err = w + ": a tolerance is NaN (a negative dx_tol or viol_tol switches its criterion off)";
    return ALTRO_INVALID_ARG;
  }
  if (rule->lookahead < 0 || rule->lookahead > N) {
    h->err = w + ": lookahead must lie in [0, N] = [0, " + std::to_string(N) + "], got " + std::to_string(rule->lookahead);
    return ALTRO_INVALID_ARG;
  }
  if (rule->lookahead > 0 && rule->ahead_tol < 0) {
    h->err = w + ": ahead_tol must not be negative with a lookahead";
    return ALTRO_INVALID_ARG;
  }
  if (BoundsRefused(h, u_lo, u_hi, who)) return ALTRO_INVALID_ARG;
  return ALTRO_OK;
}
// a handle that records the cost-to-go: masked solves refuse it (include/altro_subset.h), and so does everything built on them
altro_status TriggerCtgRefused(altro_handle h, const char* who) {
  if (!h->record_ctg) return ALTRO_OK;
  h->err = std::string(who) + ": a masked solve does not record the cost-to-go (altro_set_record_ctg): switch the records off";
  return ALTRO_UNSUPPORTED;
}
// both evaluation entry points: everything that can be refused without a device first
altro_status MpcTriggerImpl(altro_handle h, const altro_trigger_rule* rule, const altro_track_stats* tracked, const int* age,
                            const double* u_lo, const double* u_hi, unsigned char* mask, int* reason, int on_device, const char* who) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  const altro_status st = TriggerRuleCheck(h, rule, u_lo, u_hi, who);
  if (st != ALTRO_OK) return st;
  if (!h->spec.hk.empty() || !h->spec.tk.empty() || !h->spec.knot_model.empty()) {
    h->err = std::string(who) + ": per-knot steps, times or models (altro_set_steps, altro_set_times, altro_set_knot_models) do "
             "not move along the horizon yet";
    return ALTRO_UNSUPPORTED;
  }
  if (TriggerCtgRefused(h, who) != ALTRO_OK) return ALTRO_UNSUPPORTED;
  if (rule->lookahead > 0 && GainsMissing(h, who, true)) return ALTRO_NOT_READY;
  if (ReferenceMissing(h)) return ALTRO_NOT_READY;
  TriggerArgs g{};
  g.rule = RuleOf(*rule);
  g.tracked = reinterpret_cast<const TrackStats*>(tracked);
  g.age = age;
  g.u_lo = u_lo;
  g.u_hi = u_hi;
  g.mask = mask;
  g.reason = reason;
  g.track = TrackOpts(h);
  return Forward(h, [&](EngineBase& e) { return e.Trigger(g, on_device, h->ilqr_mode); });
}

}  // namespace

extern "C" {

altro_status altro_mpc_trigger(altro_handle h, const altro_trigger_rule* rule, const altro_track_stats* tracked, const int* age,
                               const double* u_lo, const double* u_hi, unsigned char* mask, int* reason) {
  return MpcTriggerImpl(h, rule, tracked, age, u_lo, u_hi, mask, reason, 0, "altro_mpc_trigger");
}
altro_status altro_mpc_trigger_device(altro_handle h, const altro_trigger_rule* rule, const void* tracked_device,
                                      const void* age_device, const void* u_lo_device, const void* u_hi_device, void* mask_device,
                                      void* reason_device) {
  return MpcTriggerImpl(h, rule, (const altro_track_stats*)tracked_device, (const int*)age_device, (const double*)u_lo_device,
                        (const double*)u_hi_device, (unsigned char*)mask_device, (int*)reason_device, 1, "altro_mpc_trigger_device");
}
altro_status altro_mpc_run_triggered(altro_handle h, int cycles, int shift, const double* w, const double* u_lo, const double* u_hi,
                                     const altro_trigger_rule* rule, double* X_cl, double* U_cl, int* iterations, int* status,
                                     altro_track_stats* track, int* reason) {
  const char* who = "altro_mpc_run_triggered";
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (cycles < 1) {
    h->err = std::string(who) + ": at least one cycle";
    return ALTRO_INVALID_ARG;
  }
  altro_status st = TriggerRuleCheck(h, rule, u_lo, u_hi, who);
  if (st != ALTRO_OK) return st;
  st = MpcCheck(h, shift, who);
  if (st == ALTRO_INVALID_ARG) return st;
  // a plan may be followed for max_age cycles: the last of them tracks knots (max_age - 1) shift .. max_age shift of it, and
  // the rule behind every cycle but that one looks `lookahead` knots ahead -- none of it may reach the held tail
  const int N = h->spec.desc.N;
  if ((long long)(rule->max_age - 1) * shift + std::max(shift, rule->lookahead) > N) {
    h->err = std::string(who) + ": (max_age - 1) * shift + max(shift, lookahead) = " +
             std::to_string((long long)(rule->max_age - 1) * shift + std::max(shift, rule->lookahead)) + " exceeds N = " + std::to_string(N) +
             ": a plan would be followed, or looked ahead, into the held tail";
    return ALTRO_INVALID_ARG;
  }
  if (st != ALTRO_OK) return st;
  if (TriggerCtgRefused(h, who) != ALTRO_OK) return ALTRO_UNSUPPORTED;
  LoopSpec spec = MakeLoopSpec(h, kLoopTriggered, cycles, shift, w);
  spec.u_lo = u_lo;
  spec.u_hi = u_hi;
  spec.rule = RuleOf(*rule);
  LoopOut out{X_cl, U_cl, iterations, status, nullptr, nullptr, reinterpret_cast<TrackStats*>(track)};
  out.reason = reason;
  return RunClosedLoop(h, who, spec, [&] { return altro_solve_al(h); }, out);
}

}  // extern "C"

// ---- closed-loop covariance (include/altro_covariance.h) ----------------------------------------------------------------
namespace {

// both propagation entry points: everything that can be refused without a device first
altro_status CovPropagateImpl(altro_handle h, int steps, const double* Sigma0, int sigma0_per_instance, const double* W, int w_mode,
                              double* Sigma, double* sx, double* su, double* rpos, int on_device, const char* who) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (StepsRefused(h, steps, who)) return ALTRO_INVALID_ARG;
  if (!Sigma && !sx && !su && !rpos) {
    h->err = std::string(who) + ": at least one of Sigma, sx, su and rpos is required";
    return ALTRO_INVALID_ARG;
  }
  if (WModeRefused(h, w_mode, who)) return ALTRO_INVALID_ARG;
  if (rpos && h->spec.desc.n < 2) {
    h->err = std::string(who) + ": rpos is the spread of the position (x[0], x[1]) and needs at least two states";
    return ALTRO_INVALID_ARG;
  }
  if (GainsMissing(h, who)) return ALTRO_NOT_READY;
  CovArgs g{};
  g.steps = steps;
  g.sigma0_per_instance = sigma0_per_instance ? 1 : 0;
  g.w_mode = w_mode;
  g.Sigma0 = Sigma0;
  g.W = W;
  g.Sigma = Sigma;
  g.sx = sx;
  g.su = su;
  g.rpos = rpos;
  return Forward(h, [&](EngineBase& e) { return e.CovPropagate(g, on_device); });
}
altro_status CovInflateImpl(altro_handle h, int index, const double* base, int rows, int per_instance, double kappa, const double* rpos,
                            int on_device, const char* who) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (NotKnotConstraint(h, index, who)) return ALTRO_INVALID_ARG;
  if (h->spec.cons[index].kind != ALTRO_CON_CIRCLE || h->spec.cons[index].nparams % 3 != 0) {
    h->err = std::string(who) + ": constraint " + std::to_string(index) + " must be an ALTRO_CON_CIRCLE";
    return ALTRO_INVALID_ARG;
  }
  if (!base || !rpos) {
    h->err = std::string(who) + ": base and rpos are required";
    return ALTRO_INVALID_ARG;
  }
  if (rows < 1) {
    h->err = std::string(who) + ": the base track needs at least one row, got " + std::to_string(rows);
    return ALTRO_INVALID_ARG;
  }
  if (NegativeRefused(h, kappa, "kappa", who)) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.CovInflate(index, base, rows, per_instance ? 1 : 0, kappa, rpos, on_device); });
}

}  // namespace

extern "C" {

altro_status altro_cov_propagate(altro_handle h, int steps, const double* Sigma0, int sigma0_per_instance, const double* W, int w_mode,
                                 double* Sigma, double* sx, double* su, double* rpos) {
  return CovPropagateImpl(h, steps, Sigma0, sigma0_per_instance, W, w_mode, Sigma, sx, su, rpos, 0, "altro_cov_propagate");
}
altro_status altro_cov_propagate_device(altro_handle h, int steps, const void* Sigma0_device, int sigma0_per_instance,
                                        const void* W_device, int w_mode, void* Sigma_device, void* sx_device, void* su_device,
                                        void* rpos_device) {
  return CovPropagateImpl(h, steps, (const double*)Sigma0_device, sigma0_per_instance, (const double*)W_device, w_mode,
                          (double*)Sigma_device, (double*)sx_device, (double*)su_device, (double*)rpos_device, 1,
                          "altro_cov_propagate_device");
}
altro_status altro_cov_inflate_circles(altro_handle h, int index, const double* base, int rows, int per_instance, double kappa,
                                       const double* rpos) {
  return CovInflateImpl(h, index, base, rows, per_instance, kappa, rpos, 0, "altro_cov_inflate_circles");
}
altro_status altro_cov_inflate_circles_device(altro_handle h, int index, const void* base_device, int rows, int per_instance,
                                              double kappa, const void* rpos_device) {
  return CovInflateImpl(h, index, (const double*)base_device, rows, per_instance, kappa, (const double*)rpos_device, 1,
                        "altro_cov_inflate_circles_device");
}

}  // extern "C"

// ---- time-varying LQR tracking gains (include/altro_lqr.h) ---------------------------------------------------------------
static_assert(ALTRO_LQR_MAX_STATES == kLqrMaxN && ALTRO_LQR_MAX_CONTROLS == kLqrMaxM, "the header states the kernels' limits");
namespace {

// what every call refuses alike, without a device: the handle, an asynchronous solve, the dimensions
altro_status LqrCheck(altro_handle h, const char* who) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  const int n = h->spec.desc.n, m = h->spec.desc.m;
  if (m < 1 || m > kLqrMaxM || n > kLqrMaxN) {
    h->err = std::string(who) + ": 1 .. " + std::to_string(kLqrMaxM) + " controls and at most " + std::to_string(kLqrMaxN) +
             " states are supported, the handle has n = " + std::to_string(n) + ", m = " + std::to_string(m);
    return ALTRO_UNSUPPORTED;
  }
  return ALTRO_OK;
}
altro_status LqrGainsImpl(altro_handle h, const double* Q, const double* R, const double* Qf, int install, double* K, double* P, int* fail,
                          int on_device, const char* who) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (!Q || !R) {
    h->err = std::string(who) + ": Q and R are required";
    return ALTRO_INVALID_ARG;
  }
  if (!install && !K && !P) {
    h->err = std::string(who) + ": nothing asked for: K or P is required unless the gains are installed";
    return ALTRO_INVALID_ARG;
  }
  altro_status st = LqrCheck(h, who);
  if (st != ALTRO_OK) return st;
  if (!on_device) {  // (the engine packs them again for its launch; a device caller's weights are checked there)
    std::vector<double> packed;
    if (!LqrPackWeights(h->spec.desc.n, h->spec.desc.m, Q, R, Qf, &packed, &h->err, who)) return ALTRO_INVALID_ARG;
  }
  const LqrArgs g{Q, R, Qf, install ? 1 : 0, K, P, fail};
  st = Forward(h, [&](EngineBase& e) { return e.LqrGains(g, on_device); });
  if (install) return GainsAfter(h, st);
  return st;
}

}  // namespace

extern "C" {

altro_status altro_lqr_gains(altro_handle h, const double* Q, const double* R, const double* Qf, int install, double* K, double* P,
                             int* fail) {
  return LqrGainsImpl(h, Q, R, Qf, install, K, P, fail, 0, "altro_lqr_gains");
}
altro_status altro_lqr_gains_device(altro_handle h, const void* Q_device, const void* R_device, const void* Qf_device, int install,
                                    void* K_device, void* P_device, void* fail_device) {
  return LqrGainsImpl(h, (const double*)Q_device, (const double*)R_device, (const double*)Qf_device, install, (double*)K_device,
                      (double*)P_device, (int*)fail_device, 1, "altro_lqr_gains_device");
}
altro_status altro_lqr_set_policy(altro_handle h, const double* Q, const double* R, const double* Qf) {
  const char* who = "altro_lqr_set_policy";
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  std::vector<double> packed;
  if (Q) {
    if (!R) {
      h->err = std::string(who) + ": R is required with Q";
      return ALTRO_INVALID_ARG;
    }
    const altro_status st = LqrCheck(h, who);
    if (st != ALTRO_OK) return st;
    if (!LqrPackWeights(h->spec.desc.n, h->spec.desc.m, Q, R, Qf, &packed, &h->err, who)) return ALTRO_INVALID_ARG;
  }
  h->lqr_policy = packed;
  if (h->uploaded) h->engine->LqrSetPolicy(h->lqr_policy);
  return ALTRO_OK;
}
altro_status altro_lqr_get_policy(altro_handle h, int* on, double* Q, double* R, double* Qf) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (!on) {
    h->err = "altro_lqr_get_policy: on is required";
    return ALTRO_INVALID_ARG;
  }
  *on = h->lqr_policy.empty() ? 0 : 1;
  if (*on) {
    const size_t nn = (size_t)h->spec.desc.n * h->spec.desc.n, mm = (size_t)h->spec.desc.m * h->spec.desc.m;
    const double* w = h->lqr_policy.data();
    if (Q) std::copy(w, w + nn, Q);
    if (R) std::copy(w + nn, w + nn + mm, R);
    if (Qf) std::copy(w + nn + mm, w + 2 * nn + mm, Qf);
  }
  return ALTRO_OK;
}

}  // extern "C"

// ---- Monte-Carlo ensembles (include/altro_ensemble.h) -------------------------------------------------------------------
static_assert(sizeof(altro_ensemble_stats) == sizeof(EnsembleStats) && sizeof(altro_ensemble_stats) == 56 &&
                  offsetof(altro_ensemble_stats, violated) == offsetof(EnsembleStats, violated) &&
                  offsetof(altro_ensemble_stats, cost_mean) == offsetof(EnsembleStats, cost_mean) &&
                  offsetof(altro_ensemble_stats, max_du) == offsetof(EnsembleStats, max_du),
              "altro_ensemble_stats and the kernel's EnsembleStats are one layout");
namespace {

// what the ensemble and the fill refuse alike, without a device
altro_status EnsCheck(altro_handle h, int steps, int samples, int w_mode, const char* who) {
  if (!h) return ALTRO_INVALID_ARG;
  if (Busy(h)) return ALTRO_NOT_READY;
  if (StepsRefused(h, steps, who)) return ALTRO_INVALID_ARG;
  if (samples < 1) {
    h->err = std::string(who) + ": at least one sample per instance, got " + std::to_string(samples);
    return ALTRO_INVALID_ARG;
  }
  if (WModeRefused(h, w_mode, who)) return ALTRO_INVALID_ARG;
  return ALTRO_OK;
}
altro_status EnsStates(altro_handle h, const char* who) {
  if (h->spec.desc.n > kEnsMaxN) {
    h->err = std::string(who) + ": models of more than " + std::to_string(kEnsMaxN) + " states are not supported";
    return ALTRO_UNSUPPORTED;
  }
  return ALTRO_OK;
}
altro_status MpcEnsembleImpl(altro_handle h, int steps, int samples, unsigned long long seed, unsigned long long instance_base,
                             const double* Sigma0, int sigma0_per_instance, const double* W, int w_mode, const double* u_lo,
                             const double* u_hi, double viol_tol, double* dev_mean, double* dev_mom2, int* alive, int* viol_count,
                             altro_ensemble_stats* summary, altro_track_stats* stats, int on_device, const char* who) {
  altro_status st = EnsCheck(h, steps, samples, w_mode, who);
  if (st != ALTRO_OK) return st;
  if (BoundsRefused(h, u_lo, u_hi, who)) return ALTRO_INVALID_ARG;
  if (NegativeRefused(h, viol_tol, "viol_tol", who)) return ALTRO_INVALID_ARG;
  if (!dev_mean && !dev_mom2 && !alive && !viol_count && !summary && !stats) {
    h->err = std::string(who) + ": at least one of dev_mean, dev_mom2, alive, viol_count, summary and stats is required";
    return ALTRO_INVALID_ARG;
  }
  if ((st = EnsStates(h, who)) != ALTRO_OK) return st;
  if (GainsMissing(h, who)) return ALTRO_NOT_READY;
  const TrackArgs t = TrackOpts(h);
  EnsembleArgs g{};
  g.steps = steps, g.S = samples, g.sigma0_per_instance = sigma0_per_instance ? 1 : 0, g.w_mode = w_mode;
  g.seed = seed, g.instance_base = instance_base;
  g.Sigma0 = Sigma0, g.W = W, g.u_lo = u_lo, g.u_hi = u_hi;
  g.viol_tol = viol_tol;
  g.dev_mean = dev_mean, g.dev_mom2 = dev_mom2, g.alive = alive, g.viol_count = viol_count;
  g.summary = reinterpret_cast<EnsembleStats*>(summary);
  g.stats = reinterpret_cast<TrackStats*>(stats);
  g.check_bounds = t.check_bounds, g.state_max = t.state_max, g.control_max = t.control_max;
  return Forward(h, [&](EngineBase& e) { return e.MpcEnsemble(g, on_device); });
}
altro_status NoiseFillImpl(altro_handle h, int steps, int samples, unsigned long long seed, unsigned long long instance_base,
                           const double* Sigma0, int sigma0_per_instance, const double* W, int w_mode, double* dx0, double* w,
                           int on_device, const char* who) {
  altro_status st = EnsCheck(h, steps, samples, w_mode, who);
  if (st != ALTRO_OK) return st;
  if (!dx0 && !w) {
    h->err = std::string(who) + ": at least one of dx0 and w is required";
    return ALTRO_INVALID_ARG;
  }
  if ((st = EnsStates(h, who)) != ALTRO_OK) return st;
  EnsembleArgs g{};
  g.steps = steps, g.S = samples, g.sigma0_per_instance = sigma0_per_instance ? 1 : 0, g.w_mode = w_mode;
  g.seed = seed, g.instance_base = instance_base;
  g.Sigma0 = Sigma0, g.W = W, g.dx0 = dx0, g.w = w;
  return Forward(h, [&](EngineBase& e) { return e.NoiseFill(g, on_device); });
}

}  // namespace

extern "C" {

altro_status altro_mpc_ensemble(altro_handle h, int steps, int samples, unsigned long long seed, unsigned long long instance_base,
                                const double* Sigma0, int sigma0_per_instance, const double* W, int w_mode, const double* u_lo,
                                const double* u_hi, double viol_tol, double* dev_mean, double* dev_mom2, int* alive,
                                int* viol_count, altro_ensemble_stats* summary, altro_track_stats* stats) {
  return MpcEnsembleImpl(h, steps, samples, seed, instance_base, Sigma0, sigma0_per_instance, W, w_mode, u_lo, u_hi, viol_tol, dev_mean,
                         dev_mom2, alive, viol_count, summary, stats, 0, "altro_mpc_ensemble");
}
altro_status altro_mpc_ensemble_device(altro_handle h, int steps, int samples, unsigned long long seed,
                                       unsigned long long instance_base, const void* Sigma0_device, int sigma0_per_instance,
                                       const void* W_device, int w_mode, const void* u_lo_device, const void* u_hi_device,
                                       double viol_tol, void* dev_mean_device, void* dev_mom2_device, void* alive_device,
                                       void* viol_count_device, void* summary_device, void* stats_device) {
  return MpcEnsembleImpl(h, steps, samples, seed, instance_base, (const double*)Sigma0_device, sigma0_per_instance,
                         (const double*)W_device, w_mode, (const double*)u_lo_device, (const double*)u_hi_device, viol_tol,
                         (double*)dev_mean_device, (double*)dev_mom2_device, (int*)alive_device, (int*)viol_count_device,
                         (altro_ensemble_stats*)summary_device, (altro_track_stats*)stats_device, 1, "altro_mpc_ensemble_device");
}
altro_status altro_noise_fill(altro_handle h, int steps, int samples, unsigned long long seed, unsigned long long instance_base,
                              const double* Sigma0, int sigma0_per_instance, const double* W, int w_mode, double* dx0, double* w) {
  return NoiseFillImpl(h, steps, samples, seed, instance_base, Sigma0, sigma0_per_instance, W, w_mode, dx0, w, 0, "altro_noise_fill");
}
altro_status altro_noise_fill_device(altro_handle h, int steps, int samples, unsigned long long seed,
                                     unsigned long long instance_base, const void* Sigma0_device, int sigma0_per_instance,
                                     const void* W_device, int w_mode, void* dx0_device, void* w_device) {
  return NoiseFillImpl(h, steps, samples, seed, instance_base, (const double*)Sigma0_device, sigma0_per_instance,
                       (const double*)W_device, w_mode, (double*)dx0_device, (double*)w_device, 1, "altro_noise_fill_device");
}
altro_status altro_multistart_perturb_gaussian(altro_handle h, int starts, unsigned long long seed, unsigned long long instance_base,
                                               const double* sigma, int keep_first) {
  const char* who = "altro_multistart_perturb_gaussian";
  const altro_status st = MsCheck(h, starts, false, who);
  if (st != ALTRO_OK) return st;
  if (!sigma) {
    h->err = std::string(who) + ": sigma is required";
    return ALTRO_INVALID_ARG;
  }
  for (int i = 0; i < h->spec.desc.m; ++i)
    if (NegativeRefused(h, sigma[i], "sigma[" + std::to_string(i) + "]", who)) return ALTRO_INVALID_ARG;
  return Forward(h, [&](EngineBase& e) { return e.MsPerturbGaussian(starts, seed, instance_base, sigma, keep_first); });
}

}  // extern "C"
