"""altro-cpp_amd: ctypes host binding of libaltro_hip.so, the MI355X-native batched AL-iLQR solver.

The directory name carries a hyphen (fixed by the project layout), so it is imported through
``__graft_entry__.load_package()`` / ``tests/conftest.py`` under the module name ``altro_cpp_amd``.

This module is a *binding*: all arithmetic happens inside the HIP library behind the C-ABI declared
in ``include/altro_hip.h``.  There is no CPU fallback; loading fails loudly when the library has not
been built (``python -c 'import __graft_entry__ as g; g.build()'``).

``BatchSolver`` mirrors the method names of the reference's
``altro::augmented_lagrangian::AugmentedLagrangianiLQR<n,m>`` (altro/augmented_lagrangian/al_solver.hpp:28-224)
and ``altro::ilqr::iLQR<n,m>`` (altro/ilqr/ilqr.hpp:47-813) with an added batch dimension.
The class is generic over (library, symbol prefix) so the parity tests can drive the CPU oracle
(`oracle/`, prefix ``oracle_``) through the very same Python code; the product itself never does.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ALTRO_HIP_LIB: load another build of the library (experiments: scripts/README.md); still no CPU fallback
LIB_PATH = os.environ.get("ALTRO_HIP_LIB") or os.path.join(_HERE, "csrc", "libaltro_hip.so")

# --- enums (include/altro_hip.h) -------------------------------------------------------------------
OK, INVALID_ARG, HIP_ERROR, NOT_READY, UNSUPPORTED = 0, 1, 2, 3, 4
F64, F32 = 0, 1
MODEL_UNICYCLE, MODEL_TRIPLE_INTEGRATOR, MODEL_QUADROTOR12 = 1, 2, 3
CON_GOAL, CON_CONTROL_BOUND, CON_CIRCLE, CON_USER = 1, 2, 3, 4
TEAM_ALL, TEAM_PRIORITY = 0, 1  # include/altro_team.h
COV_W_PER_INSTANCE, COV_W_PER_KNOT = 1, 2  # include/altro_covariance.h: w_mode bits
# include/altro_trigger.h: the bits of a reason
(TRIGGER_FIRST, TRIGGER_AGE, TRIGGER_DEVIATION, TRIGGER_VIOLATION, TRIGGER_LIMIT, TRIGGER_UNSOLVED,
 TRIGGER_AHEAD) = 1, 2, 4, 8, 16, 32, 64
# altro::SolverStatus, altro/common/solver_stats.hpp:20-31
(SOLVED, UNSOLVED, STATE_LIMIT, CONTROL_LIMIT, COST_INCREASE, MAX_ITERATIONS, MAX_OUTER_ITERATIONS,
 MAX_INNER_ITERATIONS, MAX_PENALTY, BACKWARD_PASS_REGULARIZATION_FAILED) = range(10)
HISTORY_FIELDS = ("cost", "alpha", "improvement_ratio", "gradient", "cost_decrease",
                  "regularization", "violations", "max_penalty")


class Desc(C.Structure):
    _fields_ = [("n", C.c_int), ("m", C.c_int), ("N", C.c_int), ("batch", C.c_int),
                ("dtype", C.c_int), ("device_id", C.c_int)]


class Options(C.Structure):
    """altro::SolverOptions (altro/common/solver_options.hpp:19-57)."""
    _fields_ = [
        ("max_iterations_total", C.c_int), ("max_iterations_outer", C.c_int),
        ("max_iterations_inner", C.c_int), ("cost_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double), ("bp_reg_increase_factor", C.c_double),
        ("bp_reg_enable", C.c_int), ("bp_reg_initial", C.c_double), ("bp_reg_max", C.c_double),
        ("bp_reg_min", C.c_double), ("bp_reg_fail_threshold", C.c_int),
        ("check_forwardpass_bounds", C.c_int), ("state_max", C.c_double),
        ("control_max", C.c_double), ("line_search_max_iterations", C.c_int),
        ("line_search_lower_bound", C.c_double), ("line_search_upper_bound", C.c_double),
        ("line_search_decrease_factor", C.c_double), ("constraint_tolerance", C.c_double),
        ("maximum_penalty", C.c_double), ("initial_penalty", C.c_double),
        ("reset_duals", C.c_int), ("profiler_enable", C.c_int),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("status", C.c_int), ("status_ilqr", C.c_int), ("iterations_inner", C.c_int),
        ("iterations_outer", C.c_int), ("iterations_total", C.c_int), ("reserved", C.c_int),
        ("cost", C.c_double), ("initial_cost", C.c_double), ("cost_decrease", C.c_double),
        ("gradient", C.c_double), ("violation", C.c_double), ("max_penalty", C.c_double),
        ("alpha", C.c_double), ("regularization", C.c_double), ("improvement_ratio", C.c_double),
    ]


STATS_DTYPE = np.dtype([(name, np.int32 if t is C.c_int else np.float64) for name, t in Stats._fields_])
assert STATS_DTYPE.itemsize == C.sizeof(Stats)


class TrackStats(C.Structure):
    """altro_track_stats (include/altro_mpc.h): one per (instance, sample) of mpc_track."""
    _fields_ = [("status", C.c_int), ("steps_done", C.c_int), ("cost", C.c_double), ("violation", C.c_double),
                ("max_dx", C.c_double), ("max_du", C.c_double)]


TRACK_STATS_DTYPE = np.dtype([(name, np.int32 if t is C.c_int else np.float64) for name, t in TrackStats._fields_])
assert TRACK_STATS_DTYPE.itemsize == C.sizeof(TrackStats) == 40


class EnsembleStats(C.Structure):
    """altro_ensemble_stats (include/altro_ensemble.h): one per instance of mpc_ensemble."""
    _fields_ = [("samples", C.c_int), ("stopped_state", C.c_int), ("stopped_control", C.c_int), ("violated", C.c_int),
                ("cost_mean", C.c_double), ("cost_max", C.c_double), ("violation_max", C.c_double), ("max_dx", C.c_double),
                ("max_du", C.c_double)]


ENSEMBLE_STATS_DTYPE = np.dtype([(name, np.int32 if t is C.c_int else np.float64) for name, t in EnsembleStats._fields_])
assert ENSEMBLE_STATS_DTYPE.itemsize == C.sizeof(EnsembleStats) == 56


def ensemble_covariance(dev_mean, dev_mom2):
    """The sample covariance about the sample mean from what mpc_ensemble returns: dev_mom2 - dev_mean dev_mean^T, per
    (instance, knot); dev_mean [...][n], dev_mom2 [...][n][n]."""
    mean, mom2 = np.asarray(dev_mean, dtype=np.float64), np.asarray(dev_mom2, dtype=np.float64)
    return mom2 - mean[..., :, None] * mean[..., None, :]


class TriggerRule(C.Structure):
    """altro_trigger_rule (include/altro_trigger.h): when an instance is re-planned.  The defaults re-plan by age alone."""
    _fields_ = [("max_age", C.c_int), ("dx_tol", C.c_double), ("viol_tol", C.c_double), ("on_unsolved", C.c_int),
                ("lookahead", C.c_int), ("ahead_tol", C.c_double)]

    def __init__(self, max_age=1, dx_tol=-1.0, viol_tol=-1.0, on_unsolved=0, lookahead=0, ahead_tol=0.0):
        super().__init__(int(max_age), float(dx_tol), float(viol_tol), int(on_unsolved), int(lookahead), float(ahead_tol))


assert C.sizeof(TriggerRule) == 40


class Timing(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("init_ms", C.c_double), ("expansions_ms", C.c_double),
                ("backward_pass_ms", C.c_double), ("forward_pass_ms", C.c_double), ("fused_ms", C.c_double),
                ("sweeps", C.c_int), ("fused_sweeps", C.c_int), ("launches", C.c_int), ("sweep_launches", C.c_int),
                ("instance_iterations", C.c_longlong), ("fused_instance_iterations", C.c_longlong),
                ("host_naps", C.c_int), ("twin_workgroups", C.c_int),
                ("twin_claims", C.c_int), ("twin_handovers", C.c_int),
                ("fused_workgroup_iterations", C.c_int), ("segment_columns", C.c_int),
                ("loop_ms", C.c_double), ("loop_workgroups", C.c_int), ("loop_iterations", C.c_int),
                ("loop_handover", C.c_int), ("loop_instance_iterations", C.c_longlong)]


class AltroError(RuntimeError):
    pass


_lib_cache = {}


def load_library(path=None):
    """dlopen libaltro_hip.so.  Raises (never falls back) when the HIP extension is missing."""
    path = path or LIB_PATH
    if path not in _lib_cache:
        if not os.path.exists(path):
            raise AltroError(
                f"{path} not found: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
        _lib_cache[path] = C.CDLL(path)
    return _lib_cache[path]


MODEL_USER_BASE = 1000


def register_model_source(name, source, check_jacobian=True, _lib=None, _prefix="altro_"):
    """User-defined dynamics (altro_register_model_source, include/altro_hip.h): `source` defines
    ``struct UserModel { static constexpr int n, m; f(x, u, xdot); jac(x, u, J); }``.  Compiles (or loads from the
    on-disk cache) the plugin and returns the model kind for ``BatchSolver.set_model``."""
    lib = _lib if _lib is not None else load_library()
    f = getattr(lib, _prefix + "register_model_source")
    f.restype = C.c_int
    kind = C.c_int(0)
    st = f(name.encode(), source.encode(), C.c_int(1 if check_jacobian else 0), C.byref(kind))
    if st != OK:
        g = getattr(lib, _prefix + "last_error")
        g.restype = C.c_char_p
        g.argtypes = [C.c_void_p]
        msg = g(None)
        raise AltroError(f"{_prefix}register_model_source failed ({st}): {msg.decode() if msg else ''}")
    return kind.value


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def user_model_path(kind, _lib=None):
    """Path of the cached plugin (.so) of a registered user model."""
    lib = _lib if _lib is not None else load_library()
    buf = C.create_string_buffer(4096)
    f = lib.altro_user_model_path
    f.restype = C.c_int
    if f(C.c_int(kind), buf, C.c_int(len(buf))) < 0:
        raise AltroError(f"unknown user model kind {kind}")
    return buf.value.decode()


class BatchSolver:
    """Batched AL-iLQR solver handle (one device, one stream)."""

    def __init__(self, n, m, N, batch=1, dtype=F64, device_id=0, _lib=None, _prefix="altro_"):
        self._lib = _lib if _lib is not None else load_library()
        self._p = _prefix
        self.n, self.m, self.N, self.batch, self.dtype = int(n), int(m), int(N), int(batch), int(dtype)
        self._h = C.c_void_p()
        self._knot_nparams = {}  # registration index of a knot constraint -> (nparams, knots)
        d = Desc(self.n, self.m, self.N, self.batch, self.dtype, int(device_id))
        f = self._fn("create")
        f.restype = C.c_int
        st = f(C.byref(d), C.byref(self._h))
        if st != OK:
            raise AltroError(f"{self._p}create failed ({st}): {self._errmsg(None)}")

    # -- plumbing ---------------------------------------------------------------------------------
    def _fn(self, name):
        return getattr(self._lib, self._p + name)

    def _errmsg(self, h):
        f = self._fn("last_error")
        f.restype = C.c_char_p
        f.argtypes = [C.c_void_p]
        s = f(h)
        return s.decode() if s else ""

    def _call(self, name, *args):
        f = self._fn(name)
        f.restype = C.c_int
        st = f(self._h, *args)
        if st != OK:
            raise AltroError(f"{self._p}{name} failed ({st}): {self._errmsg(self._h)}")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            f = self._fn("destroy")
            f.restype = None
            f.argtypes = [C.c_void_p]
            f(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- problem definition (altro::problem::Problem, problem.hpp:113-202) -------------------------
    def set_model(self, kind, params=()):
        p = _f64(list(params)) if len(params) else None
        self._call("set_model", C.c_int(kind), _dp(p), C.c_int(0 if p is None else p.size))

    def set_knot_models(self, model_of_knot):
        """Problem::SetDynamics(model, k) with models that differ along the horizon (problem.hpp:155-166): index of knot
        k's model (k = 0 .. N-1) in the user source's ALTRO_USER_MODELS list."""
        km = np.ascontiguousarray(model_of_knot, dtype=np.int32)
        self._call("set_knot_models", km.ctypes.data_as(C.POINTER(C.c_int)), C.c_int(km.size))

    def set_uniform_step(self, h):
        self._call("set_uniform_step", C.c_float(np.float32(h)))

    def set_steps(self, hk):
        """Trajectory::SetStep(k, h), k = 0 .. N-1 (trajectory.hpp:120): 32-bit float steps."""
        hk = np.ascontiguousarray(hk, dtype=np.float32)
        self._call("set_steps", hk.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(hk.size))

    def set_times(self, tk):
        """Trajectory::SetTime(k, t), k = 0 .. N (trajectory.hpp:119)."""
        tk = np.ascontiguousarray(tk, dtype=np.float32)
        self._call("set_times", tk.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(tk.size))

    def get_steps(self):
        hk = np.zeros(self.N, dtype=np.float32)
        tk = np.zeros(self.N + 1, dtype=np.float32)
        self._call("get_steps", hk.ctypes.data_as(C.POINTER(C.c_float)), tk.ctypes.data_as(C.POINTER(C.c_float)))
        return hk, tk

    def set_lqr_cost(self, k_begin, k_end, Q, R, xref, uref):
        Q, R, xref, uref = _f64(Q), _f64(R), _f64(xref), _f64(uref)
        # numpy matrices are row-major; Q and R are symmetric in every caller, but transpose anyway
        Qc = np.ascontiguousarray(Q.T)
        Rc = np.ascontiguousarray(R.T)
        per = (1 if xref.ndim == 2 else 0) | (2 if uref.ndim == 2 else 0)
        self._call("set_lqr_cost", C.c_int(k_begin), C.c_int(k_end), _dp(Qc), _dp(Rc), _dp(xref),
                   _dp(uref), C.c_int(per))

    def set_lqr_tracking_cost(self, k_begin, k_end, Q, R):
        """LQRCost(Q, R, xref_k, uref_k) on knots [k_begin, k_end) with the handle's reference path at every knot
        (set_reference): one cost group however many knots, the terms live on the device."""
        Q, R = _f64(Q), _f64(R)
        Qc = np.ascontiguousarray(Q.T)
        Rc = np.ascontiguousarray(R.T)
        self._call("set_lqr_tracking_cost", C.c_int(k_begin), C.c_int(k_end), _dp(Qc), _dp(Rc))

    def _reference_shape(self, Xref, Uref):
        if Xref.ndim not in (2, 3) or Xref.shape[-1] != self.n or (Xref.ndim == 3 and Xref.shape[0] != self.batch):
            raise ValueError(f"Xref must have shape (rows, {self.n}) or ({self.batch}, rows, {self.n})")
        if Uref is not None and Uref.shape != Xref.shape[:-1] + (self.m,):
            raise ValueError(f"Uref must have shape {Xref.shape[:-1] + (self.m,)}")
        return Xref.shape[-2], 1 if Xref.ndim == 3 else 0

    def set_reference(self, Xref, Uref=None):
        """The reference path of the tracking costs: Xref [rows][n], Uref [rows][m] (None: zeros), or [B][rows][.] per
        instance.  Knot k uses row min(offset + k, rows - 1); setting a path puts the offset back to 0."""
        Xref, Uref = _f64(Xref), _f64(Uref)
        rows, per = self._reference_shape(Xref, Uref)
        self._call("set_reference", _dp(Xref), _dp(Uref), C.c_int(rows), C.c_int(per))

    def set_reference_device(self, x_ptr, u_ptr, rows, per_instance):
        """set_reference with fp64 arrays in memory of this handle's device (u_ptr may be 0)."""
        self._call("set_reference_device", C.c_void_p(x_ptr or None), C.c_void_p(u_ptr or None), C.c_int(rows),
                   C.c_int(1 if per_instance else 0))

    def set_reference_offset(self, offset):
        self._call("set_reference_offset", C.c_int(offset))

    def get_reference_offset(self):
        off = C.c_int(0)
        self._call("get_reference_offset", C.byref(off))
        return off.value

    def get_reference_terms(self):
        """(q [B][N+1][n], r [B][N+1][m], c [B][N+1]): the linear and constant terms of the tracking costs as the kernels
        read them; zero on knots without a tracking cost."""
        q = np.empty((self.batch, self.N + 1, self.n))
        r = np.empty((self.batch, self.N + 1, self.m))
        c = np.empty((self.batch, self.N + 1))
        self._call("get_reference_terms", _dp(q), _dp(r), _dp(c))
        return q, r, c

    def set_user_cost(self, k_begin, k_end, params, type=0):
        """A user cost of the handle's user model (register_model_source) on knots [k_begin, k_end);
        params: [nparams] or [B][nparams]; ``type``: index of the cost class in the source's ALTRO_USER_COSTS list."""
        p = _f64(params)
        per = 1 if p.ndim == 2 else 0
        self._call("set_user_cost_type", C.c_int(type), C.c_int(k_begin), C.c_int(k_end), _dp(p), C.c_int(p.shape[-1]), C.c_int(per))

    def add_constraint(self, kind, k_begin, k_end, params):
        p = _f64(params)
        per = 1 if p.ndim == 2 else 0
        self._call("add_constraint", C.c_int(kind), C.c_int(k_begin), C.c_int(k_end), _dp(p),
                   C.c_int(p.shape[-1]), C.c_int(per))

    def add_user_constraint(self, k_begin, k_end, params, type=0):
        """A user constraint of the handle's user model on knots [k_begin, k_end); params: [nparams] or [B][nparams];
        ``type``: index of the constraint class in the source's ALTRO_USER_CONSTRAINTS list."""
        p = _f64(params)
        per = 1 if p.ndim == 2 else 0
        self._call("add_user_constraint_type", C.c_int(type), C.c_int(k_begin), C.c_int(k_end), _dp(p),
                   C.c_int(p.shape[-1]), C.c_int(per))

    def add_goal_constraint(self, k, xf):
        self.add_constraint(CON_GOAL, k, k + 1, xf)

    def add_control_bound(self, k_begin, k_end, lb, ub):
        self.add_constraint(CON_CONTROL_BOUND, k_begin, k_end, np.concatenate([_f64(lb), _f64(ub)]))

    def add_circle_constraint(self, k_begin, k_end, circles):
        """circles: [nobs][3] (cx, cy, r) or [B][nobs][3]."""
        c = _f64(circles)
        c = c.reshape(c.shape[0], -1) if c.ndim == 3 else c.reshape(-1)
        self.add_constraint(CON_CIRCLE, k_begin, k_end, c)

    # -- knot constraints (include/altro_knot_params.h): parameters that change from knot to knot --------------------------
    def add_knot_constraint(self, kind, k_begin, k_end, nparams, user_type=0):
        """A constraint of ``kind`` on knots [k_begin, k_end) whose parameters at knot k are row min(offset + k, rows - 1)
        of its track (set_constraint_track): ONE constraint however many knots.  Returns its registration index."""
        idx = C.c_int(-1)
        self._call("add_knot_constraint", C.c_int(kind), C.c_int(user_type), C.c_int(k_begin), C.c_int(k_end), C.c_int(nparams),
                   C.byref(idx))
        self._knot_nparams[idx.value] = (int(nparams), int(k_end) - int(k_begin))
        return idx.value

    def add_knot_circle_constraint(self, k_begin, k_end, ncircles, track=None):
        """Moving circles: the track rows are (cx, cy, r) per circle -- [rows][ncircles][3] or [B][rows][ncircles][3]."""
        idx = self.add_knot_constraint(CON_CIRCLE, k_begin, k_end, 3 * int(ncircles))
        if track is not None:
            t = _f64(track)
            self.set_constraint_track(idx, t.reshape(t.shape[:-2] + (-1,)) if t.shape[-1] == 3 and t.ndim >= 3 else t)
        return idx

    def add_knot_control_bound(self, k_begin, k_end, lb=None, ub=None):
        """A control bound that changes along the horizon: lb, ub are [rows][m] or [B][rows][m], every entry finite."""
        if (lb is None) != (ub is None):
            raise ValueError("a knot control bound takes lb and ub together (every entry of its track is finite)")
        idx = self.add_knot_constraint(CON_CONTROL_BOUND, k_begin, k_end, 2 * self.m)
        if lb is not None:
            self.set_constraint_track(idx, np.concatenate([_f64(lb), _f64(ub)], axis=-1))
        return idx

    def _track_shape(self, index, P):
        np_ = self._knot_nparams.get(index, (P.shape[-1], 0))[0]  # (an index this handle does not know: the library refuses it)
        if P.ndim not in (2, 3) or P.shape[-1] != np_ or (P.ndim == 3 and P.shape[0] != self.batch):
            raise ValueError(f"the track must have shape (rows, {np_}) or ({self.batch}, rows, {np_})")
        return P.shape[-2], 1 if P.ndim == 3 else 0

    def set_constraint_track(self, index, P):
        """The parameter track of knot constraint ``index``: [rows][nparams], or [B][rows][nparams] per instance.  Any time
        between solves; the window offset (set_track_offset) stays."""
        P = _f64(P)
        rows, per = self._track_shape(index, P)
        self._call("set_constraint_track", C.c_int(index), _dp(P), C.c_int(rows), C.c_int(per))

    def set_constraint_track_device(self, index, ptr, rows, per_instance):
        """set_constraint_track with an fp64 array in memory of this handle's device."""
        self._call("set_constraint_track_device", C.c_int(index), C.c_void_p(ptr or None), C.c_int(rows),
                   C.c_int(1 if per_instance else 0))

    def set_track_offset(self, offset):
        self._call("set_track_offset", C.c_int(offset))

    def get_track_offset(self):
        off = C.c_int(0)
        self._call("get_track_offset", C.byref(off))
        return off.value

    def get_knot_params(self, index):
        """[B][k_end - k_begin][nparams]: the parameters of knot constraint ``index`` as the kernels read them."""
        np_, knots = self._knot_nparams.get(index, (1, 1))  # (an unknown index: the library refuses it before it writes)
        out = np.empty((self.batch, knots, np_))
        self._call("get_knot_params", C.c_int(index), _dp(out))
        return out

    def set_initial_state(self, x0):
        x0 = _f64(x0)
        self._call("set_initial_state", _dp(x0), C.c_int(1 if x0.ndim == 2 else 0))

    def set_trajectory(self, X=None, U=None):
        X, U = _f64(X), _f64(U)
        per = 1 if (U is not None and U.ndim == 3) or (X is not None and X.ndim == 3) else 0
        self._call("set_trajectory", _dp(X), _dp(U), C.c_int(per))

    def reset_trajectory(self):
        self._call("reset_trajectory")

    def reset_stats(self):
        """solver.GetStats().Reset(): a bare iLQR solve accumulates iterations_total otherwise (quirk Q11)."""
        self._call("reset_stats")

    # -- options (solver.GetOptions()) -------------------------------------------------------------
    def default_options(self):
        o = Options()
        f = self._fn("default_options")
        f.restype = None
        f(C.byref(o))
        return o

    def get_options(self):
        o = Options()
        self._call("get_options", C.byref(o))
        return o

    def set_options(self, opts=None, **kw):
        o = opts if opts is not None else self.get_options()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        self._call("set_options", C.byref(o))

    def set_penalty(self, rho):
        self._call("set_penalty", C.c_double(rho))

    def set_penalty_scaling(self, phi):
        self._call("set_penalty_scaling", C.c_double(phi))

    # -- algorithm ------------------------------------------------------------------------------
    def solve(self):            # AugmentedLagrangianiLQR::Solve, al_solver.hpp:304-334
        self._call("solve_al")

    def solve_async(self):
        """Non-blocking AL solve on a worker thread of the library (MPC pattern); finish with wait()."""
        self._call("solve_al_async")

    def poll(self):
        done = C.c_int(0)
        self._call("solve_poll", C.byref(done))
        return bool(done.value)

    def wait(self):
        self._call("wait")

    def solve_ilqr(self):       # iLQR::Solve, ilqr.hpp:284-316
        self._call("solve_ilqr")

    def al_init(self):
        self._call("al_init")

    def solve_setup(self):
        self._call("solve_setup")

    def rollout(self):
        self._call("rollout")

    def cost(self):
        J = np.empty(self.batch)
        self._call("cost", _dp(J))
        return J

    def update_expansions(self):
        self._call("update_expansions")

    def backward_pass(self):
        self._call("backward_pass")

    def forward_pass(self):
        self._call("forward_pass")

    def update_convergence_statistics(self):
        self._call("update_convergence_statistics")

    def update_duals(self):
        self._call("update_duals")

    def update_penalties(self):
        self._call("update_penalties")

    def get_max_violation(self):
        out = np.empty(self.batch)
        self._call("get_max_violation", _dp(out))
        return out

    def max_violation(self):
        out = np.empty(self.batch)
        self._call("max_violation", _dp(out))
        return out

    def get_max_penalty(self):
        out = np.empty(self.batch)
        self._call("get_max_penalty", _dp(out))
        return out

    # -- results ----------------------------------------------------------------------------------
    def get_trajectory(self, X=None, U=None):
        """X [batch][N+1][n], U [batch][N][m]; pass C-contiguous float64 arrays of these shapes to have them filled in
        place (a caller that solves in a loop keeps its buffers: fresh pages cost more than the copy)."""
        if X is None:
            X = np.empty((self.batch, self.N + 1, self.n))
        if U is None:
            U = np.empty((self.batch, self.N, self.m))
        for a_, shape in ((X, (self.batch, self.N + 1, self.n)), (U, (self.batch, self.N, self.m))):
            if a_.dtype != np.float64 or a_.shape != shape or not a_.flags["C_CONTIGUOUS"]:
                raise ValueError(f"get_trajectory needs C-contiguous float64 arrays of shape {shape}")
        self._call("get_trajectory", _dp(X), _dp(U))
        return X, U

    def get_gains(self):
        """K[b][k] as an (m x n) matrix, d[b][k] (m)."""
        K = np.empty((self.batch, self.N, self.n, self.m))  # column-major m x n per knot
        d = np.empty((self.batch, self.N, self.m))
        self._call("get_gains", _dp(K), _dp(d))
        return np.swapaxes(K, 2, 3), d

    def set_record_ctg(self, enable=True):
        self._call("set_record_ctg", C.c_int(1 if enable else 0))

    def get_ctg(self):
        P = np.empty((self.batch, self.N + 1, self.n, self.n))
        p = np.empty((self.batch, self.N + 1, self.n))
        self._call("get_ctg", _dp(P), _dp(p))
        return np.swapaxes(P, 2, 3), p

    def get_expansion(self, k):
        n, m, B = self.n, self.m, self.batch
        AB = np.empty((B, n + m, n))
        lxx = np.empty((B, n, n))
        lxu = np.empty((B, m, n))
        luu = np.empty((B, m, m))
        lx = np.empty((B, n))
        lu = np.empty((B, m))
        self._call("get_expansion", C.c_int(k), _dp(AB), _dp(lxx), _dp(lxu), _dp(luu), _dp(lx), _dp(lu))
        AB = np.swapaxes(AB, 1, 2)
        return dict(A=AB[:, :, :n], B=AB[:, :, n:], lxx=np.swapaxes(lxx, 1, 2),
                    lxu=np.swapaxes(lxu, 1, 2), luu=np.swapaxes(luu, 1, 2), lx=lx, lu=lu)

    def get_knot_costs(self):
        c = np.empty((self.batch, self.N + 1))
        self._call("get_knot_costs", _dp(c))
        return c

    def num_constraints(self, k=None):
        if k is None:
            f = self._fn("num_constraints")
            f.restype = C.c_int
            return f(self._h)
        f = self._fn("num_constraints_at")
        f.restype = C.c_int
        return f(self._h, C.c_int(k))

    def get_duals(self):
        out = np.empty((self.batch, max(self.num_constraints(), 0)))
        if out.size:
            self._call("get_duals", _dp(out))
        return out

    def set_duals(self, lam):
        lam = _f64(lam)
        self._call("set_duals", _dp(lam))

    def get_penalties(self):
        out = np.empty((self.batch, max(self.num_constraints(), 0)))
        if out.size:
            self._call("get_penalties", _dp(out))
        return out

    def get_constraint_values(self):
        out = np.empty((self.batch, max(self.num_constraints(), 0)))
        if out.size:
            self._call("get_constraint_values", _dp(out))
        return out

    def get_stats(self):
        """numpy structured array, one record per instance (altro_stats)."""
        out = np.zeros(self.batch, dtype=STATS_DTYPE)
        self._call("get_stats", out.ctypes.data_as(C.c_void_p))
        return out

    def get_timing(self):
        t = Timing()
        self._call("get_timing", C.byref(t))
        return {k: getattr(t, k) for k, _ in Timing._fields_}

    def set_record_history(self, capacity=301):
        self._call("set_record_history", C.c_int(capacity))

    def get_history(self, instance, field, cap=1024):
        fi = HISTORY_FIELDS.index(field) if isinstance(field, str) else int(field)
        out = np.empty(cap)
        f = self._fn("get_history")
        f.restype = C.c_int
        cnt = f(self._h, C.c_int(instance), C.c_int(fi), _dp(out), C.c_int(cap))
        if cnt < 0:
            raise AltroError("get_history failed: " + self._errmsg(self._h))
        return out[:cnt].copy()

    # -- receding-horizon loops (include/altro_mpc.h) ------------------------------------------------
    def mpc_row_map(self, shift):
        """Where every dual / penalty row comes from under a shift of ``shift`` knots: the source row, or -1 for a row
        that starts afresh.  Host-only (needs no device for the built-in constraint kinds)."""
        f = self._fn("mpc_num_rows")
        f.restype = C.c_int
        rows = f(self._h)
        out = np.empty(max(rows, 1), dtype=np.int32)
        self._call("mpc_row_map", C.c_int(shift), out.ctypes.data_as(C.POINTER(C.c_int)))  # (reports what mpc_num_rows met)
        if rows < 0:
            raise AltroError(f"{self._p}mpc_num_rows failed: {self._errmsg(self._h)}")
        return out[:rows]

    def mpc_advance(self, shift, x0=None, w=None):
        """Move the solved handle ``shift`` knots forward on the device (one launch): controls, gains, duals and penalties
        shift, the tail holds; the new initial state is ``x0`` ([n] or [B][n]; default: the plan's X[shift]) plus the
        disturbance ``w`` ([B][n])."""
        x0, w = _f64(x0), _f64(w)
        if x0 is not None and x0.shape not in ((self.n,), (self.batch, self.n)):
            raise ValueError(f"x0 must have shape ({self.n},) or ({self.batch}, {self.n})")
        if w is not None and w.shape != (self.batch, self.n):
            raise ValueError(f"w must have shape ({self.batch}, {self.n})")
        self._call("mpc_advance", C.c_int(shift), _dp(x0), C.c_int(1 if x0 is not None and x0.ndim == 2 else 0), _dp(w))

    def mpc_advance_device(self, shift, x0_ptr=0, w_ptr=0):
        """mpc_advance with fp64 arrays [B][n] in memory of this handle's device (either pointer may be 0)."""
        self._call("mpc_advance_device", C.c_int(shift), C.c_void_p(x0_ptr or None), C.c_void_p(w_ptr or None))

    def _run_logs(self, cycles, shift, w, per_knot=False):
        """What every mpc_run* shares: the checked disturbance ([cycles][B][n], per_knot [cycles][B][shift][n]), the dict of the
        logs the C call fills, and their four pointers in the order of the C signatures."""
        w = _f64(w)
        shape = (cycles, self.batch, shift, self.n) if per_knot else (cycles, self.batch, self.n)
        if w is not None and w.shape != shape:
            raise ValueError("w must have shape (" + ", ".join(str(v) for v in shape) + ")")
        L = max(cycles, 0) * max(shift, 0)
        out = dict(X_cl=np.zeros((self.batch, L + 1, self.n)), U_cl=np.zeros((self.batch, L, self.m)),
                   iterations=np.zeros((self.batch, max(cycles, 0)), dtype=np.int32),
                   status=np.zeros((self.batch, max(cycles, 0)), dtype=np.int32))
        return w, out, (_dp(out["X_cl"]), _dp(out["U_cl"]), self._ip(out["iterations"]), self._ip(out["status"]))

    def mpc_run(self, cycles, shift, w=None):
        """``cycles`` x (solve; mpc_advance(shift, w=w[c])) with the closed-loop log kept on the device.  Returns
        dict(X_cl [B][cycles*shift+1][n], U_cl [B][cycles*shift][m], iterations [B][cycles], status [B][cycles])."""
        w, out, logs = self._run_logs(cycles, shift, w)
        self._call("mpc_run", C.c_int(cycles), C.c_int(shift), _dp(w), *logs)
        return out

    def _track_bounds(self, u_lo, u_hi):
        u_lo, u_hi = _f64(u_lo), _f64(u_hi)
        for name, a in (("u_lo", u_lo), ("u_hi", u_hi)):
            if a is not None and a.shape != (self.m,):
                raise ValueError(f"{name} must have shape ({self.m},)")
        return u_lo, u_hi

    def mpc_track(self, steps, samples=1, dx0=None, w=None, u_lo=None, u_hi=None, log=True):
        """Simulate every (instance, sample) for ``steps`` knots under the plan's feedback policy u = Ubar + K (x - Xbar) on
        the device (altro_mpc_track): x_0 = x0 + ``dx0`` ([B][S][n]), x+ = f(x, u) + ``w`` ([B][S][steps][n]), controls
        clipped to ``u_lo`` / ``u_hi`` ([m], both or neither).  Changes nothing on the handle.  Returns
        dict(stats [B][S] of TRACK_STATS_DTYPE, and with ``log`` X_cl [B][S][steps+1][n], U_cl [B][S][steps][m])."""
        S, K = max(int(samples), 0), max(int(steps), 0)
        dx0, w = _f64(dx0), _f64(w)
        u_lo, u_hi = self._track_bounds(u_lo, u_hi)
        if dx0 is not None and dx0.shape != (self.batch, S, self.n):
            raise ValueError(f"dx0 must have shape ({self.batch}, {S}, {self.n})")
        if w is not None and w.shape != (self.batch, S, K, self.n):
            raise ValueError(f"w must have shape ({self.batch}, {S}, {K}, {self.n})")
        stats = np.zeros((self.batch, S), dtype=TRACK_STATS_DTYPE)
        X = np.zeros((self.batch, S, K + 1, self.n)) if log else None
        U = np.zeros((self.batch, S, K, self.m)) if log else None
        self._call("mpc_track", C.c_int(steps), C.c_int(samples), _dp(dx0), _dp(w), _dp(u_lo), _dp(u_hi), _dp(X), _dp(U),
                   stats.ctypes.data_as(C.POINTER(TrackStats)))
        return dict(stats=stats, X_cl=X, U_cl=U) if log else dict(stats=stats)

    def mpc_track_device(self, steps, samples=1, dx0_ptr=0, w_ptr=0, u_lo_ptr=0, u_hi_ptr=0, x_ptr=0, u_ptr=0, stats_ptr=0):
        """mpc_track with every array in memory of this handle's device (any pointer may be 0)."""
        self._call("mpc_track_device", C.c_int(steps), C.c_int(samples), *(C.c_void_p(p or None) for p in
                   (dx0_ptr, w_ptr, u_lo_ptr, u_hi_ptr, x_ptr, u_ptr, stats_ptr)))

    def mpc_run_tracked(self, cycles, shift, w=None, u_lo=None, u_hi=None):
        """``cycles`` x (solve; mpc_track(shift, 1, w=w[c]); mpc_advance(shift, x0=the tracked state)) with the log kept on
        the device; w [cycles][B][shift][n].  Returns dict(X_cl [B][cycles*shift+1][n], U_cl [B][cycles*shift][m] -- the
        TRACKED states and controls --, iterations [B][cycles], status [B][cycles], track [B][cycles] of TRACK_STATS_DTYPE)."""
        u_lo, u_hi = self._track_bounds(u_lo, u_hi)
        w, out, logs = self._run_logs(cycles, shift, w, per_knot=True)
        out["track"] = np.zeros((self.batch, max(cycles, 0)), dtype=TRACK_STATS_DTYPE)
        self._call("mpc_run_tracked", C.c_int(cycles), C.c_int(shift), _dp(w), _dp(u_lo), _dp(u_hi), *logs,
                   out["track"].ctypes.data_as(C.POINTER(TrackStats)))
        return out

    def get_initial_state(self):
        """What the next solve starts from, [B][n]."""
        out = np.empty((self.batch, self.n))
        self._call("get_initial_state", _dp(out))
        return out

    def set_penalties(self, rho):
        """Counterpart of set_duals for the penalties, [B][rows]."""
        rho = _f64(rho)
        self._call("set_penalties", _dp(rho))

    # -- multi-start (include/altro_multistart.h) ---------------------------------------------------
    # A handle of batch = P * starts instances holds P problems; start g of problem p is instance p * starts + g.
    def _problems(self, starts):
        starts = int(starts)
        return self.batch // starts if starts >= 1 and self.batch % starts == 0 else 0

    @staticmethod
    def _ip(a):
        return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))

    def multistart_select(self, starts):
        """The winning start of every problem, int32 [P], by the rule of include/altro_multistart.h over the status, cost
        and violation ``get_stats`` reports.  Changes nothing on the handle."""
        win = np.zeros(max(self._problems(starts), 1), dtype=np.int32)
        self._call("multistart_select", C.c_int(starts), self._ip(win))
        return win[:self._problems(starts)]

    def multistart_select_device(self, starts, winner_ptr):
        self._call("multistart_select_device", C.c_int(starts), C.c_void_p(winner_ptr or None))

    def multistart_spread(self, starts):
        """Select, then copy the winner's column (X, U, gains, duals, penalties, constraint values, knot costs) over the
        other starts of its problem, on the device.  Returns the winners, int32 [P]."""
        win = np.zeros(max(self._problems(starts), 1), dtype=np.int32)
        self._call("multistart_spread", C.c_int(starts), self._ip(win))
        return win[:self._problems(starts)]

    def multistart_spread_device(self, starts, winner_ptr=0):
        self._call("multistart_spread_device", C.c_int(starts), C.c_void_p(winner_ptr or None))

    def _perturbation(self, starts, dU):
        dU = _f64(dU)
        shapes = ((int(starts), self.N, self.m), (self.batch, self.N, self.m))
        if dU is not None and dU.shape not in shapes:
            raise ValueError(f"dU must have shape {shapes[0]} or {shapes[1]}")
        # (starts == batch: both shapes coincide, and so do the two layouts)
        return dU, 1 if dU is not None and dU.shape[0] == self.batch and int(starts) != self.batch else 0

    def multistart_perturb(self, starts, dU):
        """U += dU, a plain fp64 addition on the device; dU [starts][N][m] (one block per start, shared by all problems) or
        [B][N][m]."""
        dU, per_instance = self._perturbation(starts, dU)
        self._call("multistart_perturb", C.c_int(starts), _dp(dU), C.c_int(per_instance))

    def multistart_perturb_device(self, starts, du_ptr, per_instance):
        self._call("multistart_perturb_device", C.c_int(starts), C.c_void_p(du_ptr or None), C.c_int(1 if per_instance else 0))

    def multistart_get_best(self, starts):
        """The winners only: dict(X [P][N+1][n], U [P][N][m], stats [P] of STATS_DTYPE, winner [P])."""
        P = self._problems(starts)
        X = np.zeros((max(P, 1), self.N + 1, self.n))
        U = np.zeros((max(P, 1), self.N, self.m))
        stats = np.zeros(max(P, 1), dtype=STATS_DTYPE)
        win = np.zeros(max(P, 1), dtype=np.int32)
        self._call("multistart_get_best", C.c_int(starts), _dp(X), _dp(U), stats.ctypes.data_as(C.c_void_p), self._ip(win))
        return dict(X=X[:P], U=U[:P], stats=stats[:P], winner=win[:P])

    def multistart_get_best_device(self, starts, x_ptr=0, u_ptr=0, stats_ptr=0, winner_ptr=0):
        """multistart_get_best with every array in memory of this handle's device (any pointer may be 0, not all)."""
        self._call("multistart_get_best_device", C.c_int(starts), *(C.c_void_p(p or None) for p in (x_ptr, u_ptr, stats_ptr, winner_ptr)))

    def mpc_run_multistart(self, starts, cycles, shift, w=None, dU=None):
        """``cycles`` x (solve; multistart_spread; mpc_advance(shift, w=w[c]); multistart_perturb(dU) unless it is None) with
        nothing crossing to the host inside the loop.  Returns dict(X_cl, U_cl, iterations, status as mpc_run gives them,
        per instance, and winner [P][cycles])."""
        w, out, logs = self._run_logs(cycles, shift, w)
        dU, per_instance = self._perturbation(starts, dU)
        win = np.zeros((max(self._problems(starts), 1), max(cycles, 1)), dtype=np.int32)
        self._call("mpc_run_multistart", C.c_int(starts), C.c_int(cycles), C.c_int(shift), _dp(w), _dp(dU), C.c_int(per_instance),
                   *logs, self._ip(win))
        out["winner"] = win[:self._problems(starts), :max(cycles, 0)]
        return out

    # -- teams (include/altro_team.h) ---------------------------------------------------------------
    # A handle of batch = T * agents instances holds T teams; agent a of team t is instance t * agents + a.  ``index`` is the
    # team's knot circle constraint, add_knot_constraint(CON_CIRCLE, k_begin, k_end, 3 * (agents - 1)).
    def _teams(self, agents):
        agents = int(agents)
        return self.batch // agents if agents >= 2 and self.batch % agents == 0 else 0

    def _team_radius(self, agents, radius):
        radius = _f64(radius)
        if radius is None or radius.shape not in ((int(agents),), (self.batch,)):
            raise ValueError(f"radius must have shape ({int(agents)},) or ({self.batch},)")
        # (agents == batch: both shapes coincide, and so do the two layouts)
        return radius, 1 if radius.shape[0] == self.batch and int(agents) != self.batch else 0

    def team_fill_tracks(self, agents, index, radius, mode=TEAM_ALL, blend=1.0):
        """Fill the track of the team constraint from the plans on the device: circle slot i of agent a is peer
        j = i if i < a else i + 1 with centre X_j[r][0:2] and radius radius[a] + radius[j] (0 for j > a under
        TEAM_PRIORITY); ``blend`` < 1 moves the centres only that fraction of the way from what the window shows now."""
        radius, per = self._team_radius(agents, radius)
        self._call("team_fill_tracks", C.c_int(agents), C.c_int(index), _dp(radius), C.c_int(per), C.c_int(mode), C.c_double(blend))

    def team_clearance(self, agents, index, radius):
        """[T]: per team the minimum over the constraint's knots and all pairs a < j of |p_a - p_j|^2 - (r_a + r_j)^2."""
        radius, per = self._team_radius(agents, radius)
        out = np.zeros(max(self._teams(agents), 1))
        self._call("team_clearance", C.c_int(agents), C.c_int(index), _dp(radius), C.c_int(per), _dp(out))
        return out[:self._teams(agents)]

    def team_clearance_device(self, agents, index, radius, clear_ptr):
        """team_clearance into fp64 memory [T] of this handle's device."""
        radius, per = self._team_radius(agents, radius)
        self._call("team_clearance_device", C.c_int(agents), C.c_int(index), _dp(radius), C.c_int(per), C.c_void_p(clear_ptr or None))

    def team_solve(self, agents, index, radius, mode=TEAM_ALL, blend=1.0, rounds=1):
        """``rounds`` x (team_fill_tracks; solve)."""
        radius, per = self._team_radius(agents, radius)
        self._call("team_solve", C.c_int(agents), C.c_int(index), _dp(radius), C.c_int(per), C.c_int(mode), C.c_double(blend),
                   C.c_int(rounds))

    def mpc_run_team(self, agents, index, radius, mode=TEAM_ALL, blend=1.0, rounds=1, cycles=1, shift=1, w=None):
        """``cycles`` x (team_solve(rounds); team_clearance into a device log; mpc_advance(shift, w=w[c])) with nothing
        crossing to the host inside the loop.  Returns dict(X_cl, U_cl, iterations, status as mpc_run gives them, and
        clear [T][cycles])."""
        radius, per = self._team_radius(agents, radius)
        w, out, logs = self._run_logs(cycles, shift, w)
        clear = np.zeros((max(self._teams(agents), 1), max(cycles, 1)))
        self._call("mpc_run_team", C.c_int(agents), C.c_int(index), _dp(radius), C.c_int(per), C.c_int(mode), C.c_double(blend),
                   C.c_int(rounds), C.c_int(cycles), C.c_int(shift), _dp(w), *logs, _dp(clear))
        out["clear"] = clear[:self._teams(agents), :max(cycles, 0)]
        return out

    # -- the solve mask and sequential team rounds (include/altro_subset.h) -------------------------
    def set_solve_mask(self, mask):
        """The instances the whole solves that follow run: ``mask`` [batch], non-zero = takes part; None clears it.  A
        masked-out instance keeps everything it holds, bit for bit; the step-level calls ignore the mask."""
        if mask is None:
            self._call("set_solve_mask", C.c_void_p(None))
            return
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.shape != (self.batch,):
            raise ValueError(f"mask must have shape ({self.batch},)")
        self._call("set_solve_mask", mask.ctypes.data_as(C.c_void_p))

    def set_solve_mask_device(self, mask_ptr):
        """set_solve_mask from ``batch`` bytes in memory of this handle's device."""
        self._call("set_solve_mask_device", C.c_void_p(mask_ptr or None))

    def get_solve_mask(self):
        """The mask as a bool array [batch] (all True without a mask)."""
        mask = np.zeros(max(self.batch, 1), dtype=np.uint8)
        count = C.c_int(0)
        self._call("get_solve_mask", mask.ctypes.data_as(C.c_void_p), C.byref(count))
        out = mask[:self.batch] != 0
        assert int(out.sum()) == count.value
        return out

    def team_solve_sequential(self, agents, index, radius, sweeps=1):
        """``sweeps`` x (for a in range(agents): team_fill_tracks(TEAM_ALL, blend 1); mask = agent a of every team; solve);
        the mask the handle had before is back afterwards."""
        radius, per = self._team_radius(agents, radius)
        self._call("team_solve_sequential", C.c_int(agents), C.c_int(index), _dp(radius), C.c_int(per), C.c_int(sweeps))

    # -- event-triggered re-planning (include/altro_trigger.h) ---------------------------------------
    @staticmethod
    def _rule(rule):
        if isinstance(rule, TriggerRule):
            return rule
        return TriggerRule(**rule)

    def mpc_trigger(self, rule, tracked=None, age=None, u_lo=None, u_hi=None):
        """The trigger rule for every instance (altro_mpc_trigger): ``rule`` a TriggerRule or a dict of its fields, ``tracked``
        [B] of TRACK_STATS_DTYPE (the segment just tracked; None: the tracked criteria are off), ``age`` [B] (None: 0).
        Changes nothing on the handle.  Returns (mask [B] bool, reason [B] int32 of TRIGGER_* bits)."""
        rule = self._rule(rule)
        u_lo, u_hi = self._track_bounds(u_lo, u_hi)
        if tracked is not None:
            tracked = np.ascontiguousarray(tracked, dtype=TRACK_STATS_DTYPE)
            if tracked.shape != (self.batch,):
                raise ValueError(f"tracked must have shape ({self.batch},)")
        if age is not None:
            age = np.ascontiguousarray(age, dtype=np.int32)
            if age.shape != (self.batch,):
                raise ValueError(f"age must have shape ({self.batch},)")
        mask = np.zeros(max(self.batch, 1), dtype=np.uint8)
        reason = np.zeros(max(self.batch, 1), dtype=np.int32)
        self._call("mpc_trigger", C.byref(rule), None if tracked is None else tracked.ctypes.data_as(C.POINTER(TrackStats)),
                   None if age is None else self._ip(age), _dp(u_lo), _dp(u_hi), mask.ctypes.data_as(C.c_void_p), self._ip(reason))
        return mask[:self.batch] != 0, reason[:self.batch]

    def mpc_trigger_device(self, rule, tracked_ptr=0, age_ptr=0, u_lo_ptr=0, u_hi_ptr=0, mask_ptr=0, reason_ptr=0):
        """mpc_trigger with every array in memory of this handle's device (any pointer may be 0); ``mask_ptr`` can go straight
        into set_solve_mask_device."""
        self._call("mpc_trigger_device", C.byref(self._rule(rule)), *(C.c_void_p(p or None) for p in
                   (tracked_ptr, age_ptr, u_lo_ptr, u_hi_ptr, mask_ptr, reason_ptr)))

    def mpc_run_triggered(self, cycles, shift, rule, w=None, u_lo=None, u_hi=None):
        """mpc_run_tracked that re-plans only the instances the rule triggers (altro_mpc_run_triggered): cycle 0 solves
        everyone, every later cycle the instances whose plan is ``max_age`` cycles old, was left by the plant, ...; the others
        follow their shifted plan under its gains.  Returns the dict of mpc_run_tracked (iterations 0 where an instance was
        not solved) plus reason [B][cycles] of TRIGGER_* bits, 0 where it was not solved."""
        rule = self._rule(rule)
        u_lo, u_hi = self._track_bounds(u_lo, u_hi)
        w, out, logs = self._run_logs(cycles, shift, w, per_knot=True)
        out["track"] = np.zeros((self.batch, max(cycles, 0)), dtype=TRACK_STATS_DTYPE)
        out["reason"] = np.zeros((self.batch, max(cycles, 0)), dtype=np.int32)
        self._call("mpc_run_triggered", C.c_int(cycles), C.c_int(shift), _dp(w), _dp(u_lo), _dp(u_hi), C.byref(rule), *logs,
                   out["track"].ctypes.data_as(C.POINTER(TrackStats)), self._ip(out["reason"]))
        return out

    # -- closed-loop covariance (include/altro_covariance.h) -----------------------------------------
    def _cov_inputs(self, steps, Sigma0, W):
        n, B, K = self.n, self.batch, max(int(steps), 0)
        Sigma0, W = _f64(Sigma0), _f64(W)
        if Sigma0 is not None and Sigma0.shape not in ((n, n), (B, n, n)):
            raise ValueError(f"Sigma0 must have shape ({n}, {n}) or ({B}, {n}, {n})")
        w_mode = 0
        if W is not None:
            # (batch == steps: a 3-d W is read per instance; pass [B][steps][n][n] for the other meaning)
            shapes = {(n, n): 0, (B, n, n): COV_W_PER_INSTANCE, (K, n, n): COV_W_PER_KNOT,
                      (B, K, n, n): COV_W_PER_INSTANCE | COV_W_PER_KNOT}
            if W.shape not in shapes:
                raise ValueError(f"W must have shape ({n}, {n}), ({B}, {n}, {n}), ({K}, {n}, {n}) or ({B}, {K}, {n}, {n})")
            w_mode = COV_W_PER_INSTANCE if W.shape == (B, n, n) else shapes[W.shape]
        return Sigma0, 1 if Sigma0 is not None and Sigma0.ndim == 3 else 0, W, w_mode

    def cov_propagate(self, steps, Sigma0=None, W=None, want=("Sigma", "sx", "su", "rpos")):
        """The closed-loop covariance along the plan under the gains on the device (altro_cov_propagate):
        Sigma_{k+1} = F_k Sigma_k F_k^T + W_k, F_k = A_k + B_k K_k, from ``Sigma0`` ([n][n] or [B][n][n]; None: zero) and
        ``W`` ([n][n], [B][n][n], [steps][n][n] or [B][steps][n][n]; None: zero), of which only the lower triangles are
        read.  Changes nothing on the handle.  Returns a dict of the arrays named in ``want``: Sigma [B][steps+1][n][n],
        sx [B][steps+1][n], su [B][steps][m], rpos [B][steps+1]."""
        K = max(int(steps), 0)
        Sigma0, per, W, w_mode = self._cov_inputs(steps, Sigma0, W)
        shapes = dict(Sigma=(self.batch, K + 1, self.n, self.n), sx=(self.batch, K + 1, self.n), su=(self.batch, K, self.m),
                      rpos=(self.batch, K + 1))
        unknown = [k for k in want if k not in shapes]
        if unknown:
            raise ValueError(f"want names Sigma, sx, su, rpos; got {unknown}")
        out = {k: np.zeros(shapes[k]) for k in want}
        self._call("cov_propagate", C.c_int(steps), _dp(Sigma0), C.c_int(per), _dp(W), C.c_int(w_mode),
                   *(_dp(out.get(k)) for k in ("Sigma", "sx", "su", "rpos")))
        return out

    def cov_propagate_device(self, steps, Sigma0_ptr=0, sigma0_per_instance=False, W_ptr=0, w_mode=0, Sigma_ptr=0, sx_ptr=0,
                             su_ptr=0, rpos_ptr=0):
        """cov_propagate with every array in fp64 memory of this handle's device (any pointer may be 0, not all outputs)."""
        self._call("cov_propagate_device", C.c_int(steps), C.c_void_p(Sigma0_ptr or None), C.c_int(1 if sigma0_per_instance else 0),
                   C.c_void_p(W_ptr or None), C.c_int(w_mode), *(C.c_void_p(p or None) for p in (Sigma_ptr, sx_ptr, su_ptr, rpos_ptr)))

    def cov_inflate_circles(self, index, base, kappa, rpos):
        """Write the track of knot circle constraint ``index`` on the device, per instance: the centres of ``base``
        ([rows][3 nobs] or [B][rows][3 nobs]) and the radii rad + kappa * rpos[b][min(max(r - offset, 0), N)]; ``rpos``
        [B][N+1] as cov_propagate(N) returns it.  The window offset stays."""
        base, rpos = _f64(base), _f64(rpos)
        rows, per = self._track_shape(index, base)
        if rpos.shape != (self.batch, self.N + 1):
            raise ValueError(f"rpos must have shape ({self.batch}, {self.N + 1})")
        self._call("cov_inflate_circles", C.c_int(index), _dp(base), C.c_int(rows), C.c_int(per), C.c_double(kappa), _dp(rpos))

    def cov_inflate_circles_device(self, index, base_ptr, rows, per_instance, kappa, rpos_ptr):
        """cov_inflate_circles with ``base`` and ``rpos`` in fp64 memory of this handle's device."""
        self._call("cov_inflate_circles_device", C.c_int(index), C.c_void_p(base_ptr or None), C.c_int(rows),
                   C.c_int(1 if per_instance else 0), C.c_double(kappa), C.c_void_p(rpos_ptr or None))

    # -- time-varying LQR tracking gains (include/altro_lqr.h) ---------------------------------------
    def _lqr_weights(self, Q, R, Qf):
        Q, R, Qf = _f64(Q), _f64(R), _f64(Qf)
        if Q is None or R is None:
            raise ValueError("Q and R are required")
        if Q.shape != (self.n, self.n) or R.shape != (self.m, self.m) or (Qf is not None and Qf.shape != (self.n, self.n)):
            raise ValueError(f"Q and Qf must have shape ({self.n}, {self.n}), R ({self.m}, {self.m})")
        return Q, R, Qf

    def lqr_gains(self, Q, R, Qf=None, install=False, want=("K", "P", "fail")):
        """Time-varying LQR tracking gains about the plan on the device (altro_lqr_gains): P_N = Qf (None: Q),
        K_k = -(R + B^T P B)^-1 B^T P A, P_k = Q + A^T P A + (B^T P A)^T K_k with [A | B] the discrete Jacobian of knot k at
        the plan; only the lower triangles of the weights are read.  ``install``: the gains replace K of the handle's gain
        record (d = 0) for every instance that did not fail.  Returns a dict of the arrays named in ``want``: K [B][N][m][n]
        (as get_gains returns it), P [B][N+1][n][n], fail int32 [B] (-1, or the knot at which the instance failed: its K and
        P from there down are NaN)."""
        Q, R, Qf = self._lqr_weights(Q, R, Qf)
        B, N, n, m = self.batch, self.N, self.n, self.m
        unknown = [k for k in want if k not in ("K", "P", "fail")]
        if unknown:
            raise ValueError(f"want names K, P, fail; got {unknown}")
        K = np.zeros((B, N, n, m)) if "K" in want else None  # column-major m x n per knot
        Pm = np.zeros((B, N + 1, n, n)) if "P" in want else None
        fail = np.zeros(max(B, 1), dtype=np.int32) if "fail" in want else None
        self._call("lqr_gains", _dp(Q), _dp(R), _dp(Qf), C.c_int(1 if install else 0), _dp(K), _dp(Pm), self._ip(fail))
        out = {}
        if K is not None:
            out["K"] = np.swapaxes(K, 2, 3)
        if Pm is not None:
            out["P"] = Pm
        if fail is not None:
            out["fail"] = fail[:B]
        return out

    def lqr_gains_device(self, Q_ptr, R_ptr, Qf_ptr=0, install=False, K_ptr=0, P_ptr=0, fail_ptr=0):
        """lqr_gains with every array in memory of this handle's device (fp64; ``fail`` int32); K is [B][N][m n], column-major
        m x n per knot.  Any output pointer may be 0."""
        self._call("lqr_gains_device", C.c_void_p(Q_ptr or None), C.c_void_p(R_ptr or None), C.c_void_p(Qf_ptr or None),
                   C.c_int(1 if install else 0), C.c_void_p(K_ptr or None), C.c_void_p(P_ptr or None), C.c_void_p(fail_ptr or None))

    def set_lqr_policy(self, Q=None, R=None, Qf=None):
        """While the policy is on, every whole solve of this handle ends with lqr_gains(Q, R, Qf, install=True) for the
        instances it ran (altro_lqr_set_policy).  ``Q`` None: off."""
        if Q is None:
            self._call("lqr_set_policy", None, None, None)
            return
        Q, R, Qf = self._lqr_weights(Q, R, Qf)
        self._call("lqr_set_policy", _dp(Q), _dp(R), _dp(Qf))

    def get_lqr_policy(self):
        """None while the policy is off, else the dict Q, R, Qf of the symmetric matrices it holds."""
        on = C.c_int(0)
        Q, R, Qf = np.zeros((self.n, self.n)), np.zeros((self.m, self.m)), np.zeros((self.n, self.n))
        self._call("lqr_get_policy", C.byref(on), _dp(Q), _dp(R), _dp(Qf))
        return dict(Q=Q, R=R, Qf=Qf) if on.value else None

    # -- Monte-Carlo ensembles (include/altro_ensemble.h) --------------------------------------------
    ENSEMBLE_OUTPUTS = ("dev_mean", "dev_mom2", "alive", "viol_count", "summary", "stats")

    def mpc_ensemble(self, steps, samples, seed=0, instance_base=0, Sigma0=None, W=None, u_lo=None, u_hi=None, viol_tol=0.0,
                     want=("dev_mean", "dev_mom2", "alive", "viol_count", "summary")):
        """``samples`` closed-loop runs per instance under Gaussian initial errors (covariance ``Sigma0``) and process noise
        (covariance ``W``, shapes as cov_propagate) drawn on the device, reduced there (altro_mpc_ensemble).  Returns a dict
        of the arrays named in ``want``: dev_mean [B][steps+1][n] and dev_mom2 [B][steps+1][n][n] (moments of x_k - Xbar_k
        over the samples alive at k; ``ensemble_covariance`` gives the covariance), alive and viol_count int32
        [B][steps+1], summary [B] of ENSEMBLE_STATS_DTYPE, stats [B][samples] of TRACK_STATS_DTYPE.  Changes nothing on the
        handle."""
        K, S, B, n = max(int(steps), 0), max(int(samples), 0), self.batch, self.n
        Sigma0, per, W, w_mode = self._cov_inputs(steps, Sigma0, W)
        u_lo, u_hi = self._track_bounds(u_lo, u_hi)
        make = dict(dev_mean=lambda: np.zeros((B, K + 1, n)), dev_mom2=lambda: np.zeros((B, K + 1, n, n)),
                    alive=lambda: np.zeros((B, K + 1), dtype=np.int32), viol_count=lambda: np.zeros((B, K + 1), dtype=np.int32),
                    summary=lambda: np.zeros(B, dtype=ENSEMBLE_STATS_DTYPE), stats=lambda: np.zeros((B, S), dtype=TRACK_STATS_DTYPE))
        unknown = [k for k in want if k not in make]
        if unknown:
            raise ValueError(f"want names {', '.join(self.ENSEMBLE_OUTPUTS)}; got {unknown}")
        out = {k: make[k]() for k in want}
        ptr = lambda k, t: None if k not in out else out[k].ctypes.data_as(C.POINTER(t))  # noqa: E731
        self._call("mpc_ensemble", C.c_int(steps), C.c_int(samples), C.c_ulonglong(seed), C.c_ulonglong(instance_base), _dp(Sigma0),
                   C.c_int(per), _dp(W), C.c_int(w_mode), _dp(u_lo), _dp(u_hi), C.c_double(viol_tol), _dp(out.get("dev_mean")),
                   _dp(out.get("dev_mom2")), ptr("alive", C.c_int), ptr("viol_count", C.c_int), ptr("summary", EnsembleStats),
                   ptr("stats", TrackStats))
        return out

    def mpc_ensemble_device(self, steps, samples, seed=0, instance_base=0, Sigma0_ptr=0, sigma0_per_instance=False, W_ptr=0,
                            w_mode=0, u_lo_ptr=0, u_hi_ptr=0, viol_tol=0.0, dev_mean_ptr=0, dev_mom2_ptr=0, alive_ptr=0,
                            viol_count_ptr=0, summary_ptr=0, stats_ptr=0):
        """mpc_ensemble with every array in memory of this handle's device (any pointer may be 0, not all outputs)."""
        self._call("mpc_ensemble_device", C.c_int(steps), C.c_int(samples), C.c_ulonglong(seed), C.c_ulonglong(instance_base),
                   C.c_void_p(Sigma0_ptr or None), C.c_int(1 if sigma0_per_instance else 0), C.c_void_p(W_ptr or None),
                   C.c_int(w_mode), C.c_void_p(u_lo_ptr or None), C.c_void_p(u_hi_ptr or None), C.c_double(viol_tol),
                   *(C.c_void_p(p or None) for p in (dev_mean_ptr, dev_mom2_ptr, alive_ptr, viol_count_ptr, summary_ptr, stats_ptr)))

    def noise_fill(self, steps, samples, seed=0, instance_base=0, Sigma0=None, W=None):
        """The arrays mpc_track takes, from the draws mpc_ensemble makes (altro_noise_fill): dict(dx0 [B][S][n],
        w [B][S][steps][n]); zeros for a covariance that is None."""
        K, S = max(int(steps), 0), max(int(samples), 0)
        Sigma0, per, W, w_mode = self._cov_inputs(steps, Sigma0, W)
        dx0, w = np.zeros((self.batch, S, self.n)), np.zeros((self.batch, S, K, self.n))
        self._call("noise_fill", C.c_int(steps), C.c_int(samples), C.c_ulonglong(seed), C.c_ulonglong(instance_base), _dp(Sigma0),
                   C.c_int(per), _dp(W), C.c_int(w_mode), _dp(dx0), _dp(w))
        return dict(dx0=dx0, w=w)

    def noise_fill_device(self, steps, samples, seed=0, instance_base=0, Sigma0_ptr=0, sigma0_per_instance=False, W_ptr=0, w_mode=0,
                          dx0_ptr=0, w_ptr=0):
        """noise_fill with every array in fp64 memory of this handle's device (either output may be 0, not both)."""
        self._call("noise_fill_device", C.c_int(steps), C.c_int(samples), C.c_ulonglong(seed), C.c_ulonglong(instance_base),
                   C.c_void_p(Sigma0_ptr or None), C.c_int(1 if sigma0_per_instance else 0), C.c_void_p(W_ptr or None),
                   C.c_int(w_mode), C.c_void_p(dx0_ptr or None), C.c_void_p(w_ptr or None))

    def multistart_perturb_gaussian(self, starts, seed, sigma, instance_base=0, keep_first=True):
        """U[b][k][i] += sigma[i] z with z drawn on the device (altro_multistart_perturb_gaussian); with ``keep_first`` the
        first start of every problem stays bit for bit."""
        sigma = _f64(sigma)
        if sigma is not None and sigma.shape != (self.m,):
            raise ValueError(f"sigma must have shape ({self.m},)")
        self._call("multistart_perturb_gaussian", C.c_int(starts), C.c_ulonglong(seed), C.c_ulonglong(instance_base), _dp(sigma),
                   C.c_int(1 if keep_first else 0))

    # -- device interop ---------------------------------------------------------------------------
    def pack_results_device(self, device_ptr):
        self._call("pack_results_device", C.c_void_p(device_ptr))

    def pack_trajectory_device(self, x_ptr, u_ptr):
        """X[B][N+1][n], U[B][N][m] doubles into device memory of this handle's device (either pointer may be 0)."""
        self._call("pack_trajectory_device", C.c_void_p(x_ptr or None), C.c_void_p(u_ptr or None))

    def device_info(self):
        name = C.create_string_buffer(256)
        cu = C.c_int()
        self._call("device_info", name, C.c_int(256), C.byref(cu))
        return name.value.decode(), cu.value
