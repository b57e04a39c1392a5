"""Monte-Carlo ensembles on the device (include/altro_ensemble.h): the filled noise against numpy, the ensemble against
altro_mpc_track on the filled arrays bit for bit, the per-knot moments and counts against numpy over the tracked paths, the
invariances (repeat, NULL outputs, seed, handle untouched, sharding by instance_base), the sample second moment against
altro_cov_propagate, and the Gaussian multi-start perturbation.  N = 12, B <= 4, S <= 330 unless stated."""
import ctypes

import numpy as np
import pytest

import _cov_common as CC
import _ensemble_common as EC

N = 12


def _hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the solver library has not loaded a HIP runtime")


class Dev:
    """device memory holding the bytes of a numpy array (hipMalloc / hipMemcpy through ctypes)"""

    def __init__(self, data):
        self.like = np.ascontiguousarray(data)
        self.hip = _hip_runtime()
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(self.like.nbytes, 1))) == 0
        self.ptr = p.value
        assert self.hip.hipMemcpy(ctypes.c_void_p(self.ptr), self.like.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(self.like.nbytes),
                                  ctypes.c_int(1)) == 0  # host to device

    def get(self):
        out = np.empty_like(self.like)
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr), ctypes.c_size_t(out.nbytes),
                                  ctypes.c_int(2)) == 0  # device to host
        return out

    def free(self):
        self.hip.hipFree(ctypes.c_void_p(self.ptr))


def _ptr(d):
    return 0 if d is None else d.ptr


def _mode_of(s, steps, Sigma0, W):
    _, per, _, w_mode = s._cov_inputs(steps, Sigma0, W)
    return per, w_mode


ALL = ("dev_mean", "dev_mom2", "alive", "viol_count", "summary", "stats")


def ensemble_device(A, s, steps, S, seed, base=0, Sigma0=None, W=None, lo=None, hi=None, tol=0.0, want=ALL):
    """altro_mpc_ensemble_device with every array in device memory -> dict of numpy arrays"""
    B, n = s.batch, s.n
    per, w_mode = _mode_of(s, steps, Sigma0, W)
    shapes = dict(dev_mean=np.full((B, steps + 1, n), 7.0), dev_mom2=np.full((B, steps + 1, n, n), 7.0),
                  alive=np.full((B, steps + 1), -1, dtype=np.int32), viol_count=np.full((B, steps + 1), -1, dtype=np.int32),
                  summary=np.zeros(B, dtype=A.ENSEMBLE_STATS_DTYPE), stats=np.zeros((B, S), dtype=A.TRACK_STATS_DTYPE))
    ins = {k: (None if v is None else Dev(np.asarray(v, dtype=np.float64))) for k, v in dict(Sigma0=Sigma0, W=W, lo=lo, hi=hi).items()}
    outs = {k: Dev(shapes[k]) for k in want}
    try:
        s.mpc_ensemble_device(steps, S, seed, base, _ptr(ins["Sigma0"]), per, _ptr(ins["W"]), w_mode, _ptr(ins["lo"]), _ptr(ins["hi"]), tol,
                              *(_ptr(outs.get(k)) for k in ALL))
        return {k: d.get() for k, d in outs.items()}
    finally:
        for d in list(ins.values()) + list(outs.values()):
            if d is not None:
                d.free()


def fill_device(s, steps, S, seed, base=0, Sigma0=None, W=None):
    """altro_noise_fill_device -> (dx0, w) as Dev (the caller frees)"""
    per, w_mode = _mode_of(s, steps, Sigma0, W)
    ins = [None if v is None else Dev(np.asarray(v, dtype=np.float64)) for v in (Sigma0, W)]
    dx0, w = Dev(np.full((s.batch, S, s.n), 7.0)), Dev(np.full((s.batch, S, steps, s.n), 7.0))
    try:
        s.noise_fill_device(steps, S, seed, base, _ptr(ins[0]), per, _ptr(ins[1]), w_mode, dx0.ptr, w.ptr)
    finally:
        for d in ins:
            if d is not None:
                d.free()
    return dx0, w


def track_device(A, s, steps, S, dx0, w, lo=None, hi=None):
    """altro_mpc_track_device on device arrays -> dict(X_cl, U_cl, stats)"""
    B = s.batch
    X, U = Dev(np.zeros((B, S, steps + 1, s.n))), Dev(np.zeros((B, S, steps, s.m)))
    st = Dev(np.zeros((B, S), dtype=A.TRACK_STATS_DTYPE))
    bounds = [None if v is None else Dev(np.asarray(v, dtype=np.float64)) for v in (lo, hi)]
    try:
        s.mpc_track_device(steps, S, dx0.ptr, w.ptr, _ptr(bounds[0]), _ptr(bounds[1]), X.ptr, U.ptr, st.ptr)
        return dict(X_cl=X.get(), U_cl=U.get(), stats=st.get())
    finally:
        for d in [X, U, st] + bounds:
            if d is not None:
                d.free()


def tracked_paths(A, s, steps, S, seed, base=0, Sigma0=None, W=None, lo=None, hi=None):
    dx0, w = fill_device(s, steps, S, seed, base, Sigma0, W)
    try:
        return track_device(A, s, steps, S, dx0, w, lo, hi)
    finally:
        dx0.free()
        w.free()


def _psd(rng, shape, n, scale):
    G = rng.randn(*shape, n, n)
    return scale * (G @ np.swapaxes(G, -1, -2))


def _build(A, P, make, case, B=None):
    """-> a solved handle"""
    if case in ("unicycle_f64", "clip"):
        s = P.unicycle_turn90(make, batch=B or 3, N=N)
        s.solve()
    elif case == "triple_integrator":
        s = P.triple_integrator(make, batch=B or 2, N=N)
        s.solve_ilqr()
    elif case == "quadrotor12_f32":
        s = P.quadrotor12(make, batch=B or 2, N=N, dtype=A.F32)
        s.solve()
    elif case == "moving_obstacles":
        s = P.moving_obstacles(make, batch=B or 3, N=N)
        s.solve()
    else:
        raise KeyError(case)
    return s


# ---- 6. the filled noise against numpy -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_noise_fill_against_numpy(A, P, hip_make):
    """All four w_modes, a shared and a per-instance Sigma0, the identity (1e-12 absolute), a nonzero instance_base; 1e-12 max |L|
    otherwise.  A singular W leaves exact zeros on its noiseless state; an indefinite one is refused with its place in the text."""
    B, S, n = 3, 70, 3
    s = P.unicycle_turn90(hip_make, batch=B, N=N)  # (no solve: the fill needs no gains)
    rng = np.random.RandomState(11)
    cases = [(np.eye(n), np.eye(n), 0), (_psd(rng, (), n, 1e-2), _psd(rng, (), n, 1e-4), 5),
             (_psd(rng, (B,), n, 1e-2), _psd(rng, (B,), n, 1e-4), 0), (None, _psd(rng, (N,), n, 1e-4), 2 ** 32 - 2),
             (_psd(rng, (B,), n, 1.0), _psd(rng, (B, N), n, 1e-4), 1), (_psd(rng, (), n, 1e-2), None, 0)]
    modes = set()
    for Sigma0, W, base in cases:
        modes.add(_mode_of(s, N, Sigma0, W)[1])
        dx0, w = fill_device(s, N, S, 1234567890123, base, Sigma0, W)
        got0, gotw = dx0.get(), w.get()
        dx0.free(), w.free()
        want0, wantw, top = EC.noise_arrays(B, S, N, n, 1234567890123, base, Sigma0, W, _mode_of(s, N, Sigma0, W)[1])
        tol = 1e-12 * top
        assert np.abs(got0 - want0).max() <= tol and np.abs(gotw - wantw).max() <= tol, (base, np.abs(got0 - want0).max(), np.abs(gotw - wantw).max())
        if Sigma0 is None:
            assert not got0.any()
        if W is None:
            assert not gotw.any()
    assert modes == {0, 1, 2, 3}
    # the host form gives the device form's bytes
    host = s.noise_fill(N, S, seed=99, instance_base=3, Sigma0=cases[2][0], W=cases[4][1])
    dx0, w = fill_device(s, N, S, 99, 3, cases[2][0], cases[4][1])
    assert host["dx0"].tobytes() == dx0.get().tobytes() and host["w"].tobytes() == w.get().tobytes()
    dx0.free(), w.free()
    # singular: the second state carries no noise, the third is correlated with the first
    Wz = np.array([[4e-4, 0, 0], [0, 0, 0], [1e-4, 0, 1e-4]])
    out = s.noise_fill(N, S, seed=5, W=Wz)
    assert (out["w"][..., 1] == 0).all() and out["w"][..., 0].any() and out["w"][..., 2].any()
    want = EC.noise_arrays(B, S, N, n, 5, 0, None, Wz, 0)
    assert np.abs(out["w"] - want[1]).max() <= 1e-12 * want[2]
    # indefinite: refused, naming instance and knot
    Wbad = _psd(rng, (B, N), n, 1e-4)
    Wbad[1, 5] = np.array([[1.0, 0, 0], [2.0, 1.0, 0], [0, 0, 1.0]])
    with pytest.raises(A.AltroError) as e:
        s.noise_fill(N, S, seed=5, W=Wbad)
    assert f"({A.INVALID_ARG})" in str(e.value) and "positive semidefinite" in str(e.value)
    assert "instance 1" in str(e.value) and "knot 5" in str(e.value)
    with pytest.raises(A.AltroError) as e:
        s.noise_fill(N, S, seed=5, Sigma0=-np.eye(n))
    assert "Sigma0 is not positive semidefinite" in str(e.value)
    s.close()


# ---- 7. bit for bit against the track on the filled arrays -----------------------------------------------------------------------
BITS = [("unicycle_f64", 3, 70), ("triple_integrator", 2, 70), ("quadrotor12_f32", 2, 70), ("moving_obstacles", 3, 70), ("clip", 3, 70)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,B,S", BITS)
def test_ensemble_is_the_track_on_the_filled_arrays(A, P, hip_make, case, B, S):
    """S = 70: one full chunk of 64 samples and a part.  The per-sample statistics of the ensemble are, byte for byte, those of
    altro_mpc_track_device fed with what altro_noise_fill_device wrote for the same seed."""
    s = _build(A, P, hip_make, case, B)
    n = s.n
    rng = np.random.RandomState(3)
    big = case == "clip"
    Sigma0, W = _psd(rng, (B,), n, 1e-2 if big else 1e-4 / n), _psd(rng, (B, N), n, 1e-3 if big else 1e-6 / n)
    lo, hi = (np.array([-0.6, -0.6]), np.array([0.6, 0.6])) if big else (None, None)
    seed, base = 20261020, 7
    trk = tracked_paths(A, s, N, S, seed, base, Sigma0, W, lo, hi)
    ens = ensemble_device(A, s, N, S, seed, base, Sigma0, W, lo, hi, tol=1e-3)
    assert np.isfinite(trk["stats"]["cost"]).all() and (trk["stats"]["max_dx"] > 0).all()
    if big:
        assert ((trk["U_cl"] == lo) | (trk["U_cl"] == hi)).any(), "the clip never engaged"
    assert ens["stats"].tobytes() == trk["stats"].tobytes(), case
    # steps < N: the terminal knot is not evaluated, the same bytes again
    trk7 = tracked_paths(A, s, 7, S, seed, base, Sigma0, W[:, :7], lo, hi)
    ens7 = ensemble_device(A, s, 7, S, seed, base, Sigma0, W[:, :7], lo, hi, tol=1e-3)
    assert ens7["stats"].tobytes() == trk7["stats"].tobytes() and (ens7["viol_count"][:, 7] == 0).all()
    s.close()


# ---- 8. moments and counts against numpy over the tracked paths ------------------------------------------------------------------
def _rel(got, want, axes):
    err, scale = np.abs(got - want).max(axis=axes), np.abs(want).max(axis=axes)
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), err)


def _check_moments(A, s, ens, trk, S, tol, knot_violation=None):
    """every output of the ensemble against numpy over the paths of the track (X_cl, stats)"""
    st = trk["stats"]
    Xbar = s.get_trajectory()[0]
    steps = trk["X_cl"].shape[2] - 1
    alive, mean, mom2 = EC.moments(trk["X_cl"], Xbar, st["steps_done"])
    assert np.array_equal(ens["alive"], alive)
    some = alive > 0
    assert np.isnan(ens["dev_mean"][~some]).all() and np.isnan(ens["dev_mom2"][~some]).all()
    assert _rel(ens["dev_mean"][some], mean[some], -1).max() <= 1e-12
    assert CC.matrix_rel(ens["dev_mom2"][some], mom2[some]).max() <= 1e-12
    assert ens["dev_mom2"].tobytes() == np.swapaxes(ens["dev_mom2"], 2, 3).copy().tobytes()  # symmetric bit for bit
    # the summary: the four counts exactly, the rest to rounding
    sm = ens["summary"]
    assert (np.abs(st["violation"] - tol) > 1e-9).all(), "a sample lies within 1e-9 of viol_tol: choose another"
    done = st["status"] == A.UNSOLVED
    assert (sm["samples"] == S).all()
    assert np.array_equal(sm["stopped_state"], (st["status"] == A.STATE_LIMIT).sum(axis=1))
    assert np.array_equal(sm["stopped_control"], (st["status"] == A.CONTROL_LIMIT).sum(axis=1))
    assert np.array_equal(sm["violated"], (st["violation"] > tol).sum(axis=1))
    for b in range(s.batch):
        if done[b].any():
            assert abs(sm["cost_mean"][b] - st["cost"][b][done[b]].mean()) <= 1e-12 * np.abs(st["cost"][b][done[b]]).max()
            assert sm["cost_max"][b] == st["cost"][b][done[b]].max()
        else:
            assert np.isnan(sm["cost_mean"][b]) and np.isnan(sm["cost_max"][b])
    for name, field in (("violation_max", "violation"), ("max_dx", "max_dx"), ("max_du", "max_du")):
        assert np.array_equal(sm[name], st[field].max(axis=1)), name
    if knot_violation is not None:
        v = knot_violation  # [B][S][steps + 1], numpy's own
        live = np.arange(steps + 1)[None, None, :] <= st["steps_done"][:, :, None]
        assert (np.abs(v[live] - tol) > 1e-9).all(), "a knot violation lies within 1e-9 of viol_tol: choose another"
        assert np.array_equal(ens["viol_count"], (live & (v > tol)).sum(axis=1))
    return alive


BOUND, CIRCLE, GOAL = 1.2, np.array([0.8, 0.35, 0.25]), np.array([1.5, 1.5, np.pi / 2])


def _bound_circle_problem(P, make, B):
    """unicycle_turn90 with a control bound of +-BOUND on [0, N), one circle on [1, N] and the goal constraint at N"""
    s = P.unicycle_turn90(make, batch=B, N=N, constraints=False)
    s.add_control_bound(0, N, [-BOUND, -BOUND], [BOUND, BOUND])
    s.add_circle_constraint(1, N + 1, CIRCLE[None, :])
    s.add_goal_constraint(N, GOAL)
    s.solve()
    return s


def _bound_circle_violation(trk, steps):
    """the violation at every knot, stated in numpy: max over the rows of max(c, 0), and of |x - xf| for the goal at N"""
    X, U = trk["X_cl"], trk["U_cl"]
    v = np.zeros(X.shape[:3])
    vb = np.maximum(np.maximum(U - BOUND, -BOUND - U), 0.0).max(axis=-1)
    v[:, :, :steps] = vb
    vc = np.maximum(CIRCLE[2] ** 2 - (X[..., 0] - CIRCLE[0]) ** 2 - (X[..., 1] - CIRCLE[1]) ** 2, 0.0)
    vc[:, :, 0] = 0.0
    v[:, :, steps] = np.abs(X[:, :, steps] - GOAL).max(axis=-1)
    return np.where(np.isnan(v) | np.isnan(vc), 0.0, np.maximum(v, vc))


@pytest.mark.gpu
@pytest.mark.parametrize("B,S", [(3, 70), (2, 323)])
def test_moments_and_counts_against_numpy(A, P, hip_make, B, S):
    """(2, 323): six slabs of one chunk each per instance, the last one partly filled.  The violation at a knot is the control
    bound's, the circle's and (at N) the goal's, stated in numpy; the plan touches the circle, so a good part of the samples violates."""
    s = _bound_circle_problem(P, hip_make, B)
    assert EC.slabs(B, S)[0] == (2 if S == 70 else 6)
    Sigma0, W = np.diag([4e-4, 4e-4, 1e-4]), np.diag([1e-5, 1e-5, 1e-5])
    tol = 1e-3
    trk = tracked_paths(A, s, N, S, 42, 0, Sigma0, W)
    ens = ensemble_device(A, s, N, S, 42, 0, Sigma0, W, tol=tol)
    assert ens["stats"].tobytes() == trk["stats"].tobytes()
    v = _bound_circle_violation(trk, N)
    assert np.abs(v.max(axis=2) - trk["stats"]["violation"]).max() <= 1e-12  # (numpy's statement is the device's violation)
    alive = _check_moments(A, s, ens, trk, S, tol, v)
    assert (alive == S).all()
    count = ens["viol_count"]
    assert (count > 0).any() and (count < S).any() and count[:, N].any(), count
    # the host form gives the device form's bytes
    host = s.mpc_ensemble(N, S, seed=42, Sigma0=Sigma0, W=W, viol_tol=tol, want=ALL)
    for k in ALL:
        assert host[k].tobytes() == ens[k].tobytes(), k
    cov = A.ensemble_covariance(ens["dev_mean"], ens["dev_mom2"])
    assert np.abs(cov - (ens["dev_mom2"] - np.einsum("bki,bkj->bkij", ens["dev_mean"], ens["dev_mean"]))).max() == 0
    s.close()


@pytest.mark.gpu
def test_state_limit_stops_some_samples(A, P, hip_make):
    """state_max = the norm of the plan's last state: about half of the samples cross it near the end and stop.  `alive` falls,
    the moments are those of the survivors, the costs those of the samples that ran to the end."""
    B, S = 2, 200
    s = _build(A, P, hip_make, "unicycle_f64", B)
    Xbar = s.get_trajectory()[0]
    s.set_options(check_forwardpass_bounds=1, state_max=float(np.linalg.norm(Xbar[0, N])))
    Sigma0, W = np.diag([1e-2, 1e-2, 1e-3]), np.diag([1e-4, 1e-4, 1e-5])
    trk = tracked_paths(A, s, N, S, 9, 0, Sigma0, W)
    ens = ensemble_device(A, s, N, S, 9, 0, Sigma0, W, tol=5e-2)
    assert ens["stats"].tobytes() == trk["stats"].tobytes()
    alive = _check_moments(A, s, ens, trk, S, 5e-2)
    assert (alive[:, 0] == S).all() and (alive[:, N] < S).all() and (alive[:, N] > 0).all(), alive
    assert (np.diff(alive, axis=1) <= 0).all() and (ens["summary"]["stopped_state"] == S - alive[:, N]).all()
    # a limit nobody survives: quiet NaN from the knot on where nobody is alive
    s.set_options(state_max=1e-3)
    ens = ensemble_device(A, s, N, S, 9, 0, Sigma0, W, tol=5e-2)
    trk = tracked_paths(A, s, N, S, 9, 0, Sigma0, W)
    alive = _check_moments(A, s, ens, trk, S, 5e-2)
    assert (alive[:, 1:] == 0).all() and (ens["summary"]["stopped_state"] == S).all()
    s.close()


# ---- 9. invariance ----------------------------------------------------------------------------------------------------------------
def _handle_state(s):
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    st = s.get_stats()
    return [X, U, K, d, s.get_duals(), s.get_penalties(), s.get_constraint_values(), st]


@pytest.mark.gpu
def test_invariance(A, P, hip_make):
    B, S = 4, 130
    s = P.unicycle_turn90(hip_make, batch=B, N=N)
    x0 = np.stack([[0.02 * b, -0.03 * b, 0.01 * b] for b in range(B)])
    s.set_initial_state(x0)
    s.solve()
    before = _handle_state(s)
    Sigma0, W = np.diag([4e-4, 4e-4, 1e-4]), np.diag([1e-5, 1e-5, 1e-6])
    lo, hi = np.array([-1.5, -1.5]), np.array([1.5, 1.5])
    one = ensemble_device(A, s, N, S, 77, 0, Sigma0, W, lo, hi, tol=1e-3)
    two = ensemble_device(A, s, N, S, 77, 0, Sigma0, W, lo, hi, tol=1e-3)
    for k in ALL:
        assert one[k].tobytes() == two[k].tobytes(), k
    # an output left NULL changes nothing of the others
    for leave in ALL:
        part = ensemble_device(A, s, N, S, 77, 0, Sigma0, W, lo, hi, tol=1e-3, want=tuple(k for k in ALL if k != leave))
        for k in part:
            assert part[k].tobytes() == one[k].tobytes(), (leave, k)
    only = ensemble_device(A, s, N, S, 77, 0, Sigma0, W, lo, hi, tol=1e-3, want=("dev_mom2",))
    assert only["dev_mom2"].tobytes() == one["dev_mom2"].tobytes()
    # another seed, other draws
    other = ensemble_device(A, s, N, S, 78, 0, Sigma0, W, lo, hi, tol=1e-3)
    assert (other["stats"]["max_dx"] != one["stats"]["max_dx"]).all()
    # the handle is unchanged bit for bit
    for a, b in zip(before, _handle_state(s)):
        assert a.tobytes() == b.tobytes()
    # sharding: instances 2..3 with base 0 are a two-instance handle of the same problems with base 2
    t = P.unicycle_turn90(hip_make, batch=2, N=N)
    t.set_initial_state(x0[2:])
    t.solve()
    assert t.get_trajectory()[0].tobytes() == before[0][2:].tobytes(), "the two-instance handle did not reproduce the plans"
    shard = ensemble_device(A, t, N, S, 77, 2, Sigma0, W, lo, hi, tol=1e-3)
    assert shard["stats"].tobytes() == one["stats"][2:].tobytes()
    for k in ("dev_mean", "dev_mom2", "alive", "viol_count", "summary"):
        assert shard[k].tobytes() == one[k][2:].tobytes(), k
    s.close()
    t.close()


# ---- 10. the purpose: the sample second moment against the propagated covariance --------------------------------------------------
@pytest.mark.gpu
def test_sample_moment_matches_the_propagated_covariance(A, P, hip_make):
    """The triple integrator (linear: Sigma_k is exact), no clip, no limits, B = 2, S = 4096 (16 slabs of four chunks), seed
    20261020: max |M_k - Sigma_k| <= 5 sqrt(2 / S) max diag Sigma_k at every knot -- five standard deviations of a Gaussian
    sample moment.  tests/test_ensemble_abi.py checks that the numpy statement alone stays inside the bar for this seed."""
    B, S = EC.PURPOSE_B, EC.PURPOSE_S
    assert EC.slabs(B, S) == (16, 4)
    s = P.triple_integrator(hip_make, batch=B, N=N)
    s.solve_ilqr()
    Sigma = s.cov_propagate(N, Sigma0=EC.PURPOSE_SIGMA0, W=EC.PURPOSE_W, want=("Sigma",))["Sigma"]
    ens = s.mpc_ensemble(N, S, seed=EC.PURPOSE_SEED, Sigma0=EC.PURPOSE_SIGMA0, W=EC.PURPOSE_W)
    assert (ens["alive"] == S).all()
    for k in range(N + 1):
        bar = 5.0 * np.sqrt(2.0 / S) * np.diagonal(Sigma[:, k], axis1=1, axis2=2).max(axis=1)
        err = np.abs(ens["dev_mom2"][:, k] - Sigma[:, k]).max(axis=(1, 2))
        print(f"knot {k}: max |M - Sigma| = {err}, bar = {bar}")
        assert (err <= bar).all(), (k, err, bar)
    # the chunk loop (four chunks per slab) against numpy over the tracked paths
    trk = tracked_paths(A, s, N, S, EC.PURPOSE_SEED, 0, EC.PURPOSE_SIGMA0, EC.PURPOSE_W)
    full = ensemble_device(A, s, N, S, EC.PURPOSE_SEED, 0, EC.PURPOSE_SIGMA0, EC.PURPOSE_W, tol=1.0)
    assert full["stats"].tobytes() == trk["stats"].tobytes() and full["dev_mom2"].tobytes() == ens["dev_mom2"].tobytes()
    assert not trk["stats"]["violation"].any()  # (no constraints: any viol_tol away from zero is far from every sample)
    _check_moments(A, s, full, trk, S, 1.0)
    s.close()


# ---- 11. the Gaussian multi-start perturbation ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["unicycle_f64", "quadrotor12_f32"])
def test_multistart_perturb_gaussian(A, P, hip_make, case):
    B, G = 4, 2
    s = _build(A, P, hip_make, case, B)
    m = s.m
    sigma = 0.05 * (1.0 + np.arange(m))
    X0, U0 = s.get_trajectory()
    rest = [s.get_gains()[0], s.get_duals(), s.get_penalties()]
    z = np.stack([EC.normals(31337, np.arange(N), 0, 5 + b, EC.STREAM_CONTROLS, m) for b in range(B)])  # [B][N][m]
    s.multistart_perturb_gaussian(G, 31337, sigma, instance_base=5, keep_first=True)
    X1, U1 = s.get_trajectory()
    assert U1[0::G].tobytes() == U0[0::G].tobytes()
    assert np.abs((U1 - U0)[1::G] - (sigma * z)[1::G]).max() <= 1e-12
    assert X1.tobytes() == X0.tobytes()
    for a, b in zip(rest, [s.get_gains()[0], s.get_duals(), s.get_penalties()]):
        assert a.tobytes() == b.tobytes()
    s.multistart_perturb_gaussian(G, 31337, sigma, instance_base=5, keep_first=False)
    U2 = s.get_trajectory()[1]
    assert np.abs((U2 - U1) - sigma * z).max() <= 1e-12 and (U2[0::G] != U1[0::G]).any()
    s.close()
