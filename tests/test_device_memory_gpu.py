"""The engine's device memory as its callers see it: one grow-only stage shared by the host-array calls, call-scoped blocks beside
it, and an upload that can be refused and tried again (altro-cpp_amd/csrc/altro_devmem.hpp, Engine::Uploaded, Engine::DropUpload).

* One handle makes the host-array calls in an order that takes the shared stage from small to large and back, with the calls
  that bring a block of their own (mpc_track, cov_propagate; some outputs left out) in between.  Every result equals, bit for
  bit, the same call on a FRESH handle brought to the same state, whose stage that call is the first to size: a stage that
  shrank, a stale capacity or parts that overlap would show.
* An upload that is refused (altro_set_knot_models with a model index on a single-model handle) leaves the handle usable,
  however often it is refused: the corrected call solves to the bits of a handle that never was refused, and the error text is
  the one the library always gave.

Host and device entry points are already compared bit for bit where they were introduced -- altro_mpc_track / _device in
test_mpc_track_gpu.py (test_device_pointers_and_the_asynchronous_guard), altro_cov_propagate / _device and
altro_cov_inflate_circles / _device in test_cov_gpu.py (test_exact_properties, test_fewer_steps_than_knots, test_inflation),
altro_multistart_get_best / _device in test_multistart_gpu.py (test_get_best_is_the_winner_rows) -- so nothing is added for them.

kTurn90, batch 16.
"""
import numpy as np
import pytest

import _mpc_common as M
import test_mpc_track_gpu as TT  # w_of, dx0_of

pytestmark = pytest.mark.gpu

B, STARTS, SHIFT, STEPS = 16, 4, 2, 5
REFUSAL = ("altro_set_knot_models: knot 0 asks for model 1, this handle's model is a single model (a user source with "
           "#define ALTRO_USER_MODELS A, B, ... holds several)")


def _arrays(r):
    """whatever a call returns as a flat list of arrays"""
    if isinstance(r, dict):
        return [np.ascontiguousarray(r[k]) for k in sorted(r)]
    if isinstance(r, (tuple, list)):
        return [np.ascontiguousarray(v) for v in r]
    return [np.ascontiguousarray(r)]


def _same(a, b, what):
    a, b = _arrays(a), _arrays(b)
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i)


def test_shared_stage_grows_and_is_reused(A, P, hip_make):
    n, m = 3, 2
    W = M.disturbance(1, B, n)[0]
    dU = lambda N: 1e-3 * np.sin(1.0 + np.arange(STARTS * N * m)).reshape(STARTS, N, m)  # noqa: E731
    w_short, w_long = TT.w_of(B, 1, STEPS, n), TT.w_of(B, 2, STEPS, n)
    dx0 = TT.dx0_of(B, 2, n)
    lo, hi = np.array([-1.5, -np.inf]), np.array([np.inf, 1.5])
    Sigma0 = np.tile(1e-4 * np.eye(n), (B, 1, 1))
    Wn = 1e-6 * (1.0 + np.arange(B))[:, None, None] * np.eye(n)
    x_new = np.tile(np.array([0.01, -0.02, 0.03]), (B, 1)) * (1.0 + np.arange(B))[:, None]

    # (name, the call, does it change the handle); sizes of the shared stage in doubles: 48, 4848, 4 x 503 + statistics, 96,
    # 800, 9600 (K) and 3200 (d), 48 -- the tracking and covariance calls stage in blocks of their own
    calls = [
        ("get_initial_state", lambda s: s.get_initial_state(), False),
        ("mpc_track, statistics only", lambda s: s.mpc_track(STEPS, 1, w=w_short, log=False), False),
        ("get_trajectory", lambda s: s.get_trajectory(), False),
        ("cov_propagate, sx and rpos only", lambda s: s.cov_propagate(STEPS, want=("sx", "rpos")), False),
        ("multistart_get_best", lambda s: s.multistart_get_best(STARTS), False),
        ("mpc_advance", lambda s: s.mpc_advance(SHIFT, x0=x_new, w=W), True),
        ("mpc_track, everything", lambda s: s.mpc_track(STEPS, 2, dx0=dx0, w=w_long, u_lo=lo, u_hi=hi), False),
        ("multistart_perturb", lambda s: s.multistart_perturb(STARTS, dU(s.N)), True),
        ("get_gains", lambda s: s.get_gains(), False),
        ("cov_propagate, everything", lambda s: s.cov_propagate(STEPS, Sigma0, Wn), False),
        ("get_initial_state again", lambda s: s.get_initial_state(), False),
    ]
    one = P.batch_turn90(hip_make, B)
    one.solve()
    got = [call(one) for _, call, _ in calls]
    fresh = None
    for i, (name, call, changes) in enumerate(calls):
        fresh = P.batch_turn90(hip_make, B)
        fresh.solve()
        for _, earlier, changed in calls[:i]:
            if changed:
                earlier(fresh)
        want = call(fresh)
        if changes:  # (a call that returns nothing is judged by the trajectory it leaves, and by what the later calls read)
            assert got[i] is None and want is None
            if i < len(calls) - 1:
                fresh.close()
            continue
        _same(got[i], want, name)
        if i < len(calls) - 1:
            fresh.close()
    # the last fresh handle has made every call that changes a handle, and nothing else but one read
    _same(one.get_trajectory(), fresh.get_trajectory(), "the trajectory behind every call")
    one.close()
    fresh.close()


def test_refused_upload_leaves_the_handle_usable(A, P, hip_make):
    s = P.batch_turn90(hip_make, B)
    s.set_knot_models(np.ones(s.N, dtype=np.int32))
    for _ in range(3):  # every refusal drops the upload again
        with pytest.raises(A.AltroError) as e:
            s.solve()
        assert REFUSAL in str(e.value)
    s.set_knot_models(np.zeros(s.N, dtype=np.int32))
    s.solve()
    fresh = P.batch_turn90(hip_make, B)
    fresh.solve()
    for name, f in (("statistics", lambda h: h.get_stats()), ("trajectory", lambda h: h.get_trajectory()), ("gains", lambda h: h.get_gains()),
                    ("duals", lambda h: h.get_duals()), ("penalties", lambda h: h.get_penalties())):
        _same(f(s), f(fresh), name)
    s.close()
    fresh.close()
