"""The split policy of the persistent tail (tw_keep / tw_claimable / tw_min_share, altro_kernels.hpp), asked of the
library on the host: the same functions the kernels inline.  No GPU."""
import ctypes

FLOOR = 3            # kTwinMinFloor
SEE_CLAIM = 3        # kTwinSeeClaim: iterations a publisher needs, from the progress word a claimer read, to see the claim
MAX_INNER = 100      # altro_default_options: max_iterations_inner


def _policy(lib):
    f = lib.altro_twin_policy
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)] * 3

    def ask(R, lag, minimum):
        keep, claimable, see = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        used = f(R, lag, minimum, ctypes.byref(keep), ctypes.byref(claimable), ctypes.byref(see))
        return used, keep.value, bool(claimable.value), see.value
    return ask


def test_minimum_is_clamped(A):
    ask = _policy(A.load_library())
    for asked in (-5, 0, 1, 2, FLOOR):
        assert ask(50, 1, asked)[0] == FLOOR
    for asked in (4, 6, 8, 12, 50):
        assert ask(50, 1, asked)[0] == asked
    assert ask(50, 1, 1 << 30)[0] < 1 << 20   # (twice the value still fits an int)
    assert ask(50, 1, 12)[3] == SEE_CLAIM


def test_shares_of_every_segment(A):
    """for every R up to max_iterations_inner, every lag in use and every allowed minimum: the shares add up; a claimable
    segment leaves both sides the minimum, and the publisher the iterations it needs to see the claim before its joint;
    and the smallest allowed minimum still splits something"""
    ask = _policy(A.load_library())
    for lag in (0, 1, 2, 3):
        for minimum in range(FLOOR, MAX_INNER // 2 + 2):
            n_claimable = 0
            for R in range(0, MAX_INNER + 1):
                used, keep, claimable, see = ask(R, lag, minimum)
                claimed = R - keep
                assert used == minimum and keep + claimed == R
                if claimable:
                    n_claimable += 1
                    assert keep >= minimum and claimed >= minimum, (R, lag, minimum, keep)
                    assert keep >= see + 1, (R, lag, minimum, keep)   # (one iteration to spare)
                    assert R >= 2 * minimum
                else:
                    # nothing that could be split into two shares of the minimum with the lag paid is turned away
                    assert claimed < minimum, (R, lag, minimum, keep)
            if 2 * minimum + lag + 2 <= MAX_INNER:
                assert n_claimable > 0, (lag, minimum)
    # the former rule: 12 iterations, lag 1 -- segments of 26 or more
    assert [R for R in range(40) if ask(R, 1, 12)[2]][0] == 26
