"""The ticket arithmetic of the persistent tail's worker grid (tail_worker_count / tail_grid / tail_block_of_ticket,
altro_kernels.hpp), asked of the library on the host: the same functions LaunchTail and the kernel inline.  No GPU."""
import ctypes

CUS = 256   # MI355X


def _tickets(lib):
    f = lib.altro_tail_tickets
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int)] * 2

    def ask(ninst, npool, cus, per_cu, asked, kind=0, ticket=0):
        workers, block = ctypes.c_int(), ctypes.c_int()
        grid = f(ninst, npool, cus, per_cu, asked, kind, ticket, ctypes.byref(workers), ctypes.byref(block))
        return grid, workers.value, block.value
    return ask


def test_ticket_identities_are_the_one_shot_grid_s_blocks(A):
    """primary ticket s is block s (slot s, mailbox s); pool ticket t is block ninst + t (shadow column col0 + t, mailbox
    cap + t); every block of the one-shot grid is named by exactly one ticket, primaries first; past the last: -1"""
    ask = _tickets(A.load_library())
    for ninst, npool in ((1, 255), (16, 240), (64, 192), (255, 255), (256, 256), (257, 257), (512, 320), (4096, 0)):
        blocks = [ask(ninst, npool, CUS, 1, -1, 0, s)[2] for s in range(ninst)] + [ask(ninst, npool, CUS, 1, -1, 1, t)[2] for t in range(npool)]
        assert blocks == list(range(ninst + npool)), (ninst, npool)
        for past in (0, 1, 1000):
            assert ask(ninst, npool, CUS, 1, -1, 0, ninst + past)[2] == -1
            assert ask(ninst, npool, CUS, 1, -1, 1, npool + past)[2] == -1


def test_grid_size(A):
    """unset: min(jobs, CUs x workgroups per CU) resident workers, for batches below, at and above the CU count; 0: the
    one-shot grid, a workgroup per job; n: at most n workers, never more than fit"""
    ask = _tickets(A.load_library())
    for ninst in (1, 16, 64, 255, 256, 257, 512, 4096):
        npool = max(ninst, CUS - ninst)   # (LaunchTail's pool, before the cap of the shadow columns)
        jobs = ninst + npool
        for per_cu in (1, 2):
            grid, workers, _ = ask(ninst, npool, CUS, per_cu, -1)
            assert grid == workers == min(jobs, CUS * per_cu) and grid <= CUS * per_cu
            grid, workers, _ = ask(ninst, npool, CUS, per_cu, 0)
            assert workers == 0 and grid == jobs
            for n in (1, 8, 255, 256, 257, 100000):
                grid, workers, _ = ask(ninst, npool, CUS, per_cu, n)
                assert grid == workers == min(n, jobs, CUS * per_cu)
        # an occupancy query that failed (0 workgroups per CU) must not size a grid of workers that are not all resident
        grid, workers, _ = ask(ninst, npool, CUS, 0, -1)
        assert workers == 0 and grid == jobs
    # a launch without a pool (no twins): every job is a primary
    assert ask(300, 0, CUS, 1, -1)[:2] == (256, 256) and ask(100, 0, CUS, 1, -1)[:2] == (100, 100)
