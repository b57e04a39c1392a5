"""Shared by tests/test_ensemble_abi.py, tests/test_ensemble_gpu.py and tests/test_ensemble_facade_gpu.py: the contract of
include/altro_ensemble.h in numpy -- Philox4x32-10, the draw, the semidefinite factor, the noise arrays, and the per-knot
moments and counts over per-sample paths."""
import numpy as np

import _cov_common as CC

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
KNOT_INITIAL = 0xFFFFFFFF
STREAM_NOISE, STREAM_CONTROLS = 0, 1

# (counter, key) -> output: the known answers of the issue
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# ---- the purpose test (tests/test_ensemble_gpu.py; tests/test_ensemble_abi.py checks its numpy statement on the oracle) ------------
# problems.triple_integrator (linear dynamics: Sigma_k of altro_cov_propagate is exact), N = 12, no clip, no limits
PURPOSE_B, PURPOSE_S, PURPOSE_SEED = 2, 4096, 20261020
PURPOSE_SIGMA0 = np.diag([4e-4, 4e-4, 1e-4, 1e-4, 1e-4, 1e-4])
PURPOSE_W = np.diag([1e-6] * 6)
PURPOSE_W[2, 0] = PURPOSE_W[0, 2] = 5e-7  # (position and velocity noise of the first axis correlated)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays (broadcast against each other) of counters and keys -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(a, dtype=np.uint64) & np.uint64(MASK) for a in (c0, c1, c2, c3, k0, k1)))
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # (32 x 32 bits: no overflow in 64)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def uniform53(hi, lo):
    return ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64) + 0.5) * 2.0 ** -53


def draw_words(seed, k, s, instance, stream, j):
    seed = int(seed)
    return philox(k, s, np.asarray(instance, dtype=np.uint64) & np.uint64(MASK), (int(stream) << 16) | np.asarray(j, dtype=np.uint64),
                  seed & MASK, seed >> 32)


def normal_pair(seed, k, s, instance, stream, j):
    r0, r1, r2, r3 = draw_words(seed, k, s, instance, stream, j)
    u1, u2 = uniform53(r0, r1), uniform53(r2, r3)
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


def normals(seed, k, s, instance, stream, n):
    """xi [..., n] for broadcast k, s, instance"""
    k, s, instance = np.broadcast_arrays(np.asarray(k, dtype=np.uint64), np.asarray(s, dtype=np.uint64), np.asarray(instance, dtype=np.uint64))
    j = np.arange((n + 1) // 2, dtype=np.uint64)
    z0, z1 = normal_pair(seed, k[..., None], s[..., None], instance[..., None], stream, j)
    return np.stack([z0, z1], axis=-1).reshape(k.shape + (-1,))[..., :n]


def psd_factor(W):
    """The semidefinite Cholesky factor of lower_sym(W) by the header's rule, in plain float64 loops (each product and each sum
    rounded on its own); None where W is refused."""
    W = np.asarray(W, dtype=np.float64)
    n = W.shape[0]
    top = max([abs(W[i, i]) for i in range(n)] + [0.0])
    t = 4.0 * n * 2.0 ** -52 * top
    if not t < np.inf:
        return None
    L = np.zeros((n, n))
    for j in range(n):
        s = 0.0
        for k in range(j):
            s += L[j, k] * L[j, k]
        d = W[j, j] - s
        if not d >= -t:
            return None
        if abs(d) <= t:
            continue
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            a = 0.0
            for k in range(j):
                a += L[i, k] * L[j, k]
            L[i, j] = (W[i, j] - a) / L[j, j]
    return L


def matrix_of(M, mode, b, k):
    """matrix (instance b, knot k) of an array laid out by ``mode`` (bit 0 per instance, bit 1 per knot)"""
    M = np.asarray(M)
    return M if mode == 0 else M[b] if mode == CC.W_PER_INSTANCE else M[k] if mode == CC.W_PER_KNOT else M[b, k]


def noise_arrays(B, S, steps, n, seed, instance_base=0, Sigma0=None, W=None, w_mode=0):
    """-> dx0 [B][S][n], w [B][S][steps][n] as altro_noise_fill writes them (to rounding), and max |L| over all factors"""
    dx0, w = np.zeros((B, S, n)), np.zeros((B, S, steps, n))
    s = np.arange(S)
    top = 0.0
    for b in range(B):
        if Sigma0 is not None:
            S0 = np.asarray(Sigma0)
            L = psd_factor(S0[b] if S0.ndim == 3 else S0)
            top = max(top, np.abs(L).max())
            dx0[b] = normals(seed, KNOT_INITIAL, s, instance_base + b, STREAM_NOISE, n) @ L.T
        if W is not None:
            xi = normals(seed, np.arange(steps)[None, :], s[:, None], instance_base + b, STREAM_NOISE, n)  # [S][steps][n]
            for k in range(steps):
                L = psd_factor(matrix_of(W, w_mode, b, k))
                top = max(top, np.abs(L).max())
                w[b, :, k] = xi[:, k] @ L.T
    return dx0, w, top


def moments(X_cl, Xbar, steps_done):
    """X_cl [B][S][steps + 1][n] (NaN rows behind a stop), Xbar [B][>= steps + 1][n], steps_done [B][S] ->
    alive [B][steps + 1], mean [B][steps + 1][n], mom2 [B][steps + 1][n][n] over the samples alive at k (k <= steps_done);
    NaN where nobody is"""
    B, S, K1, n = X_cl.shape
    live = np.arange(K1)[None, None, :] <= steps_done[:, :, None]  # [B][S][K1]
    e = np.where(live[..., None], X_cl - Xbar[:, None, :K1], 0.0)
    alive = live.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = e.sum(axis=1) / alive[..., None]
        mom2 = np.einsum("bski,bskj->bkij", e, e) / alive[..., None, None]
    return alive.astype(np.int32), mean, mom2


def slabs(B, S, chunk=64, fill=1024, most=16):
    """(slabs, chunks per slab) by the rule of EnsembleSlabs / EnsembleChunksPerSlab, in plain integer steps"""
    chunks = -(-S // chunk)
    want = max(1, min(chunks, -(-fill // B), most))
    per = -(-chunks // want)
    return -(-chunks // per), per
