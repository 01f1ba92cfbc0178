"""The GPTQ column sweep of include/adalog_hip.h (adalog_gptq_sweep_f32) and the factor of adalog_amd/utils/gptq.py restated in numpy
-- TEST INFRASTRUCTURE ONLY.  Written from the specification; the reference project has no GPTQ.

    run = double(W[r]);  for j ascending:  c = clamp(rne(float(run_j) / s) + rne(z), 0, 2^b - 1)      (fp32)
                                           q = (c - rne(z)) * s                                       (fp32)
                                           e = (run_j - double(q)) / U[j][j]                          (fp64)
                                           run_k = run_k - e * U[j][k],  k > j                        (fp64: multiply, then subtract)

numpy rounds every array operation on its own (no fused multiply-add), so with the order of j fixed the result is THE result of the
recurrence in IEEE arithmetic; the kernel must match it bit for bit."""
import numpy as np


def _params(scale, zero_point, R):
    s = np.asarray(scale, np.float32).reshape(-1)
    z = np.asarray(zero_point, np.float32).reshape(-1)
    assert s.size == z.size and s.size in (1, R)
    return np.broadcast_to(s, (R,)).copy(), np.rint(np.broadcast_to(z, (R,))).astype(np.float32)


def _quantise(x32, s, zr, qmax):
    """(c, q) of one column: fp32 throughout"""
    c = np.minimum(np.maximum(np.rint(x32 / s) + zr, np.float32(0.0)), qmax)
    q = (c - zr) * s
    assert c.dtype == np.float32 and q.dtype == np.float32
    return c, q


def rtn(W, scale, zero_point, n_bits):
    """round-to-nearest: (What fp32, codes uint8) of the asymmetric uniform quantiser, element by element"""
    W = np.asarray(W, np.float32)
    s, zr = _params(scale, zero_point, W.shape[0])
    c, q = _quantise(W, s[:, None], zr[:, None], np.float32(2 ** n_bits - 1))
    return q, c.astype(np.uint8)


def sweep(W, scale, zero_point, n_bits, U):
    """-> (What fp32 [R, K], codes uint8 [R, K], objective fp64 [R]): the specification, column by column"""
    W = np.asarray(W, np.float32)
    U = np.asarray(U, np.float64)
    R, K = W.shape
    s, zr = _params(scale, zero_point, R)
    qmax = np.float32(2 ** n_bits - 1)
    run = W.astype(np.float64)
    what, codes, obj = np.empty((R, K), np.float32), np.empty((R, K), np.uint8), np.zeros(R, np.float64)
    for j in range(K):
        c, q = _quantise(run[:, j].astype(np.float32), s, zr, qmax)
        what[:, j], codes[:, j] = q, c.astype(np.uint8)
        e = (run[:, j] - q.astype(np.float64)) / U[j, j]
        obj = obj + e * e
        if j + 1 < K:
            run[:, j + 1:] = run[:, j + 1:] - e[:, None] * U[j, j + 1:][None, :]
    return what, codes, obj


def sweep_blocked(W, scale, zero_point, n_bits, U, block=64):
    """The same recurrence in the order csrc/gptq.hip walks it: a block of 64 columns is swept on its own, then its 64 errors go to
    the columns behind the block one after the other.  Every element still sees its updates in ascending j, each a separately rounded
    multiply and subtract, so the result equals sweep() bit for bit (tests/test_gptq_cpu.py asserts that)."""
    W = np.asarray(W, np.float32)
    U = np.asarray(U, np.float64)
    R, K = W.shape
    s, zr = _params(scale, zero_point, R)
    qmax = np.float32(2 ** n_bits - 1)
    run = W.astype(np.float64)
    what, codes, obj = np.empty((R, K), np.float32), np.empty((R, K), np.uint8), np.zeros(R, np.float64)
    for j0 in range(0, K, block):
        j1 = min(K, j0 + block)
        errs = []
        for j in range(j0, j1):
            c, q = _quantise(run[:, j].astype(np.float32), s, zr, qmax)
            what[:, j], codes[:, j] = q, c.astype(np.uint8)
            e = (run[:, j] - q.astype(np.float64)) / U[j, j]
            obj = obj + e * e
            errs.append(e)
            if j + 1 < j1:
                run[:, j + 1:j1] = run[:, j + 1:j1] - e[:, None] * U[j, j + 1:j1][None, :]
        for j, e in zip(range(j0, j1), errs):
            if j1 < K:
                run[:, j1:] = run[:, j1:] - e[:, None] * U[j, j1:][None, :]
    return what, codes, obj


def damp(H, damp=0.01):
    """H (fp64, copied) with the diagonal of dead columns set to 1 and damp * mean(diag) added to the diagonal"""
    Hd = np.array(H, np.float64)
    d = np.diagonal(Hd).copy()
    d[d == 0] = 1.0
    d = d + damp * d.mean()
    np.fill_diagonal(Hd, d)
    return Hd


def factor(H, damp_=0.01):
    """(U, Hd): U fp64 upper triangular with Hd^-1 = U^T U, Hd = damp(H)"""
    Hd = damp(H, damp_)
    Linv = np.linalg.inv(np.linalg.cholesky(Hd))
    Hinv = Linv.T @ Linv
    U = np.linalg.cholesky((Hinv + Hinv.T) * 0.5).T
    return np.ascontiguousarray(U), Hd


def quadratic(D, Hd):
    """per row: D[r] Hd D[r]^T in fp64"""
    D = np.asarray(D, np.float64)
    return ((D @ Hd) * D).sum(axis=1)


def minmax_params(W, n_bits):
    """per-row min/max quantiser of W: (scale [R], zero point [R]) fp32"""
    W = np.asarray(W, np.float32)
    mn, mx = W.min(axis=1), W.max(axis=1)
    s = ((mx - mn) / np.float32(2 ** n_bits - 1)).astype(np.float32)
    return s, (-mn / s).astype(np.float32)


def inputs(kind, T, K, R, seed):
    """(X fp64 [T, K], W fp32 [R, K]) of the issue's outcome table: iid gaussian X, or correlated X (X . (0.3 I + G / sqrt(K)) + 0.5)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, K))
    if kind == "correlated":
        X = X @ (0.3 * np.eye(K) + rng.standard_normal((K, K)) / np.sqrt(K)) + 0.5
    else:
        assert kind == "iid"
    W = rng.standard_normal((R, K)).astype(np.float32)
    return X, W
