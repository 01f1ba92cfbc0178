"""The Hessian bit cost of include/adalog_hip.h (adalog_bit_cost_f32) and the allocation problem of adalog_amd/utils/bitplan.py restated
in numpy / plain Python -- TEST INFRASTRUCTURE ONLY.  Written from the specification; the reference project has no mixed precision.

    bits == 0:  d = double(w)
    else:       c = clamp(rne(w / s) + rne(z), 0, 2^b - 1);  q = (c - rne(z)) * s   (fp32);  d = double(w) - double(q)
    cost[i][r] = sum_jk d_j H_jk d_k   (fp64),      A[i][r] = sum_jk |d_j| |H_jk| |d_k|   (what the error bound of a sum is stated in)
"""
import itertools

import numpy as np


def _params(scale, zero_point, R):
    s = np.asarray(scale, np.float32).reshape(-1)
    z = np.asarray(zero_point, np.float32).reshape(-1)
    assert s.size == z.size and s.size in (1, R)
    return np.broadcast_to(s, (R,)).copy()[:, None], np.rint(np.broadcast_to(z, (R,))).astype(np.float32)[:, None]


def diff(W, scale, zero_point, bits):
    """(d fp64 [R, K], codes fp32 [R, K] or None) of one width"""
    W = np.asarray(W, np.float32)
    if bits == 0:
        return W.astype(np.float64), None
    s, zr = _params(scale, zero_point, W.shape[0])
    c = np.minimum(np.maximum(np.rint(W / s) + zr, np.float32(0.0)), np.float32(2 ** bits - 1))
    q = (c - zr) * s
    assert c.dtype == np.float32 and q.dtype == np.float32
    return W.astype(np.float64) - q.astype(np.float64), c


def bit_cost(W, scales, zero_points, bits, H):
    """-> (cost fp64 [n_widths, R], A fp64 [n_widths, R]); scales / zero_points: [n_widths, 1] or [n_widths, R]"""
    W = np.asarray(W, np.float32)
    H = np.asarray(H, np.float64)
    scales, zero_points = np.asarray(scales, np.float32), np.asarray(zero_points, np.float32)
    assert scales.shape == zero_points.shape and scales.shape[0] == len(bits)
    aH = np.abs(H)
    cost, A = [], []
    for i, b in enumerate(bits):
        d, _ = diff(W, scales[i], zero_points[i], int(b))
        cost.append(((d @ H) * d).sum(axis=1))
        ad = np.abs(d)
        A.append(((ad @ aH) * ad).sum(axis=1))
    return np.stack(cost), np.stack(A)


def minmax_params(W, widths):
    """the per-row min/max asymmetric quantiser at every width: (scales, zero points) fp32 [n_widths, R]; width 0 and constant rows: 1, 0"""
    W = np.asarray(W, np.float32)
    mn, mx = W.min(axis=1), W.max(axis=1)
    S, Z = [], []
    for b in widths:
        if b == 0:
            S.append(np.ones_like(mn)); Z.append(np.zeros_like(mn))
            continue
        const = mx == mn
        s = ((mx - mn) / np.float32(2 ** b - 1)).astype(np.float32)
        s = np.where(const, np.float32(1.0), s).astype(np.float32)
        z = np.where(const, np.float32(0.0), -mn / s).astype(np.float32)
        S.append(s); Z.append(z)
    return np.stack(S), np.stack(Z)


def brute_force(sizes, costs, widths, avg_bits):
    """Every assignment of a width to a layer: the feasible one (sum n b <= avg_bits sum n) of least cost, ties by fewer total bits, then by
    the lexicographically smallest width tuple.  costs[l][k]: layer l at widths[k].  -> (tuple of widths, cost) or None when none fits."""
    budget = avg_bits * sum(sizes)
    best = None
    for pick in itertools.product(range(len(widths)), repeat=len(sizes)):
        ws = tuple(widths[k] for k in pick)
        used = sum(n * b for n, b in zip(sizes, ws))
        if used > budget:
            continue
        key = (sum(costs[l][k] for l, k in enumerate(pick)), used, ws)
        if best is None or key < best:
            best = key
    return None if best is None else (best[2], best[0])
