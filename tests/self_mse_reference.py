"""The self-MSE searches' score, restated in numpy -- the specification the three device scorers (csrc/sorted_score.hip k_score_sorted,
csrc/search_ops.hip k_score_w_self and k_score_a_self) and their CPU stand-ins are held to, PER SCORE.

    score[p, seg] = -norm * sum_{i in seg} (x_i - c_i)^2                                              (uniform.py:29-36)
    level = rint(fl32(x / s)),  q = clip(fl32(level + z), 0, qmax),  c = fl32(fl32(q - z) * s)        every step in fp32

c is what every implementation must reproduce bit for bit (three fp32 operations in a fixed order); the difference, its square and
the sum are taken here in numpy.longdouble (64-bit significand: x - c of two fp32 numbers and its square are exact or rounded at
2^-64, the pairwise sum of n non-negative terms at log2(n) 2^-64), so the reference's own error is at most 2^-58 of the score for
every size used and no bar below has to make room for it.  Platforms whose long double is a plain double fall back to math.fsum.

A segment is one row of ``x2 [S, n]``: a weight row, an activation channel, or a whole tensor.  ``scale`` / ``zp`` are [P, S],
candidate-major, as the kernels take them.

The error bars of the device routes live here as well, each next to its derivation, so that the CPU tier can check them on the CPU
stand-ins before a GPU sees them.  u = 2^-24 (fp32 unit roundoff), v = 2^-53 (fp64).
"""
import math

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY32 = 2.0 ** -149                 # the smallest fp32 denormal: what one underflowing fp32 operation can lose
PB = 1024                            # csrc/sorted_score.hip: elements per prefix block
SLAB_ROWS = 128                      # csrc/search_ops.hip: rows per slab of k_score_a_self

_LD = np.longdouble
_WIDE = np.finfo(_LD).nmant >= 63


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _sum_rows(e2):
    """exact-enough row sums of non-negative long-double terms [S, n] -> float64 [S] (NaN / inf propagate)"""
    if _WIDE:
        return e2.sum(axis=1).astype(np.float64)
    out = np.empty(e2.shape[0])
    for i, row in enumerate(e2):
        out[i] = math.fsum(row.tolist()) if np.isfinite(row).all() else float(row.sum())
    return out


def dequant32(x, s, z, qmax):
    """-> (level, c) in fp32, operation by operation (numpy's float32 divide / rint / add / multiply are IEEE, round to nearest even)"""
    x, s, z = _f32(x), _f32(s), _f32(z)
    with np.errstate(all="ignore"):
        level = np.rint(x / s)
        q = np.clip(level + z, np.float32(0), np.float32(qmax))
        c = (q - z) * s
    assert level.dtype == np.float32 and c.dtype == np.float32
    return level, c


class Scores:
    """score [P, S] float64 and, per (candidate, segment), what the bars and the coverage checks need.  Per segment: sx2 = sum x^2,
    sax = sum |x|, n.  Per (p, seg): cmax = max |c|, runs = non-empty runs of the sorted segment (one per unclamped level present,
    plus the low-clamped and the high-clamped run), low / high = those two runs are non-empty, hole = at least one of the unclamped levels
    ceil(-z) .. floor(qmax - z) holds no element (its thread's run is empty), dup_edge = a run starts right after or right before a pair of EQUAL elements (the bisection
    of k_score_sorted then has to pass equal values to find the boundary)."""
    __slots__ = ("score", "sx2", "sax", "n", "cmax", "runs", "low", "high", "hole", "dup_edge")


def score_segments(x2, scale, zp, bits, norm, stats=True):
    x2 = _f32(x2)
    S, n = x2.shape
    scale, zp = _f32(scale).reshape(-1, S), _f32(zp).reshape(-1, S)
    P = scale.shape[0]
    qmax = float(2 ** bits - 1)
    xs = np.sort(x2, axis=1)                                   # sorted order (NaN last); the sum does not depend on it
    xl = xs.astype(_LD)
    r = Scores()
    r.n = n
    r.sx2 = _sum_rows(xl * xl)
    r.sax = _sum_rows(np.abs(xl))
    r.score = np.empty((P, S))
    r.cmax = np.zeros((P, S))
    r.runs = np.zeros((P, S), np.int64)
    r.low, r.high, r.hole, r.dup_edge = (np.zeros((P, S), bool) for _ in range(4))
    eq_next = np.zeros((S, n), bool)
    if n > 1:
        eq_next[:, :-1] = xs[:, 1:] == xs[:, :-1]              # element i equals element i + 1
    for p in range(P):
        s, z = scale[p][:, None], zp[p][:, None]
        level, c = dequant32(xs, s, z, qmax)
        with np.errstate(all="ignore"):
            e = xl - c.astype(_LD)
            r.score[p] = -norm * _sum_rows(e * e)
            if not stats:
                continue
            r.cmax[p] = np.abs(c.astype(np.float64)).max(axis=1)
            klo, khi = np.ceil(-z), np.floor(np.float32(qmax) - z)
            low, high = level < klo, level > khi
            rid = np.where(low, -np.inf, np.where(high, np.inf, level.astype(np.float64)))
        r.low[p], r.high[p] = low.any(axis=1), high.any(axis=1)
        if n > 1:
            edge = rid[:, 1:] != rid[:, :-1]                   # a run starts at i + 1
            r.runs[p] = 1 + edge.sum(axis=1)
            before = np.zeros_like(edge)
            before[:, 1:] = eq_next[:, :-2]                    # elements i - 1 and i are equal, the run ends at i
            after = eq_next[:, 1:]                             # elements i + 1 and i + 2 are equal, the run starts at i + 1
            r.dup_edge[p] = (edge & (before | after)).any(axis=1)
        else:
            r.runs[p] = 1
        present = r.runs[p] - r.low[p] - r.high[p]
        r.hole[p] = present < (khi - klo + 1).astype(np.float64)[:, 0]
    return r


def exact_prefix(x2):
    """-> (sorted [S, n] fp32, prefix [S, n + 1, 2] float64, mass [S, n + 1, 2] float64): exclusive prefix sums of x and x^2 along the
    sorted order, EXACT and rounded once to fp64; mass = the same sums of |x| and x^2.  Every element is an integer multiple of the
    segment's smallest power of two, so the sums are taken over Python integers.  (A long-double running sum is not good enough here:
    squares have biased low bits, its roundings do not cancel, and at half a million elements of the large-offset pattern it is off
    by 30 fp64 ulps -- as much as the bar.)"""
    import itertools
    xs = np.sort(_f32(x2), axis=1)
    S, n = xs.shape
    pf, mass = np.zeros((S, n + 1, 2)), np.zeros((S, n + 1, 2))
    for s_ in range(S):
        v = xs[s_].astype(np.float64)
        assert np.isfinite(v).all()
        nz = np.abs(v[v != 0])
        e = int(np.floor(np.log2(nz.min()))) - 24 if nz.size else 0             # every element is a multiple of 2^e
        m = [int(t) for t in np.ldexp(v, -e)]
        assert all(float(t) == u for t, u in zip(m[:64], np.ldexp(v[:64], -e)))
        for col, terms, sc in ((0, m, e), (1, [t * t for t in m], 2 * e)):
            pf[s_, 1:, col] = [math.ldexp(t, sc) for t in itertools.accumulate(terms)]
        mass[s_, 1:, 0] = [math.ldexp(t, e) for t in itertools.accumulate(abs(t) for t in m)]
    mass[:, :, 1] = pf[:, :, 1]
    return xs, pf, mass


# ------------------------------------------------------------------------------------------------ error bars
def prefix_depth(n):
    """The most fp64 roundings any term of a prefix entry passes through in k_sp_blocksum / k_sp_blockscan / k_sp_prefix, read from
    the kernels:
      block sums   3 adds over a thread's 4 elements, 6 wave-butterfly steps, 2 across the 4 waves                            11
      block scan   6 wave-scan steps, up to 3 wave totals, 2 for inclusive -> exclusive (o + a - v), and the carry: 3 to form a
                   chunk's total, then one add per following chunk of 256 blocks                                  11 + 3 + chunks
      prefix       base + (a - t): 2, up to 3 wave totals, up to 4 elements of the thread                                      9
    (an element of the entry's own block passes through fewer: 2 + 6 + 1 + 1 + 3 + 4).  One more for the second-order terms of
    (1 + v)^depth, which stay below one v for every depth that fits the 2^31-element limit."""
    chunks = -(-(-(-n // PB)) // 256)
    return 11 + 14 + chunks + 9 + 1


def prefix_bar(n, mass):
    """|entry - exact| <= depth(n) v (sum of |terms| of the entry): the standard bound for a summation tree of that depth."""
    return prefix_depth(n) * U64 * mass


def kappa(n):
    """k_score_sorted takes TWO prefix entries per difference, hence twice the depth."""
    return 2 * prefix_depth(n)


def sorted_bar(ref, norm, score=None):
    """k_score_sorted: |got - ref| <= u |ref| + TINY32 + norm (runs + 2) kappa v A,  A = sum x^2 + 2 |c|max sum |x| + n c^2max.

    Per non-empty run the kernel forms (S2b - S2a) - 2 c (S1b - S1a) + cnt c c in fp64.  The four prefix entries carry
    depth v (sum x^2) and depth v (sum |x|) each (prefix_bar), which gives kappa v (sum x^2 + 2 |c| sum |x|) per run; the five fp64
    operations of the run itself, the two adds of thread 0's clamped runs, the <= 8 steps of the group's tree and the product with
    norm round values no larger than A and number 16 <= 2 kappa in all -- the ``+ 2``.  Then ONE fp32 rounding of the result:
    u |ref|, or TINY32 where the score is denormal.  The run boundaries are exact (the reference's own predicate), so nothing else
    enters.  On the large-offset segments A / |ref| is ~1e12 and the fp64 term is the whole bar; elsewhere it is ~1e-13 |ref|."""
    sc = ref.score if score is None else score
    A = ref.sx2[None, :] + 2.0 * ref.cmax * ref.sax[None, :] + ref.n * ref.cmax ** 2
    return U32 * np.abs(sc) + TINY32 + abs(norm) * (ref.runs + 2) * kappa(ref.n) * U64 * A


def _rel(k):
    """(1 + u)^k - 1: k fp32 roundings on a non-negative term, second order included"""
    return math.expm1(k * math.log1p(U32))


def onepass_bar(ref, n_terms):
    """k_score_w_self and k_score_a_self as they are now: c in fp32 (the reference's bits), then fp64 throughout -- the difference
    (exact, or rounded at v when the exponents are 29 apart), the square (v), a chain of at most n_terms additions (K9: I sequential
    ones; K10: 32 in the thread, 3 across row groups, the finishing tree) and the product with norm: at most (n_terms + 16) v on
    non-negative terms.  Then ONE fp32 rounding of the result, u |ref|, or TINY32 where it is denormal.  This is what makes the
    one-pass routes and the sorted route agree to the last bit almost everywhere, which the layer-level test relies on; it is never
    wider than the fp32-accumulation bars below."""
    return (U32 + (n_terms + 16) * U64) * np.abs(ref.score) + TINY32


def act_chain(rows, zp):
    """Length of the fp32 addition chain of a one-pass activation scorer that accumulates in fp32, as k_score_a_self did and the
    CPU stand-in's per-term arithmetic still does.  Fast path (integral z and the thread's 32
    rows all present): 16 packed adds per half and one add of the halves, 17.  Slow path: 32 sequential adds.  Then the 3 adds across
    the four row groups.  A score whose rows are a whole number of slabs and whose z is integral sees only the fast path; any other
    may see the slow one."""
    zp = np.asarray(zp, np.float64)
    fast = (np.rint(zp) == zp) & (rows % SLAB_ROWS == 0)
    return np.where(fast, 17 + 3, 32 + 3)


def act_bar(ref, norm, rows, zp, n_terms):
    """The bar for fp32 terms and fp32 accumulation (tests/cpu_backend.py meets it; the device kernel is held to onepass_bar): every
    term (x - c)^2 >= 0, so the bar is relative to the score:
    (3 + chain) u |ref| -- c is the reference's bit for bit (med3(k, -z, qmax - z) == clip(k + z, 0, qmax) - z exactly for integral
    z), x - c rounds once (relative u, twice that on the square), the square rounds once: 3; then the chain.  The fp64 finish adds
    slabs and channels at v and the result is rounded to fp32 once: one more u covers both.  Each of the n_terms fp32 squares may
    underflow and lose up to TINY32, as may the final rounding."""
    k = 3 + act_chain(rows, zp) + 1
    return np.vectorize(_rel)(k) * np.abs(ref.score) + abs(norm) * (n_terms + 1) * TINY32 + TINY32


def weight_bar(ref, n_terms):
    """fp32 accumulation over a weight row (tests/cpu_backend.score_w_self; the device kernel is held to onepass_bar):
    (3 + I) u |ref| -- 3 per term as above, I - 1 sequential fp32 adds and the division by I; plus the underflow
    floor."""
    return _rel(3 + n_terms) * np.abs(ref.score) + 2 * TINY32
