"""Inputs with exactly known order statistics for the radix select (csrc/select.hip), shared by tests/test_order_stats_cpu.py (the
CPU specification) and tests/test_gpu_order_stats.py (the three kernel routes).

Reference: numpy.sort of the fp32 row, indexed at the rank.  It is exact, so results are compared by value with no tolerance
(``==``: a selected -0.0 or +0.0 both count as zero, everything else has one bit pattern per value; no case holds a NaN outside
the positive percentile, where NaNs are never selected).

Rows are built from chosen order-preserving uint32 keys (the inverse of the kernel's f2key), with the count of every byte of the
deciding radix pass fixed, so the ranks that sit on a cumulative-count edge of that pass are known: for each populated bin with
cumulative count e, ranks e - 1 and e, plus 0 and n - 1.  All rows of one case share one list of ranks (the kernels take one list
per launch), the union of the rows' edge ranks, in batches of eight (MAXR)."""
import functools

import numpy as np

from tests import cpu_backend as CB

MAXR = 8
# low bytes of the deciding pass: both ends, both sides of a 4-bins-per-lane boundary of pick_wave (3|4, 7|8, 251|252), and 127|128
POP = (0, 3, 4, 7, 8, 127, 128, 251, 252, 255)
_PRIORITY = (0, 255, 3, 4, 127, 128, 251, 252, 7, 8)          # which of them a row too short for all ten keeps
# shared top 24 key bits: about 1.0, about -4.0, just below FLT_MAX, just above -FLT_MAX (every low byte gives a finite value)
TOP_POS, TOP_NEG, TOP_BIG, TOP_NBIG = 0xBF8000, 0x3F8000, 0xFF7FFF, 0x008000
FLT_MAX = np.float32(np.finfo(np.float32).max)
DENORM = np.float32(1e-45)
BLOCK = 2048                                                  # planted deep-descent block of the long rows
FILLER = 1e-3                                                 # randn * FILLER: top key bytes 0xB?/0x4?, never those of the blocks


def f2key(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _rng(*seed):
    return np.random.default_rng([7919, *[int(s) & 0x7FFFFFFF for s in seed]])


def populated(n):
    return sorted(_PRIORITY[:min(int(n), len(_PRIORITY))])


def fixed_counts(n, m):
    """m unequal positive counts that sum to n (m <= n), a function of (n, m) alone"""
    w = 1 + (np.arange(m) * 7 + 3) % 5
    c = 1 + ((n - m) * w) // w.sum()
    c[m // 2] += n - c.sum()
    assert c.sum() == n and (c >= 1).all()
    return c.astype(np.int64)


def deep_keys(n, top24, bits):
    """n sorted keys that share their top `bits` (24, 16, 8) bits: the next byte takes the values of populated(n) with fixed_counts,
    the bytes below it (if any) cycle through POP."""
    if n == 0:
        return np.zeros(0, np.uint32)
    pop = populated(n)
    cnt = fixed_counts(n, len(pop))
    dec = np.repeat(np.asarray(pop, np.uint32), cnt)
    j = np.concatenate([np.arange(c) for c in cnt]).astype(np.int64)
    P = np.asarray(POP, np.uint32)
    if bits == 24:
        k = (np.uint32(top24) << np.uint32(8)) | dec
    elif bits == 16:
        k = (np.uint32(top24 >> 8) << np.uint32(16)) | (dec << np.uint32(8)) | P[j % 10]
    else:
        assert bits == 8 and (top24 >> 16) in (0xBF, 0x3F)               # 0xFF / 0x00 would reach inf and NaN
        k = (np.uint32(top24 >> 16) << np.uint32(24)) | (dec << np.uint32(16)) | (P[j % 10] << np.uint32(8)) | P[(j // 10) % 10]
    return np.sort(k.astype(np.uint32))


def edge_ranks(keys, shift):
    """ranks e - 1 and e for every cumulative count e at which (sorted key >> shift) changes"""
    ks = np.sort(keys) >> np.uint32(shift)
    e = np.nonzero(ks[1:] != ks[:-1])[0] + 1
    return sorted(set(e.tolist()) | set((e - 1).tolist()))


# ------------------------------------------------------------------------------------------------ row families
# name -> (kind, argument).  Every family comes positive, negative and mixed-sign.
SPECS = (
    ("deep24+", ("deep", 24, (TOP_POS,))), ("deep24-", ("deep", 24, (TOP_NEG,))), ("deep24+-", ("deep", 24, (TOP_NEG, TOP_POS))),
    ("deep24max", ("deep", 24, (TOP_BIG,))), ("deep24-max", ("deep", 24, (TOP_NBIG,))), ("deep24+-max", ("deep", 24, (TOP_NBIG, TOP_BIG))),
    ("deep16+", ("deep", 16, (TOP_POS,))), ("deep16-", ("deep", 16, (TOP_NEG,))), ("deep16+-", ("deep", 16, (TOP_NEG, TOP_POS))),
    ("deep16+-max", ("deep", 16, (TOP_NBIG, TOP_BIG))),
    ("deep8+", ("deep", 8, (TOP_POS,))), ("deep8-", ("deep", 8, (TOP_NEG,))), ("deep8+-", ("deep", 8, (TOP_NEG, TOP_POS))),
    ("ties+", ("values", (0.5, 1.0, 3.0))), ("ties-", ("values", (-3.0, -1.0, -0.5))), ("ties+-", ("values", (-2.0, 0.0, 1.0))),
    ("const+", ("values", (1.25,))), ("const-", ("values", (-1.25,))), ("const0", ("values", (-0.0, 0.0))),
    ("extreme+", ("values", (0.0, DENORM, 2 * DENORM, 1.0, FLT_MAX))),
    ("extreme-", ("values", (-FLT_MAX, -1.0, -2 * DENORM, -DENORM, -0.0))),
    ("extreme+-", ("values", (-FLT_MAX, -DENORM, -0.0, 0.0, DENORM, FLT_MAX))),
    ("plain", ("plain", None)),
)
INF_SPECS = (                                                  # kept off the lerp outputs: inf - inf is NaN in ATen's lerp as well
    ("inf+", ("values", (0.0, DENORM, FLT_MAX, np.inf))), ("inf-", ("values", (-np.inf, -FLT_MAX, -DENORM, -0.0))),
    ("inf+-", ("values", (-np.inf, -FLT_MAX, -0.0, 0.0, FLT_MAX, np.inf))),
)
_SPEC = dict(SPECS + INF_SPECS)
DEEP = tuple(s for s, _ in SPECS if s.startswith("deep"))
TIES = tuple(s for s, _ in SPECS if s.startswith(("ties", "const")))


def _parts(spec, n, seed):
    """-> (sorted keys of the deciding part, its deciding shift, filler values or None).  Rows longer than 2 * BLOCK plant the deep
    keys in randn * FILLER, whose top key byte differs from the block's."""
    kind = _SPEC[spec]
    if kind[0] == "plain":
        return np.zeros(0, np.uint32), 0, _rng(seed, n).standard_normal(n).astype(np.float32)
    if kind[0] == "values":
        vals = np.asarray(kind[1], np.float32)
        m = min(n, len(vals))
        keep = np.sort(np.round(np.linspace(0, len(vals) - 1, m)).astype(int))
        return np.sort(np.repeat(f2key(vals[keep]), fixed_counts(n, m))), 0, None
    _, bits, tops = kind
    nb = n if n <= 2 * BLOCK else BLOCK
    if len(tops) == 1:
        k = deep_keys(nb, tops[0], bits)
    else:
        k = np.concatenate([deep_keys(nb // 2, tops[0], bits), deep_keys(nb - nb // 2, tops[1], bits)])
    fill = None if nb == n else (_rng(seed, n, 1).standard_normal(n - nb) * FILLER).astype(np.float32)
    return k, 24 - bits, fill


def row_parts(spec, n, seed=0):
    """-> (block values, filler values), unshuffled: what the sharded tests deal out to their ranks"""
    k, _, fill = _parts(spec, n, seed)
    return key2f(k), (np.zeros(0, np.float32) if fill is None else fill)


def build_row(spec, n, seed=0):
    """-> (shuffled fp32 row [n], its edge ranks)"""
    k, shift, fill = _parts(spec, n, seed)
    if fill is None:
        keys, ranks = k, edge_ranks(k, shift)
    else:
        fk = f2key(fill)
        keys = np.concatenate([k, fk])
        ranks = []
        if len(k):                                          # the block's edges, at the offset of the filler below each part of it
            blk = np.asarray(edge_ranks(k, shift) + [0, len(k) - 1], np.int64)
            ranks = sorted(set((blk + np.searchsorted(np.sort(fk), k[blk])).tolist()))
            ranks = sorted(set(ranks) | {r + d for r in ranks for d in (-1, 1) if 0 <= r + d < n})
        else:
            ranks = _rng(seed, n, 2).integers(0, n, 6).tolist() + [n // 2]
    x = key2f(keys)
    _rng(seed, n, 3).shuffle(x)
    return x, sorted(set(ranks) | {0, n - 1})


class Case:
    """x [S, n] fp32, ranks [B, 8] int64 (shared by the rows), want [S, B, 8] = sorted rows at the ranks"""

    def __init__(self, name, specs, S, n, seed=0, extra_batches=()):
        self.name, self.S, self.n, self.specs = name, S, n, tuple(specs[s % len(specs)] for s in range(S))
        rows, ranks = [], set()
        for s, spec in enumerate(self.specs):
            x, r = build_row(spec, n, seed + 131 * s)
            rows.append(x)
            ranks |= set(r)
        self.x = np.stack(rows)
        srt = np.sort(self.x, axis=1)
        assert not np.isnan(self.x).any()
        ranks = sorted(ranks)
        ranks += [ranks[-1]] * (-len(ranks) % MAXR)
        self.ranks = np.asarray(ranks + [r for b in extra_batches for r in b], np.int64).reshape(-1, MAXR)
        self.want = srt[:, self.ranks]
        self.sorted = srt if srt.size <= (1 << 22) else None          # (the interpolated quantiles use small cases only)
        self.has_inf = bool(np.isinf(self.x).any())

    def __repr__(self):
        return f"Case({self.name}, S={self.S}, n={self.n}, batches={len(self.ranks)})"


class Rows:
    """rows dealt out by a test itself: what quantile_reference reads of a Case"""

    def __init__(self, x):
        self.x, (self.S, self.n), self.sorted = x, x.shape, np.sort(x, axis=1)


def diverging_ranks(n, spec):
    """Eight ranks of a deep16+ / deep16- row, one in each of eight different bins of pass 2 (last and first elements alternately):
    the eight states share their prefix through pass 1 and hold eight different prefixes in pass 3.  A batch of its own, unsorted."""
    assert spec in ("deep16+", "deep16-") and n >= MAXR
    nb = n if n <= 2 * BLOCK else BLOCK
    cnt = fixed_counts(nb, len(populated(nb)))
    end = np.cumsum(cnt)
    off = n - nb if spec == "deep16+" else 0                 # the filler lies below the positive block and above the negative one
    return [int(off + ((end[i] - cnt[i]) if i % 2 else end[i] - 1)) for i in range(len(cnt))][:MAXR]


@functools.lru_cache(maxsize=None)
def cases(S, n, inf=False, only=None):
    """Every family at [S, n]: ceil(len(SPECS) / S) cases of S rows (one case cycling through the families when S is larger)."""
    specs = [s for s, _ in (INF_SPECS if inf else SPECS)]
    if only is not None:
        specs = [s for s in specs if s in only]
    groups = [specs[i:i + S] for i in range(0, len(specs), S)] if S < len(specs) else [specs]
    out = []
    for gi, grp in enumerate(groups):
        extra = [diverging_ranks(n, s) for s in grp if s in ("deep16+", "deep16-") and n >= MAXR]
        out.append(Case("/".join(grp) if S < len(specs) else "all", grp, S, n, seed=1000 * gi + n % 977, extra_batches=extra))
    return tuple(out)


# The shapes at which run_select / one_block_ok change route or grid: (S, n, mbs, route, families or None for all)
ONE_BLOCK, FUSED = "k_sel_one_block", "k_sel_hist_pick"
# One row per case at S = 1, and a row of 2.1 M elements costs about 0.2 s of host time to build and sort: the whole table would take
# this one shape past five seconds.  The block cap changes only how k_sel_hist_pick strides the row, so three rows stand for it:
# both signs with a pass-3 decision, both ends of the key range with a pass-2 decision, and the control.
BIG_ONLY = ("deep24+-", "deep16+-max", "plain")
ROUTE_SHAPES = tuple((3, n, 1, ONE_BLOCK, None) for n in (1, 2, 255, 256, 257, 4097, 16384)) + (
    (3, 16385, 1, FUSED, None),                         # n > 16384 and S < 256
    (256, 65536, 1, ONE_BLOCK, None),                   # the long one-block route: S >= 256 and n <= 65536
    (256, 65537, 1, FUSED, None),
    (1, (1 << 21) + 4097, 1, FUSED, BIG_ONLY),          # ceil(n / 4096) = 514 blocks per segment, capped at 512
    (4, 300, 2, FUSED, None),                           # mbs > 1 is never one-block
)


# ------------------------------------------------------------------------------------------------ quantiles with interpolation
def ulp32(m):
    """numpy.spacing of fp32 |m| as fp64 (2**-149 below the normals), without its overflow in the top binade"""
    m = np.maximum(np.abs(np.asarray(m, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(m)) - 23)


QUANTILE_FAMILIES = DEEP + TIES + ("plain",)


def quantile_reference(case, qs, mbs):
    """-> (want [nq, S / mbs] fp64, bound [nq, S / mbs], emul [nq, S / mbs] fp32).  a, b exactly from the sort at quantile_ranks'
    fp32 positions.  want: lerp and chunk mean in fp64.  Bound: 3 ulp of max(|a|, |b|) per row (one rounding of b - a, one of the
    fmaf, |w d| <= 2 max), averaged over the chunk, plus one rounding of the chunk mean when mbs > 1.  emul: the same in the
    kernel's fp32 steps (ATen's lerp, sum in row order, one division); where it is not finite -- the fp32 sum of mbs values next
    to +-FLT_MAX overflows in the reference program as in the kernel -- no finite reference bounds the result and `assert_quantiles`
    asks for emul itself."""
    lohi, w = CB.quantile_ranks(qs, case.n)
    lohi, w32 = lohi.numpy().reshape(-1, 2), w.numpy().astype(np.float32)
    a32, b32 = case.sorted[:, lohi[:, 0]], case.sorted[:, lohi[:, 1]]                                        # [S, nq]
    a, b, w = a32.astype(np.float64), b32.astype(np.float64), w32.astype(np.float64)
    v = a + w[None] * (b - a)
    mx = np.maximum(np.abs(a), np.abs(b)).astype(np.float32)
    tol = 3.0 * ulp32(mx)
    nq = len(qs)
    with np.errstate(over="ignore", invalid="ignore"):
        d = (b32 - a32).astype(np.float64)
        v32 = np.where(np.abs(w32) < 0.5, a + w[None] * d, b + (w32 - np.float32(1.0)).astype(np.float64)[None] * d).astype(np.float32)
        v32 = v32.reshape(case.S // mbs, mbs, nq)
        emul = np.zeros((case.S // mbs, nq), np.float32)
        for m in range(mbs):
            emul = emul + v32[:, m]
        if mbs > 1:
            emul = emul / np.float32(mbs)
    v, tol, mx = (t.reshape(case.S // mbs, mbs, nq) for t in (v, tol, mx))
    want, bound = v.mean(1), tol.mean(1)
    if mbs > 1:
        bound = bound + ulp32(mx.max(1))
    return want.T, bound.T, emul.T


def assert_quantiles(got, ref, msg):
    """got fp32 [nq, S / mbs] against quantile_reference's triple: within the bound where the fp32 result is finite, else equal to it"""
    want, bound, emul = ref
    assert got.shape == want.shape and got.dtype == np.float32, msg
    fin = np.isfinite(emul)
    assert np.array_equal(got[~fin], emul[~fin], equal_nan=True), (msg, got[~fin], emul[~fin])
    err = np.abs(got.astype(np.float64) - want)[fin]
    assert (err <= bound[fin]).all(), (msg, err.max())


# ------------------------------------------------------------------------------------------------ positive percentile
# count * 0.5 is exact for count = 1000; 1e-9 gives ceil = 1, rank 0, for every count; 0.0 gives rank -1, which the clamp lifts to 0
PP_QS = (0.5, 1.0, 1e-9, 0.9, 0.013, 0.0)
PP_KINDS = ("none", "one", "all", "c1000", "c999", "c1001", "nan_inf")


def positive_rows(S, n, seed=0):
    """[S, n] rows cycling through PP_KINDS: no positive entry, exactly one, all positive, 999 / 1000 / 1001 positives, and NaNs
    and +inf among the positives."""
    rows = []
    for s in range(S):
        rng = _rng(seed, s, n, 4)
        kind = PP_KINDS[s % len(PP_KINDS)]
        mag = (np.abs(rng.standard_normal(n)) + 1e-3).astype(np.float32)
        x = -mag
        if s % 2:
            x[rng.integers(0, n, 5)] = 0.0                 # zeros and -0.0 are not positive
            x[rng.integers(0, n, 5)] = -0.0
        if kind == "one":
            x[rng.integers(0, n)] = 0.75
        elif kind == "all":
            x = mag
        elif kind.startswith("c"):
            idx = rng.permutation(n)[:int(kind[1:])]
            x[idx] = mag[idx]
        elif kind == "nan_inf":
            idx = rng.permutation(n)
            x[idx[:n // 3]] = mag[idx[:n // 3]]
            x[idx[:3]] = np.inf
            x[idx[3:40]] = np.nan
            x[idx[n // 3:n // 3 + 5]] = -np.inf
        rows.append(x.astype(np.float32))
    return np.stack(rows)


def rounding_row(which):
    """Row 0 or 1 of the two above 2**24 positives, where fp32(count) rounds to even; q = (1.0, 0.5, 0.0).
    2**24 + 1 positives: fp32(count) = 2**24, so q = 1 selects rank count - 2, the SECOND largest value (150 here, the largest is 200).
    2**24 + 3 positives and one 0.0: fp32(count) = 2**24 + 4, rank count, one past the last positive value -> 0.  The 0.0 is needed by
    the oracle, whose sorted tensor holds a NaN for it at that index; on an all-positive row its gather raises (index out of range)."""
    cnt, pad = (((1 << 24) + 1, 0), ((1 << 24) + 3, 1))[which]
    x = _rng(cnt).random(cnt + pad, dtype=np.float32) * np.float32(100) + np.float32(1e-3)
    x[5], x[7] = 200.0, 150.0
    if pad:
        x[11] = 0.0
    return x.reshape(1, -1)


ROUNDING_QS = (1.0, 0.5, 0.0)


def positive_reference(x, qs):
    """[nq, S]: rank clamp(ceil(fp32(count) * fp32(q)) - 1, 0) among the sorted entries > 0; 0 where there is none or where the rank
    lies past the last one (fp32(count) rounds up above 2**24)."""
    out = np.zeros((len(qs), x.shape[0]), np.float32)
    for s, row in enumerate(x):
        pos = np.sort(row[row > 0])
        cnt = np.float32(len(pos))
        for j, q in enumerate(qs):
            rk = max(int(np.ceil(cnt * np.float32(q))) - 1, 0)
            out[j, s] = pos[rk] if rk < len(pos) else 0.0
    return out
