"""One case table for the self-MSE scorers, shared by tests/test_self_mse_cpu.py (the CPU stand-ins) and tests/test_gpu_self_mse.py
(k_score_sorted behind the prefix build, k_score_w_self, k_score_a_self).  Reference: tests/self_mse_reference.py.

A case is a set of SEGMENTS ``x [S, n]`` with candidates ``scale`` / ``zp [P, S]`` (every segment has its own, scaled to its
range), a bit width and a norm.  ``layout`` says how the one-pass kernels see the same numbers:
    "w"   weight rows:             w2 = x          [rows = S, I = n]      k_score_w_self, norm = 1 / I
    "cw"  channel-wise activation: x2 = x^T        [rows = n, I = S]      k_score_a_self, parameters [P, I]
    "pt"  per-tensor activation:   x2 = x.view(rows, I), S = 1            k_score_a_self, parameters [P, 1]
    "seg" the sorted route only
The sorted route takes every case.  Segment s of a case holds data pattern PATTERNS[(first + s) % 9]; candidate p of a segment is
SPECIALS[p] while they last, then a random (scale, zero point) around the segment's range.
"""
import functools

import numpy as np

from tests import self_mse_reference as R

PATTERNS = ("gauss", "gelu", "const", "dups", "zeros", "offset", "outlier", "ties", "denorm")
TIE_S = 0.125                                    # the power-of-two scale the ``ties`` pattern is planted for
TIE_SPAN = 40                                    # ties are planted this many levels past both clamps of any z in [0, qmax]


def _rng(*seed):
    return np.random.default_rng([104729, *[int(s) & 0x7FFFFFFF for s in seed]])


def pattern(name, n, bits, rng):
    qmax = 2 ** bits - 1
    g = rng.standard_normal(n)
    if name == "gauss":
        x = 0.7 * g + 0.1
    elif name == "gelu":                          # post-GELU: the mass piles up just above the minimum, -0.17
        x = 0.5 * g * (1.0 + np.tanh(0.7978845608 * (g + 0.044715 * g ** 3)))
    elif name == "const":
        x = np.full(n, 0.7310586)
    elif name == "dups":                          # 1 + n / 8 distinct values: every run boundary falls between blocks of duplicates
        x = (0.5 * rng.standard_normal(1 + n // 8))[rng.integers(0, 1 + n // 8, n)]
    elif name == "zeros":
        x = np.where(np.arange(n) % 3 == 0, 0.0, np.where(np.arange(n) % 3 == 1, -0.0, 0.3 * g))
    elif name == "offset":                        # S2 - 2 c S1 + n c^2 cancels twelve digits
        x = 1000.0 + 0.01 * g
    elif name == "outlier":
        x = 0.2 * g
        x[n // 2] = 2000.0
    elif name == "ties":                          # (k + 0.5) s, k from TIE_SPAN below level -qmax to TIE_SPAN above level qmax
        k = np.arange(n) % (2 * (qmax + TIE_SPAN)) - (qmax + TIE_SPAN)
        x = (k + 0.5) * TIE_S
    elif name == "denorm":                        # fp32 denormals of both signs among ordinary values
        x = np.where(np.arange(n) % 2 == 0, 0.4 * g, rng.integers(-(1 << 23) + 1, 1 << 23, n) * 2.0 ** -149)
    else:
        raise KeyError(name)
    x = x.astype(np.float32)
    rng.shuffle(x)
    return x


def candidates(x, bits, P, rng, zmode="mixed"):
    """-> (scale [P], zp [P]) fp32 for one segment.  The specials come first, most telling first, so that P = 1 scores the integral
    in-range candidate, P = 2 adds a non-integral one, and P >= 20 holds them all."""
    qmax = 2 ** bits - 1
    x64 = x.astype(np.float64)
    lo, hi = float(np.nanmin(x64)), float(np.nanmax(x64))
    span = hi - lo if hi > lo else max(abs(hi), 2.0 ** -100)
    base = span / qmax
    z0 = float(np.clip(np.rint(-lo / base), 0, qmax))
    top = float(np.ceil(max(abs(lo), abs(hi)) / base)) + 3.0
    sp = [
        (base, z0), (base * 1.03, z0 + 0.37),                                # integral / non-integral, in range
        (base, 0.0), (base, qmax), (base, -3.0), (base, qmax + 2.0),         # both ends, and outside [0, qmax] on both sides
        (base, -2.5), (base, qmax + 1.25),                                   # ... non-integral
        (TIE_S, float(qmax // 2)), (TIE_S, 0.0), (TIE_S, float(qmax)),       # the planted ties, clamping on either side of them
        (TIE_S * (1 + 2.0 ** -23), 0.0), (TIE_S * (1 - 2.0 ** -24), 0.0),    # one ulp off the ties' scale: the quotients sit one ulp
        (TIE_S * (1 + 2.0 ** -23), float(qmax // 2)), (TIE_S * (1 - 2.0 ** -24), float(qmax // 2)),   # off k + 0.5
        (1.5e-38, z0),                                                       # x / s overflows to +-inf
        (1e30 * max(1.0, abs(lo), abs(hi)), float(qmax // 2)),               # every element on level 0
        (base, -top), (base, qmax + top),                                    # every element clamps low / high
        (base * 0.5, z0 + 0.5), (base * 2.0, z0),
    ]
    s = np.empty(P)
    z = np.empty(P)
    for p in range(P):
        if p < len(sp):
            s[p], z[p] = sp[p]
        else:
            s[p] = base * (0.5 + 1.5 * rng.random())
            z[p] = float(rng.integers(0, qmax + 1)) + (0.37 if p % 7 == 0 else 0.0)
    if zmode == "int":
        z = np.rint(z)
    elif zmode == "frac":
        z = np.floor(z) + 0.37
    return s.astype(np.float32), z.astype(np.float32)


class Case:
    def __init__(self, id, S, n, P, bits, layout="seg", I=None, first=0, zmode="mixed", only=None, grid=None, stats=True):
        self.id, self.S, self.n, self.P, self.bits, self.layout, self.zmode = id, S, n, P, bits, layout, zmode
        self.first, self.only, self.grid, self.stats = first, only, grid, stats
        self.I = {"w": n, "cw": S, "pt": I, "seg": None}[layout]
        self.rows = {"w": S, "cw": n, "pt": None if I is None else n // I, "seg": None}[layout]
        assert layout != "pt" or (S == 1 and n % I == 0)
        self.norm = 1.0 / n if layout == "w" else 0.01

    def pattern_of(self, s):
        return self.only if self.only else PATTERNS[(self.first + s) % len(PATTERNS)]

    def __repr__(self):
        return self.id


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> (x [S, n], scale [P, S], zp [P, S]) fp32, a function of the case alone"""
    if case.grid == "ties":
        return tie_grid(case)
    rng = _rng(case.S, case.n, case.P, case.bits, case.first)
    x = np.stack([pattern(case.pattern_of(s), case.n, case.bits, rng) for s in range(case.S)])
    if case.grid is not None:
        return (x,) + search_grid(case, x)
    sz = [candidates(x[s], case.bits, case.P, rng, case.zmode) for s in range(case.S)]
    scale = np.stack([a for a, _ in sz], axis=1)
    zp = np.stack([b for _, b in sz], axis=1)
    for t in (x, scale, zp):
        t.setflags(write=False)
    return x, scale, zp


TIE_ULPS = tuple(range(-6, 7))
TIE_BASES = (0.125, 0.1, 0.3, 0.7, 0.0123, 0.0371, 0.0519, 0.0933, 0.171, 0.233, 0.417, 0.583, 0.829, 1.37, 2.71, 5.3)
TIE_K0 = 192                                     # the planted levels: the top quarter, where a level off by one costs most


def tie_grid(case):
    """-> (x, scale, zp) of the unclamped tie case.  Segment c holds fl32((k + 0.5) s_c), k = TIE_K0 .. qmax - 1, for its own base scale
    s_c = fl32(TIE_BASES[c]); its candidates are z = 0 with the 13 fp32 neighbours s_c (1 + j 2^-23), j = -6 .. 6.  The exact quotient
    x / s of every element is then k + 0.5 to within a few ulps, on either side and on the tie itself, so a quotient formed as a
    product with an approximate reciprocal (relative error up to ~2^-22) falls on the other side for a good share of them; the level
    then differs by one and (x - c)^2 by about 8 (k + 0.5) |eta| of itself, eta = the quotient's relative distance from the tie.  No
    element clamps, so such terms are the whole score."""
    qmax = 2 ** case.bits - 1
    rng = _rng(case.S, case.n, 77)
    assert case.S <= len(TIE_BASES) and case.P == len(TIE_ULPS)
    xs, sc = [], []
    for c in range(case.S):
        s0 = np.float32(TIE_BASES[c])
        x = ((TIE_K0 + np.arange(case.n) % (qmax - TIE_K0) + 0.5) * float(s0)).astype(np.float32)
        rng.shuffle(x)
        xs.append(x)
        sc.append(np.asarray([float(s0) * (1.0 + j * 2.0 ** -23) for j in TIE_ULPS], np.float32))
    return np.stack(xs), np.stack(sc, axis=1), np.zeros((case.P, case.S), np.float32)


def search_grid(case, x):
    """the grids the searches themselves start from: oracle.adalog_oracle.weight_candidates / activation_candidates"""
    import torch
    from oracle import adalog_oracle as O
    xt = torch.from_numpy(x)
    if case.grid == "w":
        sc, zp = O.weight_candidates(xt.view(1, case.S, case.n), case.bits)          # [P, 1, S, 1]
        return sc.reshape(sc.shape[0], case.S).numpy(), zp.reshape(zp.shape[0], case.S).float().numpy()
    x3 = (xt.t() if case.layout == "cw" else xt.view(case.rows, case.I)).reshape(1, case.rows, case.I).contiguous()
    sc, zp = O.activation_candidates(x3, case.bits, case.layout == "cw")             # [C, P]
    return sc.t().contiguous().numpy(), zp.t().contiguous().float().numpy()


@functools.lru_cache(maxsize=None)
def reference(case):
    x, scale, zp = inputs(case)
    return R.score_segments(x, scale, zp, case.bits, case.norm, stats=case.stats)


def act_view(case, x):
    """the [rows, I] tensor k_score_a_self reads for a "cw" / "pt" case"""
    return np.ascontiguousarray(x.T) if case.layout == "cw" else x.reshape(case.rows, case.I)


# ------------------------------------------------------------------------------------------------ the sorted route's own shapes
# 25 candidates x 9 segments = 225 pairs: never a multiple of the 256 / G groups of a workgroup except at 8 bits (one group), so the
# last workgroup of every other width holds dead groups; all nine patterns, every special candidate, every width k_score_sorted is
# instantiated for
SORTED_BITS = tuple(Case(f"bits{b}_P25_S9_n777", 9, 777, 25, b) for b in range(1, 9))
SORTED_PAIRS = (
    Case("P5_S3_b4", 3, 600, 5, 4, first=3), Case("P5_S3_b7", 3, 600, 5, 7, first=6),       # 15 pairs: off 16 / off 2
    Case("P128_S1_b4", 1, 900, 128, 4), Case("P128_S1_b7", 1, 900, 128, 7, first=7),        # on a multiple of both
    Case("P1_S9_b5", 9, 333, 1, 5), Case("P300_S2_b4", 2, 500, 300, 4, first=1),            # no 256-candidate limit here
)
# prefix-build edges: the totals entry (i0 + 4 == n against i0 + e <= n), one block against two, one element
SORTED_N = tuple(Case(f"n{n}_S2_P21_b4", 2, n, 21, 4, first=0 if n % 2 else 5) for n in (1, 3, 4, 5, 1023, 1024, 1025, 4096))
# nb = 258 blocks: two chunks of k_sp_blockscan's carry loop and a ragged last block; gauss and the large offset
SORTED_CARRY = Case("carry_n263169_S2_P4_b4", 2, 262144 + 1025, 4, 4, first=0, only=None)
SORTED_CARRY_OFFSET = Case("carry_offset_n263169_S1_P4_b6", 1, 262144 + 1025, 4, 6, only="offset")
# nb = 514: a THIRD chunk, the first whose carry is a sum of two chunk totals (after one chunk `c += t` and `c = t` are the same)
SORTED_CARRY3 = Case("carry3_n525313_S1_P4_b4", 1, 2 * 262144 + 1025, 4, 4, only="gauss")
# as many segments as the entry point takes (65 535: one grid row each), eight elements long
MAX_SEGMENTS = 65535
SORTED_MANY = Case("many_S65535_n8_P2_b3", MAX_SEGMENTS, 8, 2, 3, stats=True)
SORTED_CASES = SORTED_BITS + SORTED_PAIRS + SORTED_N
SORTED_BIG = (SORTED_CARRY, SORTED_CARRY_OFFSET, SORTED_CARRY3, SORTED_MANY)

# ------------------------------------------------------------------------------------------------ k_score_a_self
# rows: below one slab, one row short of / exactly / one row past a slab, two slabs, three slabs and a row.  I: one channel, one short
# of / exactly / one past the 64-channel block, two blocks and two channels.  Layout, zero-point kind (all integral: the fast path
# wherever the slab is full; all non-integral: the slow path; mixed: both in one launch), candidate count (the LDS double buffer
# alternates on candidate parity) and width cycle so that each value meets each row count and each channel count.
_A_ROWS, _A_I = (1, 127, 128, 129, 256, 385), (1, 63, 64, 65, 130)


def _act_cases():
    out = []
    for a, rows in enumerate(_A_ROWS):
        for b, I in enumerate(_A_I):
            k = a * len(_A_I) + b
            layout = ("cw", "pt")[(a + b) % 2]
            zmode = ("int", "frac", "mixed")[(a + 2 * b) % 3]
            P = (1, 2, 128, 21)[(2 * a + b) % 4]
            if P == 128 and rows * I > 20000:
                P = 40                                       # (keeps the reference of the largest shapes under a second)
            bits = (4, 8, 3, 6)[k % 4]
            cid = f"{layout}_r{rows}_I{I}_P{P}_b{bits}_{zmode}"
            if layout == "cw":
                out.append(Case(cid, I, rows, P, bits, "cw", first=k, zmode=zmode))
            else:
                out.append(Case(cid, 1, rows * I, P, bits, "pt", I=I, first=k, zmode=zmode, only=("gauss", "ties", "gelu")[k % 3]))
    return tuple(out)


ACT_CASES = _act_cases() + (
    # the planted ties under integral zero points at 8 bits, whole slabs: every element goes through the fast path's tie zone
    Case("cw_ties_r256_I3_P21_b8_int", 3, 256, 21, 8, "cw", zmode="int", only="ties"),
    # ... and with no clamped element to drown them: scales one to six ulps either side of the ties' own
    Case("cw_ties_in_r256_I16_P13_b8", 16, 256, 13, 8, "cw", zmode="int", grid="ties", only="ties_in"),
    Case("pt_r256_I130_P128_b4_int", 1, 256 * 130, 128, 4, "pt", I=130, zmode="int", only="gauss"),     # per tensor, I > 64, P = 128
    Case("cw_r129_I65_P128_b4_mixed", 65, 129, 128, 4, "cw", zmode="mixed"),
)
# ------------------------------------------------------------------------------------------------ k_score_w_self
W_CASES = tuple(Case(f"w_r{rows}_I{I}_P{P}_b{bits}", rows, I, P, bits, "w", first=f)
                for rows, I, P, bits, f in ((1, 1, 1, 4, 0), (7, 1, 255, 3, 0), (1, 5, 256, 4, 3), (7, 5, 1, 8, 0),
                                            (1, 192, 255, 6, 7), (7, 192, 256, 4, 0), (1, 4096, 256, 4, 5), (7, 4096, 255, 8, 2)))
W_REFUSED_P = 257
W_REFUSED_I = (160 * 1024 - 1024) // 4 + 1                   # one element past k_score_w_self's LDS staging limit

# ------------------------------------------------------------------------------------------------ the searches' own grids
GRID_CASES = (
    Case("grid_w_r64_I192_b4", 64, 192, 128, 4, "w", grid="w", only="gauss"),
    Case("grid_w_r5_I192_b6", 5, 192, 128, 6, "w", grid="w"),
    Case("grid_cw_r394_I96_b4", 96, 394, 128, 4, "cw", grid="a", only="gauss"),
    Case("grid_cw_r197_I9_b6", 9, 197, 128, 6, "cw", grid="a"),
    Case("grid_pt_r394_I96_b4", 1, 394 * 96, 128, 4, "pt", I=96, grid="a", only="gelu"),
)

ALL_SMALL = SORTED_CASES + ACT_CASES + W_CASES + GRID_CASES


def accepts(route, case):
    if route == "sorted":
        return True
    if route == "act":
        return case.layout in ("cw", "pt")
    return case.layout == "w" and case.P <= 256


# ------------------------------------------------------------------------------------------------ NaN
# (case, segment, position): the NaN sits in a full slab (row 5 of 256 + 3 rows) and in the partial one (row 257)
NAN_ACT = Case("nan_cw_r259_I5_P8_b4", 5, 259, 8, 4, "cw", zmode="mixed", only="gauss")
NAN_PT = Case("nan_pt_r259_I5_P8_b4", 1, 259 * 5, 8, 4, "pt", I=5, zmode="mixed", only="gauss")
NAN_W = Case("nan_w_r5_I259_P8_b4", 5, 259, 8, 4, "w", only="gauss")
NAN_ROWS = (5, 257)
NAN_SEG = 2
