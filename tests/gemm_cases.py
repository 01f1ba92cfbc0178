"""Case table of the packed-candidate scoring GEMM's edge suite (tests/test_gemm_cases_cpu.py, tests/test_gpu_gemm_edges.py): one
frozen record per launch, the smallest shapes route_of / layout_of (csrc/gemm_score.hip) send to each kernel family with the default
switches, and ``inputs(case)``, which builds every tensor on the CPU from a generator seeded by the case's id.

Three layouts (``form``):
  grid   candidates in a grid dimension (C > 1, ref_div = 1): A [C, G, M, K], B [1, G, N, K], reference [G, M, N]; the candidate's
         factor is sa [C, gmod]; sb [gmod, N], bias [N]                                                   -> k_gemm_score
  plain  candidates innermost in the columns (ref_div = P), reference NOT transposed [G, M, ncols]; sb [P, ncols]     -> k_gemm_cand_glds
  cols   the same with the transposed reference [G, ncols, M]: the weight searches' parameters (sb [P, ncols], bias per column or
         per (candidate, column), row vectors) where G = 1 or the route is a streaming one, the attention searches' (sa [gmod],
         sb [P, gmod], no bias, no rows) on the group and window kernels
Kinds: ``spread`` (column factors log-uniform over three decades), ``hit`` (one planted candidate per score column whose fp64 product,
rounded to fp32, IS the reference), ``ext`` (operand extremes: int8 +-127 and fp8 +-15 with an all-aligned row and column, bf16 rows of
AdaLog values 30 x 2^-t at both ends of t, fp32 rows with full significands; with G >= 2 the last group -- the one after the ragged
rows of group G - 2 -- holds the extremes and a reference 10^3 x larger, the others operands of magnitude 1), ``nan`` (the spread data
with one NaN at the reference element of row M - 1, column ncols - 1, group G - 1: where the row and the column clamp both land).

Shapes of the issue's list that do not reach their route, and what stands in for them:
  k_gemm_grpw, gmod = 16 with G = 8     G must be a multiple of gmod (gemm_score.hip: "bad sizes"): G = 16
  k_gemm_win, gmod = 3 with G = 256     the same: G = 258
"""
import zlib
from dataclasses import dataclass

import torch

from tests import gemm_reference as R

I8, BF16, F32, FP8, BF16_FP8 = R.I8, R.BF16, R.F32, R.FP8, R.BF16_FP8
DT_NAME = {I8: "i8", BF16: "bf16", F32: "f32", FP8: "fp8", BF16_FP8: "bf16xfp8"}
ESZ = {I8: 1, BF16: 2, F32: 4, FP8: 1, BF16_FP8: 2}
TDT = {I8: torch.int8, BF16: torch.bfloat16, F32: torch.float32, FP8: torch.float8_e4m3fn}
NORM, SA_MUL = 0.01, 0.5


@dataclass(frozen=True)
class Case:
    id: str
    route: str
    dtype: int
    M: int
    ncols: int
    P: int                 # ref_div (1 in the grid form)
    K: int                 # row length of the stored operands, elements
    k_valid: int
    G: int
    gmod: int
    C: int
    keep_h: bool
    keep_n: bool
    bias: str              # none | n | cn
    rows: bool
    kind: str              # spread | hit | ext | nan
    form: str              # grid | plain | cols
    attn: bool             # cols form with the attention searches' parameters

    @property
    def cands(self):
        return self.C if self.form == "grid" else self.P

    @property
    def opt_out(self):
        """of the sensitivity check: a NaN score has no bar"""
        return self.kind == "nan"


def pad(kv, dtype, align):
    per = align // (1 if dtype in (I8, FP8) else ESZ[dtype])
    return (kv + per - 1) // per * per


CASES = []


def add(route, dtype, M, ncols, P, kv, G, gmod, kind, form="cols", C=1, keep_h=False, keep_n=False, bias="none", rows=False, align=128,
        K=None, attn=False):
    K = pad(kv, dtype, align) if K is None else K
    cid = "%s-%s-M%d-n%d-P%d-K%d-G%d.%d-%s%s%s%s-%s" % (route.split("<")[0][7:] + ("" if "<" not in route else "." + route.split("<")[1][:-1]),
                                                     DT_NAME[dtype], M, ncols, P if form != "grid" else C, kv, G, gmod, "h" if keep_h else "",
                                                     "n" if keep_n else "", "r" if rows else "", "" if bias == "none" else "b" + bias, kind)
    assert all(c.id != cid for c in CASES), cid
    CASES.append(Case(cid, route, dtype, M, ncols, P, K, kv, G, gmod, C, keep_h, keep_n, bias, rows, kind, form, attn))


KINDS = ("spread", "hit", "ext")
KEEPS = ((False, True), (True, False), (False, False), (True, True))

# ---- k_gemm_score: C > 1.  1 x 1 x 1, 33 x 17 x 5 (one ragged tile), 129 x 130 x 65 (2 x 2 tiles, one row and two columns past a tile)
for di, dt in enumerate((I8, BF16, F32)):
    for si, (M, N, kv, G, gmod) in enumerate(((1, 1, 1, 1, 1), (33, 17, 5, 4, 2), (129, 130, 65, 2, 2))):
        for ki, kind in enumerate(KINDS):
            kh, kn = KEEPS[(di + si + ki) % 4] if si < 2 else (True, True)    # (the largest shape keeps both axes: 129 elements per score)
            add("k_gemm_score", dt, M, N, 1, kv, G, gmod, kind, "grid", C=3, keep_h=kh, keep_n=kn, bias=("n", "none")[(si + ki) % 2])
add("k_gemm_score", I8, 33, 17, 1, 1100, 2, 1, "ext", "grid", C=2, keep_n=True, bias="n")        # |D| = 127^2 x 1100 > 2^24
add("k_gemm_score", I8, 129, 130, 1, 65, 2, 2, "nan", "grid", C=3, keep_h=True, keep_n=True, bias="n")

# ---- k_gemm_cand_glds: C = 1, not a streaming shape -- the reference not transposed (epilogue2), or transposed with 32 candidates
# per column (epilogue_lds).  Row tiles of 64 and 128 rows: M at 1, at and one past each; N = 3 x 128 and 5 x 32 leave the last
# 256-column tile ragged
for mi, M in enumerate((1, 64, 65, 128, 129)):
    for ki, kind in enumerate(KINDS):
        dt = (I8, BF16, F32)[(mi + ki) % 3]
        lds = (mi + ki) % 2 == 1
        add("k_gemm_cand_glds", dt, M, 5 if lds else 3, 32 if lds else 128, (40, 200, 9)[(mi + 2 * ki) % 3], 1 if mi % 2 else 2, 1, kind,
            "cols" if lds else "plain", keep_n=(mi + ki) % 3 != 0, bias=("none", "n", "cn")[(mi + ki) % 3], rows=(mi + ki) % 2 == 0)
add("k_gemm_cand_glds", I8, 65, 3, 128, 1100, 1, 1, "ext", "plain", keep_n=True)
add("k_gemm_cand_glds", I8, 129, 3, 128, 40, 2, 1, "nan", "plain", keep_n=True, bias="n", rows=True)
add("k_gemm_cand_glds", BF16, 65, 5, 32, 40, 2, 1, "nan", "cols", keep_n=True, bias="cn")

# ---- k_gemm_stream, narrow form (M < 192): 128-row tiles, M at 1 and around the tile; ncols x P leaves the last 256-column tile
# partly masked; K = 1 and one element past a 64-byte K-step
STEP = {I8: 64, FP8: 64, BF16: 32, F32: 16}
for di, dt in enumerate((I8, FP8, BF16, F32)):
    for mi, M in enumerate((1, 127, 128, 129)):
        kind = KINDS[(mi + di) % 3]
        ncols, P = ((1, 64), (5, 64), (1, 128), (5, 128), (1, 256), (5, 256))[(2 * mi + di) % 6]
        gm = (mi + di) % 4 == 3
        add("k_gemm_stream<%s>" % DT_NAME[dt], dt, M, ncols, P, 1 if (mi + di) % 2 else STEP[dt] + 1, 4 if gm else (1, 3)[mi % 2], 2 if gm else 1,
            kind, keep_h=gm, keep_n=(mi + di) % 2 == 0, bias=("none", "n", "cn")[(mi + di) % 3], rows=(mi + 2 * di) % 2 == 0)
add("k_gemm_stream<i8>", I8, 129, 5, 64, 65, 3, 1, "nan", keep_n=True, bias="n", rows=True)
add("k_gemm_stream<fp8>", FP8, 127, 5, 128, 65, 4, 2, "nan", keep_h=True)

# ---- ... wide form (pick_wide: >= 512 valid bytes of K, M >= 192): 192-row tiles at M = 192 and 257, 256-row tiles at 193 and 256;
# K the first that qualifies, and one that is no multiple of the K-step
for di, dt in enumerate((I8, FP8, BF16, F32)):
    for mi, M in enumerate((192, 193, 256, 257)):
        kind = KINDS[(mi + di + 1) % 3]
        first = 512 // ESZ[dt]
        ncols, P = ((3, 64), (5, 64), (1, 128), (3, 128), (1, 256), (3, 256))[(mi + 2 * di) % 6]
        add("k_gemm_stream<%s>" % DT_NAME[dt], dt, M, ncols, P, first if mi % 2 == 0 else first + 5 + di, (1, 2)[(mi + di) % 2], 1, kind,
            keep_n=(mi + di) % 2 == 1, bias=("n", "cn", "none")[(mi + di) % 3], rows=(mi + di) % 2 == 0)
add("k_gemm_stream<i8>", I8, 193, 3, 64, 1100, 1, 1, "ext", keep_n=True)                          # |D| > 2^24
add("k_gemm_stream<bf16>", BF16, 257, 3, 64, 261, 2, 1, "nan", keep_n=True, bias="cn")

# ---- k_gemm_slab (G = 1, 65 .. 384 bytes of K, M % 32 = 0, M >= 768).  M = 768: 24 units, the ranges of 8 end with the slab;
# M = 800 with 5 x 64 columns: 25 units per slab, the fourth range ends inside the second slab, whose last 192 columns are masked
for di, dt in enumerate((I8, FP8)):
    for si, (M, ncols, P, kv) in enumerate(((768, 1, 128, 65), (800, 5, 64, 384), (768, 1, 256, 384), (800, 1, 64, 65))):
        add("k_gemm_slab<%s>" % DT_NAME[dt], dt, M, ncols, P, kv, 1, 1, KINDS[(si + di) % 3], keep_n=(si + di) % 2 == 0,
            bias=("none", "n", "cn")[(si + di) % 3], rows=si % 2 == 1)
add("k_gemm_slab<i8>", I8, 800, 5, 64, 384, 1, 1, "nan", keep_n=True, bias="n")
# ---- k_gemm_slab128 (385 .. 768 bytes of K, 64 or 128 candidates)
for di, dt in enumerate((I8, FP8)):
    for si, (M, ncols, P, kv) in enumerate(((768, 1, 64, 385), (800, 3, 128, 768), (768, 3, 64, 768))):
        add("k_gemm_slab128<%s>" % DT_NAME[dt], dt, M, ncols, P, kv, 1, 1, KINDS[(si + di) % 3], keep_n=(si + di) % 2 == 1,
            bias=("n", "none", "cn")[(si + di) % 3], rows=si % 2 == 0)
add("k_gemm_slab128<fp8>", FP8, 800, 3, 128, 385, 1, 1, "nan", keep_n=True)

# ---- k_gemm_grpw (q.k^T searches: 129 .. 224 rows, G >= 8, one K-step, column axis summed).  The 9-column cases keep the heads so that
# a score sums few enough elements for one of them to show (sensitivity check)
for di, dt in enumerate((I8, FP8)):
    for si, (M, ncols, P, kv, G, gmod, kh) in enumerate(((129, 1, 64, 1, 8, 1, False), (131, 9, 128, 64, 8, 4, True), (224, 9, 64, 64, 16, 16, True))):
        add("k_gemm_grpw<%s>" % DT_NAME[dt], dt, M, ncols, P, kv, G, gmod, KINDS[(si + di) % 3], keep_h=kh, align=64, attn=True)
add("k_gemm_grpw<i8>", I8, 131, 9, 256, 64, 8, 4, "nan", keep_h=True, align=64, attn=True)
# ---- k_gemm_grpk (bf16, 193 .. 224 elements of K)
for si, (M, ncols, P, kv, G, gmod, kh) in enumerate(((197, 2, 64, 193, 8, 4, True), (224, 1, 128, 224, 8, 1, False), (129, 3, 256, 193, 8, 2, True))):
    add("k_gemm_grpk<bf16>", BF16, M, ncols, P, kv, G, gmod, KINDS[si], keep_h=kh, align=64, attn=True)
add("k_gemm_grpk<bf16>", BF16, 131, 2, 64, 224, 8, 4, "nan", keep_h=True, align=64, attn=True)

# ---- k_gemm_win (<= 64 rows, G >= 256, one K-step; rows of 32 bytes where K <= 32, of 64 otherwise).  64 reference columns only with
# 4 / 5 rows and the heads kept (reference cost, and the sensitivity check)
WIN = ((4, 64, 64, 1, 256, 32, True), (5, 64, 64, 33, 256, 32, True), (32, 1, 128, 32, 258, 3, False), (33, 1, 64, 64, 256, 1, False),
       (64, 1, 256, 32, 258, 3, True))
for di, dt in enumerate((I8, FP8)):
    for si, (M, ncols, P, kv, G, gmod, kh) in enumerate(WIN):
        add("k_gemm_win<%s>" % DT_NAME[dt], dt, M, ncols, P, kv, G, gmod, KINDS[(si + di) % 3], keep_h=kh, K=32 if kv <= 32 else 64, attn=True)
add("k_gemm_win<fp8>", FP8, 33, 1, 64, 33, 256, 32, "nan", keep_h=True, K=64, attn=True)

# ---- mixed operands (bf16 rows x fp8 columns): wide streaming kernel at K = 257, window kernel at K = 1 and 64, four-step group kernel
# at K = 256, its trimmed form (rows of 208 elements) at K = 193 (13 MFMAs per block) and 208 (14)
for si, (M, ncols, P, G) in enumerate(((193, 3, 128, 1), (256, 1, 64, 2), (200, 3, 128, 1))):
    add("k_gemm_stream<bf16xfp8>", BF16_FP8, M, ncols, P, 257, G, 1, KINDS[si], keep_n=si != 1, bias=("cn", "none", "n")[si], K=320)
add("k_gemm_stream<bf16xfp8>", BF16_FP8, 193, 3, 128, 257, 1, 1, "nan", keep_n=True, K=320)
for si, (M, ncols, kv, G, gmod) in enumerate(((5, 3, 1, 256, 4), (33, 1, 64, 256, 1), (64, 1, 64, 258, 3))):
    add("k_gemm_winb<bf16xfp8>", BF16_FP8, M, ncols, 128, kv, G, gmod, KINDS[si], keep_h=si != 1, K=64, attn=True)
add("k_gemm_winb<bf16xfp8>", BF16_FP8, 33, 2, 128, 64, 256, 4, "nan", keep_h=True, K=64, attn=True)
for si, (M, ncols, G, gmod) in enumerate(((197, 2, 8, 4), (129, 1, 8, 1), (224, 1, 8, 2))):
    add("k_gemm_grpk8<bf16xfp8>", BF16_FP8, M, ncols, 128, 256, G, gmod, KINDS[si], keep_h=si != 1, K=256, attn=True)
add("k_gemm_grpk8<bf16xfp8>", BF16_FP8, 131, 2, 128, 256, 8, 4, "nan", keep_h=True, K=256, attn=True)
for kv, nk in ((193, 13), (208, 14)):
    for si, (M, ncols, G, gmod) in enumerate(((197, 2, 8, 4), (129, 1, 8, 1), (224, 1, 8, 2))):
        add("k_gemm_grpk8t<%d,bf16xfp8>" % nk, BF16_FP8, M, ncols, 128, kv, G, gmod, KINDS[si], keep_h=si != 1, K=208, attn=True)
add("k_gemm_grpk8t<13,bf16xfp8>", BF16_FP8, 131, 2, 128, 193, 8, 4, "nan", keep_h=True, K=208, attn=True)

ROUTES = sorted({c.route for c in CASES})


# ---------------------------------------------------------------------------------------------------------------- inputs
def adalog_values():
    """the bf16 values an AdaLog operand of base q = 37 holds at 4 bits: 30 x 2^-t, t = 0 .. 15 -- the largest numerator of the
    table at both ends of the exponent (ops.adalog_value_lut is the packer's own table)"""
    from adalog_amd import ops
    mant37 = torch.round(30.0 * torch.exp2(-torch.arange(37.0) / 37.0))
    bits = ops.adalog_value_lut(torch.tensor([37.0]), 4, mant37)[:16, 0]
    vals = bits.to(torch.int16).view(torch.bfloat16).float()
    assert vals[0] == 30.0 and vals[15] == 30.0 * 2.0 ** -15
    return vals


def _signs(shape, gen):
    return torch.randint(0, 2, shape, generator=gen).float() * 2 - 1


def _operands(case, gen):
    """A [C | 1, G, M, K] and B [1, G, cols, K] as float values (zero past k_valid), exact in their storage types"""
    c, kv = case, case.k_valid
    cols = c.ncols * (c.P if c.form != "grid" else 1)
    ca = c.C if c.form == "grid" else 1
    ashape, bshape = (ca, c.G, c.M, kv), (1, c.G, cols, kv)
    if c.kind != "ext":
        a = torch.randint(1, 16, ashape, generator=gen).float() * _signs(ashape, gen)
        b = torch.randint(1, 16, bshape, generator=gen).float() * _signs(bshape, gen)
        if c.dtype == F32:
            a = a * 0.25
        if c.dtype == BF16_FP8:
            a = a.abs()                                           # (AdaLog values are not negative)
    else:
        top = 127.0 if c.dtype == I8 else 15.0
        big = torch.zeros(c.G, dtype=torch.bool)
        big[c.G - 1] = True                                        # the last group holds the extremes; with G = 1 it is the only one
        gsel = big.view(1, c.G, 1, 1)
        b = torch.where(gsel, torch.full(bshape, top), torch.ones(bshape)) * _signs(bshape, gen)
        if c.dtype in (I8, FP8):
            a = torch.where(gsel, torch.full(ashape, top), torch.ones(ashape)) * _signs(ashape, gen)
            a[:, c.G - 1, 0, :] = top; b[:, c.G - 1, 0, :] = top                  # all signs aligned: |D| = top^2 K at (row 0, column 0)
            a[:, c.G - 1, c.M - 1, :] = -top; b[:, c.G - 1, cols - 1, :] = top     # ... and -top^2 K at the last row and column
        elif c.dtype == F32:
            a = torch.randn(ashape, generator=gen) * torch.where(gsel, torch.tensor(1000.0), torch.tensor(1.0))     # full significands
        else:
            vals = adalog_values()
            pick = vals[torch.randint(0, 16, ashape, generator=gen)]
            ends = torch.where(torch.randint(0, 2, ashape, generator=gen) == 0, vals[0], vals[15])
            a = torch.where(gsel, torch.where(torch.rand(ashape, generator=gen) < 0.5, ends, pick), vals[15].expand(ashape))
            a[:, c.G - 1, 0, :] = vals[0]
            a[:, c.G - 1, c.M - 1, :] = vals[15]
    A = torch.zeros(ca, c.G, c.M, c.K); B = torch.zeros(1, c.G, cols, c.K)
    A[..., :kv] = a; B[..., :kv] = b
    dta = TDT[BF16 if c.dtype == BF16_FP8 else c.dtype]
    dtb = TDT[FP8 if c.dtype == BF16_FP8 else c.dtype]
    As, Bs = A.to(dta), B.to(dtb)
    assert torch.equal(As.float(), A) and torch.equal(Bs.float(), B)
    return As, Bs


def star_columns(case):
    """``hit``: the planted candidate of every reference column -- it varies with the column where the candidates' factors do (sb
    [P, ncols]) and the column axis is kept"""
    n = case.cands
    if case.keep_n and case.form != "grid" and not case.attn:
        return (7 * torch.arange(case.ncols) + 3) % n
    return torch.full((case.ncols,), 3 % n)


def _factors(case, gen):
    """the candidates' factors [cands, ncols] (one column where they do not vary with it)"""
    n = case.cands
    w = case.ncols if (case.form != "grid" and not case.attn) else 1
    if case.kind in ("spread", "nan"):
        f = 10.0 ** (-3.0 * torch.randperm(n, generator=gen).float() / max(n - 1, 1))
        f = f.view(n, 1).expand(n, w)
    elif case.kind == "hit":
        away = (1.0 + 2.0 * torch.rand(n, w, generator=gen)) * _signs((n, w), gen)      # one to three decades either way ...
        f = 10.0 ** away
        star = star_columns(case)[:w]
        f[star, torch.arange(w)] = 1.0                                                  # ... from the planted candidate's
    else:
        f = (torch.rand(n, generator=gen) * 0.5 + 0.5).view(n, 1).expand(n, w)
    return f.float()


def params(case, i, mod):
    """the epilogue parameters of a call as ``mod``.Strided (mod: ops, cpu_backend or gemm_reference with Par) -> (sa, sb, bias)"""
    S = getattr(mod, "Strided", None) or mod.Par
    c = case
    if c.form == "grid":
        sa, sb = S(i["sa"], c=c.gmod, g=1), S(i["sb"], g=c.ncols, n=1)
        b = S(i["bias"], n=1) if c.bias == "n" else None
    elif c.attn:
        sa, sb, b = S(i["sa"], g=1), S(i["sb"], c=c.gmod, g=1), None
    else:
        sa, sb = S(i["sa"]), S(i["sb"], c=c.ncols, n=1)
        b = {"none": None, "n": S(i["bias"], n=1) if c.bias == "n" else None, "cn": S(i["bias"], c=c.ncols, n=1) if c.bias == "cn" else None}[c.bias]
    return sa, sb, b


def call_args(case, i, mod, A=None, B=None, move=lambda t: t):
    """positional and keyword arguments of ``mod``.gemm_score for the case (``move``: to the device)"""
    c = case
    sa, sb, b = params(c, {k: (move(v) if torch.is_tensor(v) else v) for k, v in i.items() if k in ("sa", "sb", "bias")}, mod)
    A = move(i["A"]) if A is None else A
    B = move(i["B"]) if B is None else B
    args = (c.dtype, A, B, c.M, c.ncols, c.cands, c.G, c.gmod, move(i["ref"]), sa, sb, b, c.keep_h, c.keep_n, NORM)
    kw = dict(sa_mul=SA_MUL, ref_div=c.P if c.form != "grid" else 1, order=2, ref_transposed=c.form == "cols",
              row_scale=move(i["rs"]) if c.rows else None, row_bias=move(i["rb"]) if c.rows else None)
    return args, kw


def reference_terms(case, i, ref=None):
    c = case
    sa, sb, b = params(c, i, R)
    return R.terms(c.dtype, i["A"], i["B"], c.M, c.ncols, c.cands, c.G, c.gmod, i["ref"] if ref is None else ref, sa, sb, b, c.keep_h, c.keep_n,
                   NORM, sa_mul=SA_MUL, ref_div=c.P if c.form != "grid" else 1, ref_transposed=c.form == "cols",
                   row_scale=i["rs"] if c.rows else None, row_bias=i["rb"] if c.rows else None, k_valid=c.k_valid,
                   k_count=R.roundings(c.route, c.dtype, c.rows, c.bias))


def case_bar(case, t):
    return R.bar(t, NORM, case.route, case.dtype, case.M, case.ncols, case.P, case.rows, case.bias)


def inputs(case):
    """dict: A, B (stored types), ref (stored layout), sa, sb, bias, rs, rb, terms (gemm_reference.terms of the case), and for ``hit``
    planted [cols] (the planted candidate of every score column)."""
    c = case
    gen = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    A, B = _operands(c, gen)
    N, n_c = c.ncols, c.cands
    f = _factors(c, gen)
    if c.form == "grid":
        sa = (torch.rand(1, c.gmod, generator=gen) * 0.01 + 0.01) * f
        sb = torch.rand(c.gmod, N, generator=gen) * 0.5 + 0.5
    elif c.attn:
        sa = torch.rand(c.gmod, generator=gen) * 0.01 + 0.01
        sb = (torch.rand(1, c.gmod, generator=gen) * 0.5 + 0.5) * f
    else:
        sa = torch.rand(1, generator=gen) * 0.01 + 0.01
        sb = (torch.rand(1, N, generator=gen) * 0.5 + 0.5) * f
    i = dict(A=A, B=B, sa=sa.float().contiguous(), sb=sb.float().contiguous(), bias=None, rs=None, rb=None)
    # the size of the product at factor 1, per group: everything else is scaled to it
    D, _ = R.products(A, B, c.M, N, n_c, c.G, c.P if c.form != "grid" else 1)
    base = (D[0].double() ** 2).mean(dim=(1, 2)).sqrt() * float(sa.reshape(-1)[0]) * SA_MUL          # [G]
    base = base.clamp(min=1e-30)
    lvl = float(base[0])                                                                            # (rows and bias are shared by the groups)
    small = 0.005 if c.kind in ("spread", "nan") else 1.0
    if c.rows:
        i["rs"] = (torch.rand(c.M, generator=gen) + 0.5).float()
        i["rb"] = (torch.randn(c.M, generator=gen) * lvl * small).float()
    if c.bias == "n":
        i["bias"] = (torch.randn(N, generator=gen) * lvl * small).float()
    elif c.bias == "cn":
        i["bias"] = (torch.randn(n_c, N, generator=gen) * lvl * small).float()
    rscale = base * small
    if c.kind == "ext" and c.G >= 2:
        rscale[c.G - 1] = max(float(rscale[c.G - 1]), 1000.0 * float(rscale[:c.G - 1].max()))
    ref = (torch.randn(c.G, c.M, N, generator=gen).double() * rscale.view(c.G, 1, 1)).float()        # [G, M, N]
    # the elements the sensitivity check's mutants touch (tests/test_gemm_cases_cpu.py) are not left to chance
    ref[c.G - 1, c.M - 1, N - 1] = 2.0 * float(rscale[c.G - 1])
    ref[c.G - 1, 0, N - 1] = -2.0 * float(rscale[c.G - 1]) if c.M > 1 else ref[c.G - 1, 0, N - 1]
    store = (lambda r: r.transpose(1, 2).contiguous()) if c.form == "cols" else (lambda r: r.contiguous())
    i["ref"] = store(ref)
    if c.kind == "hit":
        # the planted candidate of every score column: it varies with the column where the column axis is kept
        cols = (c.gmod if c.keep_h else 1) * (N if c.keep_n else 1)
        star_n = star_columns(c)
        out = reference_terms(c, i)["out"]                                                          # [cands, G, M, N] fp64
        ref = out[star_n, :, :, torch.arange(N)].permute(1, 2, 0).float()                           # [G, M, N]: fp32 of the fp64 product
        i["ref"] = store(ref)
        i["planted"] = (star_n if c.keep_n else star_n[:1]).repeat(c.gmod if c.keep_h else 1)
        assert i["planted"].numel() == cols
        others = torch.ones(n_c, f.shape[1], dtype=torch.bool)
        others[star_n[:f.shape[1]], torch.arange(f.shape[1])] = False
        assert bool(((f[others] >= 10.0) | (f[others] <= 0.1)).all())
    if c.kind == "nan":
        r = i["ref"]
        if c.form == "cols":
            r[c.G - 1, N - 1, c.M - 1] = float("nan")
        else:
            r[c.G - 1, c.M - 1, N - 1] = float("nan")
    t = reference_terms(c, i)
    i["terms"] = t
    if c.kind == "spread":
        s = t["score"].abs()
        assert bool((s.amax(0) >= 1e3 * s.amin(0)).all()), (c.id, float((s.amax(0) / s.amin(0)).min()))
    if c.kind == "hit":
        assert torch.equal(t["score"].argmax(0), i["planted"]), c.id
    if c.kind == "ext" and c.dtype in (I8, FP8):
        top = 127.0 if c.dtype == I8 else 15.0
        Dm = R.products(A, B, c.M, N, n_c, c.G, c.P if c.form != "grid" else 1)[0]
        assert float(Dm.abs().max()) == top * top * c.k_valid
    return i
