"""fp64 reference of the packed-candidate scoring GEMM (csrc/gemm_score.hip, adalog_gemm_score) with the terms a PER-SCORE error bar
needs (tests/test_gemm_cases_cpu.py, tests/test_gpu_gemm_edges.py; the cases are tests/gemm_cases.py's).

``terms`` is a second, independent statement of what tests/cpu_backend._gemm_score specifies -- it does not call it:
    out[c, g, m, n] = D * (sa * sa_mul * sb) [* row_scale[m] + row_bias[m]] + bias,   D = sum_k A[., g, m, k] B[., g, (n, c), k]
    e = ref - out,   score = -norm * sum e^2   over the rows, the images (g // gmod) and, unless kept, the heads (g % gmod) / columns
and returns per score, besides ``score``:  S = sum e^2,  T1 = sum |e| a,  T2 = sum a^2  with, per element,
    a = |D alpha rs| + |rb| + |beta| + |ref|   (+ the share of an inexact fp32 accumulation, see ``bar``).
Everything is torch fp64 on the CPU; operands are read as stored (int8 / fp8 / bf16 / fp32 values are exact in fp64).
"""
import torch

F64 = torch.float64
U = 2.0 ** -24
TINY32 = 2.0 ** -149                                   # the spacing of fp32 denormals: a score that underflows

I8, BF16, F32, FP8, BF16_FP8 = 0, 1, 2, 3, 4


class Par:
    """an epilogue parameter: fp32 tensor and its (candidate, head, column) element strides -- ops.Strided / cpu_backend.Strided"""
    def __init__(self, t, c=0, g=0, n=0):
        self.t, self.c, self.g, self.n = t, int(c), int(g), int(n)

    def at(self, C, G, gmod, N):
        """[C, G, 1, N] fp64"""
        flat = self.t.reshape(-1).double()
        ci = torch.arange(C).view(C, 1, 1) * self.c
        gi = (torch.arange(G) % gmod).view(1, G, 1) * self.g
        ni = torch.arange(N).view(1, 1, N) * self.n
        return flat[ci + gi + ni].view(C, G, 1, N)


def _operand(X, C, G, rows):
    """[C | 1, G | 1, rows, Kp] stored operand -> [C, G, rows, Kp] fp64"""
    Xd = X.to(torch.float32).double() if X.dtype not in (torch.float32, torch.float64) else X.double()
    return Xd.expand(C if Xd.shape[0] > 1 else Xd.shape[0], G if Xd.shape[1] > 1 else Xd.shape[1], rows, Xd.shape[-1])


def products(A, B, M, N, C, G, ref_div):
    """D and sum_k |a_k b_k|, both [C, G, M, N] fp64.  ref_div = P > 1: B is [1, G, N * P, Kp] with column (n, c) at n * P + c."""
    if ref_div > 1:
        B = B.reshape(G, N, ref_div, B.shape[-1]).permute(2, 0, 1, 3)                # [P, G, N, Kp]
    Ad, Bd = _operand(A, C, G, M), _operand(B, C, G, N)
    D = torch.matmul(Ad, Bd.transpose(-1, -2))
    Dabs = torch.matmul(Ad.abs(), Bd.abs().transpose(-1, -2))
    return D.expand(C, G, M, N), Dabs.expand(C, G, M, N)


def out_tensor(A, B, M, N, C, G, gmod, sa, sb, bias, sa_mul=1.0, ref_div=1, row_scale=None, row_bias=None):
    """the fp64 product with its epilogue, [C, G, M, N], and the pieces ``terms`` needs"""
    D, Dabs = products(A, B, M, N, C, G, ref_div)
    mul32 = float(torch.tensor(sa_mul, dtype=torch.float32))                          # sa_mul crosses the C ABI as a float
    alpha = sa.at(C, G, gmod, 1) * mul32 * sb.at(C, G, gmod, N)                        # [C, G, 1, N]
    rs = row_scale.double().view(1, 1, M, 1) if row_scale is not None else None
    rb = row_bias.double().view(1, 1, M, 1) if (row_scale is not None and row_bias is not None) else None
    lin = D * alpha
    scale_abs = alpha.abs()
    if rs is not None:
        lin = lin * rs
        scale_abs = scale_abs * rs.abs()
    out = lin
    if rb is not None:
        out = out + rb
    beta = bias.at(C, G, gmod, N) if bias is not None else None
    if beta is not None:
        out = out + beta
    return dict(out=out, lin=lin, Dabs=Dabs, scale_abs=scale_abs, rb=rb, beta=beta)


def ref_view(ref, G, M, N, ref_transposed):
    """the reference as [1, G, M, N] fp64 from its stored layout ([G, N, M] when transposed)"""
    r = ref.reshape(G, N, M).transpose(1, 2) if ref_transposed else ref.reshape(G, M, N)
    return r.double().unsqueeze(0)


def reduce_scores(x, C, G, gmod, M, N, keep_h, keep_n):
    """[C, G, M, N] -> [C, (gmod if keep_h) * (N if keep_n)]: sums over rows, images and what is not kept"""
    x = x.reshape(C, G // gmod, gmod, M, N).sum(dim=3).sum(dim=1)                      # [C, gmod, N]
    if not keep_n:
        x = x.sum(dim=2, keepdim=True)
    if not keep_h:
        x = x.sum(dim=1, keepdim=True)
    return x.reshape(C, -1)


def acc_roundings(dtype, k_valid):
    """fp32 roundings of the MFMA accumulation, as a multiple of u sum_k |a_k b_k|: 0 where every partial sum is exact (int8: int32
    accumulator; fp8 operands of the cases are integers in [-15, 15] and 225 K < 2^24), K for bf16 rows or columns (products of two
    8-bit significands are exact in fp32, every addition may round), 2 K for fp32 operands (the product rounds as well)."""
    return {I8: 0, FP8: 0, BF16: k_valid, BF16_FP8: k_valid, F32: 2 * k_valid}[dtype]


def terms(dtype, A, B, M, N, C, G, gmod, ref, sa, sb, bias, keep_h, keep_n, norm, sa_mul=1.0, ref_div=1, ref_transposed=False,
          row_scale=None, row_bias=None, k_valid=None, k_count=1):
    """dict of fp64: score, S, T1, T2 [C_eff, cols];  e2 [C_eff, G, M, N], out, lin = D alpha rs, r (the reference as [1, G, M, N]) and ``reduce``
    (for the mutants of the sensitivity check).
    ``k_count``: the roundings of the route (``roundings``): the accumulation share of a is (acc_roundings / k_count) sum|a_k b_k| |alpha rs|,
    so that k_count u a bounds every rounding between the accumulator and e."""
    Ce = ref_div if ref_div > 1 else C
    o = out_tensor(A, B, M, N, Ce, G, gmod, sa, sb, bias, sa_mul, ref_div, row_scale, row_bias)
    r = ref_view(ref, G, M, N, ref_transposed)
    e = r - o["out"]
    a = o["lin"].abs() + r.abs()
    if o["rb"] is not None:
        a = a + o["rb"].abs()
    if o["beta"] is not None:
        a = a + o["beta"].abs()
    kv = A.shape[-1] if k_valid is None else k_valid
    na = acc_roundings(dtype, kv)
    if na:
        a = a + (na / k_count) * o["Dabs"] * o["scale_abs"]
    red = lambda x: reduce_scores(x.expand(Ce, G, M, N), Ce, G, gmod, M, N, keep_h, keep_n)
    e2 = (e * e).expand(Ce, G, M, N)
    S = red(e2)
    return dict(score=-norm * S, S=S, T1=red(e.abs() * a), T2=red(a * a), e2=e2, reduce=red, out=o["out"], lin=o["lin"], r=r)


# ---------------------------------------------------------------------------------------------------------------- the bar
def roundings(route, dtype, rows, bias):
    """k of ``bar``: fp32 roundings between the accumulator and e = ref - out, the same count in every epilogue:
      alpha           sa * sa_mul, * sb                                                                                      2
      (float) acc     int32 accumulator only (int8 operands; exact below 2^24, the ext cases go above)                       1
      D alpha, - ref  one multiplication and one addition (a single fma where the compiler contracts them: one rounding less)    2
      rows            * row_scale, and row_bias: added to the product or subtracted from the staged reference                   2
      bias            added to the product, or subtracted from the staged reference (shared by the candidates) or the error      1
    read from
      k_gemm_score                 gemm_k_basic.inc:100-101 (alpha, beta), :111 / :129 (cvt, *, +), :114 / :132 (ref - o)
      k_gemm_cand_glds             gemm_k_basic.inc:211-212 / :310-311, :243-245 / :333-335, :252 / :336   (epilogue2 / epilogue_lds)
      k_gemm_stream, bf16xfp8      gemm_k_stream.inc:299 ((ref - rb) - cb), :308 (alpha), :346-351 (cvt, * rs, - beta, t * na + r)
      k_gemm_slab, slab128         gemm_k_slab.inc:294 (alpha), :420-421 (r - rb - bias), :426-429 (cvt, * rs, fma, - column bias)
      k_gemm_grpw / win / grpk     gemm_k_grp.inc:1221 / :953 / :322 (alpha), :1312-1314 / :1033-1035 / :388-390 (cvt, t * na + r)
      k_gemm_grpk8 / grpk8t / winb gemm_k_grp.inc:529 / :748 / :1101 (alpha) and the same t * na + r (no conversion: fp32 accumulator)
    The group and window kernels take neither row vectors nor a bias."""
    del route
    return 2 + (1 if dtype == I8 else 0) + 2 + (2 if rows else 0) + (1 if bias != "none" else 0)


def chain(route, M, ncols, P):
    """L of ``bar``: the longest chain of fp32 additions a sum of e^2 goes through before it is widened to fp64 (in the kernel, or in
    gemm_finish.inc, whose sums are all fp64: k_finish :42, ordered_sum :65, k_finish_rows :114, k_finish_wgacc :161).
      k_gemm_score      2 x 16 per lane (gemm_k_basic.inc:115 / :133), lane pair :138, two row waves :148, tile total :154-156 (1 + 6)   41
      k_gemm_cand_glds  TM x 16 <= 32 per lane (:253 / :337), lane pair :264 / :345, two row waves :715, tile total :720-722 (2 + 6)      42
      k_gemm_stream     per half of the packed pair RI x 4 x 2 <= 32 (gemm_k_stream.inc:353), halves :405, lane pair :406, row waves :414  35
      k_gemm_slab       16 per 32-row unit (gemm_k_slab.inc:430) over the <= R = 8 units of a workgroup's range (gemm_score.hip:146: R = 8
                        while a launch has <= 8 units per CU -- the cases have <= 512 units, 64 CUs), lane pair :457 / :274, 8 waves :465        137
      k_gemm_grpw       per half 8 per row block and reference column (gemm_k_grp.inc:1315) over <= ceil(M / 32) blocks and <= ncols
                        columns of a chunk, halves :1329, lane pair :1330
      k_gemm_win        the same over the group's ncols columns (:1036, :1051-1052)
      k_gemm_grpk, grpk8, grpk8t   8 per reference column over a chunk's <= ncols columns for the wave's one row block (:391, :416-417)
      k_gemm_winb       as k_gemm_win"""
    if route == "k_gemm_score":
        return 41
    if route == "k_gemm_cand_glds":
        return 42
    if route.startswith("k_gemm_stream"):
        return 35
    if route.startswith("k_gemm_slab"):
        return 137
    rb = (M + 31) // 32
    if route.startswith("k_gemm_grpw") or route.startswith("k_gemm_win"):
        return 8 * rb * ncols + 2
    if route.startswith("k_gemm_grpk"):
        return 8 * ncols + 2
    raise KeyError(route)


def bar(t, norm, route, dtype, M, ncols, P, rows=False, bias="none"):
    """Per score:  norm (2 k u T1 + k^2 u^2 T2 + (L + 2) u S) + 2^-24 |score| + 2^-149,   u = 2^-24.

    With e' = e + d, |d| <= k u a (k roundings, each of a quantity no larger than a): e'^2 - e^2 = 2 e d + d^2, summed: the first two
    terms.  The square rounds once, the sum of squares goes through a chain of L fp32 additions (then fp64, whose 2^-53 the + 2
    covers with the square): (L + 2) u S.  The score is rounded to fp32 once.  k: ``roundings``; L: ``chain`` -- both counted from the
    kernel source, the lines are in their docstrings.  Where the MFMA accumulates in fp32 and the operands are not integers (bf16 AdaLog
    values, fp32), ``terms`` has added the accumulation term (K | 2 K) u sum_k |a_k b_k| |alpha rs| to a's rounding share
    (``acc_roundings``); it is added for every bf16 / fp32 case, also where the operands happen to be integers.
    The kernel's output never sets or scales this bar."""
    k, L = roundings(route, dtype, rows, bias), chain(route, M, ncols, P)
    return norm * (2 * k * U * t["T1"] + k * k * U * U * t["T2"] + (L + 2) * U * t["S"]) + U * t["score"].abs() + TINY32


def to_f32(score):
    return score.float()


def ulp32(x):
    """spacing of fp32 at |x| (x fp32 tensor)"""
    ax = x.abs().double().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 23)
