"""The case table of the BRECQ autograd-route tests (tests/test_brecq_grads_cpu.py, tests/test_gpu_brecq_grads.py): the smallest
shapes that reach every branch of adalog_amd/train_mm.py and of ops.gemm_f32x3_ok, the route each one must take (``native``: the
product runs on csrc/brecq_gemm.hip; otherwise train_mm hands it to the library GEMM), its fp32 inputs and -- computed once per
case and shared, never modified -- its fp64 reference (tests/brecq_grad_reference.py).
"""
import functools
from typing import NamedTuple, Optional, Tuple

import torch

from tests import brecq_grad_reference as R


# ------------------------------------------------------------------------------------------------- linear / quant_linear
class LinearCase(NamedTuple):
    id: str
    M: int
    K: int
    N: int
    bias: bool
    addend: Optional[str]          # None | "fused" (fp32, the result's shape) | "fp64" | "bcast" ([N]): the last two do not qualify
    native: bool                   # what train_mm._usable must decide
    why: str


_SHAPES = [
    # id, M, K, N, bias, native, why
    ("197x64x48_b", 197, 64, 48, True, True, "bias fused, N % 16 == 0, odd M"),
    ("130x36x20_b", 130, 36, 20, True, False, "bias with N % 16 != 0: _usable is false"),
    ("130x36x20", 130, 36, 20, False, True, "no bias: native with N off a multiple of 16"),
    ("33x1000x16_b", 33, 1000, 16, True, True, "long K"),
    ("1x64x64_b", 1, 64, 64, True, True, "M = 1"),
    ("70x38x32_b", 70, 38, 32, True, False, "K % 4 != 0: rows not 16-byte aligned, falls back"),
    ("394x384x96_b", 394, 384, 96, True, True, "dL/dw (96 x 384 over K = 394) is split along K"),
]

LINEAR_CASES = [LinearCase(i, m, k, n, b, None, nat, why) for (i, m, k, n, b, nat, why) in _SHAPES] + [
    LinearCase("197x64x48_b+add", 197, 64, 48, True, "fused", True, "addend inside the product's launch"),
    LinearCase("394x384x96_b+add", 394, 384, 96, True, "fused", True, "addend, leading dims [2, 197]"),
    LinearCase("130x36x20+add", 130, 36, 20, False, "fused", True, "addend, N off 16, no bias"),
    LinearCase("70x38x32_b+add", 70, 38, 32, True, "fused", False, "addend on the library route"),
    LinearCase("130x36x20+add64", 130, 36, 20, False, "fp64", True, "fp64 addend: added behind the product"),
    LinearCase("197x64x48_b+addN", 197, 64, 48, True, "bcast", True, "broadcast [N] addend: added behind the product"),
]


class QuantCase(NamedTuple):
    id: str
    M: int
    K: int
    N: int
    bias: bool
    bits: int
    z: str                         # "zero" | "max" (2^bits - 1) | "mid"
    addend: bool
    native: bool
    why: str


def _zp(bits, kind):
    return {"zero": 0.0, "max": float(2 ** bits - 1), "mid": float(2 ** (bits - 1) - 1)}[kind]


QUANT_CASES = [QuantCase(i + "_a4", m, k, n, b, 4, "mid", False, nat, why) for (i, m, k, n, b, nat, why) in _SHAPES] + [
    QuantCase(f"130x36x20_a{bits}_z{z}", 130, 36, 20, False, bits, z, False, True,
              "n_bits = 8 is not fused: quantiser, then the general product" if bits == 8 else "fused integer activation")
    for bits in (3, 4, 6, 8) for z in ("zero", "max", "mid")] + [
    QuantCase("197x64x48_b_a6+add", 197, 64, 48, True, 6, "mid", True, True, "addend behind the fused product"),
    QuantCase("394x384x96_b_a8+add", 394, 384, 96, True, 8, "mid", True, True, "addend through linear() (8 bits: not fused)"),
]

# which leaves require a gradient: every needs_input_grad arm of _QuantLinearFn.backward / _LinearFn.backward
GRAD_SUBSETS = {"x": ("x",), "s": ("s",), "w": ("w",), "all": ("x", "s", "w", "b")}
SUBSET_CASE = "197x64x48_b_a4"


def _lead(M):
    return (2, M // 2) if M % 2 == 0 else (M,)


def _seed(text):
    return sum((i + 1) * ord(c) for i, c in enumerate(text)) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def linear_inputs(case: LinearCase):
    g = R.gen(_seed("linear" + case.id))
    lead = _lead(case.M)
    d = {"x": torch.randn(*lead, case.K, generator=g), "w": torch.randn(case.N, case.K, generator=g) * 0.3,
         "b": torch.randn(case.N, generator=g) if case.bias else None, "gy": torch.randn(*lead, case.N, generator=g), "addend": None}
    if case.addend == "fused":
        d["addend"] = torch.randn(*lead, case.N, generator=g)
    elif case.addend == "fp64":
        d["addend"] = torch.randn(*lead, case.N, generator=g, dtype=torch.float64)
    elif case.addend == "bcast":
        d["addend"] = torch.randn(case.N, generator=g)
    return d


@functools.lru_cache(maxsize=None)
def quant_inputs(case: QuantCase):
    g = R.gen(_seed("quant" + case.id))
    lead = _lead(case.M)
    s, z = torch.tensor([0.11]), torch.tensor([_zp(case.bits, case.z)])
    x, k = R.off_tie_input((*lead, case.K), s, z, case.bits, g)
    return {"x": x, "k": k, "s": s, "z": z, "bits": case.bits, "w": torch.randn(case.N, case.K, generator=g) * 0.3,
            "b": torch.randn(case.N, generator=g) if case.bias else None, "gy": torch.randn(*lead, case.N, generator=g),
            "addend": torch.randn(*lead, case.N, generator=g) if case.addend else None}


@functools.lru_cache(maxsize=None)
def linear_reference(case: LinearCase):
    d = linear_inputs(case)
    return R.linear(d["x"], d["w"], d["b"], d["addend"], d["gy"])


@functools.lru_cache(maxsize=None)
def quant_reference(case: QuantCase):
    d = quant_inputs(case)
    return R.quant_linear(d["x"], d["s"], d["z"], d["bits"], d["w"], d["b"], d["gy"], d["addend"])


# ---------------------------------------------------------------------------------------------------------------- matmul
class MatmulCase(NamedTuple):
    id: str
    dims: Tuple[int, ...]          # (B, H, N, D), or (G, N, D)
    form: str
    native: bool                   # what the fits() logic of train_mm.matmul must decide (after its contiguous copies)
    copies: bool                   # fits() is false for the operands as given: the contiguous-copy branch runs


# forms: the operands handed to train_mm.matmul, built from the contiguous leaves a, b
#   qk           a [.., N, D] @ b.transpose(-1, -2), b = k [.., N, D]: the gradient must land on k in k's own order
#   pv           a [.., N, N] @ b, b = v [.., N, D], the result merged (4-D) -- heads_last off
#   pv_hl        the same with heads_last on: the result is written as [B, N, H, D] storage, the gradient arrives through the view
#   qk_strided   qk with a read through a last-dim stride of 2: the kernel cannot read it in place
#   pv_strided   pv_hl with b (v) read through a last-dim stride of 2
#   qk_bcast     qk with one k shared by the whole batch (leading shapes differ): library route
#   qk_offset    qk with a starting 4 bytes off a 16-byte boundary: no copy can fix that, library route
MATMUL_FORMS = {"qk": (True, False), "pv": (True, False), "pv_hl": (True, False), "qk_strided": (True, True), "pv_strided": (True, True),
                "qk_bcast": (False, False), "qk_offset": (False, True)}
_MM_DIMS = [(2, 3, 197, 64), (3, 4, 49, 32), (2, 3, 70, 20), (4, 33, 16)]
MATMUL_CASES = [MatmulCase("x".join(map(str, dims)) + "_" + form, dims, form, *MATMUL_FORMS[form])
                for dims in _MM_DIMS for form in ("qk", "pv", "pv_hl", "qk_strided")] + [
    MatmulCase("3x4x49x32_pv_strided", (3, 4, 49, 32), "pv_strided", *MATMUL_FORMS["pv_strided"]),
    MatmulCase("4x33x16_qk_bcast", (4, 33, 16), "qk_bcast", *MATMUL_FORMS["qk_bcast"]),
    MatmulCase("2x3x70x20_qk_offset", (2, 3, 70, 20), "qk_offset", *MATMUL_FORMS["qk_offset"]),
]


def matmul_merges(case: MatmulCase):
    """softmax.v of an attention block: the 4-D result passes through transpose(1, 2).reshape(B, N, H * D)."""
    return case.form.startswith("pv") and len(case.dims) == 4


@functools.lru_cache(maxsize=None)
def matmul_inputs(case: MatmulCase):
    g = R.gen(_seed("matmul" + case.id))
    *lead, N, D = case.dims
    if case.form.startswith("qk"):
        a = torch.randn(*lead, N, D, generator=g)
        b = torch.randn(*((1,) if case.form == "qk_bcast" else lead), N, D, generator=g)
        gy = torch.randn(*lead, N, N, generator=g)
    else:
        a = torch.softmax(torch.randn(*lead, N, N, generator=g) * 2, -1)
        b = torch.randn(*lead, N, D, generator=g)
        gy = torch.randn(lead[0], N, lead[1] * D, generator=g) if matmul_merges(case) else torch.randn(*lead, N, D, generator=g)
    return {"a": a, "b": b, "gy": gy}


@functools.lru_cache(maxsize=None)
def matmul_reference(case: MatmulCase):
    d = matmul_inputs(case)
    return R.matmul(d["a"], d["b"], case.form.startswith("qk"), matmul_merges(case), d["gy"])


# ------------------------------------------------------------------------------------------------------- attention chain
class AttnCase(NamedTuple):
    id: str
    B: int
    N: int
    H: int
    D: int
    per_head: bool
    bits: Tuple[int, int, int]


ATTN_CASES = [AttnCase("2x197x3x64_tensor", 2, 197, 3, 64, False, (4, 6, 4)),
              AttnCase("3x49x4x32_head", 3, 49, 4, 32, True, (6, 4, 8))]


@functools.lru_cache(maxsize=None)
def attention_inputs(case: AttnCase):
    g = R.gen(_seed("attn" + case.id))
    B, N, H, D = case.B, case.N, case.H, case.D
    n = H if case.per_head else 1
    scales, zps, parts, ks = [], [], [], []
    for p, bits in enumerate(case.bits):
        # |x_sim| <~ 1.2: logits of a few units, a softmax that is neither flat nor one-hot
        s = (2.0 / 2 ** bits) * (1 + 0.125 * torch.arange(n, dtype=torch.float32) + 0.0625 * p)
        z = float(2 ** (bits - 1)) + (torch.arange(n) % 3 - 1).float()
        x, k = R.off_tie_input((B, H, N, D), s.reshape(1, -1, 1, 1), z.reshape(1, -1, 1, 1), bits, g)
        scales.append(s.reshape(1, n, 1, 1)); zps.append(z.reshape(1, n, 1, 1)); parts.append(x); ks.append(k)
    x = torch.stack(parts, 0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * H * D).contiguous()
    return {"x": x, "k": ks, "parts": parts, "scales": scales, "zps": zps, "bits": case.bits, "mul": D ** -0.5,
            "gy": torch.randn(B, N, H * D, generator=g)}


@functools.lru_cache(maxsize=None)
def attention_reference(case: AttnCase):
    d = attention_inputs(case)
    return R.attention(d["x"], case.H, d["scales"], d["zps"], d["bits"], d["mul"], d["gy"])
