"""The case table of the BRECQ training-kernel tests (tests/test_brecq_kernels_cpu.py, tests/test_gpu_brecq_kernels.py): seeded,
deterministic fp32 inputs at the shapes, bit widths and planted edge values where the kernels of csrc/brecq.hip branch, and -- computed
once per case and shared, never modified -- the fp64 reference of each (tests/brecq_kernel_reference.py).
"""
import functools
import zlib
from typing import NamedTuple, Optional, Tuple

import torch

from oracle import adalog_oracle as O
from tests import brecq_kernel_reference as R


def gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) & 0x7FFFFFFF)


# ---------------------------------------------------------------------------------------------------------------- uniform
class UniformCase(NamedTuple):
    id: str
    xshape: Tuple[int, ...]
    sshape: Tuple[int, ...]        # (1,): per tensor (the kernel's last block finishes); otherwise per channel (k_param_grad_finish)
    bits: int
    sym: bool
    z: str                         # "int" | "half_even" (k + 0.5, k even) | "half_odd"
    gy: str                        # "randn" | "zero"
    planted: bool                  # s a power of two and the edge / tie elements of plant_uniform() at the front of every channel


UNIFORM_CASES = [
    UniformCase("tensor_1_b4", (1,), (1,), 4, False, "int", "randn", False),                      # inner = 1
    UniformCase("tensor_3_b6", (3,), (1,), 6, False, "half_odd", "randn", False),                 # inner = 3, one block
    UniformCase("tensor_100003_b3_plant", (100003,), (1,), 3, False, "half_even", "randn", True),  # scalar path, 49 blocks, last-block finish
    UniformCase("tensor_28800_b8_sym_plant", (6, 50, 96), (1,), 8, True, "int", "randn", True),   # vector path, 15 blocks
    UniformCase("tensor_28800_b4_gy0", (6, 50, 96), (1,), 4, False, "int", "zero", False),
    UniformCase("channel_48x13_b4_plant", (48, 13), (48, 1), 4, False, "half_odd", "randn", True),
    UniformCase("channel_40x260_b6_sym_plant", (40, 260), (40, 1), 6, True, "int", "randn", True),
    UniformCase("channel_33x64_b8_plant", (33, 64), (33, 1), 8, False, "half_even", "randn", True),
    UniformCase("heads_3x5x1x4_b3", (3, 5, 1, 4), (1, 5, 1, 1), 3, False, "int", "randn", False),
    UniformCase("heads_4x6x20x16_b4_sym", (4, 6, 20, 16), (1, 6, 1, 1), 4, True, "int", "randn", False),
    UniformCase("heads_1025x4x1x3_b4_plant", (1025, 4, 1, 3), (1, 4, 1, 1), 4, False, "int", "randn", True),   # 4100 rows > gridDim.y = 4096, scalar
    UniformCase("rows_3x16x64_b4", (3, 16, 64), (3, 16, 1), 4, False, "int", "randn", False),
    UniformCase("rows_4100x1x4_b6_sym", (4100, 1, 4), (4100, 1, 1), 6, True, "int", "randn", False),            # the row loop on the vector path
    UniformCase("rows_7x3x13_b8_plant", (7, 3, 13), (7, 3, 1), 8, False, "half_odd", "randn", True),
]


def plant_uniform(bits, sym, zr):
    """(r, t) pairs: t on qmin - 1, qmin, qmax, qmax + 1 and ties r = k + 0.5 with k even and odd (inside the range)."""
    L = 2 ** (bits - 1)
    qmin, qmax = (-L, L - 1) if sym else (0, 2 * L - 1)
    rs = [float(t - zr) for t in (qmin - 1, qmin, qmax, qmax + 1)]
    mid = (qmin + qmax) // 2 - int(zr)
    k_even, k_odd = mid - (mid % 2), mid - (mid % 2) + 1
    rs += [k_even + 0.5, k_odd + 0.5, qmin - zr - 0.5, qmax - zr + 0.5]        # the last two: ties that decide inside / outside
    return rs


@functools.lru_cache(maxsize=None)
def _uniform_inputs(case):
    g = gen("uniform/" + case.id)
    L = 2 ** (case.bits - 1)
    nlev = 2 * L
    x = torch.randn(case.xshape, generator=g)
    if case.planted:
        s = torch.exp2(-torch.randint(2, 5, case.sshape, generator=g).float())
    else:
        s = torch.rand(case.sshape, generator=g) * 0.5 + 0.5
    s = s * (4.5 / nlev)                                  # x / s spans about twice the range: both clamp sides are populated
    if case.planted:
        s = torch.exp2(torch.round(torch.log2(s)))
    z = None
    if not case.sym:
        z = torch.randint(L - 2, L + 2, case.sshape, generator=g).float()
        if case.z != "int":
            z = 2 * torch.floor(z / 2) + (0.5 if case.z == "half_even" else 1.5)
    gy = torch.randn(case.xshape, generator=g) if case.gy == "randn" else torch.zeros(case.xshape)
    plants = []
    if case.planted:
        n_ch, inner = _layout(case)
        xf = x.reshape(-1, inner)
        sf, zf = s.reshape(-1), (None if z is None else z.reshape(-1))
        for row in range(min(xf.shape[0], 2 * n_ch)):
            ch = row % n_ch
            zr = 0.0 if zf is None else float(torch.round(zf[ch]))
            rs = plant_uniform(case.bits, case.sym, zr)
            for j, r in enumerate(rs[:inner]):
                col = (j + row) % inner if inner >= len(rs) else j
                xf[row, col] = r * float(sf[ch])
                plants.append((row * inner + col, r, ch))
        x = xf.reshape(case.xshape)
    return {"x": x, "s": s, "z": z, "gy": gy, "plants": plants}


def _layout(case):
    from adalog_amd.ops import broadcast_layout
    return broadcast_layout(case.xshape, case.sshape)


def uniform_inputs(case):
    return _uniform_inputs(case)


@functools.lru_cache(maxsize=None)
def uniform_reference(case):
    i = _uniform_inputs(case)
    return R.uniform_backward(i["gy"], i["x"], i["s"], i["z"], case.bits, case.sym)


# uniform_int: per tensor, asymmetric, n % 4 in {0, 1, 2, 3}, the planted edges of the uniform case
class UniformIntCase(NamedTuple):
    id: str
    n: int
    bits: int
    z: str


UNIFORM_INT_CASES = [UniformIntCase(f"n{n}_b{b}_{z}", n, b, z) for n, b, z in
                     [(16, 4, "int"), (17, 3, "half_even"), (18, 6, "half_odd"), (19, 8, "int"), (4100, 4, "half_odd"), (100003, 8, "half_even")]]


@functools.lru_cache(maxsize=None)
def uniform_int_inputs(case):
    g = gen("uniform_int/" + case.id)
    L = 2 ** (case.bits - 1)
    s = torch.tensor([2.0 ** -3])
    z = torch.tensor([float(L - 1)])
    if case.z != "int":
        z = 2 * torch.floor(z / 2) + (0.5 if case.z == "half_even" else 1.5)
    x = torch.randn(case.n, generator=g) * (L * float(s))
    rs = plant_uniform(case.bits, False, float(torch.round(z)))
    for j, r in enumerate(rs[:case.n]):
        x[(case.n - 1 - j) if j < 3 else j] = r * float(s)                # the first three plants sit in the n % 4 tail
    return {"x": x, "s": s, "z": z, "rs": rs}


# ----------------------------------------------------------------------------------------------------------------- AdaLog
class LogCase(NamedTuple):
    id: str
    n: int
    q: int
    bits: int
    sub_shift: bool
    pre_gelu: bool
    shift: bool = True
    salt: int = 0                  # picks the seed: chosen so that the reference's ``near`` mask meets the cap (test_brecq_kernels_cpu.py)


LOG_CASES = [
    LogCase("n4096_q23_b4_sub", 4096, 23, 4, True, False),
    LogCase("n4097_q37_b3_noshift", 4097, 37, 3, False, False, False),
    LogCase("n25603_q90_b6_sub", 25603, 90, 6, True, False),
    LogCase("n4097_q23_b6_pre", 4097, 23, 6, False, True),
    LogCase("n4096_q37_b4_pre_sub", 4096, 37, 4, True, True),
    LogCase("n263_q90_b3_pre", 263, 90, 3, False, True),
    LogCase("n300003_q37_b4_noshift", 300003, 37, 4, False, False, False),   # 1024 blocks and more than one turn of the grid-stride loop
]


@functools.lru_cache(maxsize=None)
def log_inputs(case):
    """Post-GELU activations (pre_gelu: the GELU's own input), the GELU shift, s = 0.8 of the largest value (so some u > 1).  Planted
    at the front (as values of the quantiser's input xs = v + shift): xs <= 0, u just under 1e-15, u == 1, u > 1, a bin past the last."""
    g = gen(f"log/{case.id}/{case.salt}")
    pre = 2 * torch.randn(case.n, generator=g)
    sh = torch.tensor([O.GELU_SHIFT if case.shift else 0.0])
    act = torch.nn.functional.gelu(pre)
    s = torch.tensor([float(act.max()) * 0.8])
    s = torch.exp2(torch.round(torch.log2(s)))                       # a power of two: u == 1 can be planted exactly
    past = float(s) * 2.0 ** (-(2 ** case.bits + 1) * case.q / 37.0)       # bin 2^bits + 1
    plants = {"nonpos": -float(sh) - 0.25, "tiny": 0.5e-15 * float(s) - float(sh), "one": float(s) - float(sh),
              "above": 1.5 * float(s) - float(sh), "past": past - float(sh)}
    x = pre if case.pre_gelu else act
    where = {}
    if not case.pre_gelu:                                                 # (behind a GELU the quantiser's input cannot be planted exactly)
        for j, (name, v) in enumerate(plants.items()):
            x[j + 1] = v
            where[name] = j + 1
        if case.shift:
            where.pop("tiny")                                             # (x + shift cannot land that close to zero: it lands on xs == 0)
    gy = torch.randn(case.n, generator=g)
    return {"x": x, "s": s, "q": case.q, "shift": sh if case.shift else None, "gy": gy, "plants": where}


@functools.lru_cache(maxsize=None)
def log_reference(case):
    i = log_inputs(case)
    return R.log_backward(i["gy"], i["x"], i["s"], i["q"], case.bits, i["shift"], case.sub_shift, case.pre_gelu)


# --------------------------------------------------------------------------------------------------------------- AdaRound
ALPHA_SPECIALS = [0.0, -0.0, 2.3, -2.3, 2.5, -2.5, 30.0, -30.0, 100.0, -100.0]


class RoundCase(NamedTuple):
    id: str
    rows: int
    inner: int
    bits: int


ADAROUND_CASES = [RoundCase(f"{r}x{i}_b{b}", r, i, b) for (r, i), b in
                  zip([(1, 1), (33, 5), (32, 32), (31, 97), (100, 70)], [4, 3, 8, 4, 3])] + [RoundCase("33x5_b8", 33, 5, 8),
                                                                                            RoundCase("31x97_b8", 31, 97, 8)]


def alpha_field(n, g):
    """alpha ~ N(0, 2^2) with the special values mixed in at seeded positions (every special at least once where n allows)."""
    a = torch.randn(n, generator=g) * 2
    pos = torch.randperm(n, generator=g)
    for j in range(min(n, 3 * len(ALPHA_SPECIALS))):
        a[pos[j]] = ALPHA_SPECIALS[j % len(ALPHA_SPECIALS)]
    return a


@functools.lru_cache(maxsize=None)
def adaround_inputs(case):
    """w, per-row power-of-two s and integral z, alpha_field; planted (row 0 onwards, flat order): w / s exactly integral, and
    floor + z on -1, 0, qmax - 1, qmax each with alpha = +100 and -100 (h saturated at 1 and at 0)."""
    g = gen("adaround/" + case.id)
    qmax = 2 ** case.bits - 1
    n = case.rows * case.inner
    s = torch.exp2(-torch.randint(3, 6, (case.rows,), generator=g).float())
    z = torch.randint(qmax // 2 - 1, qmax // 2 + 2, (case.rows,), generator=g).float()
    w = (torch.randn(case.rows, case.inner, generator=g) * (qmax / 3.0)) * s.view(-1, 1)
    alpha = alpha_field(n, g).view(case.rows, case.inner)
    plants = []
    wf, af = w.view(-1), alpha.view(-1)
    combos = [(fz, a) for fz in (-1, 0, qmax - 1, qmax) for a in (100.0, -100.0)] + [(qmax // 2, None)]
    for j, (fz, a) in enumerate(combos):
        if j >= n:
            break
        row = j // case.inner
        wf[j] = (fz - float(z[row])) * float(s[row])
        if a is not None:
            af[j] = a
        plants.append((j, fz - float(z[row])))
    gy = torch.randn(case.rows, case.inner, generator=g)
    return {"w": w, "alpha": alpha, "s": s, "z": z, "gy": gy, "plants": plants}


@functools.lru_cache(maxsize=None)
def adaround_reference(case, soft):
    i = adaround_inputs(case)
    return R.adaround(i["w"], i["alpha"], i["s"], i["z"], case.bits, soft, gy=i["gy"])


# ------------------------------------------------------------------------------------------------------------- round loss
ROUND_LOSS_NS = [1, 5, 255, 256, 257, 100003]
ROUND_LOSS_BS = [20.0, 11.0, 7.3, 2.0]


@functools.lru_cache(maxsize=None)
def round_loss_alpha(n):
    return alpha_field(n, gen(f"round_loss/{n}"))


@functools.lru_cache(maxsize=None)
def round_loss_reference(n, b):
    return R.round_loss(round_loss_alpha(n), b)


MULTI_NS = [1, 5, 255, 256, 257, 1023, 1024, 1025, 4097, 3, 70, 7000, 513, 64, 30001, 100003]      # sixteen tensors in one launch


@functools.lru_cache(maxsize=None)
def multi_alphas():
    return tuple(alpha_field(n, gen(f"round_loss_multi/{t}")) for t, n in enumerate(MULTI_NS))


# --------------------------------------------------------------------------------------------------------------- rec loss
REC_LOSS_NS = [1, 2, 3, 4, 5, 1023, 1025, 100003]


@functools.lru_cache(maxsize=None)
def rec_loss_inputs(n, cancel):
    """cancel: tgt = pred + 1e-6 |pred| noise with |pred| ~ 10 (the differences are a few fp32 ulp of the operands)."""
    g = gen(f"rec_loss/{n}/{cancel}")
    pred = torch.randn(n, generator=g) * 10
    tgt = pred + 1e-6 * pred.abs() * torch.randn(n, generator=g) if cancel else torch.randn(n, generator=g) * 10
    return {"pred": pred, "tgt": tgt, "scale": 0.1 * 7.0 / max(n, 7), "gmul": torch.tensor([0.37])}


# ---------------------------------------------------------------------------------------------------------------- softmax
SOFTMAX_NS = [1, 2, 63, 64, 65, 127, 128, 129, 197, 960, 961, 1023, 1024]
SOFTMAX_ROWS = [1, 3, 4, 5, 1029]
SOFTMAX_SCALE = 0.125
SOFTMAX_TOO_WIDE = 1025                    # ops.scaled_softmax documents rows of <= 1024 values: anything wider is an error
ROW_KINDS = ["random", "random", "random", "equal", "dominant", "neg_inf"]


def softmax_rows_for(n):
    """Every width meets every row count once over the table (1029 rows only at a few widths: the reference is O(rows n))."""
    i = SOFTMAX_NS.index(n)
    rows = [SOFTMAX_ROWS[i % 4]]
    if n in (1, 65, 197, 1024):
        rows.append(1029)
    return rows


@functools.lru_cache(maxsize=None)
def softmax_inputs(rows, n):
    g = gen(f"softmax/{rows}/{n}")
    x = torch.randn(rows, n, generator=g) * 8
    kinds = [ROW_KINDS[r % len(ROW_KINDS)] for r in range(rows)]
    for r, kind in enumerate(kinds):
        if kind == "equal":
            x[r] = float(x[r, 0])
        elif kind == "dominant":                                      # +-80 after scaling around one dominant value
            x[r] = (torch.rand(n, generator=g) * 2 - 1) * (80.0 / SOFTMAX_SCALE) - 80.0 / SOFTMAX_SCALE
            x[r, (7 * r) % n] = 80.0 / SOFTMAX_SCALE
        elif kind == "neg_inf" and n > 1:
            x[r, (5 * r + 1) % n] = float("-inf")
    gy = torch.randn(rows, n, generator=g)
    return {"x": x, "gy": gy, "kinds": kinds}


# ------------------------------------------------------------------------------------------------------------------- Adam
ADAM_SIZES = [1, 255, 256, 1023, 1024, 1025, 4097]
ADAM_STEPS = [0, 1, 999, 19999]
ADAM_GRADS = ["mixed", "zero", "tiny"]
ADAM_HYPER = {"lr": 1e-3, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8}


@functools.lru_cache(maxsize=None)
def adam_inputs(grads, sixteen):
    """Non-zero m and v; gradients all zero, all 1e-20, or mixed (randn with zeros, 1e-20 and large entries)."""
    sizes = (ADAM_SIZES * 3)[:16] if sixteen else ADAM_SIZES
    g = gen(f"adam/{grads}/{sixteen}")
    out = {"p": [], "g": [], "m": [], "v": []}
    for n in sizes:
        out["p"].append(torch.randn(n, generator=g))
        out["m"].append(torch.randn(n, generator=g) * 0.1)
        out["v"].append(torch.rand(n, generator=g) * 0.01 + 1e-6)
        if grads == "zero":
            gr = torch.zeros(n)
        elif grads == "tiny":
            gr = torch.full((n,), 1e-20)
        else:
            gr = torch.randn(n, generator=g)
            gr[::5] = 0.0
            gr[1::7] = 1e-20
            gr[2::11] *= 100.0
        out["g"].append(gr)
    return out


# ------------------------------------------------------------------------------------------------------- alpha_step_multi
# adalog_alpha_step_multi (csrc/brecq.hip) gives a block 4 096 values once the launch's tensors hold 4 << 20 = 4 194 304 values
# in total, 1 024 below that; the wrapper reports no launch shape, so the threshold is stated here and both sides are run.
ALPHA_STEP_SWITCH = 4 << 20


class AlphaStepCase(NamedTuple):
    id: str
    layers: Tuple[Tuple[int, int, int], ...]      # (rows, inner, bits)
    none_gw: Optional[int]                        # index of the layer whose dL/dw_sim is None
    gmul: bool
    gate: Optional[float]
    b: float
    b_dev: bool
    lr_dev: bool
    steps: int


_SMALL = tuple((c.rows, c.inner, c.bits) for c in ADAROUND_CASES)
ALPHA_STEP_CASES = [
    AlphaStepCase("small_gmul_gate1_b20", _SMALL, 1, True, 1.0, 20.0, False, False, 2),
    AlphaStepCase("small_gmul_gate0_b7.3dev", _SMALL, None, True, 0.0, 7.3, True, True, 2),
    AlphaStepCase("small_nogmul_b2", _SMALL, 2, False, None, 2.0, False, False, 2),
    AlphaStepCase("small_gmul_nogate_b11dev", _SMALL, 0, True, None, 11.0, True, False, 2),
    AlphaStepCase("below_switch", ((4095, 1024, 4), (1, 1023, 3)), None, True, 1.0, 11.0, False, False, 1),      # 4 194 303 values: 1 024 per block
    AlphaStepCase("at_switch", ((4095, 1024, 4), (1, 1024, 3)), None, True, 1.0, 11.0, False, False, 1),         # 4 194 304 values: 4 096 per block
]
assert sum(r * i for r, i, _ in ALPHA_STEP_CASES[-2].layers) == ALPHA_STEP_SWITCH - 1
assert sum(r * i for r, i, _ in ALPHA_STEP_CASES[-1].layers) == ALPHA_STEP_SWITCH


@functools.lru_cache(maxsize=2)
def alpha_step_inputs(case):
    g = gen("alpha_step/" + case.id)
    layers = []
    for t, (rows, inner, bits) in enumerate(case.layers):
        small = next((c for c in ADAROUND_CASES if (c.rows, c.inner, c.bits) == (rows, inner, bits)), None)
        if small is not None:
            i = adaround_inputs(small)
            w, alpha, s, z = i["w"], i["alpha"], i["s"], i["z"]
        else:
            qmax = 2 ** bits - 1
            s = torch.exp2(-torch.randint(3, 6, (rows,), generator=g).float())
            z = torch.full((rows,), float(qmax // 2))
            w = (torch.randn(rows, inner, generator=g) * (qmax / 3.0)) * s.view(-1, 1)
            alpha = alpha_field(rows * inner, g).view(rows, inner)
        n = rows * inner
        layers.append({"w": w, "alpha": alpha, "s": s, "z": z, "bits": bits, "inner": inner,
                       "gw": None if case.none_gw == t else torch.randn(rows, inner, generator=g) * 0.01,
                       "m": torch.randn(n, generator=g).view(rows, inner) * 1e-3, "v": torch.rand(n, generator=g).view(rows, inner) * 1e-5 + 1e-9})
    return {"layers": layers, "gmul": torch.tensor([0.73]) if case.gmul else None,
            "gate": None if case.gate is None else torch.tensor([case.gate]), "weight": 0.01, "step0": 7.0, "lr": 1e-3,
            "beta1": 0.9, "beta2": 0.999, "eps": 1e-8}
