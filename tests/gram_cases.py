"""The case tables of the Gram-form search tests (tests/test_gram_cases_cpu.py, tests/test_gpu_gram_edges.py): seeded, deterministic
fp32 inputs at the shapes, bit widths and planted values where csrc/gram.hip and csrc/gram_act.hip branch.

Weight search.  k_gram_score's grid is min(blocks, WPC x CUs) workgroups (blocks = O P / 32; WPC = 2, or 1 at K = 768), so on the 256
CUs of an MI355X a workgroup gets MORE than one block only from 513 blocks (257 at K = 768), and a full pass of 4 CB blocks (CB = 4
up to K = 192, else 2) only from 512 x 4 CB: the cases marked ``big`` have up to 1025 output rows for that and no other reason; their
references are evaluated on the device.  The comments give blocks per workgroup as low | high for that grid.
"""
import functools
import zlib
from typing import NamedTuple

import torch

from tests import gram_reference as R


def gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) & 0x7FFFFFFF)


# ---------------------------------------------------------------------------------------------------------------- weight search
class WCase(NamedTuple):
    id: str
    K: int
    T: int
    O: int
    P: int
    a_bits: int
    w_bits: int
    bias: bool
    kind: str = "rand"             # rand | sat | sat_alt | satx (saturated activation, random weights) | expo
    big: bool = False
    reuse: bool = False            # also: a second step from the same state, and the first one repeated


def _w(K, T, O, P, a, w, bias, kind="rand", big=False, reuse=False, tag=""):
    return WCase(f"{tag or kind}_K{K}_T{T}_O{O}_P{P}_a{a}w{w}{'_b' if bias else ''}", K, T, O, P, a, w, bias, kind, big, reuse)


W_SHAPES = [
    # (a) every instantiated NJ; both GRP (w_bits <= 4 | > 4) at each
    _w(32, 1, 1, 32, 4, 4, False),                      # one block, one token, one row
    _w(32, 9000, 8, 64, 4, 6, True),                    # r_nchunk = 2, several token splits summed
    _w(32, 128, 1023, 256, 4, 4, True, big=True),       # 15 | 16 of 4 CB = 16: nbw = 4, 4, 4, 3 and the full pass
    _w(32, 127, 1025, 256, 3, 6, False, big=True),      # 16 | 17: a full pass, then a tail of one
    _w(64, 49, 2, 32, 3, 5, True),                      # 2 blocks
    _w(64, 127, 7, 96, 6, 3, False),                    # 21 blocks, P = 96
    _w(96, 128, 3, 32, 4, 4, True),                     # 3 blocks
    _w(96, 129, 200, 256, 5, 6, False),                 # 3 | 4: thin passes, nbw = 1, 1, 1, 0
    _w(128, 1000, 4, 32, 4, 2, True),                   # NJ = 4, 4 blocks
    _w(128, 64, 5, 128, 2, 6, False),
    _w(192, 127, 672, 256, 4, 4, True, big=True),       # 10 | 11: nbw = 3, 3, 2, 2 and 3, 3, 3, 2
    _w(192, 128, 1, 64, 6, 6, False),
    _w(256, 129, 192, 128, 4, 4, True, reuse=True),     # NJ = 8: 1 | 2 -> GRAM_COOP(1), GRAM_COOP(2)
    _w(256, 49, 200, 256, 3, 6, False),                 # 3 | 4 > CB: nbw = 1, 1, 1, 0 / 1, 1, 1, 1
    _w(256, 128, 511, 256, 4, 5, True, big=True),       # 7 | 8 of 4 CB = 8: one fewer, exactly
    _w(256, 128, 513, 256, 4, 4, False, big=True),      # 8 | 9: a full pass, then a cooperative tail of one
    _w(384, 1000, 1, 32, 4, 4, True),                   # NJ = 12
    _w(384, 127, 192, 128, 6, 6, False, reuse=True),    # 1 | 2, cooperative
    _w(384, 64, 513, 256, 4, 3, True, big=True),        # 8 | 9
    _w(512, 128, 2, 64, 4, 4, True),                    # NJ = 16 (no cooperative pass)
    _w(512, 129, 200, 256, 6, 6, False),                # 3 | 4
    _w(512, 64, 513, 256, 4, 5, True, big=True),        # 8 | 9
    _w(768, 1, 1, 32, 4, 4, False),                     # NJ = 24: one workgroup per CU
    _w(768, 127, 96, 128, 6, 6, True, reuse=True),      # 384 blocks on 256 workgroups: 1 | 2, cooperative
    _w(768, 128, 200, 256, 4, 5, False),                # 6 | 7: nbw = 2, 2, 1, 1 / 2, 2, 2, 1
    _w(768, 64, 255, 256, 4, 4, True, big=True),        # 7 | 8
    _w(768, 64, 257, 256, 3, 6, False, big=True),       # 8 | 9
]

W_BITS = [
    _w(128, 200, 5, 64, 2, 2, True, tag="bits"), _w(128, 200, 5, 64, 2, 7, False, tag="bits"), _w(128, 200, 5, 64, 7, 2, True, tag="bits"),
    _w(128, 200, 5, 64, 3, 5, False, tag="bits"), _w(128, 200, 5, 64, 5, 3, True, tag="bits"), _w(256, 200, 5, 64, 7, 7, True, tag="bits"),
    _w(768, 200, 5, 64, 6, 6, False, tag="bits"),
]
W_REJECTED = [(200, 5, 128, 4, 8, 64),                 # (T, O, K, a_bits, w_bits, P): 8-bit weights
              (128, 4, 384, 7, 7, 64), (128, 4, 512, 7, 7, 64)]       # 7-bit weights past K = 256: four row-dot products can pass 2^31

# (c) the largest K adalog_gram_supported admits per weight width; T = 128 of a saturated 7-bit activation: G = 0x1F8080 everywhere
W_SAT = [_w(K, 128, 4, 96, 7, w, True, kind) for kind in ("sat", "sat_alt") for K, w in ((768, 4), (768, 6), (256, 7))]

# (d) the limb-count switches of g_limbs (recomputed from the formula in the CPU tier), G = T qmax^2 exactly
W_LIMBS = [_w(32, T, 4, 32, a, 4, False, "satx") for a in (2, 4, 7) for pair in R.limb_switches(a, 40000) for T in pair]

W_EXPO = [_w(64, 100, 12, 32, 4, 4, True, "expo"), _w(256, 100, 12, 32, 4, 6, True, "expo")]

W_CASES = W_SHAPES + W_BITS + W_SAT + W_LIMBS + W_EXPO

# the columns of an ``expo`` case: (column, what max |raw_out - bias| is)
EXPO_COLUMNS = {0: "pow2", 1: "pow2_minus_ulp", 2: "smallest_normal", 3: "denormal", 4: "zero", 5: "low_limbs_only", 6: "loud_2^40"}


def _tie_cands(P):
    return P // 3, (2 * P) // 3


@functools.lru_cache(maxsize=None)
def weight_inputs(case):
    """dict: x [T, K], sa, za, W [O, K], sc / zp [P, O], ref [T, O] (raw_out), bias [O] or None, norm."""
    g = gen("w/" + case.id)
    T, O, K, P = case.T, case.O, case.K, case.P
    qa, qw = 2 ** case.a_bits - 1, 2 ** case.w_bits - 1
    b = torch.randn(O, generator=g) * 0.1 if case.bias else None
    if case.kind in ("sat", "sat_alt"):
        x = torch.full((T, K), 1.0e4)
        sa, za = torch.tensor([1.0]), torch.tensor([0.0])
        o_, k_ = torch.arange(O).view(O, 1), torch.arange(K).view(1, K)
        sign = 1.0 - 2.0 * ((o_ + (k_ if case.kind == "sat_alt" else 0)) % 2).float()
        W = (sign * 1.0e3).expand(O, K).contiguous()
        sc = (0.01 * torch.linspace(0.9, 1.1, P)).view(P, 1).expand(P, O).contiguous()
        # candidates in three groups: zp = 0 (rows +qmax | 0), zp = qmax (0 | -qmax), zp in the middle (qmax - z | -z)
        zp = torch.tensor([0.0, float(qw), float((qw + 1) // 2)])[torch.arange(P) % 3].view(P, 1).expand(P, O).contiguous()
        ref = 0.01 * qa * qw * K * 0.5 * (1.0 + 0.3 * torch.randn(T, O, generator=g))
        if b is not None:
            ref = ref + b
        return dict(x=x, sa=sa, za=za, W=W, sc=sc, zp=zp, ref=ref, bias=b, norm=1.0 / T)
    W = torch.randn(O, K, generator=g) * 0.05
    w_lo, w_hi = W.min(1).values, W.max(1).values
    sc = ((w_hi - w_lo) / qw).view(1, O) * torch.linspace(0.6, 1.2, P).view(P, 1)
    zp = torch.round(-w_lo.view(1, O) / sc).clamp(0, qw)
    p1, p2 = _tie_cands(P)
    W[:, 5] = sc[p1] * 2.5                                  # exact ties of candidate p1 (and near-ties of its neighbours)
    W[:, 9] = sc[p2] * -1.5
    if case.kind == "satx":
        x = torch.full((T, K), 1.0e4)
        sa, za = torch.tensor([1.0]), torch.tensor([0.0])
        xq = torch.full((T, K), float(qa))
    else:
        x = torch.randn(T, K, generator=g)
        x[:, : max(1, K // 8)] *= 3.0
        sa = torch.tensor([x.abs().max().item() * 1.2 / qa])
        # the zero point is rounded to nearest-even before use: a tie (3 bits: 3.5 -> 4, 5 bits: 15.5 -> 16) and a plain fraction
        za = torch.tensor([float(2 ** (case.a_bits - 1) - 1) + {3: 0.5, 5: 0.5, 6: 0.3}.get(case.a_bits, 0.0)])
        xq = x
    ref = torch.nn.functional.linear(xq, W, b)
    ref = ref + 0.05 * ref.abs().mean() * torch.randn(T, O, generator=g)
    if O > 3 and case.kind != "expo":
        ref[:, 3] *= 40.0                                   # a loud output column: the per-column fixed-point exponent
    if case.kind == "expo":
        assert b is not None and O >= 12
        r = ref - b                                         # columns of r = raw_out - bias; bias is dropped where r must be exact

        def column(j, top, others=1.0):
            t_ = int(r[:, j].abs().argmax())
            col = r[:, j] / r[t_, j].abs() * (top * others)
            col[t_] = top
            r[:, j] = col
            b[j] = 0.0

        column(0, 8.0)
        column(1, 8.0 - 2.0 ** -21)                         # one ulp below 2^3
        column(2, 2.0 ** -126)                              # the smallest normal; every other entry a denormal
        column(3, 2.0 ** -140)
        column(5, 3.0, 2.0 ** -20)                          # the other entries survive only in the low limbs
        column(6, 2.0 ** 40 * 1.37)
        ref = r + b
        ref[:, 4] = b[4]                                    # raw_out == bias: r = 0 exactly
    return dict(x=x, sa=sa, za=za, W=W, sc=sc, zp=zp, ref=ref, bias=b, norm=1.0 / max(1, T // 4))


def weight_blocks(case, cus=256):
    """(blocks, workgroups) of k_gram_score's launch on a device of ``cus`` CUs."""
    nblk = case.O * case.P // 32
    wpc = 1 if case.K == 768 else 2
    return nblk, min(nblk, wpc * cus)


# sharded builds (g): (id, K, O, a_bits, w_bits, shard token counts, equal)
class SCase(NamedTuple):
    id: str
    K: int
    O: int
    a_bits: int
    w_bits: int
    shards: tuple
    equal: bool                    # True: S0 adds in the one-call build's order


S_CASES = [
    SCase("chunk_boundary", 32, 8, 4, 4, (8192, 300), True),
    SCase("limbs_2_2_to_3", 64, 6, 4, 4, (100, 100), False),
    SCase("short_shard", 96, 5, 6, 6, (300, 77), False),
]


def shard_case(s):
    return _w(s.K, sum(s.shards), s.O, 64, s.a_bits, s.w_bits, True, tag="shard")


# ---------------------------------------------------------------------------------------------------------------- activation search
class ACase(NamedTuple):
    id: str
    K: int
    T: int
    O: int
    P: int
    a_bits: int
    w_bits: int
    bias: bool
    kind: str = "rand"     # rand | runs | const | zeros | ties | clamp | clamp_neg | wsat | wzero | rowbias
    big: bool = False


def _a(K, T, O, P, a, w, bias, kind="rand", big=False):
    return ACase(f"{kind}_K{K}_T{T}_O{O}_P{P}_a{a}w{w}{'_b' if bias else ''}", K, T, O, P, a, w, bias, kind, big)


A_CASES = [
    # (a) every NJ of ga_nj_ok; T around the 32-token chunk and the 128-token pad
    _a(32, 1, 3, 1, 4, 4, False), _a(32, 31, 40, 32, 3, 3, True), _a(64, 32, 20, 32, 4, 4, True), _a(96, 33, 50, 32, 6, 6, False),
    _a(128, 127, 30, 32, 4, 4, True), _a(192, 128, 64, 32, 4, 6, False), _a(256, 129, 40, 32, 6, 4, True), _a(384, 33, 100, 32, 4, 4, False),
    _a(384, 200, 50, 1, 4, 4, True),                     # P = 1: as many token splits as chunks -- one chunk per (role, split)
    _a(512, 33, 100, 32, 4, 4, True),                    # two quad roles + one 8 x 8 rect; O < 2 K
    _a(512, 64, 1100, 16, 6, 6, False, big=True),        # ... O > 2 K
    _a(512, 200, 60, 2, 4, 4, True),                     # one chunk per role and split
    _a(768, 31, 100, 32, 4, 4, False),                   # two quad roles + two rect roles; O < 2 K
    _a(768, 64, 1600, 16, 6, 6, True, big=True),         # ... O > 2 K
    _a(768, 129, 60, 2, 3, 3, True),
    # (b) candidate counts
    _a(64, 100, 20, 1, 4, 4, True), _a(64, 100, 20, 2, 4, 4, False), _a(64, 100, 20, 33, 4, 4, True), _a(64, 100, 20, 100, 6, 6, False),
    _a(64, 100, 20, 128, 3, 3, True), _a(64, 100, 20, 256, 4, 4, False),
    # (c) bit widths
    _a(96, 150, 30, 32, 2, 7, True), _a(96, 150, 30, 32, 7, 2, False), _a(96, 150, 30, 32, 3, 5, True), _a(96, 150, 30, 32, 5, 3, False),
    _a(96, 150, 30, 32, 2, 2, True), _a(96, 150, 30, 32, 7, 7, False),
    # (d) sort and prefix edges
    _a(64, 100, 16, 64, 4, 4, True, "runs"), _a(64, 100, 16, 64, 4, 4, False, "const"), _a(64, 100, 16, 64, 4, 4, True, "zeros"),
    _a(64, 100, 16, 64, 4, 4, True, "ties"), _a(64, 100, 16, 64, 6, 6, False, "ties"), _a(64, 100, 16, 63, 4, 4, True, "clamp"),
    _a(64, 100, 16, 63, 3, 3, False, "clamp_neg"),
    # (e) weights
    _a(64, 100, 16, 32, 4, 7, True, "wsat"), _a(64, 100, 16, 32, 4, 4, True, "wzero"), _a(64, 100, 16, 32, 4, 4, True, "rowbias"),
]


@functools.lru_cache(maxsize=None)
def act_inputs(case):
    """dict: x [T, K], W [O, K], sw / zw [O], sc / zp [P], ref [T, O] (raw_out), bias, norm."""
    g = gen("a/" + case.id)
    T, O, K, P = case.T, case.O, case.K, case.P
    qa, qw = 2 ** case.a_bits - 1, 2 ** case.w_bits - 1
    x = torch.randn(T, K, generator=g)
    x[:, : max(1, K // 8)] *= 3.0
    W = torch.randn(O, K, generator=g) * 0.05
    b = torch.randn(O, generator=g) * 0.1 if case.bias else None
    if case.kind == "wsat":                                 # every quantised weight at an end of its range: H at its largest
        W = torch.where(torch.rand(O, K, generator=g) < 0.5, -1.0, 1.0) * 10.0
        sw, zw = torch.full((O,), 0.01), torch.full((O,), float((qw + 1) // 2))
        zw[::3] = 0.0
        zw[1::3] = float(qw)
    else:
        if case.kind == "wzero":
            W[3] = 0.0
        w_lo, w_hi = W.min(1).values, W.max(1).values
        sw = ((w_hi - w_lo) / qw).clamp(min=1e-4)
        zw = torch.round(-w_lo / sw).clamp(0, qw)
    if case.kind == "runs":                                 # five distinct values in long runs
        x = torch.tensor([-1.5, -0.25, 0.0, 0.75, 2.0])[torch.randint(0, 5, (T, K), generator=g)]
    elif case.kind == "const":
        x = torch.full((T, K), 0.8125)
    elif case.kind == "zeros":
        pick = torch.randint(0, 4, (T, K), generator=g)
        x = torch.where(pick == 0, torch.tensor(0.0), torch.where(pick == 1, torch.tensor(-0.0), x))
    elif case.kind == "clamp":
        x = x.abs() + 0.1
    elif case.kind == "clamp_neg":
        x = -x.abs() - 0.1
    amax = max(x.abs().max().item(), 1e-3)
    lin = torch.linspace(0.5, 1.1, P) if P > 1 else torch.tensor([0.8])
    sc = (2 * amax / qa) * lin
    zp = torch.round(torch.linspace(qa / 2 - 2, qa / 2 + 2, P) if P > 1 else torch.tensor([qa / 2])).clamp(0, qa)
    if case.kind in ("clamp", "clamp_neg"):
        third = P // 3
        sc[:third] = 1.0e-6 * torch.linspace(1.0, 2.0, third)            # every element clamps to one end of the grid
        sc[third:2 * third] = 1.0e4 * torch.linspace(1.0, 2.0, third)    # every element in the bin of zero
    if case.kind == "ties":
        # values exactly on rounding ties (k + 0.5) s_p of several candidates, and the fp32 neighbours of those values
        flat = x.view(-1)
        i = 0
        for p_ in range(0, P, max(1, P // 8)):
            for k_ in (-2.5, -0.5, 0.5, 1.5, 3.5):
                v = (sc[p_] * k_).reshape(())
                for val in (v, torch.nextafter(v, torch.tensor(10.0)), torch.nextafter(v, torch.tensor(-10.0))):
                    flat[(i * 37) % flat.numel()] = val
                    i += 1
    elif case.kind == "rand" and T * K > 40 and P > 20:
        x[5 % T, 3] = (sc[P // 7] * 2.5).item()
        x[7 % T, 1] = (sc[(5 * P) // 7] * -1.5).item()
    ref = torch.nn.functional.linear(x, W, b)
    ref = ref + 0.05 * ref.abs().mean().clamp(min=1e-3) * torch.randn(T, O, generator=g)
    if case.kind == "rowbias":
        ref[T // 2] = b                                     # a token row of raw_out equal to the bias: r = 0, exponent 0
    return dict(x=x, W=W, sw=sw, zw=zw, sc=sc, zp=zp, ref=ref, bias=b, norm=1.0 / (max(1, T // 4) * O))
