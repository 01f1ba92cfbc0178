"""`-m gpu`: quant_forward of Swin against the fp64 reference (tests/qf_reference.py: the Swin section), per element.

The other Swin tests compare HIP kernels with HIP kernels (fused route against module route, the one-launch core against the three
launches it replaces); a defect common to both sides, or a wrong reading of the window attention, passes them.  Here every stage of a
Swin block -- on the module route, the fused route and the fused route with the one-launch core -- the window-core kernels on their
own, PatchMerging's reduction and the 4 x 4 patch-embedding conv are held to an independent restatement.  The bars are the
reference's: 2^-22 for int8 products, (K + 4) 2^-24 for the bf16 form, the boundary-flip allowance (with the ambiguous share capped),
plus the fp32 rounding of the bias and mask adds (qf_reference.window_core)."""
from types import SimpleNamespace

import pytest
import torch

from tests import qf_cases as QC
from tests import qf_reference as QR
from tests.test_gpu_long_seq import _report, _switches
from tests.test_qf_reference_cpu import (SWIN_BLOCKS, check_patch_merging, make_patch_embed_conv, make_patch_merging,
                                         make_swin_case)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import ops as O
    return O


def _count_calls(monkeypatch):
    from tests.test_gpu_attn_core import _count_calls as count
    return count(monkeypatch)


# ================================================================================================= 1. blocks, three routes
ROUTES = (("module", dict(QF_FUSED=False, QF_ATTN_CORE=False), dict(core=0, softmax=0, softmax_bias=0)),
          ("fused", dict(QF_FUSED=True, QF_ATTN_CORE=False), dict(core=0, softmax=0, softmax_bias=1)),
          ("fused_core", dict(QF_FUSED=True, QF_ATTN_CORE=True), dict(core=1, softmax=0, softmax_bias=0)))


@pytest.mark.parametrize("case", SWIN_BLOCKS, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_swin_block_stages_against_fp64(monkeypatch, case):
    """The CPU tier's Swin blocks and one of head dimension 32 with 32 windows (several per mask pattern), each on the module route,
    the fused route and the fused route with the one-launch core: every stage within its fp64 bar on its recorded input
    (qf_cases.run_and_check_swin_block), the ambiguous shares under the caps, the expected launches, the three outputs bit-equal."""
    calls = _count_calls(monkeypatch)
    blk, x = make_swin_case(case, DEV)
    ys = {}
    for name, switches, want in ROUTES:
        with _switches(**switches):
            calls.update(core=0, softmax=0, softmax_bias=0)
            rep = QC.run_and_check_swin_block(blk, x, fused_expected=switches["QF_FUSED"])
        ys[name] = rep.pop("y")
        _report({"case": "swin_block", "shape": list(case[:5]), "bits": case[5], "images": case[6], "route": name, **rep})
        assert calls == want, (name, calls)
        assert rep["amb_core"] < 1e-3 and rep["amb_fc2"] < 1e-2, (name, rep)
    assert torch.equal(ys["fused"], ys["module"]) and torch.equal(ys["fused_core"], ys["module"])


# ================================================================================================= 2. the window-core kernels alone
def window_core_case(res, ws, shift, bits, per_head, D=16, H=3, images=2, device="cpu"):
    """A randn qkv in window order with the planted rows of tests/test_gpu_attn_core._plant, random on-grid q / k / v quantisers at
    3 / 5 / 7 bits, a N(0, 1) bias table, the block's index and mask, a post-softmax quantiser at ``bits`` -- and stand-ins for
    matmul1 / matmul2 that carry just the parameters the reference reads.  Built on the CPU; ``device``: where the tensors end up."""
    from adalog_amd import quant_layers as Q
    from adalog_amd.utils import models as M
    from tests.test_gpu_attn_core import _plant
    blk = M.SwinTransformerBlock(D * H, (res, res), H, window_size=ws, shift_size=shift)
    N = blk.attn.window_area
    Bw = images * (res // ws) ** 2
    gen = g(41000 + res + shift + 7 * bits + D + (1 if per_head else 0))
    qkv = torch.randn(Bw, N, 3 * H * D, generator=gen) * 1.3
    _plant(qkv, Bw, N, H, D)
    table = torch.randn(blk.attn.relative_position_bias_table.shape, generator=gen)
    n = H if per_head else 1
    par = []
    for b in (3, 5, 7):
        s_, z_ = torch.rand(n, generator=gen) * 0.2 + 0.05, torch.randint(0, 2 ** b, (n,), generator=gen).float()
        par.append((s_.to(device), z_.to(device), b))
    ps = Q.PostSoftmaxAsymmetricallyBatchingQuantMatMul(bits, bits, "quant_forward", head_channel_wise=True, num_heads=H, fpcs=True,
                                                       quantizer="adalog").to(device)
    ps.A_quantizer.q.fill_(29)
    ps.A_quantizer.update_table(29)
    ps._q_host = None
    quant = [SimpleNamespace(scale=s, zero_point=z, n_bits=b) for s, z, b in par]
    m1 = SimpleNamespace(A_quantizer=quant[0], B_quantizer=quant[1], _heads=lambda: n)
    m2 = SimpleNamespace(A_quantizer=ps.A_quantizer, B_quantizer=quant[2], table_scale=ps.table_scale, _heads=lambda: n)
    mask = None if blk.attn_mask is None else blk.attn_mask.to(device)
    return SimpleNamespace(qkv=qkv.to(device), table=table.to(device), index=blk.attn.relative_position_index.to(device), mask=mask,
                           par=par, ps=ps, m1=m1, m2=m2, N=N, D=D, H=H, Bw=Bw, gmod=n, per_head=per_head, bits=bits)


def window_core_reference(c):
    """-> (scores ref, scores bar), (core ref, core bar, ambiguous fraction)"""
    q_mul = c.D ** -0.5
    return (QR.window_scores(c.qkv, c.m1, c.m2, c.H, q_mul),
            QR.window_core(c.qkv, c.m1, c.m2, c.H, c.table, c.index, c.mask, q_mul=q_mul))


# The share of elements on a boundary-flip allowance, from the reference alone on the CPU, is at most 1.4e-4 over these cases
# (two scale forms, two bit widths each; cap 1e-3).
WINDOWS = [(8, 4, 2), (14, 7, 3), (24, 12, 6), (14, 7, 0)]


@pytest.mark.parametrize("res,ws,shift", WINDOWS)
@pytest.mark.parametrize("bits", [3, 6])
@pytest.mark.parametrize("per_head", [True, False])
def test_window_core_kernels_against_fp64(ops, res, ws, shift, bits, per_head):
    """No block: attn_split_pack_ex(q_mul = D^-0.5) of a randn qkv with planted rows (a row of equal scores, rows of equal pairs, an
    image of extreme codes), then both routes of the core -- gemm_out(I8) -> softmax_bias_adalog_pack -> gemm_out(BF16, heads_last),
    and attn_core(table=, index=, mask=) -- each against qf_reference.window_core; the int8 scores against the fp64 scores."""
    from tests.test_gpu_attn_core import _one_launch, _three_launches
    c = window_core_case(res, ws, shift, bits, per_head, device=DEV)
    (s_ref, s_bar), (ref, bar, amb) = window_core_reference(c)
    qp, kp, vp = ops.attn_split_pack_ex(c.qkv, c.H, c.par[0], c.par[1], c.par[2], per_head, D=c.D, q_mul=c.D ** -0.5)
    bias = (c.table, c.index, c.mask)
    three, scores, _, qv, a_scale = _three_launches(ops, qp, kp, vp, c.N, c.D, c.H, c.gmod, c.par, c.ps, bits, bias=bias)
    one = _one_launch(ops, qp, kp, vp, c.N, c.D, c.H, c.gmod, c.par, c.ps, bits, qv, a_scale, bias=bias)
    rep = {"scores": QR.check(scores.view(s_ref.shape), s_ref, s_bar, "int8 q . k^T"),
           "three_launches": QR.check(three.reshape(ref.shape), ref, bar, "three-launch window core"),
           "attn_core": QR.check(one.reshape(ref.shape), ref, bar, "one-launch window core"), "amb": amb}
    _report({"case": "window_core", "shape": [res, ws, shift], "bits": bits, "per_head": per_head, **rep})
    assert amb < 1e-3, amb
    assert ref.abs().max().item() > 0


# ================================================================================================= 3. patch merging, patch embedding
@pytest.mark.parametrize("bits", [3, 4, 6])
def test_patch_merging_and_patch_embed_against_fp64(bits):
    """PatchMerging at K = 4 * 32 and 4 * 96 (the 2 x 2 regroup bit for bit, the bias-free reduction at the int8 bar) and Swin's
    4 x 4 / stride-4 patch embedding of 3 channels at a 56 x 56 input."""
    rep = {}
    for dim in (32, 96):
        pm, x = make_patch_merging(dim, bits, 14, 3, DEV, seed=80 + bits + dim)
        rep["reduction_%d" % (4 * dim)] = check_patch_merging(pm, x)
    lay, x = make_patch_embed_conv(bits, 3, 32, 56, 4, DEV, seed=90 + bits)
    ref, bar = QR.conv_qf(lay, x)
    with torch.no_grad():
        rep["conv"] = QR.check(lay(x), ref, bar, "patch embedding conv")
    _report({"case": "patch_merging_and_embed", "bits": bits, **rep})
