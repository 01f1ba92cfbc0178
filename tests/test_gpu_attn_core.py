"""`-m gpu`: the one-launch attention core of quant_forward (csrc/attn_core.hip, ops.attn_core, models.QF_ATTN_CORE).

The kernel restates the arithmetic of the three launches it replaces -- gemm_out(I8) -> softmax_(bias_)adalog_pack -> gemm_out(BF16,
heads_last) -- so everything here is an equality: the kernel against those launches on the same packed operands, blocks and models
with the switch on against the switch off, the captured graph against the eager forward.  The fp64 stage check of
tests/qf_cases.py runs over the one-launch route as well, with the bar and the ambiguity bound of tests/test_gpu_quant_forward.py."""
import json

import pytest
import torch

from tests import qf_cases as QC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import ops as O
    return O


def _report(rec):
    print(json.dumps(rec))


def _post_softmax(bits, H, q=29, scale=None):
    from adalog_amd import quant_layers as Q
    ps = Q.PostSoftmaxAsymmetricallyBatchingQuantMatMul(bits, bits, "quant_forward", head_channel_wise=True, num_heads=H, fpcs=True,
                                                       quantizer="adalog").to(DEV)
    ps.A_quantizer.q.fill_(q)
    ps.A_quantizer.update_table(q)
    if scale is not None:
        ps.A_quantizer.scale.data.fill_(scale)
    ps._q_host = None
    return ps


def _quantisers(H, per_head, gen, bits3=(3, 5, 7)):
    n = H if per_head else 1
    par = []
    for bits in bits3:
        s_ = torch.rand(n, generator=gen) * 0.2 + 0.05
        z_ = torch.randint(0, 2 ** bits, (n,), generator=gen).float()
        par.append((s_.to(DEV), z_.to(DEV), bits))
    return par


def _three_launches(ops, qp, kp, vp, N, D, H, gmod, par, ps, bits, mul=None, bias=None):
    """the route ops.attn_core replaces, on the same packed operands"""
    G = qp.shape[1]
    pg = 1 if gmod > 1 else 0
    sA, sB, sV = par[0][0], par[1][0], par[2][0]
    qv = torch.tensor([float(int(ps.A_quantizer.q.item()))], device=DEV)
    a_scale = ps.A_quantizer.scale.data.view(-1)
    scores = ops.gemm_out(ops.I8, qp, kp, N, N, G, gmod, ops.Strided(sA, g=pg), ops.Strided(sB, g=pg), None)
    if bias is None:
        ap = ops.softmax_adalog_pack(scores, mul, a_scale, qv, bits, ps._mant37(DEV))
    else:
        ap = ops.softmax_bias_adalog_pack(scores, H, bias[0], bias[1], bias[2], a_scale, qv, bits, ps._mant37(DEV))
    out = ops.gemm_out(ops.BF16, ap, vp, N, D, G, gmod, ops.Strided(a_scale), ops.Strided(sV, g=pg), None, sa_mul=ps._ts32(),
                       heads_last=H)
    return out, scores, ap, qv, a_scale


def _one_launch(ops, qp, kp, vp, N, D, H, gmod, par, ps, bits, qv, a_scale, mul=None, bias=None):
    kw = {} if bias is None else dict(table=bias[0], index=bias[1], mask=bias[2])
    return ops.attn_core(qp, kp, vp, N, D, H, gmod, par[0][0], par[1][0], par[2][0], 1.0 if mul is None else mul, a_scale, qv, bits,
                         ps._mant37(DEV), ps._ts32(), **kw)


def _plant(qkv, B, N, H, D):
    """hard rows, in place: image 0 / token 0 has q = 0 (every score of the row equal), image 1 has its keys in equal pairs (pairs of
    equal scores in every row), the last image has q and k far past their quantisers' ranges (codes at the ends of the
    grids: the largest scores these operands can form, most probabilities in the AdaLog quantiser's zero bin)"""
    v = qkv.view(B, N, 3, H, D)
    v[0, 0, 0] = 0.0
    if N >= 2 and B > 1:
        v[1, N // 2: 2 * (N // 2), 1] = v[1, : N // 2, 1]
    v[B - 1, :, :2] *= 8.0


# ================================================================================================= 1. the kernel against its three launches
@pytest.mark.parametrize("D", [16, 32, 48, 64])
@pytest.mark.parametrize("N", [1, 16, 49, 65, 144, 197, 256])
@pytest.mark.parametrize("per_head", [True, False])
def test_attn_core_plain_equals_the_three_launches(ops, D, N, per_head):
    """Plain form (ViT / DeiT: softmax(scores * mul)) for every head dimension and token counts on both sides of the 32- / 64-row
    tile and 64-key block edges; H = 3 with G = 15 (not a multiple of 8); per-head and per-tensor scales; q / k / v at 3 / 5 / 7
    bits; post-softmax quantiser at 3, 6 and 7 bits, default and off-default scale."""
    H, B = 3, 5
    gen = g(21000 + D * 7 + N + (1 if per_head else 0))
    qkv = torch.randn(B, N, 3 * H * D, generator=gen) * 1.3
    _plant(qkv, B, N, H, D)
    par = _quantisers(H, per_head, gen)
    qp, kp, vp = ops.attn_split_pack_ex(qkv.to(DEV), H, par[0], par[1], par[2], per_head, D=D)
    gmod = H if per_head else 1
    mul = D ** -0.5
    zero_bin = {}
    for bits, scale in ((3, 1.0), (6, 0.7), (7, None)):
        ps = _post_softmax(bits, H, scale=scale)
        want, scores, ap, qv, a_scale = _three_launches(ops, qp, kp, vp, N, D, H, gmod, par, ps, bits, mul=mul)
        got = _one_launch(ops, qp, kp, vp, N, D, H, gmod, par, ps, bits, qv, a_scale, mul=mul)
        assert got.shape == want.shape == (B, N, H, D) and got.dtype == torch.float32
        assert torch.equal(got, want), (bits, (got - want).abs().max().item(), (got != want).float().mean().item())
        zero_bin[bits] = (ap.view(1, B, H, N, -1)[0, B - 1, :, :, :N] == 0).float().mean().item()
    # the planted rows are what they claim to be
    sc = scores.view(B, H, N, N)
    assert (sc[0, :, 0] == sc[0, :, 0, :1]).all()
    if N >= 2:
        assert torch.equal(sc[1, :, :, : N // 2], sc[1, :, :, N // 2: 2 * (N // 2)])
    # 3 bits, scale 1, q = 29: level k >= 8 is the zero bin, i.e. p <= 2^(-7.5 * 29 / 37) = 0.0170; a row holds at most 58 larger
    # probabilities, so from 144 keys on at least 86 / 144 of every row is in the zero bin whatever the scores are
    if N >= 144:
        assert zero_bin[3] > 0.5, zero_bin


@pytest.mark.parametrize("res,ws,shift", [(8, 4, 2), (14, 7, 3), (24, 12, 6), (8, 4, 0), (14, 7, 0), (24, 12, 0)])
@pytest.mark.parametrize("bits", [3, 6])
@pytest.mark.parametrize("D", [16, 32])
def test_attn_core_bias_equals_the_three_launches(ops, res, ws, shift, bits, D):
    """Bias form (Swin: relative-position bias, then the shift mask, in front of the softmax): the (resolution, window, shift) cases of
    tests/test_gpu_swin_quant_forward.py::test_softmax_bias_pack_equals_module_route, several windows per mask pattern (the -100 mask
    wipes most of some rows out), the planted rows above, and the table read fresh after an edit."""
    from adalog_amd.utils import models as M
    H, images = 3, 3
    blk = M.SwinTransformerBlock(D * H, (res, res), H, window_size=ws, shift_size=shift)
    att = blk.attn.to(DEV)
    N = att.window_area
    mask = None if blk.attn_mask is None else blk.attn_mask.to(DEV)
    nW = (res // ws) ** 2
    Bw = images * nW
    gen = g(22000 + res + shift + bits + D)
    qkv = torch.randn(Bw, N, 3 * H * D, generator=gen) * 1.3
    _plant(qkv, Bw, N, H, D)
    att.relative_position_bias_table.data.copy_(torch.randn(att.relative_position_bias_table.shape, generator=gen).to(DEV))
    for per_head in (True, False):
        par = _quantisers(H, per_head, gen)
        qp, kp, vp = ops.attn_split_pack_ex(qkv.to(DEV), H, par[0], par[1], par[2], per_head, D=D, q_mul=D ** -0.5)
        gmod = H if per_head else 1
        ps = _post_softmax(bits, H)
        for _ in range(2):
            bias = (att.relative_position_bias_table.data, att.relative_position_index, mask)
            want, scores, ap, qv, a_scale = _three_launches(ops, qp, kp, vp, N, D, H, gmod, par, ps, bits, bias=bias)
            got = _one_launch(ops, qp, kp, vp, N, D, H, gmod, par, ps, bits, qv, a_scale, bias=bias)
            assert got.shape == want.shape == (Bw, N, H, D)
            assert torch.equal(got, want), ((got - want).abs().max().item(), (got != want).float().mean().item())
            att.relative_position_bias_table.data.mul_(-3.0).add_(0.25)      # an edited table is read fresh


def test_attn_core_beyond_65535_groups(ops):
    """More groups than a grid dimension of 65 535 holds (Swin at thousands of images): every group is served."""
    B, N, H, D = 21900, 16, 3, 16                                          # G = 65 700
    gen = g(23000)
    qkv = torch.randn(B, N, 3 * H * D, generator=gen) * 1.2
    par = _quantisers(H, True, gen, bits3=(4, 4, 4))
    qp, kp, vp = ops.attn_split_pack_ex(qkv.to(DEV), H, par[0], par[1], par[2], True, D=D, q_mul=0.25)
    ps = _post_softmax(4, H)
    idx = torch.randint(0, 49, (N, N), generator=gen).to(DEV)
    table = torch.randn(49, H, generator=gen).to(DEV)
    mask = (torch.rand(4, N, N, generator=gen) < 0.3).float().mul(-100.0).to(DEV)
    for bias in (None, (table, idx, mask)):
        mul = None if bias else 0.25
        want, _, _, qv, a_scale = _three_launches(ops, qp, kp, vp, N, D, H, H, par, ps, 4, mul=0.25 if bias is None else None, bias=bias)
        got = _one_launch(ops, qp, kp, vp, N, D, H, H, par, ps, 4, qv, a_scale, mul=mul, bias=bias)
        assert torch.equal(got, want)


# ================================================================================================= 2. against fp64, stage by stage
def _fused_blocks():
    from tests.test_gpu_quant_forward import BLOCKS
    return [b for b in BLOCKS if b[-1]]


@pytest.mark.parametrize("dim,heads,B,N,bits,hcw,reparamed,fused", _fused_blocks())
def test_one_launch_block_stages_against_fp64(monkeypatch, dim, heads, B, N, bits, hcw, reparamed, fused):
    """The fused entries of tests/test_gpu_quant_forward.py's BLOCKS with the switch on: every stage within its fp64 bar
    (tests/qf_cases.run_and_check_block; the attention core against qf_reference.attention_core), the same ambiguity bound, and the
    route taken: one attn_core call, no softmax_adalog_pack call."""
    from adalog_amd import ops
    from adalog_amd.utils import models as M
    calls = {"core": 0, "softmax": 0}
    core0, soft0 = ops.attn_core, ops.softmax_adalog_pack
    monkeypatch.setattr(ops, "attn_core", lambda *a, **k: calls.__setitem__("core", calls["core"] + 1) or core0(*a, **k))
    monkeypatch.setattr(ops, "softmax_adalog_pack", lambda *a, **k: calls.__setitem__("softmax", calls["softmax"] + 1) or soft0(*a, **k))
    blk, x = QC.make_block(dim, heads, bits, B, N, DEV, head_channel_wise=hcw, bias_reparamed=reparamed, seed=dim + B + bits)
    old = M.QF_ATTN_CORE
    try:
        M.QF_ATTN_CORE = False
        with torch.no_grad():
            y_off = blk(x)
        calls.update(core=0, softmax=0)
        M.QF_ATTN_CORE = True
        rep = QC.run_and_check_block(blk, x, fused_expected=True)
    finally:
        M.QF_ATTN_CORE = old
    assert calls == {"core": 1, "softmax": 0}, calls
    assert rep["amb_core"] < 1e-3 and rep["amb_fc2"] < 1e-2, rep
    assert torch.equal(rep["y"], y_off)
    _report({"case": "block_one_launch", "shape": [dim, heads, B, N], "bits": bits, **{k: v for k, v in rep.items() if k != "y"}})


# ================================================================================================= 3. blocks and models, switch on against off
def _kernels(model, x):
    from tests.test_gpu_swin_quant_forward import _kernels as k
    return k(model, x)


def _count_calls(monkeypatch):
    from adalog_amd import ops
    calls = {"core": 0, "softmax": 0, "softmax_bias": 0}
    for key, name in (("core", "attn_core"), ("softmax", "softmax_adalog_pack"), ("softmax_bias", "softmax_bias_adalog_pack")):
        fn0 = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _k=key, _f=fn0, **kw: calls.__setitem__(_k, calls[_k] + 1) or _f(*a, **kw))
    return calls


def _on_against_off(model, x, blocks, branch, monkeypatch):
    """-> (kernels off, kernels on): the attention branch of every block and the logits with the switch on equal the switch-off
    ones bit for bit; one attn_core call per block and no softmax-pack call; graph capture + two replays equal the eager result"""
    from adalog_amd.utils import models as M
    from adalog_amd.utils.graph_forward import GraphedForward
    calls = _count_calls(monkeypatch)
    inputs = {}
    hooks = [b.register_forward_pre_hook(lambda m, a, i=i: inputs.__setitem__(i, a[0].clone())) for i, b in enumerate(blocks)]
    old = M.QF_ATTN_CORE
    try:
        M.QF_ATTN_CORE = False
        y_off, n_off = _kernels(model, x)
        assert calls["core"] == 0 and calls["softmax"] + calls["softmax_bias"] == 2 * len(blocks), calls
        calls.update(core=0, softmax=0, softmax_bias=0)
        M.QF_ATTN_CORE = True
        y_on, n_on = _kernels(model, x)
        assert calls == {"core": 2 * len(blocks), "softmax": 0, "softmax_bias": 0}, calls
        assert torch.equal(y_on, y_off)
        for h in hooks:                                          # (in place for both counted forwards: their copies are kernels too)
            h.remove()
        with torch.no_grad():
            for i, b in enumerate(blocks):
                M.QF_ATTN_CORE = False
                want = branch(b, inputs[i])
                M.QF_ATTN_CORE = True
                assert torch.equal(branch(b, inputs[i]), want), i
        gf = GraphedForward(model)
        y_g1 = gf(x)
        y_g2 = gf(x)
        y_g3 = gf(x)
        assert torch.equal(y_g1, y_on) and torch.equal(y_g2, y_on) and torch.equal(y_g3, y_on)
    finally:
        M.QF_ATTN_CORE = old
        for h in hooks:
            h.remove()
    assert n_on == n_off - 2 * len(blocks), (n_on, n_off, len(blocks))
    return n_off, n_on


def _swin_branch(b, xi):
    assert b._fused_ok(xi)
    return b._fused_attn_residual(xi)


def _vit_branch(b, xi):
    assert b.attn._fused_quant_forward_ok(b.norm1(xi))
    return b.attn(b.norm1(xi), residual=xi)


def test_deit_small_32_images_switch_on_equals_off(monkeypatch):
    """A calibrated deit_small (built as test_deit_small_at_validate_batch_fused_module_and_graph builds it) at 32 images."""
    from tests.test_gpu_e2e import _cfg
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.models import Block, create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    torch.manual_seed(6)
    model = wrap_modules_in_net(create_model("deit_small").eval(), _cfg(4), reparam=True).to(DEV)
    xc = torch.randn(16, 3, 224, 224, generator=g(6)).to(DEV)
    QuantCalibrator(model, [(xc, None)], capture="block").batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model).to(DEV).eval()
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
        if hasattr(m, "mode"):
            m.mode = "quant_forward"
    x = torch.randn(32, 3, 224, 224, generator=g(7)).to(DEV)
    blocks = [m for m in model.modules() if isinstance(m, Block)]
    assert len(blocks) == 12
    n_off, n_on = _on_against_off(model, x, blocks, _vit_branch, monkeypatch)
    _report({"case": "deit_small_32", "kernels_off": n_off, "kernels_on": n_on})


def test_small_swin_switch_on_equals_off(monkeypatch):
    """The head-dimension-16 Swin of tests/test_gpu_swin_quant_forward.py (shifted and unshifted blocks) at 32 images."""
    from tests.test_gpu_swin_quant_forward import _blocks, _calibrated, _small_swin
    model = _calibrated(_small_swin(), torch.randn(8, 3, 56, 56, generator=g(31)).to(DEV))
    x = torch.randn(32, 3, 56, 56, generator=g(32)).to(DEV)
    blocks = _blocks(model)
    assert len(blocks) == 4 and any(b.shift_size != (0, 0) for b in blocks) and any(b.shift_size == (0, 0) for b in blocks)
    n_off, n_on = _on_against_off(model, x, blocks, _swin_branch, monkeypatch)
    _report({"case": "small_swin_32", "kernels_off": n_off, "kernels_on": n_on})


def test_swin_tiny_32_images_switch_on_equals_off(monkeypatch):
    """swin_tiny (two blocks per stage: every stage has a shifted block) at 224 px and 32 images."""
    from tests.test_gpu_swin_quant_forward import _blocks, _calibrated
    from adalog_amd.utils.models import create_model
    torch.manual_seed(7)
    model = create_model("swin_tiny", depth=2)
    model = _calibrated(model, torch.randn(8, 3, 224, 224, generator=g(71)).to(DEV), bits=4, steps=2)
    x = torch.randn(32, 3, 224, 224, generator=g(72)).to(DEV)
    blocks = _blocks(model)
    assert len(blocks) == 8
    n_off, n_on = _on_against_off(model, x, blocks, _swin_branch, monkeypatch)
    _report({"case": "swin_tiny_32", "kernels_off": n_off, "kernels_on": n_on})


def test_window_12_stage_switch_on_equals_off(monkeypatch):
    """swin_base_384's window: 12 x 12 (N = 144), shift 6, head dimension 32."""
    from tests.test_gpu_swin_quant_forward import _blocks, _calibrated
    from adalog_amd.utils.models import SwinTransformer
    torch.manual_seed(12)
    model = SwinTransformer(img_size=96, patch_size=4, embed_dim=64, depths=(2,), num_heads=(2,), window_size=12, num_classes=10)
    x = torch.randn(8, 3, 96, 96, generator=g(121)).to(DEV)
    model = _calibrated(model, x, bits=4, steps=2)
    blocks = _blocks(model)
    assert blocks[1].attn.window_area == 144 and blocks[1].shift_size == (6, 6)
    n_off, n_on = _on_against_off(model, x, blocks, _swin_branch, monkeypatch)
    _report({"case": "window12", "kernels_off": n_off, "kernels_on": n_on})


# ================================================================================================= 4. gate and fallback
def test_switch_on_leaves_ungated_blocks_on_their_routes(monkeypatch):
    """With the switch on, a block of 257 tokens (module route) and a block whose post-softmax quantiser is in training mode (module
    route) take the routes they take with the switch off -- no attn_core call -- and give the same output."""
    from adalog_amd.utils import models as M
    calls = _count_calls(monkeypatch)
    old = M.QF_ATTN_CORE
    try:
        for N, training in ((257, False), (65, True)):
            blk, x = QC.make_block(384, 6, 4, 2, N, DEV, seed=400 + N)
            blk.attn.matmul2.A_quantizer.training_mode = training
            assert not blk.attn._fused_quant_forward_ok(blk.norm1(x))
            M.QF_ATTN_CORE = False
            with torch.no_grad():
                y_off = blk(x)
            M.QF_ATTN_CORE = True
            with torch.no_grad():
                y_on = blk(x)
            assert calls["core"] == 0 and torch.equal(y_on, y_off), (N, training, calls)
        # and the gate itself: the backend refuses what the kernel does not take
        from adalog_amd import ops
        assert ops.attn_core_ok(256, 64) and ops.attn_core_ok(49, 16) and not ops.attn_core_ok(257, 64) and not ops.attn_core_ok(49, 24)
    finally:
        M.QF_ATTN_CORE = old
