"""`-m gpu`: quant_forward of a Swin block on the fused route (utils/models.py: SwinTransformerBlock._fused_attn_residual).

Every fused launch restates the arithmetic of the module-route launches it replaces, so each kernel is compared BIT FOR BIT with the
composition it replaces (split + q * scale + packs; bias + mask + softmax + AdaLog pack; row gather / scatter in the uniform-activation
GEMM), then whole blocks and models: the attention branch of every block bit for bit, the logits, the launch count, the graph replay."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import ops as O
    return O


def _report(rec):
    """the measured launch counts and logit differences, one JSON line on stdout (shown with pytest -s)"""
    print(json.dumps(rec))


# ================================================================================================= a. split + q * scale + three packs
@pytest.mark.parametrize("D", [16, 32, 64])
@pytest.mark.parametrize("N", [16, 49, 144, 197])
@pytest.mark.parametrize("per_head", [True, False])
@pytest.mark.parametrize("q_mul", [None, "scale"])
def test_attn_split_pack_ex_equals_the_module_route_packs(ops, D, N, per_head, q_mul):
    """q / k / v of a window attention split, q multiplied by the head scale, quantised and packed in one launch
    (adalog_attn_split_pack) against what the module route packs: pack_uniform of (q * scale) (ATen's fp32 product), of k and of
    v^T -- identical bytes, padding included; values on rounding ties of k and v by construction."""
    H, B = 3, 5
    gen = g(11000 + D * 7 + N + (1 if per_head else 0) + (2 if q_mul else 0))
    qkv = torch.randn(B, N, 3 * H * D, generator=gen) * 1.3
    n = H if per_head else 1
    par = []
    for i, bits in enumerate((3, 5, 7)):
        s_ = torch.rand(n, generator=gen) * 0.2 + 0.05
        z_ = torch.randint(0, 2 ** bits, (n,), generator=gen).float()
        par.append((s_.to(DEV), z_.to(DEV), bits))
        if i:                                                          # ties: x / s = k + 0.5 for k (i = 1) and v (i = 2)
            view = qkv.view(B, N, 3, H, D)[:, :, i]
            k = torch.randint(-20, 20, view.shape, generator=gen).float()
            tie = torch.rand(view.shape, generator=gen) < 0.1
            s_h = s_.view(1, 1, -1, 1) if per_head else s_.view(1, 1, 1, 1)
            view[tie] = ((k + 0.5) * s_h.expand_as(view))[tie]
    qkv = qkv.to(DEV)
    mul = D ** -0.5 if q_mul else None
    qp, kp, vp = ops.attn_split_pack_ex(qkv, H, par[0], par[1], par[2], per_head, D=D, q_mul=mul)
    q, k, v = qkv.reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    if mul is not None:
        q = q * mul                                                    # utils/models.py WindowAttention.forward
    pg, gm = (1, H) if per_head else (0, 1)
    want_q = ops.pack_uniform(q.reshape(B * H, N, D), par[0][0], par[0][1], 1, 0, gm, pg, 0, par[0][2], ops.I8)
    want_k = ops.pack_uniform(k.reshape(B * H, N, D), par[1][0], par[1][1], 1, 0, gm, pg, 0, par[1][2], ops.I8)
    want_v = ops.pack_uniform(v.transpose(-2, -1).reshape(B * H, D, N), par[2][0], par[2][1], 1, 0, gm, pg, 0, par[2][2], ops.BF16)
    assert qp.shape == want_q.shape == (1, B * H, N, 128) and torch.equal(qp, want_q)
    assert torch.equal(kp, want_k)
    assert vp.shape == want_v.shape and torch.equal(vp.float(), want_v.float())


def test_attn_split_pack_ex_beyond_65535_images(ops):
    """More images (windows) than grid z holds: the launcher splits them, every image is packed."""
    B, N, H, D = 65537 + 3, 16, 1, 16
    gen = g(11500)
    qkv = (torch.randn(B, N, 3 * H * D, generator=gen) * 1.1).to(DEV)
    par = [(torch.tensor([0.07], device=DEV), torch.tensor([3.0], device=DEV), 4)] * 3
    qp, kp, vp = ops.attn_split_pack_ex(qkv, H, par[0], par[1], par[2], False, D=D, q_mul=0.25)
    q, k, v = qkv.reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    want_q = ops.pack_uniform((q * 0.25).reshape(B * H, N, D), *par[0][:2], 1, 0, 1, 0, 0, 4, ops.I8)
    want_v = ops.pack_uniform(v.transpose(-2, -1).reshape(B * H, D, N), *par[2][:2], 1, 0, 1, 0, 0, 4, ops.BF16)
    assert torch.equal(qp, want_q) and torch.equal(vp.float(), want_v.float())
    assert torch.equal(kp, ops.pack_uniform(k.reshape(B * H, N, D), *par[1][:2], 1, 0, 1, 0, 0, 4, ops.I8))


# ================================================================================================= b. bias + mask + softmax + AdaLog pack
def _post_softmax(bits, H, q=29):
    from adalog_amd import quant_layers as Q
    ps = Q.PostSoftmaxAsymmetricallyBatchingQuantMatMul(bits, bits, "quant_forward", head_channel_wise=True, num_heads=H, fpcs=True,
                                                       quantizer="adalog").to(DEV)
    ps.A_quantizer.q.fill_(q)
    ps.A_quantizer.update_table(q)
    ps._q_host = None
    return ps


@pytest.mark.parametrize("res,ws,shift", [(8, 4, 2), (14, 7, 3), (24, 12, 6), (8, 4, 0), (14, 7, 0), (24, 12, 0)])
@pytest.mark.parametrize("bits", [3, 6])
def test_softmax_bias_pack_equals_module_route(ops, res, ws, shift, bits):
    """(scores + relative-position bias) + shift mask -> softmax -> AdaLog quantiser -> bf16 operand in one launch
    (adalog_softmax_bias_adalog_pack_bf16) against the module route's ATen adds, torch softmax (16-, 64- and 256-wide warp forms for
    N = 16, 49, 144: the kernel's 64-lane butterfly must give the same sums and maxima) and the packer -- bit for bit, over several
    windows of each mask pattern, rows the -100 mask wipes out mostly, exact ties, and the table read fresh after an edit."""
    from adalog_amd.utils import models as M
    H, images = 3, 2
    blk = M.SwinTransformerBlock(16 * H, (res, res), H, window_size=ws, shift_size=shift)
    att = blk.attn.to(DEV)
    N = att.window_area
    mask = None if blk.attn_mask is None else blk.attn_mask.to(DEV)
    nW = (res // ws) ** 2
    Bw = images * nW
    gen = g(12000 + res + shift + bits)
    s = torch.randn(Bw * H, N, N, generator=gen) * 4
    s[0, 0] = 1.5                                                      # a row of exact ties
    s[1, 2, : N // 2] = s[1, 2, N // 2: 2 * (N // 2)]                  # pairs of equal scores
    s = s.to(DEV)
    ps = _post_softmax(bits, H)
    qv = torch.tensor([29.0], device=DEV)
    a_scale = ps.A_quantizer.scale.data.view(-1)

    def module_route():
        attn = s.view(Bw, H, N, N) + att._get_rel_pos_bias()
        if mask is not None:
            attn = attn.view(-1, nW, H, N, N) + mask.unsqueeze(1).unsqueeze(0)
            attn = attn.view(-1, H, N, N)
        return ps._pack_A_adalog(attn.softmax(dim=-1).reshape(Bw * H, N, N), qv, a_scale, 1, True)

    def fused():
        return ops.softmax_bias_adalog_pack(s, H, att.relative_position_bias_table.data, att.relative_position_index, mask, a_scale, qv,
                                            bits, ps._mant37(DEV))
    with torch.no_grad():
        for _ in range(2):
            want, got = module_route(), fused()
            assert got.shape == want.shape and got.dtype == torch.bfloat16
            same = (got.view(torch.int16) == want.view(torch.int16)).float().mean().item()
            assert same == 1.0, same
            assert (got[..., N:] == 0).all()
            att.relative_position_bias_table.data.mul_(-3.0).add_(0.25)   # an edited table is read fresh


# ================================================================================================= c. row gather / scatter in the GEMM
@pytest.mark.parametrize("L,images,K,N", [(16, 5, 48, 144), (49, 3, 96, 288), (196, 7, 32, 96), (49, 700, 96, 288)])
@pytest.mark.parametrize("bits", [4, 6])
def test_gemm_out_gen_rows_equals_gather_and_scatter(ops, L, images, K, N, bits):
    """adalog_gemm_out_gen_rows against gemm_out_gen on the gathered rows x[P] (qkv behind roll + window partition) and against the
    scattered store + separate add (proj in front of window reverse + roll back + the residual add), bit for bit; M not a multiple of
    the row tile, several images per launch, both row-tile forms (64-row tiles for small M, 128-row tiles at 34 300 rows)."""
    from adalog_amd import _lib
    from adalog_amd.utils import models as M
    side = int(round(L ** 0.5))
    ws = 7 if side % 7 == 0 else 4
    rows = M.swin_token_rows((side, side), (ws, ws), (ws // 2, ws // 2)).to(DEV)
    Mrows = L * images
    src = rows.long().repeat(images) + torch.arange(images, device=DEV).repeat_interleave(L) * L
    gen = g(13000 + L + images + bits)
    scale = torch.tensor([0.0371]); zp = torch.tensor([float(2 ** (bits - 1) - 1)])
    x = torch.randn(Mrows, K, generator=gen) * 0.3
    ties = torch.randint(0, 2 ** bits, (Mrows, K), generator=gen).float()
    tie_mask = torch.rand(Mrows, K, generator=gen) < 0.05
    x[tie_mask] = ((ties + 0.5 - zp) * scale)[tie_mask]
    w = torch.randint(-(2 ** (bits - 1)), 2 ** (bits - 1), (1, 1, N, K), generator=gen).to(torch.int8)
    Kp = ops.pad_k(K, ops.I8)
    wp = torch.zeros(1, 1, N, Kp, dtype=torch.int8); wp[..., :K] = w
    sb = torch.rand(N, generator=gen) * 0.01 + 0.001
    bias = torch.randn(N, generator=gen)
    add = torch.randn(Mrows, N, generator=gen).to(DEV)
    xd, wd, sc, z = x.to(DEV), wp.to(DEV), scale.to(DEV), zp.to(DEV)
    sa_, sb_, bi_ = ops.Strided(sc), ops.Strided(sb.to(DEV), n=1), ops.Strided(bias.to(DEV), n=1)
    plain = ops.gemm_out_gen(xd[src].unsqueeze(0), sc, z, bits, wd, N, 1, sa_, sb_, bi_)[0]
    got = ops.gemm_out_gen_rows(xd, sc, z, bits, wd, N, sa_, sb_, bi_, a_rows=rows, period=L)
    assert _lib.load().adalog_last_kernel().decode() == "k_gemm_cand_gen_rows"
    assert torch.equal(got, plain), (got - plain).abs().max().item()
    y = ops.gemm_out_gen(xd.unsqueeze(0), sc, z, bits, wd, N, 1, sa_, sb_, bi_)[0]
    want = torch.empty_like(y)
    want[src] = y + add[src]
    got = ops.gemm_out_gen_rows(xd, sc, z, bits, wd, N, sa_, sb_, bi_, o_rows=rows, period=L, addend=add)
    assert _lib.load().adalog_last_kernel().decode() == "k_gemm_cand_gen_rows"
    assert torch.equal(got, want), (got - want).abs().max().item()
    want2 = torch.empty_like(y)
    want2[src] = plain + add[src]                                      # both maps at once (the identity of the Swin block's two GEMMs)
    got2 = ops.gemm_out_gen_rows(xd, sc, z, bits, wd, N, sa_, sb_, bi_, a_rows=rows, o_rows=rows, period=L, addend=add)
    assert torch.equal(got2, want2)


# ================================================================================================= d. blocks and models
def _cfg(bits=6, rounds=1, steps=3):
    from tests.test_gpu_e2e import _cfg as cfg
    return cfg(bits, rounds, steps)


def _calibrated(model, xc, bits=6, steps=3):
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    model = wrap_modules_in_net(model.eval().to(DEV), _cfg(bits, 1, steps), reparam=True)
    QuantCalibrator(model, [(xc[i:i + 4], None) for i in range(0, xc.shape[0], 4)]).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model).to(DEV).eval()
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
        if hasattr(m, "mode"):
            m.mode = "quant_forward"
    return model


def _small_swin():
    """the model of test_gpu_e2e.py::test_swin_stage_calibration: 14 x 14 then 7 x 7 tokens, window 7, shift 3, head dimension 16"""
    from adalog_amd.utils.models import SwinTransformer
    torch.manual_seed(3)
    model = SwinTransformer(img_size=56, patch_size=4, embed_dim=32, depths=(2, 2), num_heads=(2, 4), window_size=7, num_classes=10)
    for p in model.parameters():
        p.data.mul_(6.0)
    return model


def _blocks(model):
    from adalog_amd.utils.models import SwinTransformerBlock
    return [m for m in model.modules() if isinstance(m, SwinTransformerBlock)]


def _kernels(model, x):
    from torch.profiler import ProfilerActivity, profile
    with torch.no_grad():
        model(x)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            y = model(x)
            torch.cuda.synchronize()
    return y, sum(e.count for e in prof.key_averages() if "DeviceType.CUDA" in str(getattr(e, "device_type", "")))


def _compare_routes(model, x, monkeypatch):
    """-> (y_module, y_fused, n_module, n_fused, softmax-bias-pack calls, per-block attention-branch equality)"""
    from adalog_amd import ops
    from adalog_amd.utils import models as M
    blocks = _blocks(model)
    inputs = {}
    hooks = [b.register_forward_pre_hook(lambda m, a, i=i: inputs.__setitem__(i, a[0].clone())) for i, b in enumerate(blocks)]
    calls = []
    soft0 = ops.softmax_bias_adalog_pack
    monkeypatch.setattr(ops, "softmax_bias_adalog_pack", lambda *a, **k: calls.append(1) or soft0(*a, **k))
    try:
        M.QF_FUSED = False
        y_mod, n_mod = _kernels(model, x)
        assert not calls
        M.QF_FUSED = True
        with torch.no_grad():
            model(x)
        n_calls = len(calls)
        y_fused, n_fused = _kernels(model, x)
        for h in hooks:
            h.remove()
        branch_equal = []
        with torch.no_grad():
            for i, b in enumerate(blocks):
                xi = inputs[i]
                B, Hh, W, C = xi.shape
                M.QF_FUSED = False
                want = (xi + b._attn(b.norm1(xi))).reshape(-1, C)
                M.QF_FUSED = True
                assert b._fused_ok(xi)
                got = b._fused_attn_residual(xi)
                branch_equal.append(bool(torch.equal(got, want)))
    finally:
        M.QF_FUSED = True
        for h in hooks:
            h.remove()
    return y_mod, y_fused, n_mod, n_fused, n_calls, branch_equal


def _logits_agree(y_mod, y_fused):
    diff = (y_fused - y_mod).abs().max().item()
    rel = ((y_fused - y_mod).norm() / y_mod.norm()).item()
    assert torch.isfinite(y_fused).all() and (torch.equal(y_fused, y_mod) or rel <= 1e-6), (diff, rel)
    return diff, rel


def test_small_swin_fused_route_equals_module_route(monkeypatch):
    """The calibrated two-stage Swin of test_swin_stage_calibration (shifted 14 x 14 windows, then one 7 x 7 window; head dimension
    16): every block takes the fused route, its attention branch equals the module route's bit for bit, the logits agree, and the
    fused route launches at most 0.6x the module route's kernels."""
    model = _small_swin()
    x = torch.randn(8, 3, 56, 56, generator=g(31)).to(DEV)
    model = _calibrated(model, x)
    y_mod, y_fused, n_mod, n_fused, n_calls, eq = _compare_routes(model, x, monkeypatch)
    assert n_calls == len(_blocks(model)) == 4, n_calls
    assert all(eq), eq
    diff, rel = _logits_agree(y_mod, y_fused)
    assert n_fused <= 0.6 * n_mod, (n_fused, n_mod)
    _report({"case": "small_swin", "kernels_module": n_mod, "kernels_fused": n_fused, "logits_max_abs_diff": diff, "rel": rel})


def test_swin_tiny_fused_route_and_graph_replay(monkeypatch):
    """A calibrated swin_tiny (two blocks per stage: every stage has a shifted block) at 224 px and 32 images: the same checks, and the
    captured-graph replay (utils/graph_forward.py) of the fused route bit-identical to its eager forward."""
    from adalog_amd.utils.graph_forward import GraphedForward
    from adalog_amd.utils.models import create_model
    torch.manual_seed(7)
    model = create_model("swin_tiny", depth=2)
    xc = torch.randn(8, 3, 224, 224, generator=g(71)).to(DEV)
    model = _calibrated(model, xc, bits=4, steps=2)
    x = torch.randn(32, 3, 224, 224, generator=g(72)).to(DEV)
    y_mod, y_fused, n_mod, n_fused, n_calls, eq = _compare_routes(model, x, monkeypatch)
    assert n_calls == len(_blocks(model)) == 8, n_calls
    assert all(eq), eq
    diff, rel = _logits_agree(y_mod, y_fused)
    assert n_fused <= 0.6 * n_mod, (n_fused, n_mod)
    gf = GraphedForward(model)
    y_g1 = gf(x)
    y_g2 = gf(x)
    assert torch.equal(y_g1, y_fused) and torch.equal(y_g2, y_fused)
    _report({"case": "swin_tiny_32", "kernels_module": n_mod, "kernels_fused": n_fused, "logits_max_abs_diff": diff, "rel": rel})


def test_window_12_stage_fused_route(monkeypatch):
    """swin_base_384's window: 24 x 24 tokens in 12 x 12 windows (N = 144, the 256-wide softmax form), shift 6, head dimension 32."""
    from adalog_amd.utils.models import SwinTransformer
    torch.manual_seed(12)
    model = SwinTransformer(img_size=96, patch_size=4, embed_dim=64, depths=(2,), num_heads=(2,), window_size=12, num_classes=10)
    x = torch.randn(8, 3, 96, 96, generator=g(121)).to(DEV)
    model = _calibrated(model, x, bits=4, steps=2)
    blk = _blocks(model)[1]
    assert blk.attn.window_area == 144 and blk.shift_size == (6, 6) and blk.attn.dim // blk.attn.num_heads == 32
    y_mod, y_fused, n_mod, n_fused, n_calls, eq = _compare_routes(model, x, monkeypatch)
    assert n_calls == 2 and all(eq), (n_calls, eq)
    diff, rel = _logits_agree(y_mod, y_fused)
    _report({"case": "window12", "kernels_module": n_mod, "kernels_fused": n_fused, "logits_max_abs_diff": diff, "rel": rel})


def test_block_beyond_65535_windows():
    """One shifted block of the small Swin at 16 400 images: 65 600 windows, past grid z's limit of the split-pack launch -- served
    (not refused), and its attention branch still equal to the module route's bit for bit."""
    from adalog_amd.utils import models as M
    model = _small_swin()
    model = _calibrated(model, torch.randn(8, 3, 56, 56, generator=g(31)).to(DEV))
    blk = _blocks(model)[1]
    assert blk.shift_size == (3, 3)
    xi = torch.randn(16400, 14, 14, 32, generator=g(99)).to(DEV) * 2
    try:
        with torch.no_grad():
            assert blk._fused_ok(xi)
            got = blk._fused_attn_residual(xi)
            M.QF_FUSED = False
            want = (xi + blk._attn(blk.norm1(xi))).reshape(-1, 32)
    finally:
        M.QF_FUSED = True
    assert torch.equal(got, want)
