"""CPU tier of the fp64 quant_forward reference (tests/qf_reference.py): its layer forwards against the oracle's compositions
(oracle/adalog_oracle.py: *_quant_forward) and against the layers' own quant_forward on the CPU specification backend
(tests/cpu_backend.py); its block stages against a module-route run of a wrapped block; its flip allowance on planted boundary
elements."""
import pytest
import torch

from adalog_amd import backend
from oracle import adalog_oracle as O
from tests import cpu_backend, qf_cases as QC, qf_reference as QR


@pytest.fixture(autouse=True)
def _cpu_backend():
    backend.set_backend(cpu_backend)
    yield
    backend.set_backend(None)


def _close(got, ref, bar, what):
    """fp32 compositions accumulate in fp32: the bf16-form bar (K + 4) 2^-24 sum |a b| bounds them as well."""
    QR.check(got, ref, bar, what)


@pytest.mark.parametrize("bits", [3, 4, 6])
def test_linear_forwards_equal_oracle_and_spec(bits):
    from adalog_amd import quant_layers as Q
    g = torch.Generator().manual_seed(10 + bits)
    T, D, O_ = 23, 48, 40
    for cls in ("linear", "linear_channelwise"):
        C = Q.AsymmetricallyBatchingQuantLinear if cls == "linear" else Q.AsymmetricallyChannelWiseBatchingQuantLinear
        lay = C(D, O_, True, "quant_forward", bits, bits, n_V=2 if cls == "linear" else 1, fpcs=True)
        lay.bias.data.copy_(torch.randn(O_, generator=g) * 0.1)
        x = torch.randn(3, T, D, generator=g) * (0.5 + torch.rand(D, generator=g))
        QC.arm(lay.w_quantizer, *QC.minmax_params(lay.weight.data.view(lay.n_V, lay.crb_rows, D), bits, per=(0, 1)))
        QC.arm(lay.a_quantizer, *QC.minmax_params(x, bits, per=(2,) if cls != "linear" else None))
        lay.calibrated = True
        ref, bar = QR.linear_qf(lay, x, kind="f32")
        p = O.LinearParams(w_scale=lay.w_quantizer.scale.data, w_zp=lay.w_quantizer.zero_point.data,
                           a_scale=lay.a_quantizer.scale.data.view(-1), a_zp=lay.a_quantizer.zero_point.data.view(-1),
                           weight=lay.weight.data, bias=lay.bias.data)
        _close(O.linear_quant_forward(x, p, bits, bits, lay.n_V), ref, bar, cls + " vs oracle")
        with torch.no_grad():
            _close(lay(x), ref, bar, cls + " vs spec backend")


@pytest.mark.parametrize("bits", [3, 4, 6])
@pytest.mark.parametrize("reparamed", [False, True])
def test_postgelu_forward_equals_oracle_and_spec(bits, reparamed):
    from adalog_amd import quant_layers as Q
    g = torch.Generator().manual_seed(20 + bits)
    T, D, O_ = 19, 64, 24
    lay = Q.PostGeluLogBasedBatchingQuantLinear(D, O_, True, "quant_forward", bits, bits, quantizer="adalog", fpcs=True)
    lay.bias.data.copy_(torch.randn(O_, generator=g) * 0.1)
    h = 2.0 * torch.randn(2, T, D, generator=g)
    x = torch.nn.functional.gelu(h)
    QC.arm(lay.w_quantizer, *QC.minmax_params(lay.weight.data.view(1, O_, D), bits, per=(0, 1)))
    aq = lay.a_quantizer
    aq.scale.data.fill_((float(x.max()) + QC.GELU_SHIFT) * 0.9)
    aq.q.fill_(41)
    aq.update_table(41)
    aq.inited = True
    lay._q_host = None
    lay.calibrated = True
    bias0 = lay.bias.data.clone()
    if reparamed:
        lay.reparam_bias()
    ref, bar, amb = QR.postgelu_qf(lay, x)
    assert amb < 0.01
    p = O.LinearParams(w_scale=lay.w_quantizer.scale.data, w_zp=lay.w_quantizer.zero_point.data, a_scale=aq.scale.data, a_q=41,
                       weight=lay.weight.data, bias=bias0)
    got = O.postgelu_quant_forward(x, p, bits, bits, bias_reparamed=reparamed, bias=lay.bias.data if reparamed else None)
    _close(got, ref, bar, "postgelu vs oracle")
    with torch.no_grad():
        _close(lay(x), ref, bar, "postgelu vs spec backend")
    ref2, bar2, _ = QR.postgelu_qf(lay, h, pre_gelu=True)          # GELU taken inside the reference (fc1's output as input)
    with torch.no_grad():
        _close(lay(torch.nn.functional.gelu(h)), ref2, bar2, "postgelu(pre_gelu) vs spec backend")


@pytest.mark.parametrize("bits", [3, 4, 6])
@pytest.mark.parametrize("head_wise", [True, False])
def test_matmul_forwards_equal_oracle_and_spec(bits, head_wise):
    from adalog_amd import quant_layers as Q
    g = torch.Generator().manual_seed(30 + bits)
    Bn, H, S, Dh = 2, 3, 17, 16
    hp = (1,) if head_wise else None
    mm = Q.AsymmetricallyBatchingQuantMatMul(bits, bits, "quant_forward", head_channel_wise=head_wise, num_heads=H, fpcs=True)
    A = torch.randn(Bn, H, S, Dh, generator=g) * (0.5 + torch.rand(1, H, 1, 1, generator=g))
    Bt = torch.randn(Bn, H, S, Dh, generator=g).transpose(-2, -1)
    QC.arm(mm.A_quantizer, *QC.minmax_params(A, bits, per=hp))
    QC.arm(mm.B_quantizer, *QC.minmax_params(Bt, bits, per=hp))
    mm.calibrated = True
    ref, bar = QR.matmul_qf(mm, A, Bt, kind="f32")
    p = O.MatMulParams(A_scale=mm.A_quantizer.scale.data, A_zp=mm.A_quantizer.zero_point.data,
                       B_scale=mm.B_quantizer.scale.data, B_zp=mm.B_quantizer.zero_point.data)
    _close(O.matmul_quant_forward(A, Bt, p, bits, bits), ref, bar, "matmul vs oracle")
    with torch.no_grad():
        _close(mm(A, Bt), ref, bar, "matmul vs spec backend")

    ps = Q.PostSoftmaxAsymmetricallyBatchingQuantMatMul(bits, bits, "quant_forward", head_channel_wise=head_wise, num_heads=H,
                                                       fpcs=True, quantizer="adalog")
    P = (torch.randn(Bn, H, S, S, generator=g) * 3).softmax(-1)
    V = torch.randn(Bn, H, S, Dh, generator=g)
    QC.arm(ps.B_quantizer, *QC.minmax_params(V, bits, per=hp))
    ps.A_quantizer.q.fill_(29)
    ps.A_quantizer.update_table(29)
    ps._q_host = None
    ps.calibrated = True
    ref, bar, amb = QR.postsoftmax_qf(ps, P, V)
    assert amb < 0.01
    p = O.MatMulParams(A_scale=ps.A_quantizer.scale.data, B_scale=ps.B_quantizer.scale.data, B_zp=ps.B_quantizer.zero_point.data,
                       A_q=29)
    _close(O.matmul_quant_forward(P, V, p, bits, bits, post_softmax=True), ref, bar, "postsoftmax vs oracle")
    with torch.no_grad():
        _close(ps(P, V), ref, bar, "postsoftmax vs spec backend")


@pytest.mark.parametrize("bits", [3, 4, 6])
def test_conv_forward_equals_oracle_and_spec(bits):
    from adalog_amd import quant_layers as Q
    g = torch.Generator().manual_seed(40 + bits)
    lay = Q.AsymmetricallyBatchingQuantConv2d(3, 8, 4, 4, mode="quant_forward", w_bit=bits, a_bit=8, fpcs=True)
    x = torch.randn(2, 3, 16, 16, generator=g)
    QC.arm(lay.w_quantizer, *QC.minmax_params(lay.weight.data.view(8, -1), bits, per=(0,)))
    lay.a_quantizer.scale.data.fill_(float(x.abs().max()) / 127)
    lay.a_quantizer.inited = True
    lay.calibrated = True
    ref, bar = QR.conv_qf(lay, x)
    got = O.conv_quant_forward(x, lay.weight.data, lay.bias.data, lay.w_quantizer.scale.data, lay.w_quantizer.zero_point.data,
                               bits, lay.stride)
    _close(got, ref, bar, "conv vs oracle")
    with torch.no_grad():
        _close(lay(x), ref, bar, "conv vs spec backend")


@pytest.mark.parametrize("bits,reparamed,head_wise", [(3, False, True), (4, True, True), (6, False, False)])
def test_block_stages_equal_the_module_route(bits, reparamed, head_wise):
    """A wrapped block on the CPU specification backend runs the module route (no fused extras there): each stage's recorded output
    meets the reference's bar on that stage's recorded input, and the reference's chained stages reproduce the block's output."""
    blk, x = QC.make_block(64, 2, bits, 2, 17, "cpu", head_channel_wise=head_wise, bias_reparamed=reparamed, seed=bits)
    rep = QC.run_and_check_block(blk, x, fused_expected=False)
    assert rep["amb_core"] < 0.01 and rep["amb_fc2"] < 0.01
    chained = QR.block_stages(blk, x)
    y = rep["y"].double()
    assert ((chained["mlp"] - y).norm() / y.norm()).item() < 1e-5


def test_flip_allowance_covers_a_planted_boundary_and_rejects_two_bins():
    """A probability planted on a rounding boundary of the AdaLog bins is flagged, and the allowance covers the neighbouring bin's
    value (either rounding is right); an output off by two bins of one element is outside the bar."""
    q, bits, ts = 29, 4, 1.0 / (4 * 8 - 2)
    S = 24
    g = torch.Generator().manual_seed(3)
    p = torch.softmax(torch.randn(1, 2, S, generator=g, dtype=torch.float64) * 2, -1)
    k_mid = 3.5                                                     # v = -log2(p) 37 / q = 3.5: half-way between bins 3 and 4
    p[0, 0, 5] = 2.0 ** (-k_mid * q / 37.0)
    p[0, 1, 7] = 2.0 ** (-1.0 * q / 37.0)                           # bin 1, far from a boundary
    val, dval, amb = QR.softmax_adalog(p, q, bits, ts)
    assert bool(amb[0, 0, 5]) and float(amb.double().mean()) < 0.1
    mant = QR.adalog_numerators(q, bits, ts)
    v3, v4 = (float(QR.adalog_value(torch.tensor(k), q, bits, mant)) for k in (3, 4))
    assert float(dval[0, 0, 5]) == pytest.approx(abs(v3 - v4))
    cv = torch.randint(-7, 8, (1, 4, S), generator=g).double()
    ref, bar = QR.product(val, cv, torch.ones(1), torch.ones(1), sa_mul=ts, kind="bf16", amb_A=dval)
    other = val.clone()
    other[0, 0, 5] = v3 if float(val[0, 0, 5]) == v4 else v4           # the kernel rounded the other way
    got_flip, _ = QR.product(other, cv, torch.ones(1), torch.ones(1), sa_mul=ts, kind="bf16")
    QR.check(got_flip, ref, bar, "one flipped boundary element")
    two = val.clone()
    assert not bool(amb[0, 1, 7])
    two[0, 1, 7] = QR.adalog_value(torch.tensor(3), q, bits, mant)    # bin 3 instead of 1: two bins off
    cv2 = cv.clone()
    cv2[0, :, 7] = 5.0
    ref2, bar2 = QR.product(val, cv2, torch.ones(1), torch.ones(1), sa_mul=ts, kind="bf16", amb_A=dval)
    got2, _ = QR.product(two, cv2, torch.ones(1), torch.ones(1), sa_mul=ts, kind="bf16")
    with pytest.raises(AssertionError):
        QR.check(got2, ref2, bar2, "two bins off")


# ============================================================================================================ Swin
# (dim, heads, res, ws, shift, bits, images, head_channel_wise, bias_reparamed); the last entry (head dimension 32, 32 windows: several
# per mask pattern) is run by the GPU tier only (tests/test_gpu_swin_fp64.py).  The seeds were checked on the CPU with
# tests/qf_reference.py alone (qf_cases.make_swin_block on the CPU specification backend): the share of the core's elements on a
# boundary-flip allowance is 0, 0, 2.6e-5, 6.0e-6 and 2.0e-5 in this order (cap 1e-3), of fc2's 3.7e-4, 4.5e-4, 3.0e-4, 6.1e-4 and
# 7.0e-4 (cap 1e-2).
SWIN_BLOCKS = [
    (48, 3, 8, 4, 2, 4, 2, True, False), (48, 3, 8, 4, 0, 3, 2, False, False), (32, 2, 14, 7, 3, 6, 2, True, True),
    (64, 2, 24, 12, 6, 4, 1, True, False), (64, 2, 14, 7, 3, 4, 8, True, False)]


def swin_seed(dim, res, ws, shift, bits):
    return dim + res + ws + shift + bits


def make_swin_case(case, device):
    dim, heads, res, ws, shift, bits, B, hcw, reparamed = case
    return QC.make_swin_block(dim, heads, res, ws, shift, bits, B, device, head_channel_wise=hcw, bias_reparamed=reparamed,
                              seed=swin_seed(dim, res, ws, shift, bits))


_SWIN_RUNS = {}


def _swin_run(i):
    """the armed block of SWIN_BLOCKS[i] and one recorded module-route forward of it, shared by the tests below"""
    if i not in _SWIN_RUNS:
        backend.set_backend(cpu_backend)
        blk, x = make_swin_case(SWIN_BLOCKS[i], "cpu")
        _SWIN_RUNS[i] = (blk, x) + QC.record_swin_block(blk, x)
    return _SWIN_RUNS[i]


@pytest.mark.parametrize("i", range(4))
def test_swin_block_stages_equal_the_module_route(i):
    """A wrapped Swin block on the CPU specification backend (module route): the reference's row map and shift mask, built from
    coordinates, equal the block's; every stage's recorded output meets the reference's bar on its recorded input; the chained
    reference reproduces the block's output."""
    blk, x, r, y = _swin_run(i)
    res, ws, shift = SWIN_BLOCKS[i][2:5]
    assert torch.equal(QR.swin_window_rows((res, res), (ws, ws), (shift, shift)), blk.token_rows.long())
    mask = QR.swin_shift_mask((res, res), (ws, ws), (shift, shift))
    assert (mask is None and blk.attn_mask is None) if shift == 0 else torch.equal(mask, blk.attn_mask)
    rep = QC.check_swin_record(blk, x, r, y, fused_expected=False)
    print({k: v for k, v in rep.items() if k != "y"})
    assert rep["amb_core"] < 1e-3 and rep["amb_fc2"] < 1e-2, rep
    chained = QR.swin_block_stages(blk, x)
    y64 = y.double().reshape(chained["mlp"].shape)
    assert ((chained["mlp"] - y64).norm() / y64.norm()).item() < 1e-5


SHIFTED = [i for i in range(4) if SWIN_BLOCKS[i][4]]


@pytest.mark.parametrize("i", SHIFTED)
def test_swin_reference_rejects_a_mask_rolled_by_one_window(i):
    blk, x, r, y = _swin_run(i)
    with pytest.raises(AssertionError, match="window attention core"):
        QC.check_swin_record(blk, x, r, y, core=lambda qkv: QR.window_attention_core(qkv, blk.attn, blk.attn_mask.roll(1, 0)))


@pytest.mark.parametrize("i", range(4))
def test_swin_reference_rejects_the_transposed_bias_index(i):
    blk, x, r, y = _swin_run(i)
    a = blk.attn

    def core(qkv):
        return QR.window_core(qkv, a.matmul1, a.matmul2, a.num_heads, a.relative_position_bias_table.data,
                              a.relative_position_index.t(), blk.attn_mask, q_mul=a.scale)
    with pytest.raises(AssertionError, match="window attention core"):
        QC.check_swin_record(blk, x, r, y, core=core)


@pytest.mark.parametrize("i", range(4))
def test_swin_reference_rejects_the_scale_applied_after_the_quantiser(i):
    """ViT's reading of the core: q through its quantiser as it is, the scores multiplied by the head scale"""
    blk, x, r, y = _swin_run(i)
    a = blk.attn

    def core(qkv):
        return QR.window_core(qkv, a.matmul1, a.matmul2, a.num_heads, a.relative_position_bias_table.data, a.relative_position_index,
                              blk.attn_mask, q_mul=None, s_mul=a.scale)
    with pytest.raises(AssertionError, match="window attention core"):
        QC.check_swin_record(blk, x, r, y, core=core)


@pytest.mark.parametrize("i", SHIFTED)
def test_swin_reference_rejects_the_unshifted_row_map(i):
    blk, x, r, y = _swin_run(i)
    res, ws = SWIN_BLOCKS[i][2:4]
    with pytest.raises(AssertionError, match="row map of qkv"):
        QC.check_swin_record(blk, x, r, y, rows=QR.swin_window_rows((res, res), (ws, ws), (0, 0)))


def make_patch_merging(dim, bits, res, B, device, seed):
    """A wrapped PatchMerging whose reduction (K = 4 dim, no bias) is armed as make_block arms a Linear -> (module, x [B, res, res, dim])"""
    from adalog_amd.utils.models import PatchMerging
    from adalog_amd.utils.wrap_net import wrap_modules_in_net
    g = torch.Generator().manual_seed(seed)
    pm = PatchMerging(dim)
    pm.reduction.weight.data.copy_(torch.randn(pm.reduction.weight.shape, generator=g) * 0.06)
    pm.norm.weight.data.copy_(1.0 + 0.2 * torch.randn(4 * dim, generator=g))
    pm.norm.bias.data.copy_(0.1 * torch.randn(4 * dim, generator=g))
    pm = wrap_modules_in_net(pm.eval(), QC.cfg(bits)).to(device)
    x = (torch.randn(B, res, res, dim, generator=g) * 1.5).to(device)
    lay = pm.reduction
    assert lay.bias is None and lay.in_features == 4 * dim
    with torch.no_grad():
        QC.arm(lay.a_quantizer, *QC.minmax_params(pm.norm(QR.patch_merging_rows(x)), bits))
    QC.arm(lay.w_quantizer, *QC.minmax_params(lay.weight.data.view(lay.n_V, lay.crb_rows, -1), bits, per=(0, 1)))
    lay.calibrated = True
    lay.mode = "quant_forward"
    return pm, x


def check_patch_merging(pm, x, kind="i8"):
    """the module's regroup is the reference's, bit for bit; its output meets the bar of the reference's reduction"""
    seen = {}
    h = pm.norm.register_forward_hook(lambda m, a, out: seen.update(x=a[0].detach().clone(), out=out.detach().clone()))
    with torch.no_grad():
        y = pm(x)
    h.remove()
    assert torch.equal(seen["x"], QR.patch_merging_rows(x))
    ref, bar = QR.linear_qf(pm.reduction, seen["out"], kind=kind)
    return QR.check(y, ref, bar, "PatchMerging.reduction")


def make_patch_embed_conv(bits, chans, out, size, B, device, seed):
    """Swin's patch embedding: a 4 x 4 / stride-4 conv (fp32 input at 8 activation bits), weights armed per output channel"""
    from adalog_amd import quant_layers as Q
    g = torch.Generator().manual_seed(seed)
    lay = Q.AsymmetricallyBatchingQuantConv2d(chans, out, 4, 4, mode="quant_forward", w_bit=bits, a_bit=8, fpcs=True)
    lay.weight.data.copy_(torch.randn(lay.weight.shape, generator=g) * 0.1)
    lay.bias.data.copy_(torch.randn(out, generator=g) * 0.1)
    lay = lay.to(device)
    x = torch.randn(B, chans, size, size, generator=g).to(device)
    QC.arm(lay.w_quantizer, *QC.minmax_params(lay.weight.data.view(out, -1), bits, per=(0,)))
    lay.a_quantizer.scale.data.fill_(float(x.abs().max()) / 127)
    lay.a_quantizer.inited = True
    lay.calibrated = True
    return lay, x


@pytest.mark.parametrize("bits", [3, 4, 6])
def test_patch_merging_and_patch_embed_equal_spec(bits):
    pm, x = make_patch_merging(32, bits, 8, 2, "cpu", seed=60 + bits)
    check_patch_merging(pm, x, kind="f32")
    lay, x = make_patch_embed_conv(bits, 3, 32, 16, 2, "cpu", seed=70 + bits)
    ref, bar = QR.conv_qf(lay, x)
    with torch.no_grad():
        QR.check(lay(x), ref, bar, "patch embedding conv vs spec backend")
