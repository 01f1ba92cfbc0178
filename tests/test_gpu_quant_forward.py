"""`-m gpu`: quant_forward's products and fused ViT block against the fp64 reference (tests/qf_reference.py), per element.

a. the store-form products (ops.gemm_out / gemm_out_gen) at every row tile (TM = 1 / 2 / 4, forced through ADALOG_GEMM_TM), every
   epilogue, ragged shapes;  b. the layer classes' products at validate()'s shapes with the tile heuristic choosing;  c. the fused
   block stage by stage;  d. a calibrated deit_small at 200 images (fused vs module route, graph replay vs eager);  e. zero points
   at and beyond the ends of the grid.  The references are computed on the device in fp64."""
import json
import os

import pytest
import torch

from tests import qf_cases as QC
from tests import qf_reference as QR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _report(entry):
    """Largest |err| / bar per case, appended as a JSON line to the file named by ADALOG_QF_REPORT (unset: nothing is written)."""
    path = os.environ.get("ADALOG_QF_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(entry) + "\n")


def pick_tm_out(M, N, G, gen=False):
    """Mirror of pick_tm_out (adalog_amd/csrc/gemm_score.hip): the largest row tile (TM x 64 rows) that still gives every CU two
    workgroups of 256-column tiles; gemm_out_gen caps it at 2."""
    want = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    tm = next((t for t in (4, 2, 1) if -(-M // (64 * t)) * (-(-N // 256)) * G >= want), 1)
    return min(tm, 2) if gen else tm


# ================================================================================================= a. store-form products
EPILOGUES = ("plain", "bias", "addend", "addend_bias", "heads_last", "sa_mul")
MS = (1, 63, 65, 197, 255, 257, 39400)
NS = (64, 65, 197, 384, 1000)


def _operands(dt, G, M, N, K, g, bcast=None):
    """A [1, GA, M, Kp], B [1, GB, N, Kp] with zero padding beyond K (what the packers write); int8 codes over the whole range,
    bf16 AdaLog-like values m * 2^-t against integer codes."""
    from adalog_amd import ops
    Kp = ops.pad_k(K, dt)
    GA, GB = (1 if bcast == "A" else G), (1 if bcast == "B" else G)
    if dt == ops.I8:
        A = torch.zeros(1, GA, M, Kp, dtype=torch.int8)
        B = torch.zeros(1, GB, N, Kp, dtype=torch.int8)
        A[..., :K] = torch.randint(-128, 128, (1, GA, M, K), generator=g, dtype=torch.int8)
        B[..., :K] = torch.randint(-128, 128, (1, GB, N, K), generator=g, dtype=torch.int8)
    else:
        A = torch.zeros(1, GA, M, Kp, dtype=torch.bfloat16)
        B = torch.zeros(1, GB, N, Kp, dtype=torch.bfloat16)
        m = torch.randint(15, 31, (1, GA, M, K), generator=g).float()
        A[..., :K] = (m * torch.pow(2.0, -torch.randint(0, 12, (1, GA, M, K), generator=g).float())).bfloat16()
        B[..., :K] = torch.randint(-127, 128, (1, GB, N, K), generator=g).bfloat16()
    return A.to(DEV), B.to(DEV)


def _store_case(dt, M, N, K, G, H, epi, g, bcast=None):
    from adalog_amd import ops
    from adalog_amd.ops import Strided
    A, B = _operands(dt, G, M, N, K, g, bcast)
    gmod = H if H > 1 else 1
    sa = (0.5 + torch.rand(gmod, generator=g)).mul(1e-2).to(DEV)
    per_col = epi != "heads_last" and G == 1
    sb = ((0.5 + torch.rand(N if per_col else gmod, generator=g)) * 1e-2).to(DEV)
    sbs = Strided(sb, n=1) if per_col else Strided(sb, g=1 if gmod > 1 else 0)
    bias = (torch.randn(N, generator=g) * 3).to(DEV) if epi in ("bias", "addend_bias") else None
    addend = (torch.randn(G, M, N, generator=g) * 5).to(DEV) if epi in ("addend", "addend_bias") else None
    sa_mul = 1.0 / 14 if epi == "sa_mul" else 1.0
    kw = {}
    if addend is not None:
        kw["addend"] = addend
    if epi == "heads_last":
        kw["heads_last"] = H
    got = ops.gemm_out(dt, A, B, M, N, G, gmod, Strided(sa, g=1 if gmod > 1 else 0), sbs,
                       None if bias is None else Strided(bias, n=1), sa_mul=sa_mul, **kw)
    ref, bar = QR.product(A[0], B[0], sa, sb, bias, addend, sa_mul=sa_mul, gmod=gmod, heads_last=H if epi == "heads_last" else 0,
                          k_valid=K, kind="i8" if dt == ops.I8 else "bf16", sb_cols=per_col)
    return QR.check(got, ref, bar, f"gemm_out dt={dt} M={M} N={N} K={K} G={G} H={H} {epi} bcast={bcast}")


@pytest.mark.parametrize("tm", [1, 2, 4])
@pytest.mark.parametrize("dt_name", ["i8", "bf16"])
def test_gemm_out_store_forms_against_fp64(monkeypatch, dt_name, tm):
    """Every epilogue of the store form at a forced row tile, on shapes ragged against every tile (M, N) and a K whose last K-step
    is partly padding; per-head scales over G = B * H groups and a broadcast operand."""
    from adalog_amd import ops
    monkeypatch.setenv("ADALOG_GEMM_TM", str(tm))
    dt = ops.I8 if dt_name == "i8" else ops.BF16
    g = torch.Generator().manual_seed(100 * tm + dt)
    worst = {}
    i = 0
    for M in MS:
        for N in NS:
            epi = EPILOGUES[i % len(EPILOGUES)]
            i += 1
            K = 200 if dt == ops.I8 else 72
            if M >= 39400:                                   # one group at the largest M
                G, H = (2, 2) if epi == "heads_last" else (1, 1)
            else:
                G, H = (6, 3) if epi in ("heads_last", "sa_mul", "plain") else (1, 1)
            w = _store_case(dt, M, N, K, G, H, epi, g)
            worst[epi] = max(worst.get(epi, 0.0), w)
    for epi in EPILOGUES:                                    # every epilogue on a ragged multi-tile shape with per-head scales
        G, H = (6, 3) if epi in ("heads_last", "sa_mul", "plain") else (1, 1)
        worst[epi] = max(worst[epi], _store_case(dt, 257, 197, 136 if dt == ops.I8 else 200, G, H, epi, g))
    worst["bcast_B"] = _store_case(dt, 197, 384, 64, 12, 6, "plain", g, bcast="B")
    worst["bcast_A"] = _store_case(dt, 65, 197, 64, 12, 6, "sa_mul", g, bcast="A")
    _report({"case": "gemm_out", "dt": dt_name, "tm": tm, "worst_err_over_bar": worst})


def _gen_case(M, N, K, G, H, bits, per_head, addend, g, x_view=False, plant=True):
    """gemm_out_gen: the A operand quantised inside the loader from fp32 x, against the oracle's fp32 bins and an fp64 product."""
    from adalog_amd import ops
    from adalog_amd.ops import Strided
    qmax = 2 ** bits - 1
    Kp = ops.pad_k(K, ops.I8)
    hs = H if per_head else 1
    s = (0.01 + 0.05 * torch.rand(hs, generator=g))
    z = torch.round(torch.rand(hs, generator=g) * qmax)
    if x_view:                                               # the class-token view x[:, 0] of [G, T, K] tokens (row stride T * K)
        full = torch.randn(G, M, 3, K, generator=g) * 2
        x = full.to(DEV)[:, :, 0]
    else:
        x = (torch.randn(G, M, K, generator=g) * 2).to(DEV)
    if plant:                                                # rounding ties (x / s = n + 0.5) and values beyond both clamps
        sg = s[torch.arange(G) % hs].view(G, 1, 1).to(DEV)
        n = torch.randint(-40, 40, x[:, :, :8].shape, generator=g).to(DEV).float()
        x[:, :, :8] = (n + 0.5) * sg
        x[:, :, 8:10] = 1e3 * sg
        x[:, :, 10:12] = -1e3 * sg
    W = torch.zeros(1, 1 if G > 1 and not per_head else G, N, Kp, dtype=torch.int8)
    W[..., :K] = torch.randint(-128, 128, W[..., :K].shape, generator=g, dtype=torch.int8)
    W = W.to(DEV)
    sw = ((0.5 + torch.rand(N, generator=g)) * 1e-2).to(DEV)
    bias = (torch.randn(N, generator=g)).to(DEV)
    add = (torch.randn(G, M, N, generator=g) * 4).to(DEV) if addend else None
    s, z = s.to(DEV), z.to(DEV)
    gmod = H if per_head else 1
    got = ops.gemm_out_gen(x, s, z, bits, W, N, gmod, Strided(s, g=1 if per_head else 0), Strided(sw, n=1), Strided(bias, n=1),
                           addend=add)
    cx = QR.uniform_codes(x, QR.per_group(s, G, gmod, DEV).float(), QR.per_group(z, G, gmod, DEV).float(), bits)
    ref, bar = QR.product(cx, W[0], s, sw, bias, add, gmod=gmod, k_valid=K, kind="i8", sb_cols=True)
    return QR.check(got, ref, bar, f"gemm_out_gen M={M} N={N} K={K} G={G} H={H} bits={bits} per_head={per_head} addend={addend}")


@pytest.mark.parametrize("tm", [1, 2, 4])
def test_gemm_out_gen_against_fp64(monkeypatch, tm):
    """The activation quantised in the GEMM's loader: TM 1 / 2 and a requested 4 (capped to 2), per-tensor and per-head
    parameters, the row-strided class-token view, planted ties and clamps, bits 2..7, with and without the residual addend."""
    monkeypatch.setenv("ADALOG_GEMM_TM", str(tm))
    g = torch.Generator().manual_seed(7 + tm)
    worst = 0.0
    cases = [(39400, 384, 384, 1, 1, 4, False, True), (257, 1000, 192, 1, 1, 2, False, False), (255, 65, 64, 1, 1, 7, False, True),
             (197, 197, 64, 6, 3, 3, True, False), (65, 64, 80, 4, 2, 5, True, True), (1, 197, 48, 1, 1, 6, False, False),
             (63, 384, 768, 1, 1, 7, False, False), (197, 64, 64, 12, 6, 6, True, True)]
    for M, N, K, G, H, bits, ph, add in cases:
        worst = max(worst, _gen_case(M, N, K, G, H, bits, ph, add, g))
    worst = max(worst, _gen_case(200, 1000, 384, 1, 1, 4, False, False, g, x_view=True))      # class token of 200 images
    _report({"case": "gemm_out_gen", "tm_requested": tm, "worst_err_over_bar": worst})


# ================================================================================================= b. validate()'s shapes
def _linear(cls_name, I, O_, bits, g, n_V=1):
    from adalog_amd import quant_layers as Q
    if cls_name == "postgelu":
        lay = Q.PostGeluLogBasedBatchingQuantLinear(I, O_, True, "quant_forward", bits, bits, quantizer="adalog", fpcs=True).to(DEV)
    else:
        lay = Q.AsymmetricallyBatchingQuantLinear(I, O_, True, "quant_forward", bits, bits, n_V=n_V, fpcs=True).to(DEV)
    lay.weight.data.copy_((torch.randn(O_, I, generator=g) * 0.05).to(DEV))
    lay.bias.data.copy_((torch.randn(O_, generator=g) * 0.1).to(DEV))
    QC.arm(lay.w_quantizer, *QC.minmax_params(lay.weight.data.view(lay.n_V, lay.crb_rows, I), bits, per=(0, 1)))
    lay.calibrated = True
    return lay


@pytest.mark.parametrize("model,images", [("deit_small", 200), ("vit_base", 200), ("vit_base", 48)])
def test_layer_products_at_validate_shapes(model, images):
    """The attention and MLP products of one block at validate()'s batch through the layer classes' own quant_forward, the tile
    heuristic choosing: these are the TM = 4 / TM = 2 instances the default --val-batch-size runs."""
    from adalog_amd import quant_layers as Q
    D, H = {"deit_small": (384, 6), "vit_base": (768, 12)}[model]
    T, bits = 197, 4
    M = images * T
    g = torch.Generator().manual_seed(images + D)
    tms = {"qkv": pick_tm_out(M, 3 * D, 1, gen=True), "fc1": pick_tm_out(M, 4 * D, 1, gen=True),
           "proj": pick_tm_out(M, D, 1, gen=True), "fc2": pick_tm_out(M, D, 1), "qk": pick_tm_out(T, T, images * H),
           "sv": pick_tm_out(T, 64, images * H)}
    if images == 200 and model == "deit_small":
        assert tms["qk"] == 4 and tms["sv"] == 4 and tms["fc2"] == 2 and tms["qkv"] == 2 and tms["proj"] == 2, tms
    if images == 48:
        assert tms["qk"] == 4, tms
    worst = {}
    with torch.no_grad():
        x = (torch.randn(images, T, D, generator=g) * 1.5).to(DEV)
        for name, I, O_, nv in (("qkv", D, 3 * D, 3), ("proj", D, D, 1), ("fc1", D, 4 * D, 1)):
            lay = _linear("linear", I, O_, bits, g, nv)
            QC.arm(lay.a_quantizer, *QC.minmax_params(x, bits))
            add = x if name == "proj" else None
            got = lay.quant_forward(x, addend=add)
            ref, bar = QR.linear_qf(lay, x, addend=add)
            worst[name] = QR.check(got, ref, bar, f"{model} {name}")
            del got, ref, bar
        lay = _linear("postgelu", 4 * D, D, bits, g)
        h = (torch.randn(images, T, 4 * D, generator=g) * 2).to(DEV)
        aq = lay.a_quantizer
        aq.scale.data.fill_((float(torch.nn.functional.gelu(h).max()) + QC.GELU_SHIFT) * 0.9)
        aq.q.fill_(41)
        aq.update_table(41)
        aq.inited = True
        lay._q_host = None
        got = lay.quant_forward(h, addend=x, pre_gelu=True)
        ref, bar, amb = QR.postgelu_qf(lay, h, pre_gelu=True, addend=x)
        worst["fc2"] = QR.check(got, ref, bar, f"{model} fc2")
        worst["amb_fc2"] = amb
        assert amb < 1e-2                                    # (GELU's fp32 error widens delta where GELU(x) + shift is near 0)
        del h, got, ref, bar
        mm = Q.AsymmetricallyBatchingQuantMatMul(bits, bits, "quant_forward", head_channel_wise=True, num_heads=H, fpcs=True).to(DEV)
        q = (torch.randn(images, H, T, 64, generator=g) * (0.5 + torch.rand(1, H, 1, 1, generator=g))).to(DEV)
        kt = (torch.randn(images, H, T, 64, generator=g) * 1.3).to(DEV).transpose(-2, -1)
        QC.arm(mm.A_quantizer, *QC.minmax_params(q, bits, per=(1,)))
        QC.arm(mm.B_quantizer, *QC.minmax_params(kt, bits, per=(1,)))
        mm.calibrated = True
        ref, bar = QR.matmul_qf(mm, q, kt)
        worst["qk"] = QR.check(mm(q, kt), ref, bar, f"{model} q.k^T")
        del q, kt, ref, bar
        ps = Q.PostSoftmaxAsymmetricallyBatchingQuantMatMul(bits, bits, "quant_forward", head_channel_wise=True, num_heads=H, fpcs=True,
                                                           quantizer="adalog").to(DEV)
        P = (torch.randn(images, H, T, T, generator=g) * 3).to(DEV).softmax(-1)
        v = (torch.randn(images, H, T, 64, generator=g) * 1.2).to(DEV)
        QC.arm(ps.B_quantizer, *QC.minmax_params(v, bits, per=(1,)))
        ps.A_quantizer.q.fill_(29)
        ps.A_quantizer.update_table(29)
        ps._q_host = None
        ps.calibrated = True
        ref, bar, amb = QR.postsoftmax_qf(ps, P, v)
        worst["sv"] = QR.check(ps(P, v), ref, bar, f"{model} softmax.v")
        worst["amb_sv"] = amb
        assert amb < 1e-3
    _report({"case": "validate_shapes", "model": model, "images": images, "tm": tms, "worst_err_over_bar": worst})


# ================================================================================================= c. the fused block, stage by stage
BLOCKS = [  # (dim, heads, B, N, bits, head_channel_wise, bias_reparamed, fused)
    (192, 3, 8, 197, 4, True, False, True), (384, 6, 200, 197, 4, True, True, True), (768, 12, 48, 197, 6, True, False, True),
    (384, 6, 1, 1, 3, True, True, True), (384, 6, 3, 65, 6, True, False, True), (384, 6, 5, 256, 4, True, True, True),
    (384, 6, 3, 65, 2, True, False, True), (192, 3, 8, 197, 7, True, True, True), (192, 3, 8, 197, 3, False, False, True),
    (384, 6, 2, 257, 4, True, False, False), (256, 8, 4, 50, 6, True, True, False)]


@pytest.mark.parametrize("dim,heads,B,N,bits,hcw,reparamed,fused", BLOCKS)
def test_fused_block_stages_against_fp64(monkeypatch, dim, heads, B, N, bits, hcw, reparamed, fused):
    """A wrapped ViT block armed with on-grid min/max parameters: every stage of one quant_forward (qkv; attention core; proj +
    residual; fc1; GELU -> AdaLog -> fc2 + residual) within its bar on its recorded input, the stages' plumbing bit for bit, and
    the route the block took (fused: the split-pack and softmax-pack launches ran; > 256 tokens or head_dim != 64: module route)."""
    from adalog_amd import ops
    calls = {"split": 0, "softmax": 0}
    split0, soft0 = ops.attn_split_pack, ops.softmax_adalog_pack

    def split(*a, **k):
        calls["split"] += 1
        return split0(*a, **k)

    def soft(*a, **k):
        calls["softmax"] += 1
        return soft0(*a, **k)
    monkeypatch.setattr(ops, "attn_split_pack", split)
    monkeypatch.setattr(ops, "softmax_adalog_pack", soft)
    blk, x = QC.make_block(dim, heads, bits, B, N, DEV, head_channel_wise=hcw, bias_reparamed=reparamed, seed=dim + B + bits)
    calls.update(split=0, softmax=0)
    rep = QC.run_and_check_block(blk, x, fused_expected=fused)
    assert (calls["split"] == 1 and calls["softmax"] == 1) if fused else (calls["split"] == 0 and calls["softmax"] == 0), calls
    assert rep["amb_core"] < 1e-3 and rep["amb_fc2"] < 1e-2, rep
    _report({"case": "block", "shape": [dim, heads, B, N], "bits": bits, "head_channel_wise": hcw, "bias_reparamed": reparamed,
             "fused": fused, **{k: v for k, v in rep.items() if k != "y"}})


# ================================================================================================= d. whole model at validate()'s batch
def test_deit_small_at_validate_batch_fused_module_and_graph(monkeypatch):
    """A calibrated deit_small at 200 images: the fused block route against the module route (<= 1e-5, as
    test_gpu_e2e.py::test_fused_block_quant_forward_matches_the_module_route requires at 8 images), and the captured-graph replay
    (utils/graph_forward.py) bit-identical to the eager forward."""
    from tests.test_gpu_e2e import _cfg
    from adalog_amd.utils import models as M
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.graph_forward import GraphedForward
    from adalog_amd.utils.models import create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    torch.manual_seed(6)
    model = wrap_modules_in_net(create_model("deit_small").eval(), _cfg(4), reparam=True).to(DEV)
    xc = torch.randn(16, 3, 224, 224, generator=torch.Generator().manual_seed(6)).to(DEV)
    QuantCalibrator(model, [(xc, None)], capture="block").batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model).to(DEV).eval()
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
        if hasattr(m, "mode"):
            m.mode = "quant_forward"
    x = torch.randn(200, 3, 224, 224, generator=torch.Generator().manual_seed(7)).to(DEV)
    from adalog_amd import ops
    calls = []
    split0 = ops.attn_split_pack
    monkeypatch.setattr(ops, "attn_split_pack", lambda *a, **k: calls.append(1) or split0(*a, **k))
    try:
        M.QF_FUSED = False
        with torch.no_grad():
            y_mod = model(x)
        assert not calls
        M.QF_FUSED = True
        with torch.no_grad():
            y_fused = model(x)
    finally:
        M.QF_FUSED = True
    assert len(calls) == 12, len(calls)                      # every block took the fused route
    rel = ((y_fused - y_mod).norm() / y_mod.norm()).item()
    assert torch.isfinite(y_fused).all() and rel <= 1e-5, rel
    gf = GraphedForward(model)
    y_g1 = gf(x)
    y_g2 = gf(x)                                             # a replay of the captured graph
    assert torch.equal(y_g1, y_fused) and torch.equal(y_g2, y_fused)
    _report({"case": "deit_small_200", "fused_vs_module_rel": rel})


# ================================================================================================= e. zero points at the grid's edges
def _zp_linear(bits, z, g, w_z=None):
    lay = _linear("linear", 64, 96, bits, g)
    x = (torch.randn(3, 40, 64, generator=g) * 2).to(DEV)
    s = (x.max() - x.min()) / (2 ** bits - 1)
    QC.arm(lay.a_quantizer, s.view(1), torch.tensor([float(z)], device=DEV))
    if w_z is not None:
        lay.w_quantizer.zero_point.data.fill_(float(w_z))
        lay.invalidate_packed_weight()
    return lay, x


@pytest.mark.parametrize("bits,z", [(4, 0), (4, 15), (6, 0), (6, 63), (7, 127), (6, -70), (6, 200), (7, -5), (7, 140)])
def test_zero_points_at_and_beyond_the_grid(monkeypatch, bits, z):
    """Zero points 0 and 2^b - 1 run on the packed int8 routes; zero points outside [qmax - 127, 128] give codes q - rne(z) beyond
    int8 and must still produce the reference's value clamp(rne(x / s) + rne(z), 0, qmax) - rne(z): through a Linear on both its
    routes (the generating loader, and pack + gemm_out), its weight quantiser, the q . k^T layer and the fused attention split."""
    from adalog_amd import quant_layers as Q
    g = torch.Generator().manual_seed(bits * 1000 + z % 997)
    inside = (2 ** bits - 1) - 127 <= z <= 128
    kind = "i8" if inside else "f32"
    with torch.no_grad():
        for gen in ("1", "0"):
            monkeypatch.setenv("ADALOG_QF_GEN", gen)
            lay, x = _zp_linear(bits, z, g)
            ref, bar = QR.linear_qf(lay, x, kind=kind)
            QR.check(lay(x), ref, bar, f"linear a_zp={z} gen={gen}")
            lay, x = _zp_linear(bits, 3, g, w_z=z)
            ref, bar = QR.linear_qf(lay, x, kind=kind)
            QR.check(lay(x), ref, bar, f"linear w_zp={z} gen={gen}")
        monkeypatch.delenv("ADALOG_QF_GEN")
        H = 3
        mm = Q.AsymmetricallyBatchingQuantMatMul(bits, bits, "quant_forward", head_channel_wise=True, num_heads=H, fpcs=True).to(DEV)
        A = torch.randn(2, H, 33, 64, generator=g).to(DEV)
        Bt = torch.randn(2, H, 33, 64, generator=g).to(DEV).transpose(-2, -1)
        sA, _ = QC.minmax_params(A, bits, per=(1,))
        QC.arm(mm.A_quantizer, sA, torch.tensor([float(z), 1.0, 2.0], device=DEV))
        QC.arm(mm.B_quantizer, *QC.minmax_params(Bt, bits, per=(1,)))
        mm.calibrated = True
        ref, bar = QR.matmul_qf(mm, A, Bt, kind=kind)
        QR.check(mm(A, Bt), ref, bar, f"q.k^T a_zp={z}")
    blk, x = QC.make_block(384, 6, bits, 2, 65, DEV, seed=bits)
    kq = blk.attn.matmul1.B_quantizer
    kq.zero_point.data[0, 1] = float(z)                      # one head's k zero point
    kq.forget_codes_fit()
    vq = blk.attn.matmul2.B_quantizer
    rep = QC.run_and_check_block(blk, x, fused_expected=inside)
    _report({"case": "zero_point", "bits": bits, "z": z, "inside": inside, **{k: v for k, v in rep.items() if k != "y"}})
    assert vq.codes_fit(-256, 256)
