"""`-m gpu`: the fused quant_forward route for 257 to 1024 tokens per attention group (models.QF_LONG; ops.softmax_adalog_pack_long,
ops.attn_core_long; csrc/operand.hip, csrc/attn_core.hip) and for ViT head dimensions 16, 32 and 48.

Everything here is an equality, as for the <= 256-token kernels: the long softmax pack against torch's softmax followed by the packer
(the kernel restates ATen's per-warp softmax at 8 and 16 slots per lane, which ATen uses up to 1024 elements per row -- the bound
of the feature), the long attention core against the three launches it replaces, blocks and a 384-px model with the switch on against
the module route, the captured graph against the eager forward.  The fp64 stage check of tests/qf_cases.py runs over the long route
with the bars and the ambiguity caps of tests/test_gpu_quant_forward.py."""
import json
import os

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


def _report(entry):
    """printed, and appended as a JSON line to the file named by ADALOG_QF_REPORT (unset: nothing is written)"""
    print(json.dumps(entry))
    path = os.environ.get("ADALOG_QF_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(entry) + "\n")


class _switches:
    """models.QF_FUSED / QF_LONG / QF_ATTN_CORE set for a `with` block and put back"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from adalog_amd.utils import models as M
        self.old = {k: getattr(M, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(M, k, v)

    def __exit__(self, *exc):
        from adalog_amd.utils import models as M
        for k, v in self.old.items():
            setattr(M, k, v)


def _count_calls(monkeypatch):
    from adalog_amd import ops
    names = {"core": "attn_core", "core_long": "attn_core_long", "softmax": "softmax_adalog_pack", "softmax_long": "softmax_adalog_pack_long",
             "split": "attn_split_pack", "split_ex": "attn_split_pack_ex"}
    calls = {k: 0 for k in names}
    for key, name in names.items():
        fn0 = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _k=key, _f=fn0, **kw: calls.__setitem__(_k, calls[_k] + 1) or _f(*a, **kw))
    return calls


def _zero(calls):
    for k in calls:
        calls[k] = 0


# ================================================================================================= 1. the long softmax pack
@pytest.mark.parametrize("bits", [3, 4, 6])
@pytest.mark.parametrize("S", [257, 320, 511, 512, 513, 577, 785, 1024])
def test_softmax_adalog_pack_long_equals_softmax_then_pack(ops, bits, S):
    """The comparison of tests/test_gpu_kernels.py::test_softmax_adalog_pack_equals_softmax_then_pack for long rows: bit-equal to
    pack_adalog of (x * mul).softmax(-1) as ATen computes it.  Row counts that are no multiple of the rows a workgroup takes; rows with
    one dominant score, with every score equal, with equal pairs, with saturating exponents, and with most probabilities in the
    quantiser's masked bin."""
    from tests.test_gpu_kernels import _adalog_pack_params
    G, R = 3, 43
    gen = g(31000 + bits * 7 + S)
    x = torch.randn(G, R, S, generator=gen) * 6
    x[0, 0] = 0.0                                                     # every score equal
    x[0, 1, :3] = torch.tensor([80.0, -80.0, 79.5])                   # saturating exponents
    x[0, 2] = torch.randn(S, generator=gen) * 0.01
    x[0, 2, S - 1] = 400.0                                            # one dominant score, in the last slot: all else in the masked bin
    x[0, 3, S // 2: 2 * (S // 2)] = x[0, 3, : S // 2]                 # equal pairs
    x[0, 4] = torch.randint(-3, 4, (S,), generator=gen).float() * 8   # many exact ties
    x[1, :, 256:] -= 600.0                                            # slots past the short kernel's four: masked bin
    x[2] *= 4.0                                                       # peaked rows: probabilities on many levels at every bit width
    x = x.to(DEV)
    mant, qv = _adalog_pack_params(bits)
    scale = torch.ones(1, device=DEV)
    mul = 0.125
    assert ops.softmax_adalog_pack_long_ok(S) and not ops.softmax_adalog_pack_ok(S)
    probs = (x * mul).softmax(dim=-1)
    want = ops.pack_adalog(probs, scale, qv, 1, 0, 1, 0, bits, mant, shift=None, clamp_u=True)
    got = ops.softmax_adalog_pack_long(x, mul, scale, qv, bits, mant)
    assert got.shape == want.shape == (1, G, R, ops.pad_k(S, ops.BF16)) and got.dtype == torch.bfloat16
    same = (got.view(torch.int16) == want.view(torch.int16)).float().mean().item()
    assert same == 1.0, same
    assert (got[..., S:] == 0).all()
    # the planted rows are what they claim: a dominant row quantises to one non-zero code, image 1's tail is in the masked bin
    assert (got[0, 0, 2, :S] != 0).sum().item() == 1 and got[0, 0, 2, S - 1] != 0
    assert (got[0, 1, :, 256:S] == 0).all()
    assert (got[0, 2, :, :S] != 0).sum(-1).min().item() >= 1 and got[0, 2, :, :S].float().unique().numel() >= 2 ** (bits - 1)
    assert getattr(got, "k_valid", None) == S


# ================================================================================================= 2. the long attention core
def _three_launches_long(ops, qp, kp, vp, N, D, H, gmod, par, ps, bits, mul):
    """the route ops.attn_core_long replaces, on the same packed operands"""
    G = qp.shape[1]
    pg = 1 if gmod > 1 else 0
    sA, sB, sV = par[0][0], par[1][0], par[2][0]
    qv = torch.tensor([float(int(ps.A_quantizer.q.item()))], device=DEV)
    a_scale = ps.A_quantizer.scale.data.view(-1)
    scores = ops.gemm_out(ops.I8, qp, kp, N, N, G, gmod, ops.Strided(sA, g=pg), ops.Strided(sB, g=pg), None)
    ap = ops.softmax_adalog_pack_long(scores, mul, a_scale, qv, bits, ps._mant37(DEV))
    out = ops.gemm_out(ops.BF16, ap, vp, N, D, G, gmod, ops.Strided(a_scale), ops.Strided(sV, g=pg), None, sa_mul=ps._ts32(),
                       heads_last=H)
    return out, scores, ap, qv, a_scale


@pytest.mark.parametrize("D", [16, 32, 48, 64])
@pytest.mark.parametrize("N", [257, 577, 1024])
@pytest.mark.parametrize("per_head", [True, False])
def test_attn_core_long_equals_the_three_launches(ops, D, N, per_head):
    """torch.equal to gemm_out(I8) -> softmax_adalog_pack_long -> gemm_out(BF16, heads_last) on the same packed operands: both slot
    counts (8 and 16), a last row tile of one row (257, 577) and a full one (1024), every head dimension, per-head and per-tensor
    scales, q / k / v at 3 / 5 / 7 bits, the post-softmax quantiser at 3, 6 and 7 bits; the planted rows of
    tests/test_gpu_attn_core.py (a row of equal scores, rows of equal pairs, an image of extreme codes)."""
    from tests.test_gpu_attn_core import _plant, _post_softmax, _quantisers
    H, B = 3, 3
    gen = g(32000 + D * 7 + N + (1 if per_head else 0))
    qkv = torch.randn(B, N, 3 * H * D, generator=gen) * 1.3
    _plant(qkv, B, N, H, D)
    par = _quantisers(H, per_head, gen)
    qp, kp, vp = ops.attn_split_pack_ex(qkv.to(DEV), H, par[0], par[1], par[2], per_head, D=D)
    gmod = H if per_head else 1
    mul = D ** -0.5
    assert ops.attn_core_long_ok(N, D) and not ops.attn_core_ok(N, D)
    for bits, scale in ((3, 1.0), (6, 0.7), (7, None)):
        ps = _post_softmax(bits, H, scale=scale)
        want, scores, ap, qv, a_scale = _three_launches_long(ops, qp, kp, vp, N, D, H, gmod, par, ps, bits, mul)
        got = ops.attn_core_long(qp, kp, vp, N, D, H, gmod, par[0][0], par[1][0], par[2][0], mul, a_scale, qv, bits, ps._mant37(DEV),
                                 ps._ts32())
        assert got.shape == want.shape == (B, N, H, D) and got.dtype == torch.float32
        assert torch.equal(got, want), (bits, (got - want).abs().max().item(), (got != want).float().mean().item())
        assert bits < 7 or want.abs().max().item() > 0                      # (coarse quantisers may put a whole long row in the zero bin)
    sc = scores.view(B, H, N, N)
    assert (sc[0, :, 0] == sc[0, :, 0, :1]).all()
    assert torch.equal(sc[1, :, :, : N // 2], sc[1, :, :, N // 2: 2 * (N // 2)])


def test_attn_core_long_at_short_rows_equals_attn_core(ops):
    """the entry point takes every N from 1 on (four slots per lane up to 256): there it equals attn_core"""
    from tests.test_gpu_attn_core import _plant, _post_softmax, _quantisers
    H, B, D = 3, 2, 32
    for N in (1, 65, 197, 256):
        gen = g(32500 + N)
        qkv = torch.randn(B, N, 3 * H * D, generator=gen) * 1.3
        _plant(qkv, B, N, H, D)
        par = _quantisers(H, True, gen)
        qp, kp, vp = ops.attn_split_pack_ex(qkv.to(DEV), H, par[0], par[1], par[2], True, D=D)
        ps = _post_softmax(4, H)
        qv = torch.tensor([float(int(ps.A_quantizer.q.item()))], device=DEV)
        a_scale = ps.A_quantizer.scale.data.view(-1)
        args = (qp, kp, vp, N, D, H, H, par[0][0], par[1][0], par[2][0], D ** -0.5, a_scale, qv, 4, ps._mant37(DEV), ps._ts32())
        assert torch.equal(ops.attn_core_long(*args), ops.attn_core(*args)), N


# ================================================================================================= 3. blocks: route, module route, fp64
# (dim, heads, B, N, bits, head_channel_wise, bias_reparamed).  The seeds were checked first on the CPU with tests/qf_reference.py alone
# (qf_cases.make_block on the CPU specification backend, qf_reference.block_stages): the share of the core's elements on a boundary-flip
# allowance is 3.3e-4, 6.3e-4, 6.8e-5, 3.8e-4 and 4.3e-5 in this order (cap 1e-3), of fc2's 2.0e-3 to 2.9e-3 (cap 1e-2).
LONG_BLOCKS = [
    (384, 6, 2, 577, 4, True, False), (768, 12, 2, 577, 6, True, True), (192, 6, 2, 577, 4, True, False),
    (384, 6, 2, 577, 3, False, True), (192, 6, 3, 197, 4, True, False)]


def _block_seed(dim, B, bits, N):
    return dim + B + bits + N


@pytest.mark.parametrize("dim,heads,B,N,bits,hcw,reparamed", LONG_BLOCKS)
def test_long_block_routes_module_route_and_fp64(monkeypatch, dim, heads, B, N, bits, hcw, reparamed):
    """A wrapped ViT block (tests/qf_cases.make_block) at 577 tokens -- head dimension 64 (dim 384 / 6 heads, dim 768 / 12 heads) and
    32 (dim 192 / 6 heads) -- and a head-dimension-32 block at 197 tokens.  Switch off: the module route, as before.  Switch on: the
    fused route through the long softmax pack (or, for <= 256 tokens, the short one), with the attention core switch as well the
    one-launch core; the output torch.equal to the module route's either way; every stage within its fp64 bar
    (qf_cases.run_and_check_block, unchanged) with the share of elements that use a boundary-flip allowance under the caps of
    tests/test_gpu_quant_forward.py (written to the ADALOG_QF_REPORT file)."""
    calls = _count_calls(monkeypatch)
    blk, x = QC.make_block(dim, heads, bits, B, N, DEV, head_channel_wise=hcw, bias_reparamed=reparamed,
                           seed=_block_seed(dim, B, bits, N))
    D = dim // heads
    long_rows = N > 256
    with torch.no_grad():
        xn = blk.norm1(x)
    with _switches(QF_FUSED=True, QF_LONG=False, QF_ATTN_CORE=True):
        assert not blk.attn._fused_quant_forward_ok(xn)                      # today's default: declined
    with _switches(QF_FUSED=False, QF_LONG=True, QF_ATTN_CORE=False):
        assert not blk.attn._fused_quant_forward_ok(xn)
        _zero(calls)
        with torch.no_grad():
            y_mod = blk(x)
        assert not any(calls.values()), calls
    want_split = {"split": 1, "split_ex": 0} if D == 64 else {"split": 0, "split_ex": 1}
    rep = {}
    for core in (False, True):
        with _switches(QF_FUSED=True, QF_LONG=True, QF_ATTN_CORE=core):
            with torch.no_grad():
                assert blk.attn._fused_quant_forward_ok(xn)
            _zero(calls)
            rep[core] = QC.run_and_check_block(blk, x, fused_expected=True)
        want = dict(core=0, core_long=0, softmax=0, softmax_long=0, **want_split)
        want[("core_long" if long_rows else "core") if core else ("softmax_long" if long_rows else "softmax")] = 1
        assert calls == want, (core, calls)
        r = rep[core]
        _report({"case": "long_block", "shape": [dim, heads, B, N], "bits": bits, "head_channel_wise": hcw, "bias_reparamed": reparamed,
                 "attn_core": core, "equal_to_module_route": bool(torch.equal(r["y"], y_mod)),
                 "max_abs_diff_to_module_route": (r["y"] - y_mod).abs().max().item(), **{k: v for k, v in r.items() if k != "y"}})
        assert r["amb_core"] < 1e-3 and r["amb_fc2"] < 1e-2, r
        assert torch.equal(r["y"], y_mod), (core, (r["y"] - y_mod).abs().max().item())
    assert torch.equal(rep[True]["y"], rep[False]["y"])


def test_switch_on_keeps_other_blocks_on_their_routes(monkeypatch):
    """With QF_LONG on: 1025 tokens and a head dimension of 24 stay on the module route; a 197-token head-dimension-64 block takes the
    launches it takes with the switch off (attn_split_pack, softmax_adalog_pack) and gives the same bits."""
    calls = _count_calls(monkeypatch)
    for dim, heads, N in ((384, 6, 1025), (144, 6, 65)):
        blk, x = QC.make_block(dim, heads, 4, 1, N, DEV, seed=500 + N)
        with _switches(QF_FUSED=True, QF_LONG=True, QF_ATTN_CORE=True), torch.no_grad():
            assert not blk.attn._fused_shape_ok(N) and not blk.attn._fused_quant_forward_ok(blk.norm1(x))
            _zero(calls)
            y_on = blk(x)
            assert not any(calls.values()), calls
        with _switches(QF_FUSED=False):
            with torch.no_grad():
                assert torch.equal(blk(x), y_on)
    blk, x = QC.make_block(384, 6, 4, 2, 197, DEV, seed=597)
    with _switches(QF_FUSED=True, QF_LONG=False, QF_ATTN_CORE=False), torch.no_grad():
        y_off = blk(x)
    with _switches(QF_FUSED=True, QF_LONG=True, QF_ATTN_CORE=False), torch.no_grad():
        _zero(calls)
        y_on = blk(x)
    assert calls == dict(core=0, core_long=0, softmax=1, softmax_long=0, split=1, split_ex=0), calls
    assert torch.equal(y_on, y_off)


# ================================================================================================= 4. a 384-px model
def _armed_deit_small_384(bits=4):
    """create_model("deit_small", depth=2, img_size=384), wrapped; the quantisers of its two blocks armed as qf_cases.make_block arms a
    block's (on-grid min/max parameters from a raw forward of the model's own input) and switched to quant_forward; the patch embedding
    and the head stay raw.  -> (model, x [4, 3, 384, 384], blocks)"""
    from adalog_amd.utils.models import Block, create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net
    torch.manual_seed(38)
    model = create_model("deit_small", depth=2, img_size=384).eval()
    gen = g(384)
    for m in model.modules():
        if isinstance(m, torch.nn.Linear) and m.weight.shape[0] != 1000:
            m.weight.data.copy_(torch.randn(m.weight.shape, generator=gen) * 0.06)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=gen) * 0.05)
    model = wrap_modules_in_net(model, QC.cfg(bits)).to(DEV)
    x = torch.randn(4, 3, 384, 384, generator=gen).to(DEV)
    blocks = [m for m in model.modules() if isinstance(m, Block)]
    assert len(blocks) == 2
    seen = {}
    hooks = []
    for i, b in enumerate(blocks):
        for name, mod in (("qkv", b.attn.qkv), ("proj", b.attn.proj), ("fc1", b.mlp.fc1), ("fc2", b.mlp.fc2)):
            hooks.append(mod.register_forward_pre_hook(lambda m, a, k=(i, name): seen.__setitem__(k, a[0])))
        for name, mod in (("mm1", b.attn.matmul1), ("mm2", b.attn.matmul2)):
            hooks.append(mod.register_forward_pre_hook(lambda m, a, k=(i, name): seen.__setitem__(k, a)))
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    for i, b in enumerate(blocks):
        attn, mlp = b.attn, b.mlp
        for lay in (attn.qkv, attn.proj, mlp.fc1, mlp.fc2):
            QC.arm(lay.w_quantizer, *QC.minmax_params(lay.weight.data.view(lay.n_V, lay.crb_rows, -1), bits, per=(0, 1)))
        for name, lay in (("qkv", attn.qkv), ("proj", attn.proj), ("fc1", mlp.fc1)):
            QC.arm(lay.a_quantizer, *QC.minmax_params(seen[(i, name)], bits))
        m1, m2 = attn.matmul1, attn.matmul2
        QC.arm(m1.A_quantizer, *QC.minmax_params(seen[(i, "mm1")][0], bits, per=(1,)))
        QC.arm(m1.B_quantizer, *QC.minmax_params(seen[(i, "mm1")][1], bits, per=(1,)))
        QC.arm(m2.B_quantizer, *QC.minmax_params(seen[(i, "mm2")][1], bits, per=(1,)))
        m2.A_quantizer.q.fill_(29)
        m2.A_quantizer.update_table(29)
        m2._q_host = None
        aq = mlp.fc2.a_quantizer
        aq.shift.data.fill_(QC.GELU_SHIFT)
        aq.scale.data.fill_((float(seen[(i, "fc2")].max()) + QC.GELU_SHIFT) * 0.9)
        aq.q.fill_(41)
        aq.update_table(41)
        aq.inited = True
        mlp.fc2._q_host = None
        for m in b.modules():
            if hasattr(m, "calibrated"):
                m.calibrated = True
                m.mode = "quant_forward"
    return model, x, blocks


def test_deit_small_384_long_route_equals_module_route_and_graph(monkeypatch):
    """deit_small at 384 px (577 tokens), two blocks, 4 images: with the switch off the attention of every block takes the module
    route even with QF_FUSED on (today's behaviour); with it on, one long softmax pack per block and far fewer
    kernels; with the attention core as well, one attn_core_long per block and two kernels fewer per block.  The logits of both equal
    the module route's bit for bit, and a captured graph replays to the eager result."""
    from tests.test_gpu_swin_quant_forward import _kernels
    from adalog_amd.utils.graph_forward import GraphedForward
    model, x, blocks = _armed_deit_small_384()
    calls = _count_calls(monkeypatch)
    nb = len(blocks)
    with _switches(QF_FUSED=False, QF_LONG=True, QF_ATTN_CORE=True):
        y_mod, n_mod = _kernels(model, x)
        assert not any(calls.values()), calls
    with _switches(QF_FUSED=True, QF_LONG=False, QF_ATTN_CORE=True):
        y_off, n_off = _kernels(model, x)
        assert not any(calls.values()), calls                               # the attention declines (the MLP's fused half still runs)
    with _switches(QF_FUSED=True, QF_LONG=True, QF_ATTN_CORE=False):
        _zero(calls)
        y_long, n_long = _kernels(model, x)
        assert calls == dict(core=0, core_long=0, softmax=0, softmax_long=2 * nb, split=2 * nb, split_ex=0), calls
        gf = GraphedForward(model)
        assert all(torch.equal(gf(x), y_long) for _ in range(3))
    with _switches(QF_FUSED=True, QF_LONG=True, QF_ATTN_CORE=True):
        _zero(calls)
        y_core, n_core = _kernels(model, x)
        assert calls == dict(core=0, core_long=2 * nb, softmax=0, softmax_long=0, split=2 * nb, split_ex=0), calls
        gf = GraphedForward(model)
        assert all(torch.equal(gf(x), y_core) for _ in range(3))
    _report({"case": "deit_small_384_depth2", "kernels_module": n_mod, "kernels_long_off": n_off, "kernels_long_on": n_long,
             "kernels_long_on_core": n_core, "long_equal": bool(torch.equal(y_long, y_mod)),
             "long_max_abs_diff": (y_long - y_mod).abs().max().item()})
    assert torch.isfinite(y_mod).all() and y_mod.abs().max().item() > 0
    assert torch.equal(y_long, y_mod) and torch.equal(y_core, y_mod)
    # a block's module route is 22 launches, its fused route 11, with the one-launch core 9
    assert n_long == n_mod - 11 * nb, (n_mod, n_long)
    assert n_core == n_long - 2 * nb, (n_long, n_core)
