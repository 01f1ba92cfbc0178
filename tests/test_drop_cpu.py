"""QDrop on the CPU tier: the Philox keep mask of adalog_amd/quantizers/_drop.py against an independent numpy generator
(tests/drop_reference.py), the quantisers' composed drop route against fp64 autograd of where(mask, fq(x), x), and the
reconstruction loop with drop_prob."""
import math

import numpy as np
import pytest
import torch

from adalog_amd import backend
from adalog_amd.quantizers import _drop
from adalog_amd.quantizers.logarithm import AdaLogQuantizer, ShiftAdaLogQuantizer
from adalog_amd.quantizers.uniform import UniformQuantizer
from tests import cpu_backend, drop_reference as DR

SEEDS = (1234, 0xC0FFEE1234567890)


@pytest.fixture(autouse=True)
def _cpu_backend():
    backend.set_backend(cpu_backend)
    yield
    backend.set_backend(None)


def test_reference_generator_known_answers():
    for ctr, key, want in DR.KAT:
        got = tuple(int(v) for v in DR.philox4x32_10(ctr, key))
        assert got == want, [hex(v) for v in got]
        mine = tuple(int(v) for v in _drop.philox4x32_10(*[torch.tensor(c, dtype=torch.int64) for c in ctr], *key))
        assert mine == want


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
@pytest.mark.parametrize("seed", SEEDS)
def test_keep_mask_equals_the_numpy_generator(n, seed):
    for stream in (0, 5):
        for it in (0, 1, 2 ** 31 - 1):
            for p in (0.25, 0.5):
                got = _drop.philox_keep_mask(seed, stream, it, n, p, "cpu")
                assert got.dtype == torch.bool and got.shape == (n,)
                assert np.array_equal(got.numpy(), DR.keep_mask(seed, stream, it, n, p)), (stream, it, p)
                state = _drop.make_state(seed, it, "cpu")
                assert torch.equal(_drop.keep_mask_from_state(state, stream, n, p), got)


def test_keep_mask_extremes_and_streams():
    assert bool(_drop.philox_keep_mask(1234, 0, 0, 1027, 1.0, "cpu").all())
    assert not bool(_drop.philox_keep_mask(1234, 0, 0, 1027, 0.0, "cpu").any())
    a = _drop.philox_keep_mask(1234, 0, 0, 1027, 0.5, "cpu")
    for other in (_drop.philox_keep_mask(1234, 1, 0, 1027, 0.5, "cpu"), _drop.philox_keep_mask(1234, 0, 1, 1027, 0.5, "cpu"),
                  _drop.philox_keep_mask(1235, 0, 0, 1027, 0.5, "cpu")):
        assert not torch.equal(a, other)


@pytest.mark.parametrize("p", [0.25, 0.5])
def test_kept_fraction(p):
    """|kept / n - p| <= 5 sigma of the binomial (deterministic for the fixed seed)"""
    n = 65536
    for seed in SEEDS:
        kept = int(_drop.philox_keep_mask(seed, 0, 0, n, p, "cpu").sum())
        print(f"seed {seed:#x} p {p}: kept/n = {kept / n:.6f}")
        assert abs(kept / n - p) <= 5 * math.sqrt(p * (1 - p) / n)


# ------------------------------------------------------------------------------------------------ quantisers, composed route
def _uniform(sym, per_head):
    q = UniformQuantizer(n_bits=4, symmetric=sym)
    n = 3 if per_head else 1
    shape = (1, n, 1, 1) if per_head else (1,)
    q.scale = torch.nn.Parameter((0.21 + 0.05 * torch.arange(n, dtype=torch.float32)).reshape(shape))
    q.zero_point = torch.nn.Parameter((7.0 + torch.arange(n, dtype=torch.float32)).reshape(shape), requires_grad=False)
    q.inited = True
    return q


def _adalog(shift):
    q = (ShiftAdaLogQuantizer if shift else AdaLogQuantizer)(n_bits=4)
    q.scale = torch.nn.Parameter(torch.tensor([2.3]))
    if shift:
        q.shift.data.fill_(0.17)
    q.inited = True
    return q


def _fq64_uniform(x, s, z, bits, sym):
    L = 2 ** (bits - 1)
    ste = lambda v: (v.round() - v).detach() + v
    if sym:
        return ste(x / s).clamp(-L, L - 1) * s
    return ((ste(x / s) + z.round()).clamp(0, 2 * L - 1) - z.round()) * s


def _fq64_adalog(x, s, q, bits, shift, sub):
    L = 2 ** (bits - 1)
    ste = lambda v: (v.round() - v).detach() + v
    xs = x if shift is None else x + shift
    u = (xs / s).clamp(min=1e-15, max=1.0)
    k = ste(-u.log2() * 37.0 / q)
    mask = k < 2 * L
    out = 2 ** (-1 * torch.clamp(k, 0, 2 * L - 1) * q / 37.0) * s * mask
    return out - shift if sub else out


@pytest.mark.parametrize("kind", ["uniform", "uniform_sym", "uniform_heads", "uniform_kT", "adalog", "shift_adalog", "shift_adalog_reparamed"])
def test_quantiser_drop_route_against_fp64_autograd(kind):
    gen = torch.Generator().manual_seed(77)
    state = _drop.make_state(SEEDS[1], 3, "cpu")
    stream, p = 2, 0.5
    if kind.startswith("uniform"):
        q = _uniform(kind == "uniform_sym", kind in ("uniform_heads", "uniform_kT"))
        x = torch.randn(2, 3, 5, 7, generator=gen) * 1.5
        if kind == "uniform_kT":
            x = x.transpose(-1, -2)                          # a transposed view: quantised (and indexed) in its storage order
    else:
        q = _adalog(kind != "adalog")
        if kind == "shift_adalog_reparamed":
            q.mark_bias_reparamed()
        x = torch.nn.functional.gelu(2 * torch.randn(2, 5, 33, generator=gen))
    gy = torch.randn(x.shape, generator=gen)
    q.init_training()
    # drop_prob = 1.0 / no state attached: bitwise today's route
    xr = x.clone().requires_grad_(True)
    y1 = q(xr)
    y1.backward(gy)
    g1 = (xr.grad.clone(), q.scale.grad.clone())
    q.scale.grad = None
    q.drop_prob = 1.0
    q.attach_drop_state(state, stream)
    xr2 = x.clone().requires_grad_(True)
    y1b = q(xr2)
    y1b.backward(gy)
    assert torch.equal(y1b, y1) and torch.equal(xr2.grad, g1[0]) and torch.equal(q.scale.grad, g1[1])
    assert type(y1b.grad_fn).__name__ == type(y1.grad_fn).__name__
    q.scale.grad = None
    # drop_prob = 0.5
    q.drop_prob = p
    xd = x.clone().requires_grad_(True)
    yd = q(xd)
    yd.backward(gy)
    order = x.transpose(-1, -2) if kind == "uniform_kT" else x
    mask = _drop.philox_keep_mask(SEEDS[1], stream, 3, x.numel(), p, "cpu").view(order.shape)
    assert np.array_equal(mask.reshape(-1).numpy(), DR.keep_mask(SEEDS[1], stream, 3, x.numel(), p))
    if kind == "uniform_kT":
        mask = mask.transpose(-1, -2)
    assert 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(yd.detach(), torch.where(mask, y1.detach(), x))
    # fp64 autograd of the same expression
    x64 = x.double().clone().requires_grad_(True)
    s64 = q.scale.detach().double().clone().requires_grad_(True)
    if kind.startswith("uniform"):
        fq = _fq64_uniform(x64, s64, q.zero_point.detach().double(), 4, q.sym)
    else:
        shift, sub = q._shift_args()
        fq = _fq64_adalog(x64, s64, float(q.q.item()), 4, None if shift is None else shift.detach().double(), sub)
    torch.where(mask, fq, x64).backward(gy.double())
    if kind.startswith("uniform"):                           # the bars of tests/test_gpu_kernels.py test_uniform_backward
        torch.testing.assert_close(xd.grad.double(), x64.grad, rtol=1e-6, atol=0)
        torch.testing.assert_close(q.scale.grad.double(), s64.grad, rtol=1e-4, atol=1e-4)
    else:                                                    # ... test_adalog_backward
        torch.testing.assert_close(xd.grad.double(), x64.grad, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(q.scale.grad.double(), s64.grad, rtol=1e-3, atol=1e-3)
    assert torch.equal(xd.grad[~mask], gy[~mask])            # a dropped element passes its gradient through
    # evaluation ignores drop_prob
    with torch.no_grad():
        y_ng = q(x)
    q.end_training()
    assert q.drop_state is None
    with torch.no_grad():
        y_eval = q(x)
    q.drop_prob = 1.0
    with torch.no_grad():
        assert torch.equal(q(x), y_eval)
    q.init_training()
    with torch.no_grad():
        assert torch.equal(q(x), y_ng)
    assert not torch.equal(y_ng, yd.detach())


# ------------------------------------------------------------------------------------------------ the loop
def _run_loop(golden, own=1.0, **kw):
    from adalog_amd.utils.block_recon import BlockReconstructor
    g = golden("brecq_traj")
    blk, perms = DR.traj_block(g, torch.device("cpu"))
    for q_ in _drop.activation_quantizers(blk):
        q_.drop_prob = own
    rec = object.__new__(BlockReconstructor)
    rec.index_source = lambda it, n, b: perms[it][:b]
    iters, bs = [int(v) for v in g["cfg"]]
    rec.reconstruct_single_block("blk", blk, torch.device("cpu"), batch_size=bs, iters=iters, quant_act=True, **kw)
    for q_ in _drop.activation_quantizers(blk):
        assert q_.drop_state is None and q_.drop_prob == own
    return DR.trained_tensors(blk)


def test_loop_with_drop_prob(golden):
    base = _run_loop(golden)
    one = _run_loop(golden, drop_prob=1.0)
    assert base.keys() == one.keys() and len(base) == 8
    for k in base:
        assert torch.equal(base[k], one[k]), k
    half = _run_loop(golden, drop_prob=0.5)
    assert any(not torch.equal(base[k], half[k]) for k in base if k.endswith(".scale"))
    assert any(not torch.equal(base[k], half[k]) for k in base if k.endswith(".alpha"))
    again = _run_loop(golden, drop_prob=0.5)
    for k in half:
        assert torch.equal(half[k], again[k]), k


def test_loop_takes_the_quantisers_own_drop_prob(golden):
    """what a config's drop_prob (wrap_modules_in_net) or reconstruct_model's leaves on the quantisers is what a call without the
    argument trains with"""
    half, own = _run_loop(golden, drop_prob=0.5), _run_loop(golden, own=0.5)
    for k in half:
        assert torch.equal(half[k], own[k]), k


def test_drop_prob_without_activation_quantisers_is_ignored(golden, caplog):
    from adalog_amd.utils import block_recon
    from adalog_amd.utils.block_recon import BlockReconstructor
    g = golden("brecq_traj")
    outs = []
    for kw in ({}, {"drop_prob": 0.5}):
        blk, perms = DR.traj_block(g, torch.device("cpu"))
        rec = object.__new__(BlockReconstructor)
        rec.index_source = lambda it, n, b: perms[it][:b]
        block_recon._DROP_IGNORED_LOGGED = False
        with caplog.at_level("INFO"):
            rec.reconstruct_single_block("blk", blk, torch.device("cpu"), batch_size=4, iters=5, quant_act=False, **kw)
        outs.append(DR.trained_tensors(blk))
    assert any("is ignored" in r.getMessage() for r in caplog.records)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_drop_seed_mixes_block_and_rank():
    from adalog_amd.utils.block_recon import drop_seed
    seeds = {drop_seed(b, r) for b in range(14) for r in range(8)}
    assert len(seeds) == 14 * 8 and all(0 <= s < 2 ** 64 for s in seeds)


# ------------------------------------------------------------------------------------------------ the CLI's and the config's route to the loop
class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(2, 2)
        self.fc.a_quantizer = UniformQuantizer(n_bits=4)
        self.act = torch.nn.Identity()
        self.act.A_quantizer = AdaLogQuantizer(n_bits=4)


def _stub_reconstructor(monkeypatch):
    from adalog_amd.utils.block_recon import BlockReconstructor
    rec = object.__new__(BlockReconstructor)
    rec.model = _Toy()
    rec.blocks = {"b0": rec.model}
    rec.full_blocks = {"b0": rec.model}
    seen = []
    monkeypatch.setattr(BlockReconstructor, "init_block_raw_data", lambda self, *a, **k: None)
    monkeypatch.setattr(BlockReconstructor, "reconstruct_single_block",
                        lambda self, name, block, *a, **k: seen.append([q_.drop_prob for q_ in _drop.activation_quantizers(block)]))
    return BlockReconstructor, rec, seen


def test_reconstruct_model_sets_the_probability_the_blocks_train_with(monkeypatch):
    cls, rec, seen = _stub_reconstructor(monkeypatch)
    assert cls.drop_prob is None
    rec.reconstruct_model(quant_act=True, iters=1)
    assert seen[-1] == [1.0, 1.0]                                  # nothing given anywhere: off
    rec.reconstruct_model(quant_act=True, iters=1, drop_prob=0.5)
    assert seen[-1] == [0.5, 0.5]
    rec.reconstruct_model(quant_act=True, iters=1)                 # none given: the quantisers' own (a config's, wrap_modules_in_net)
    assert seen[-1] == [0.5, 0.5]
    monkeypatch.setattr(cls, "drop_prob", 0.25)                    # the command line's (quant_qdrop.py)
    rec.reconstruct_model(quant_act=True, iters=1)
    assert seen[-1] == [0.25, 0.25]
    rec.reconstruct_model(quant_act=True, iters=1, drop_prob=1.0)  # the argument wins, and 1.0 switches off
    assert seen[-1] == [1.0, 1.0]
    with pytest.raises(ValueError):
        rec.reconstruct_model(quant_act=True, iters=1, drop_prob=1.5)


def test_config_drop_prob_reaches_the_activation_quantisers():
    import importlib.util
    import os
    from adalog_amd.quant_layers.linear import AsymmetricallyChannelWiseBatchingQuantLinear
    from adalog_amd.utils.models import VisionTransformer
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("cfg4dropcpu", os.path.join(root, "configs", "4bit.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    for want in (1.0, 0.5):
        cfg = mod.Config()
        if want < 1.0:
            cfg.drop_prob = want
        model = VisionTransformer(img_size=32, patch_size=16, embed_dim=24, depth=1, num_heads=3, num_classes=4).eval()
        model = wrap_modules_in_net(model, cfg, reparam=True)
        qs = _drop.activation_quantizers(model)
        assert len(qs) >= 8 and all(q_.drop_prob == want for q_ in qs)
        for m in model.modules():                                 # (what calibration's reparametrisation leaves: per-tensor parameters)
            if isinstance(m, AsymmetricallyChannelWiseBatchingQuantLinear):
                m.a_quantizer.scale = torch.nn.Parameter(torch.ones(1))
                m.a_quantizer.zero_point = torch.nn.Parameter(torch.zeros(1))
        qs = _drop.activation_quantizers(wrap_reparamed_modules_in_net(model))   # (re-instantiates the channel-wise layers)
        assert len(qs) >= 8 and all(q_.drop_prob == want for q_ in qs)
    cfg.drop_prob = -0.1
    with pytest.raises(ValueError):
        wrap_modules_in_net(VisionTransformer(img_size=32, patch_size=16, embed_dim=24, depth=1, num_heads=3, num_classes=4), cfg)


def test_cli_rejects_a_probability_outside_the_unit_interval():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "quant_qdrop.py"), "--drop-prob", "1.5"], capture_output=True, text=True, cwd=root)
    assert r.returncode == 2 and "must lie in [0, 1]" in r.stderr
