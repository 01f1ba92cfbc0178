"""`-m gpu`: the QDrop HIP kernels (adalog_*_drop) against the device-agnostic definition adalog_amd/quantizers/_drop.py, the fused
q/k/v drop route, fresh masks under HIP-graph replay, the reconstruction loop with drop_prob and the CLI switch."""
import copy
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import adalog_oracle as O
from tests import cpu_backend as CB, drop_reference as DR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SEED = 0xC0FFEE1234567890
G_MAX = 8192                                   # the largest block count of any launch here (csrc/fakequant.hip grid_for)
SIZES = [1, 3, 4, 5, 1023, 4 * 256 * G_MAX + 1, 4 * 256 * G_MAX + 4]      # the last two: every grid-stride loop wraps (scalar / float4 path)
PS = [0.0, 0.5, 1.0]


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import backend
    backend.set_backend(None)
    return backend.get()


@pytest.fixture(scope="module")
def D():
    from adalog_amd.quantizers import _drop
    return _drop


def g(seed):
    return torch.Generator().manual_seed(seed)


def _mask(D, state, n, p, it=7):
    m = D.keep_mask_from_state(state[0], state[1], n, p)
    if n <= 1023:                              # ... and the definition itself against the independent numpy generator
        assert np.array_equal(m.cpu().numpy(), DR.keep_mask(SEED, state[1], it, n, p))
    return m


def _check_uniform(ops, D, x, s, z, bits, sym, p, state, gy):
    n = x.numel()
    y = ops.uniform_fake_quant_drop(x, s, z, bits, sym, p, state)
    y_ref = D.uniform_drop_forward(ops, x, s, z, bits, sym, p, state)
    assert torch.equal(y, y_ref)
    mask = _mask(D, state, n, p).view(x.shape)
    gx, gs, gz = ops.uniform_fake_quant_backward_drop(gy, x, s, z, bits, sym, True, not sym, p, state)
    rx, rs, rz = D.uniform_drop_backward(ops, gy, x, s, z, bits, sym, True, not sym, p, state)
    assert torch.equal(gx[~mask], gy[~mask])
    torch.testing.assert_close(gx[mask], rx[mask], rtol=1e-6, atol=0)
    # parameter gradients against fp64 autograd of the same expression (kept elements only), at test_uniform_backward's bars
    g64 = torch.where(mask, gy, torch.zeros_like(gy)).cpu().double()
    _, ws, wz = CB.uniform_fake_quant_backward(g64, x.cpu().double(), s.cpu().double(), None if sym else z.cpu().double(), bits, sym, True, not sym)
    torch.testing.assert_close(gs.cpu().double(), ws, rtol=1e-4, atol=1e-4)
    if not sym:
        torch.testing.assert_close(gz.cpu().double(), wz, rtol=1e-4, atol=1e-5)
    if p == 1.0:                               # bitwise the undropped ABI calls
        assert torch.equal(y, ops.uniform_fake_quant(x, s, z, bits, sym=sym))
        ux, us, uz = ops.uniform_fake_quant_backward(gy, x, s, z, bits, sym, True, not sym)
        assert torch.equal(gx, ux) and torch.equal(gs, us) and (sym or torch.equal(gz, uz))
    if p == 0.0:
        assert torch.equal(y, x) and torch.equal(gx, gy) and float(gs.abs().max()) == 0.0


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", SIZES)
def test_uniform_per_tensor(ops, D, n, p):
    gen = g(100 + n % 1000)
    x = (torch.randn(n, generator=gen) * 2).to(DEV)
    gy = torch.randn(n, generator=gen).to(DEV)
    state = (D.make_state(SEED, 7, DEV), 3)
    s, z = torch.tensor([0.21], device=DEV), torch.tensor([7.0], device=DEV)
    _check_uniform(ops, D, x, s, z, 4, False, p, state, gy)
    if n <= 1023:
        _check_uniform(ops, D, x, s * 3, None, 4, True, p, state, gy)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("rows,inner", [(6, 3), (6, 4), (3, 197)])
def test_uniform_rows(ops, D, rows, inner, p):
    """x [2, n_ch, inner'] with per-channel parameters: rows = 2 * n_ch, channel = row % n_ch"""
    gen = g(200 + rows * inner)
    n_ch = rows // 2 if rows % 2 == 0 else rows
    x = (torch.randn(rows // n_ch, n_ch, inner, generator=gen) * 2).to(DEV)
    gy = torch.randn(x.shape, generator=gen).to(DEV)
    s = (torch.rand(1, n_ch, 1, generator=gen) * 0.3 + 0.1).to(DEV)
    z = torch.randint(4, 12, (1, n_ch, 1), generator=gen).float().to(DEV)
    _check_uniform(ops, D, x, s, z, 4, False, p, (D.make_state(SEED, 7, DEV), 1), gy)


def _check_adalog(ops, D, x, s, qd, sh, sub, pre, p, state, gy):
    bits = 4
    y = ops.log_fake_quant_drop(x, s, qd, bits, sh, sub, pre, p, state)
    assert torch.equal(y, D.log_drop_forward(ops, x, s, qd, bits, sh, sub, pre, p, state))
    mask = _mask(D, state, x.numel(), p).view(x.shape)
    gx, gs = ops.log_fake_quant_backward_drop(gy, x, s, qd, bits, sh, sub, pre, p, state)
    rx, rs = D.log_drop_backward(ops, gy, x, s, qd, bits, sh, sub, pre, p, state)
    if pre:                                    # gy * GELU' at the bar of test_adalog_training_form_with_the_gelu_prologue
        torch.testing.assert_close(gx[~mask], rx[~mask], rtol=1e-4, atol=1e-7)
    else:
        assert torch.equal(gx[~mask], gy[~mask])
    torch.testing.assert_close(gx[mask], rx[mask], rtol=1e-4, atol=1e-6)
    # the scale gradient against fp64 autograd over the kept elements (test_adalog_backward's bar)
    xin = torch.nn.functional.gelu(x.cpu().double()) if pre else x.cpu().double()
    g64 = torch.where(mask, gy, torch.zeros_like(gy)).cpu().double()
    _, ws = CB.log_fake_quant_backward(g64, xin, None, s.cpu().double(), qd.cpu(), bits, None if sh is None else sh.cpu().double(), sub)
    torch.testing.assert_close(gs.cpu().double(), ws, rtol=1e-3, atol=1e-3)
    kw = {"pre_gelu": True} if pre else {}
    if p == 1.0:
        u = ops.log_fake_quant(x, s, qd, None, None, bits, shift=sh, sub_shift=sub, train_form=True, **kw)
        ux, us = ops.log_fake_quant_backward(gy, x, u, s, qd, bits, sh, sub, **kw)
        assert torch.equal(y, u) and torch.equal(gx, ux) and torch.equal(gs, us)
    if p == 0.0:
        assert torch.equal(y, torch.nn.functional.gelu(x) if pre else x) and float(gs.abs().max()) == 0.0


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", ["plain", "shift_sub", "shift", "pre_gelu"])
def test_adalog(ops, D, form, n, p):
    gen = g(300 + n % 1000)
    pre = form == "pre_gelu"
    raw = 1.7 * torch.randn(n, generator=gen)
    x = (raw if pre else torch.nn.functional.gelu(raw)).to(DEV)
    gy = torch.randn(n, generator=gen).to(DEV)
    s = torch.tensor([2.3], device=DEV); qd = torch.tensor([23], device=DEV)
    sh = None if form == "plain" else torch.tensor([O.GELU_SHIFT], device=DEV)
    _check_adalog(ops, D, x, s, qd, sh, form in ("shift_sub", "pre_gelu"), pre, p, (D.make_state(SEED, 7, DEV), 2), gy)


def test_unaligned_views_take_the_scalar_path_with_the_same_mask(ops, D):
    """x, gy as views one element into their allocations (4-byte aligned only): same outputs as the aligned tensors"""
    n = 4096
    gen = g(400)
    state = (D.make_state(SEED, 7, DEV), 0)
    s, z = torch.tensor([0.21], device=DEV), torch.tensor([7.0], device=DEV)
    base_x, base_g = (torch.randn(n + 1, generator=gen) * 2).to(DEV), torch.randn(n + 1, generator=gen).to(DEV)
    xv, gv = base_x[1:], base_g[1:]
    assert xv.data_ptr() % 16 == 4 and xv.is_contiguous()
    xa, ga = xv.clone(), gv.clone()
    assert torch.equal(ops.uniform_fake_quant_drop(xv, s, z, 4, False, 0.5, state), ops.uniform_fake_quant_drop(xa, s, z, 4, False, 0.5, state))
    a = ops.uniform_fake_quant_backward_drop(gv, xv, s, z, 4, False, True, True, 0.5, state)
    b = ops.uniform_fake_quant_backward_drop(ga, xa, s, z, 4, False, True, True, 0.5, state)
    assert torch.equal(a[0], b[0])
    torch.testing.assert_close(a[1], b[1], rtol=1e-5, atol=1e-5)      # (another partial-sum order)
    xl = torch.nn.functional.gelu(xv); xla = xl.clone()
    s2 = torch.tensor([2.3], device=DEV); qd = torch.tensor([37], device=DEV); sh = torch.tensor([O.GELU_SHIFT], device=DEV)
    xlv = torch.cat([xl[:1], xl])[1:]
    assert xlv.data_ptr() % 16 == 4
    assert torch.equal(ops.log_fake_quant_drop(xlv, s2, qd, 4, sh, True, False, 0.5, state), ops.log_fake_quant_drop(xla, s2, qd, 4, sh, True, False, 0.5, state))
    a = ops.log_fake_quant_backward_drop(gv, xlv, s2, qd, 4, sh, True, False, 0.5, state)
    b = ops.log_fake_quant_backward_drop(ga, xla, s2, qd, 4, sh, True, False, 0.5, state)
    assert torch.equal(a[0], b[0])
    torch.testing.assert_close(a[1], b[1], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("per_head", [False, True])
@pytest.mark.parametrize("Dh", [32, 64])
@pytest.mark.parametrize("H", [2, 3])
@pytest.mark.parametrize("N", [5, 197])
def test_qkv_drop_route_matches_split_and_three_dropped_quantisers(ops, D, N, H, Dh, per_head):
    B, bits = 2, 4
    gen = g(500 + N + H + Dh)
    x = (torch.randn(B, N, 3 * H * Dh, generator=gen) * 1.5).to(DEV)
    n = H if per_head else 1
    scales = [(torch.rand(1, n, 1, 1, generator=gen) * 0.2 + 0.2).to(DEV) for _ in range(3)]
    zps = [torch.randint(1, 15, (1, n, 1, 1), generator=gen).float().to(DEV) for _ in range(3)]
    buf = D.make_state(SEED, 7, DEV)
    ps, streams = (0.5, 0.25, 1.0), (4, 5, 9)
    nb = (bits,) * 3
    ys = ops.qkv_split_quant_drop(x, H, scales, zps, nb, ps, (buf, streams))
    gys = [torch.randn(B, H, N, Dh, generator=gen).to(DEV) for _ in range(3)]
    gx, gs = ops.qkv_merge_quant_backward_drop(gys, x, H, scales, zps, nb, ps, (buf, streams))
    parts = x.reshape(B, N, 3, H, Dh).permute(2, 0, 3, 1, 4)
    gx_want = []
    for i in range(3):
        xp = parts[i].contiguous()
        st = (buf, streams[i])
        assert torch.equal(ys[i], ops.uniform_fake_quant_drop(xp, scales[i], zps[i], bits, False, ps[i], st)), i
        assert torch.equal(ys[i], D.uniform_drop_forward(ops, xp, scales[i], zps[i], bits, False, ps[i], st)), i
        wx, wsg, _ = ops.uniform_fake_quant_backward_drop(gys[i], xp, scales[i], zps[i], bits, False, True, False, ps[i], st)
        gx_want.append(wx)
        err = float((gs[i].double() - wsg.double()).abs().max() / wsg.double().abs().max().clamp_min(1e-30))
        assert err <= 1e-5, (i, err)          # the bar of test_qkv_split_quant_matches_the_separate_route
    assert torch.equal(gx, torch.stack(gx_want, 0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * H * Dh))
    one = ops.qkv_split_quant_drop(x, H, scales, zps, nb, (1.0, 1.0, 1.0), (buf, streams))
    for a, b in zip(one, ops.qkv_split_quant(x, H, scales, zps, nb)):
        assert torch.equal(a, b)


def test_graph_replay_draws_a_fresh_mask_per_iteration(ops, D):
    """one dropped forward + backward captured; the iteration word advanced the way the loop's table mode advances it (the
    schedule-row copy that lands on word 2 of the shared buffer)"""
    from adalog_amd import _lib
    from adalog_amd.quantizers.uniform import UniformQuantizer
    _lib.check(_lib.load().adalog_brecq_init(), "adalog_brecq_init")
    n, p, stream = 1027, 0.5, 6
    q = UniformQuantizer(n_bits=4)
    q.scale = torch.nn.Parameter(torch.tensor([0.21], device=DEV))
    q.zero_point = torch.nn.Parameter(torch.tensor([7.0], device=DEV), requires_grad=False)
    q.inited = True
    q.init_training()
    q.drop_prob = p
    words = torch.zeros(6, dtype=torch.int32, device=DEV)
    words[:3] = D.make_state(SEED, 0, DEV)
    state, sched_dev = words[0:3], words.view(torch.float32)[2:6]
    q.attach_drop_state(state, stream)
    x = (torch.randn(n, generator=g(600)) * 2).to(DEV).requires_grad_(True)
    gy = torch.randn(n, generator=g(601)).to(DEV)
    rows = torch.cat([torch.arange(0, 8, dtype=torch.int32).view(torch.float32).unsqueeze(1), torch.rand(8, 3)], dim=1).to(DEV)
    for it in range(2):                        # eager warm-up
        sched_dev.copy_(rows[it])
        q(x).backward(gy)
    x.grad = None
    q.scale.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    sched_dev.copy_(rows[2])
    with torch.cuda.graph(graph):
        y = q(x)
        y.backward(gy)
    fq = ops.uniform_fake_quant(x.detach(), q.scale.data, q.zero_point.data, 4)
    seen = []
    for it in (2, 3, 4):
        sched_dev.copy_(rows[it])
        graph.replay()
        torch.cuda.synchronize()
        assert int(state[2]) == it
        want = torch.from_numpy(DR.keep_mask(SEED, stream, it, n, p)).to(DEV)
        assert torch.equal(D.philox_keep_mask(SEED, stream, it, n, p, DEV), want)
        assert torch.equal(y.detach(), torch.where(want, fq, x.detach()))
        assert torch.equal(x.grad[~want], gy[~want])              # the backward regenerated the forward's mask
        seen.append(want)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])


def test_last_dim_channel_parameters_take_the_composed_route(ops, D):
    """parameters along the last dim (inner == 1), which the uniform drop kernel does not take: the forward composes, same mask,
    same semantics (a channel-wise layer before its reparametrisation; BRECQ never trains one)"""
    rows, ch, p, stream = 5, 12, 0.5, 2
    x = (torch.randn(rows, ch, generator=g(650)) * 2).to(DEV).requires_grad_(True)
    s = (torch.rand(ch, generator=g(651)) * 0.2 + 0.1).to(DEV).requires_grad_(True)
    z = torch.randint(1, 15, (ch,), generator=g(652)).float().to(DEV)
    gy = torch.randn(rows, ch, generator=g(653)).to(DEV)
    buf = D.make_state(SEED, 7, DEV)
    y = D.UniformDropSTE.apply(x, s, z, 4, False, p, buf, stream)
    mask = torch.from_numpy(DR.keep_mask(SEED, stream, 7, rows * ch, p)).to(DEV).view(rows, ch)
    assert 0 < int(mask.sum()) < rows * ch
    assert torch.equal(y.detach(), torch.where(mask, ops.uniform_fake_quant(x.detach(), s.detach(), z, 4), x.detach()))
    with pytest.raises(NotImplementedError):                      # as without dropping: ops has no training gradient for this layout
        y.backward(gy)


def test_brecq_prepare_lands_the_iteration_on_the_state_word(ops, D):
    """the replay path's own way of advancing the iteration: adalog_brecq_prepare writes the schedule row {iteration (int32 bit
    pattern), b, gate, lr} over words 2..5 of the six-word buffer whose words 0..2 are the drop state"""
    from adalog_amd import _lib
    _lib.check(_lib.load().adalog_brecq_init(), "adalog_brecq_init")
    words = torch.zeros(6, dtype=torch.int32, device=DEV)
    words[:3] = D.make_state(SEED, 0, DEV)
    state, sched_dev = words[0:3], words.view(torch.float32)[2:6]
    seed_words = state[:2].clone()
    src_in = torch.randn(6, 8, generator=g(700)).to(DEV)
    src_out = torch.randn(6, 4, generator=g(701)).to(DEV)
    idx = torch.tensor([4, 0, 5], device=DEV)
    dst_in, dst_out = torch.zeros(3, 8, device=DEV), torch.zeros(3, 4, device=DEV)
    n, p, stream = 1027, 0.5, 3
    x = (torch.randn(n, generator=g(702)) * 2).to(DEV)
    s, z = torch.tensor([0.21], device=DEV), torch.tensor([7.0], device=DEV)
    fq = ops.uniform_fake_quant(x, s, z, 4)
    for it in (1, 2, 7, 2 ** 31 - 1):
        tail = torch.rand(3, generator=g(710 + it % 97))
        row = torch.cat([torch.tensor([it], dtype=torch.int32).view(torch.float32), tail]).to(DEV)
        assert ops.brecq_prepare(src_in, src_out, idx, dst_in, dst_out, row, sched_dev)
        assert int(words[2]) == it
        assert torch.equal(state[:2], seed_words)
        assert torch.equal(sched_dev[1:].cpu(), tail)
        assert torch.equal(dst_in, src_in[idx]) and torch.equal(dst_out, src_out[idx])
        want = torch.from_numpy(DR.keep_mask(SEED, stream, it, n, p)).to(DEV)       # ... and the kernels read it from there
        assert torch.equal(ops.uniform_fake_quant_drop(x, s, z, 4, False, p, (state, stream)), torch.where(want, fq, x))


# ------------------------------------------------------------------------------------------------ the loop
@pytest.fixture(scope="module")
def tiny_block():
    """a calibrated depth-1 deit_tiny (random weights) and 32 random images -> factory of fresh (reconstructor, block) pairs"""
    from adalog_amd import backend
    from adalog_amd.utils.block_recon import BlockReconstructor
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.models import VisionTransformer
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    backend.set_backend(None)
    spec = importlib.util.spec_from_file_location("cfg4drop", os.path.join(ROOT, "configs", "4bit.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    cfg = mod.Config()
    cfg.search_round, cfg.steps = 1, 2
    torch.manual_seed(11)
    model = VisionTransformer(img_size=224, patch_size=16, embed_dim=192, depth=1, num_heads=3, num_classes=16).eval()
    for p_ in model.parameters():
        p_.data.mul_(4.0)
    model.to(DEV)
    full = copy.deepcopy(model)
    x = torch.randn(32, 3, 224, 224, generator=g(12)).to(DEV)
    loader = [(x[:16], None), (x[16:], None)]
    model = wrap_modules_in_net(model, cfg, reparam=True)
    QuantCalibrator(model, loader).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model)

    def run(graph, **kw):
        m = copy.deepcopy(model)
        rec = BlockReconstructor(m, full, loader)
        name = "blocks.0"
        block = rec.blocks[name]
        rec.init_block_raw_data(block, rec.full_blocks[name], name, torch.device(DEV))
        prev = os.environ.get("ADALOG_BRECQ_GRAPH")
        os.environ["ADALOG_BRECQ_GRAPH"] = "1" if graph else "0"
        try:
            rec.reconstruct_single_block(name, block, torch.device(DEV), batch_size=8, iters=12, quant_act=True, **kw)
        finally:
            if prev is None:
                os.environ.pop("ADALOG_BRECQ_GRAPH", None)
            else:
                os.environ["ADALOG_BRECQ_GRAPH"] = prev
        torch.cuda.synchronize()
        return DR.trained_tensors(block)
    return run


def test_loop_eager_and_graph_see_the_same_masks(tiny_block, monkeypatch):
    from adalog_amd import backend
    be = backend.get()
    calls = {"qkv": 0, "uni": 0, "log": 0}
    for key, name in (("qkv", "qkv_split_quant_drop"), ("uni", "uniform_fake_quant_drop"), ("log", "log_fake_quant_drop")):
        orig = getattr(be, name)

        def spy(*a, _o=orig, _k=key, **k):
            calls[_k] += 1
            return _o(*a, **k)
        monkeypatch.setattr(be, name, spy)
    eager = tiny_block(False, drop_prob=0.5)
    assert all(v > 0 for v in calls.values()), calls              # the fused q/k/v route, the Linear inputs, fc2's AdaLog input
    graph = tiny_block(True, drop_prob=0.5)
    assert eager.keys() == graph.keys() and len(eager) >= 10
    for k in eager:                                               # the bar of the eager-vs-replay trajectory test (test_gpu_layers.py)
        err = float((eager[k] - graph[k]).abs().max() / eager[k].abs().max().clamp(min=1e-12))
        print(k, err)
        assert err <= 1e-3, (k, err)


@pytest.mark.parametrize("graph", [False, True])
def test_loop_drop_prob_one_is_bit_identical_to_omitting_it(tiny_block, graph):
    base, one = tiny_block(graph), tiny_block(graph, drop_prob=1.0)
    for k in base:
        assert torch.equal(base[k], one[k]), k
    half = tiny_block(graph, drop_prob=0.5)
    assert any(not torch.equal(base[k], half[k]) for k in base)


def test_cli_optimize_with_drop_prob(tmp_path):
    from PIL import Image
    rng = np.random.RandomState(0)
    root = tmp_path / "toy_imagenet"
    for split, per in (("train", 6), ("val", 3)):
        for ci in range(4):
            d = root / split / f"n{ci:04d}"
            d.mkdir(parents=True)
            for j in range(per):
                Image.fromarray((rng.rand(70 + 8 * j, 96 - 5 * ci, 3) * 255).astype(np.uint8)).save(d / f"img{j}.jpg")
    out = str(tmp_path / "run_drop")
    cmd = [sys.executable, os.path.join(ROOT, "quant_qdrop.py"), "--model", "deit_tiny", "--config", os.path.join(ROOT, "configs", "4bit.py"),
           "--dataset", str(root), "--calibrate", "--optimize", "--drop-prob", "0.5", "--optim-iters", "12", "--calib-size", "16",
           "--calib-batch-size", "8", "--val-batch-size", "4", "--num-workers", "0", "--output-dir", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ckpts = [f for f in os.listdir(out) if "optimsize" in f and f.endswith(".pth")]
    assert len(ckpts) == 1, os.listdir(out)
    cmd2 = [sys.executable, os.path.join(ROOT, "test_quant.py"), "--model", "deit_tiny", "--config", os.path.join(ROOT, "configs", "4bit.py"),
            "--dataset", str(root), "--load-optimize-checkpoint", os.path.join(out, ckpts[0]), "--test-optimize-checkpoint",
            "--val-batch-size", "4", "--num-workers", "0", "--output-dir", str(tmp_path / "run_drop2")]
    r2 = subprocess.run(cmd2, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-4000:]
    assert "Prec@1" in r2.stdout + r2.stderr
