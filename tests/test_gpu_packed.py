"""`-m gpu`: packed low-bit weight codes (csrc/packed.hip, ops.pack_codes / unpack_codes) against the numpy reference of the format
and the existing fake-quantiser / operand packer, and packed checkpoints (utils/packed.py) of calibrated models end to end: the
reloaded model's quant_forward logits are bit-identical to the calibrated model's."""
import copy
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests.test_packed_cpu import np_pack, np_unpack

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SHAPES = [(1, 1), (3, 31), (2, 32), (5, 33), (4, 197), (64, 384)]
BITS = list(range(2, 9))


def _ops():
    from adalog_amd import backend, ops
    backend.set_backend(None)
    return ops


def _zero_points(b, R, per_row):
    """zero points on the grid [0, 2^b - 1]: 0, 2^b - 1, and two with fraction .5 (rne: 2.5 -> 2, 1.5 -> 2 -- ties to even)"""
    qmax = float(2 ** b - 1)
    pool = [0.0, qmax, 2.5, 1.5, qmax / 2 + 0.25, 1.0]
    if per_row:
        return [torch.tensor([pool[i % len(pool)] for i in range(R)])]
    return [torch.tensor([z]) for z in pool[:4]]


def _cases(b, per_row):
    """(w [R, K], scale, zero point) on the device; rne(w / s) + z spans [-0.3 qmax, 1.3 qmax], so both clamps are hit"""
    g = torch.Generator().manual_seed(100 * b + per_row)
    qmax = float(2 ** b - 1)
    for R, K in SHAPES:
        n = R if per_row else 1
        s = (0.01 + 0.05 * torch.rand(n, generator=g))
        for z in _zero_points(b, R, per_row):
            t = torch.rand(R, K, generator=g) * (1.6 * qmax) - 0.3 * qmax          # the code before the clamp
            w = (t - torch.round(z).view(-1, 1)) * s.view(-1, 1)
            if R * K >= 2:
                w.view(-1)[0], w.view(-1)[-1] = -1e4, 1e4                            # far beyond either clamp
            yield w.to(DEV), s.to(DEV), z.to(DEV)


@pytest.mark.parametrize("per_row", [0, 1])
@pytest.mark.parametrize("b", BITS)
def test_pack_codes_matches_the_format(b, per_row):
    ops = _ops()
    lo = hi = 0
    for w, s, z in _cases(b, per_row):
        R, K = w.shape
        y, bins = ops.uniform_fake_quant(w, s.view(-1, 1), z.view(-1, 1), b, want_bins=True)
        packed = ops.pack_codes(w, s, z, b)
        assert packed.dtype == torch.int32 and tuple(packed.shape) == (R, ops.packed_row_words(K, b)) == (R, b * -(-K // 32))
        want = np_pack(bins.cpu().numpy(), b)
        assert np.array_equal(packed.cpu().numpy(), want), (R, K)
        lo, hi = lo + int((bins == 0).sum()), hi + int((bins == 2 ** b - 1).sum())
    assert lo > 0 and hi > 0


@pytest.mark.parametrize("per_row", [0, 1])
@pytest.mark.parametrize("b", BITS)
def test_unpack_is_the_fake_quantiser_and_repacks_to_the_same_words(b, per_row):
    ops = _ops()
    for w, s, z in _cases(b, per_row):
        R, K = w.shape
        y = ops.uniform_fake_quant(w, s.view(-1, 1), z.view(-1, 1), b)
        packed = ops.pack_codes(w, s, z, b)
        w1 = ops.unpack_codes(packed, K, s, z, b)
        assert w1.dtype == torch.float32 and tuple(w1.shape) == (R, K)
        assert torch.equal(w1.view(torch.int32), y.view(torch.int32)), (R, K)      # bit for bit (signed zeros included)
        again = ops.pack_codes(w1, s, z, b)
        assert torch.equal(again, packed), (R, K)
        assert torch.equal(ops.unpack_codes(again, K, s, z, b).view(torch.int32), w1.view(torch.int32))
        # rows wider than K: the columns beyond K stay as they were (a row pitch that is / is not a multiple of four)
        for ldo in (K + 5, (K + 3) // 4 * 4 + 4):
            out = torch.full((R, ldo), -7.25, device=DEV)
            r = ops.unpack_codes(packed, K, s, z, b, out=out)
            assert r is out and torch.equal(out[:, :K].contiguous().view(torch.int32), y.view(torch.int32))
            assert bool((out[:, K:] == -7.25).all())


@pytest.mark.parametrize("per_row", [0, 1])
@pytest.mark.parametrize("b", BITS[:-1])
def test_operand_images_equal_pack_uniform(b, per_row):
    """unpack_codes(I8 / BF16, Kp) is byte for byte the image ops.pack_uniform writes for the same weight, zero padding included.

    One exception that no decoder can avoid, bf16 only: the sign of a zero.  The packers compute med3(rne(w / s), -z, qmax - z), so an
    element whose code equals rne(z) comes out as -0.0 when the weight was negative (rne(w / s) = -0.0, or a negative value clamped
    at a bound that is -0.0) and as +0.0 otherwise -- the sign of the original weight, which the code does not hold.  So against
    pack_uniform(w) the bf16 image must be equal as numbers everywhere and differ in bits only where pack_uniform wrote -0.0; and it
    must be byte for byte pack_uniform of the weight rebuilt from the codes, the image _pack_w_cached() builds after load_packed."""
    ops = _ops()
    for w, s, z in _cases(b, per_row):
        R, K = w.shape
        packed = ops.pack_codes(w, s, z, b)
        w1 = ops.unpack_codes(packed, K, s, z, b)
        for dt, tdt, view in ((ops.I8, torch.int8, torch.int8), (ops.BF16, torch.bfloat16, torch.int16)):
            Kp = ops.pad_k(K, dt)
            want = ops.pack_uniform(w.unsqueeze(0), s, z, 1, 0, 1, 0, per_row, b, dt)
            want1 = ops.pack_uniform(w1.unsqueeze(0), s, z, 1, 0, 1, 0, per_row, b, dt)
            assert tuple(want.shape) == tuple(want1.shape) == (1, 1, R, Kp)
            want, want1 = want.view(R, Kp), want1.view(R, Kp)
            got = ops.unpack_codes(packed, K, s, z, b, dtype=dt, Kp=Kp)
            assert got.dtype == tdt and tuple(got.shape) == (R, Kp)
            assert torch.equal(got.view(view), want1.view(view)), (R, K, dt)
            assert torch.equal(got.float(), want.float()), (R, K, dt)
            differs = got.view(view) != want.view(view)
            if dt == ops.I8:
                assert not bool(differs.any()), (R, K, dt)
            else:
                assert bool((want.view(view)[differs] == -32768).all()), (R, K, dt)       # 0x8000: -0.0
            assert bool((got[:, K:].view(view) == 0).all())
            assert torch.equal(ops.unpack_codes(packed, K, s, z, b, dtype=dt).view(view), got.view(view))   # Kp defaults to pad_k(K, dtype)


def test_wrappers_reject_what_the_kernels_cannot_take():
    ops = _ops()
    from adalog_amd._lib import AdalogHipError
    w = torch.randn(4, 40, device=DEV)
    s, z = torch.full((4,), 0.1, device=DEV), torch.full((4,), 3.0, device=DEV)
    p8 = ops.pack_codes(w, s, z, 8)
    with pytest.raises(AdalogHipError, match="int8"):
        ops.unpack_codes(p8, 40, s, z, 8, dtype=ops.I8)
    with pytest.raises(ValueError):
        ops.unpack_codes(p8, 40, s, z, 7)                        # word count does not match the bit width
    with pytest.raises(ValueError):
        ops.pack_codes(w, s[:3], z[:3], 4)                       # neither one pair nor one per row
    with pytest.raises(ValueError):
        ops.packed_row_words(40, 9)


# ------------------------------------------------------------------------------------------------ whole models
def _cfg(bits):
    import importlib.util
    spec = importlib.util.spec_from_file_location(f"cfg{bits}pk", os.path.join(ROOT, "configs", f"{bits}bit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = mod.Config()
    cfg.search_round, cfg.steps = 1, 2
    return cfg


def _cfg_path(bits):
    return os.path.join(ROOT, "configs", f"{bits}bit.py")


def _logits(model, x):
    """quant_forward logits on the default route and module by module (ADALOG_QF_FUSED=0)"""
    from adalog_amd.utils import models as M
    out = []
    try:
        for fused in (True, False):
            M.QF_FUSED = fused
            with torch.no_grad():
                out.append(model(x).clone())
    finally:
        M.QF_FUSED = os.environ.get("ADALOG_QF_FUSED", "1") != "0"
    return out


_CALIBRATED = {}


def _calibrated(name, depth, bits):
    """the calibrated model, its 4 synthetic images and its logits on both routes -- computed once per configuration"""
    key = (name, depth, bits)
    if key not in _CALIBRATED:
        _ops()
        from adalog_amd.utils.calibrator import QuantCalibrator
        from adalog_amd.utils.models import create_model
        from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
        torch.manual_seed(5)
        model = wrap_modules_in_net(create_model(name, depth=depth).eval().to(DEV), _cfg(bits), reparam=True).to(DEV)
        x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(5)).to(DEV)
        QuantCalibrator(model, [(x, None)]).batching_quant_calib()
        model = wrap_reparamed_modules_in_net(model).to(DEV).eval()
        for m in model.modules():
            if hasattr(m, "reparam_bias"):
                m.reparam_bias()
        _CALIBRATED[key] = (model, x, _logits(model, x))
    return _CALIBRATED[key]


def _formula_bytes(meta):
    return sum(i["rows"] * i["n_bits"] * -(-i["cols"] // 32) * 4 for i in meta["packed"].values())


def _packed_bytes(state):
    return sum(v.numel() * v.element_size() for k, v in state.items() if k.endswith("weight_packed"))


def _assert_same_logits(got, want):
    for g, w, route in zip(got, want, ("default route", "ADALOG_QF_FUSED=0")):
        assert torch.isfinite(w).all()
        assert torch.equal(g, w), (route, (g - w).abs().max().item())


@pytest.mark.parametrize("name,depth,bits", [("deit_tiny", 2, 4), ("swin_tiny", 1, 4), ("deit_tiny", 2, 3), ("deit_tiny", 2, 6)])
def test_packed_checkpoint_reproduces_the_calibrated_model(name, depth, bits, tmp_path, monkeypatch):
    from adalog_amd import _lib, ops
    from adalog_amd.utils import packed as P
    model, x, want = _calibrated(name, depth, bits)
    path = str(tmp_path / "packed.pth")
    P.save_packed(model, path)
    on_disk = torch.load(path, map_location="cpu")
    meta = on_disk["meta"]
    layers = [n for n, m in model.named_modules() if hasattr(m, "w_quantizer")]
    assert sorted(meta["packed"]) == sorted(layers) and meta["kept_fp32"] == {}
    assert all(i["n_bits"] == bits for i in meta["packed"].values())
    assert _packed_bytes(on_disk["state"]) == _formula_bytes(meta) == meta["weight_bytes"]["packed"]
    if name == "deit_tiny":                                                    # every K a multiple of 32: exactly bits / 32 of fp32
        assert meta["weight_bytes"]["fp32"] * bits == 32 * meta["weight_bytes"]["packed"]
    assert os.path.getsize(path) < meta["weight_bytes"]["fp32"]

    monkeypatch.delenv("ADALOG_PACKED_DIRECT", raising=False)
    loaded = P.load_packed(P.build_wrapped(name, _cfg_path(bits), DEV, depth=depth), path, DEV)
    assert all(m.mode == "quant_forward" for m in loaded.modules() if hasattr(m, "mode"))
    assert not any("_wp_cache" in m.__dict__ for m in loaded.modules())
    _assert_same_logits(_logits(loaded, x), want)

    # ADALOG_PACKED_DIRECT=1: the operand images come from the codes, the first forward packs no weight
    monkeypatch.setenv("ADALOG_PACKED_DIRECT", "1")
    direct = P.load_packed(P.build_wrapped(name, _cfg_path(bits), DEV, depth=depth), path, DEV)
    linears = [(n, m) for n, m in direct.named_modules() if hasattr(m, "_pack_w_cached")]
    assert linears and all("_wp_cache" in m.__dict__ for _, m in linears)
    for n, m in linears:
        key, img = m.__dict__["_wp_cache"]
        dt = key[0]
        fresh = m._pack_w_fixed(dt)
        assert key == m._wp_cache_key(dt, False) and img.dtype == fresh.dtype and tuple(img.shape) == tuple(fresh.shape), n
        assert getattr(img, "k_valid", None) == fresh.k_valid == m.in_features
        assert torch.equal(img.view(torch.int8 if dt == ops.I8 else torch.int16), fresh.view(torch.int8 if dt == ops.I8 else torch.int16)), n
    weights = {m.weight.data_ptr() for _, m in linears}
    packs = []
    real = ops.pack_uniform

    def spy(x3, *a, **k):
        if x3.data_ptr() in weights:
            packs.append(tuple(x3.shape))
        return real(x3, *a, **k)
    monkeypatch.setattr(ops, "pack_uniform", spy)
    with torch.no_grad():
        y = direct(x)
    assert packs == [], packs
    assert not _lib.load().adalog_last_kernel().decode().startswith("k_pack")
    assert torch.equal(y, want[0])
    monkeypatch.setattr(ops, "pack_uniform", real)
    _assert_same_logits(_logits(direct, x), want)


def test_packed_checkpoint_after_block_reconstruction(tmp_path):
    """BRECQ leaves AdaRound quantisers with the hard rounding committed (round_mode 'nearest', no alpha): their weights export too.

    The reference for the logits is the model's plain checkpoint reloaded (load_model of test_quant.py), not the in-process model:
    while a layer still carries its AdaRoundQuantizer, quant_forward composes fake-quant + fp32 product for it, and only a reloaded
    model (UniformQuantizer again) takes the integer routes -- a difference of product routes (1.8e-7 on these logits), present
    with plain checkpoints alike.  What does not depend on the route is asserted against the in-process model: every reloaded weight
    is its w_quantizer(weight) bit for bit."""
    _ops()
    from adalog_amd.quantizers.adaround import AdaRoundQuantizer
    from adalog_amd.utils import packed as P
    from adalog_amd.utils.block_recon import BlockReconstructor
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.models import create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    torch.manual_seed(7)
    cfg = _cfg(4)
    model = create_model("deit_tiny", depth=1).eval().to(DEV)
    full = copy.deepcopy(model)
    x = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(7)).to(DEV)
    loader = [(x, None)]
    model = wrap_modules_in_net(model, cfg, reparam=True).to(DEV)
    QuantCalibrator(model, loader).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model).to(DEV)
    BlockReconstructor(model, full, loader).reconstruct_model(quant_act=cfg.train_act, keep_gpu=cfg.keep_gpu, iters=6)
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    model.eval()
    assert any(isinstance(m.w_quantizer, AdaRoundQuantizer) for m in model.modules() if hasattr(m, "w_quantizer"))
    path, plain = str(tmp_path / "optimized_packed.pth"), str(tmp_path / "optimized_plain.pth")
    torch.save(model.state_dict(), plain)
    obj = P.save_packed(model, path)
    assert obj["meta"]["kept_fp32"] == {} and _packed_bytes(obj["state"]) == _formula_bytes(obj["meta"])
    reference = P.load_plain(P.build_wrapped("deit_tiny", _cfg_path(4), DEV, depth=1), plain, DEV)
    want = _logits(reference, x[:4])
    loaded = P.load_packed(P.build_wrapped("deit_tiny", _cfg_path(4), DEV, depth=1), path, DEV)
    _assert_same_logits(_logits(loaded, x[:4]), want)
    src = dict(model.named_modules())
    for name in obj["meta"]["packed"]:
        with torch.no_grad():
            assert torch.equal(dict(loaded.named_modules())[name].weight.data, src[name].quant_weight_bias()[0]), name
    for g, w in zip(want, _logits(model, x[:4])):                          # the in-process model: same numbers to fp32 rounding
        torch.testing.assert_close(g, w, rtol=1e-5, atol=1e-5)


def test_command_line_converts_a_plain_checkpoint(tmp_path):
    sys.path.insert(0, ROOT)
    import test_quant
    from adalog_amd.utils import packed as P
    model, x, want = _calibrated("deit_tiny", 2, 4)
    cfg = _cfg(4)
    plain = test_quant.save_model(model, types.SimpleNamespace(model="deit_tiny"), cfg, str(tmp_path), mode="calibrate")
    out = str(tmp_path / "converted.pth")
    r = subprocess.run([sys.executable, "-m", "adalog_amd.utils.packed", "--model", "deit_tiny", "--depth", "2", "--config", _cfg_path(4),
                        "--checkpoint", plain, "--out", out], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if "weight entries" in ln]
    assert len(lines) == 1, r.stdout
    obj = torch.load(out, map_location="cpu")
    wb = obj["meta"]["weight_bytes"]
    assert f"{wb['fp32']} bytes -> {wb['packed']} bytes" in lines[0] and wb["fp32"] == 8 * wb["packed"]
    assert _packed_bytes(obj["state"]) == _formula_bytes(obj["meta"])
    assert os.path.getsize(out) < os.path.getsize(plain)
    loaded = P.load_packed(P.build_wrapped("deit_tiny", _cfg_path(4), DEV, depth=2), out, DEV)
    _assert_same_logits(_logits(loaded, x), want)
