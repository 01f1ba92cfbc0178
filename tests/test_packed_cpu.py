"""Packed checkpoints (adalog_amd/utils/packed.py, format adalog-packed-v1) without a device: the numpy reference of the storage
format, argument rejection of the three C entry points, and the host logic of packed_state_dict / save_packed / load_packed on a
depth-1 toy model with a stand-in backend (tests.cpu_backend plus pack_codes / unpack_codes from the numpy reference)."""
import copy
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from adalog_amd import backend
from tests import cpu_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I8, BF16, F32 = 0, 1, 2
BITS = range(2, 9)


# ------------------------------------------------------------------------------------------------ the format, in numpy
def np_pack(codes, b):
    """uint8 [R, K] codes -> '<i4' [R, b * ceil(K / 32)]: the low b bits of each code, rows padded to a multiple of 32 codes, as
    one little-endian bit stream per row (a group of 32 codes then fills exactly b words)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    R, K = codes.shape
    Kp = -(-K // 32) * 32
    c = np.zeros((R, Kp), np.uint8)
    c[:, :K] = codes
    bits = np.unpackbits(c[:, :, None], axis=-1, bitorder="little")[:, :, :b]
    stream = np.ascontiguousarray(bits.reshape(R, Kp * b))
    return np.ascontiguousarray(np.packbits(stream, axis=-1, bitorder="little")).view("<i4")


def np_unpack(words, K, b):
    """the inverse: '<i4' [R, b * ceil(K / 32)] -> uint8 [R, K]"""
    words = np.ascontiguousarray(words).astype("<i4", copy=False)
    R = words.shape[0]
    Kp = -(-K // 32) * 32
    assert words.shape[1] * 32 == Kp * b, (words.shape, K, b)
    stream = np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")
    bits = np.zeros((R, Kp, 8), np.uint8)
    bits[:, :, :b] = stream.reshape(R, Kp, b)
    return np.packbits(bits, axis=-1, bitorder="little").reshape(R, Kp)[:, :K]


@pytest.mark.parametrize("b", BITS)
def test_numpy_reference_round_trip_and_bit_positions(b):
    rng = np.random.default_rng(b)
    for K in (1, 31, 32, 33, 197):
        codes = rng.integers(0, 2 ** b, size=(3, K), dtype=np.uint8)
        w = np_pack(codes, b)
        assert w.shape == (3, b * -(-K // 32))
        assert np.array_equal(np_unpack(w, K, b), codes)
        u = w.view("<u4").astype(np.uint64)
        for i in (0, K // 2, K - 1):                       # code i of group g: bits [i b, (i + 1) b) of the group's b words
            g, j = divmod(i, 32)
            got = 0
            for t in range(b):
                bit = j * b + t
                got |= int((u[1, g * b + bit // 32] >> np.uint64(bit % 32)) & np.uint64(1)) << t
            assert got == codes[1, i]


# ------------------------------------------------------------------------------------------------ C ABI, no device
def _lib():
    from adalog_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def test_packed_row_words():
    lib = _lib()
    for b in BITS:
        for K in (1, 31, 32, 33, 197, 384):
            assert lib.adalog_packed_row_words(K, b) == b * -(-K // 32)
    for K, b in ((0, 4), (-5, 4), (32, 1), (32, 9), (32, 0)):
        assert lib.adalog_packed_row_words(K, b) == -1


def test_pack_and_unpack_reject_bad_arguments_without_a_device():
    lib = _lib()
    buf = (ctypes.c_float * 64)()                       # a valid host address: a rejected call never reads it
    a = ctypes.addressof(buf)
    err = lambda: lib.adalog_last_error().decode()
    for w, s, z, o in ((None, a, a, a), (a, None, a, a), (a, a, None, a), (a, a, a, None)):
        assert lib.adalog_pack_codes_f32(w, 2, 32, 32, s, z, 0, 4, o, None) == -1 and "pack_codes" in err() and "null" in err()
        assert lib.adalog_unpack_codes(w, 2, 32, s, z, 0, 4, 2, o, 32, None) == -1 and "unpack_codes" in err() and "null" in err()
    for nb in (1, 9):
        assert lib.adalog_pack_codes_f32(a, 2, 32, 32, a, a, 0, nb, a, None) == -1 and "n_bits" in err()
        assert lib.adalog_unpack_codes(a, 2, 32, a, a, 0, nb, 2, a, 32, None) == -1 and "n_bits" in err()
    assert lib.adalog_unpack_codes(a, 2, 32, a, a, 0, 8, 0, a, 128, None) == -1 and "int8" in err()
    assert lib.adalog_unpack_codes(a, 2, 32, a, a, 0, 4, 3, a, 128, None) == -1 and "out_dtype" in err()
    assert lib.adalog_pack_codes_f32(a, 0, 32, 32, a, a, 0, 4, a, None) == -1 and "sizes" in err()
    assert lib.adalog_pack_codes_f32(a, 2, 32, 31, a, a, 0, 4, a, None) == -1 and "sizes" in err()      # ldw < K
    assert lib.adalog_unpack_codes(a, 2, 33, a, a, 0, 4, 2, a, 32, None) == -1 and "sizes" in err()      # ldo < K


# ------------------------------------------------------------------------------------------------ stand-in backend
class PackedCpuBackend:
    """tests.cpu_backend plus the two packed-code functions of adalog_amd/ops.py, from the numpy reference"""

    def __getattr__(self, name):
        return getattr(cpu_backend, name)

    @staticmethod
    def _params(scale, zero_point, R):
        s, z = scale.reshape(-1).float(), zero_point.reshape(-1).float()
        assert s.numel() == z.numel() and s.numel() in (1, R)
        return s.view(-1, 1), z.view(-1, 1)

    def pack_codes(self, w2, scale, zero_point, n_bits):
        s, z = self._params(scale, zero_point, w2.shape[0])
        _, q = cpu_backend.uniform_fake_quant(w2, s, z, n_bits, want_bins=True)
        return torch.from_numpy(np_pack(q.numpy(), n_bits).astype(np.int32))

    def unpack_codes(self, packed, K, scale, zero_point, n_bits, dtype=F32, Kp=None):
        s, z = self._params(scale, zero_point, packed.shape[0])
        q = torch.from_numpy(np_unpack(packed.numpy(), K, n_bits).astype(np.float32))
        c = q - torch.round(z)
        if dtype == F32:
            return c * s
        Kp = cpu_backend.pad_k(K, dtype) if Kp is None else Kp
        out = torch.zeros((packed.shape[0], Kp), dtype=cpu_backend._TORCH_DT[dtype])
        out[:, :K] = c.to(out.dtype)
        return out


@pytest.fixture(scope="module")
def be():
    impl = PackedCpuBackend()
    backend.set_backend(impl)
    yield impl
    backend.set_backend(None)


def _cfg(bits=6):
    spec = importlib.util.spec_from_file_location(f"cfg{bits}p", os.path.join(ROOT, "configs", f"{bits}bit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = mod.Config()
    cfg.search_round, cfg.steps = 1, 2
    return cfg


def _fresh():
    from adalog_amd.utils.models import VisionTransformer
    torch.manual_seed(5)
    model = VisionTransformer(img_size=32, patch_size=8, embed_dim=32, depth=1, num_heads=2, num_classes=10).eval()
    for p in model.parameters():
        p.data.mul_(8.0)
    return model


LAYERS = ["patch_embed.proj", "blocks.0.attn.qkv", "blocks.0.attn.proj", "blocks.0.mlp.fc1", "blocks.0.mlp.fc2", "head"]


@pytest.fixture(scope="module")
def toy(be):
    """a calibrated depth-1 model (W6A6), its input and its quant_forward logits"""
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    model = wrap_modules_in_net(_fresh(), _cfg(), reparam=True)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    QuantCalibrator(model, [(x[:2], None), (x[2:], None)]).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model)
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    with torch.no_grad():
        y = model(x)
    return model, x, y


def _formula_bytes(meta):
    return sum(i["rows"] * i["n_bits"] * -(-i["cols"] // 32) * 4 for i in meta["packed"].values())


def _packed_bytes(state):
    return sum(v.numel() * v.element_size() for k, v in state.items() if k.endswith("weight_packed"))


def test_packed_state_dict_keys_and_meta(toy):
    from adalog_amd.utils import packed as P
    model, _, _ = toy
    obj = P.packed_state_dict(model)
    assert obj["format"] == "adalog-packed-v1" and set(obj) == {"format", "meta", "state"}
    meta, state, plain = obj["meta"], obj["state"], model.state_dict()
    assert sorted(meta["packed"]) == sorted(LAYERS) and meta["kept_fp32"] == {}
    mods = dict(model.named_modules())
    for name in LAYERS:
        m, info = mods[name], meta["packed"][name]
        assert name + ".weight" not in state
        pk = state[name + ".weight_packed"]
        rows, cols = m.weight.shape[0], m.weight.numel() // m.weight.shape[0]
        assert pk.dtype == torch.int32 and pk.device.type == "cpu" and tuple(pk.shape) == (rows, 6 * -(-cols // 32))
        assert info == {"n_bits": 6, "rows": rows, "cols": cols, "per_row": True, "shape": list(m.weight.shape)}
    assert len(meta["packed"]["patch_embed.proj"]["shape"]) == 4                 # a conv weight keeps its 4-D shape
    # a packed checkpoint differs from a plain one in the weight entries only: same keys in the same order, same tensors
    assert [k.replace("weight_packed", "weight") for k in state] == list(plain)
    for k, v in plain.items():
        if k not in {n + ".weight" for n in LAYERS}:
            assert torch.equal(state[k], v), k
    assert _packed_bytes(state) == _formula_bytes(meta) > 0
    assert meta["weight_bytes"] == {"fp32": sum(mods[n].weight.numel() * 4 for n in LAYERS), "packed": _formula_bytes(meta)}
    # the stored codes are the quantiser's own bins
    for name in LAYERS:
        m = mods[name]
        rows, cols = m.weight.shape[0], m.weight.numel() // m.weight.shape[0]
        wq = m.w_quantizer
        bins = cpu_backend.uniform_fake_quant(m.weight.data.reshape(rows, cols), wq.scale.data.reshape(rows, 1),
                                              wq.zero_point.data.reshape(rows, 1), 6, want_bins=True)[1]
        assert np.array_equal(np_unpack(state[name + ".weight_packed"].numpy(), cols, 6), bins.numpy())


def test_ineligible_modules_keep_fp32_and_are_listed(toy):
    from adalog_amd.utils import packed as P
    model = copy.deepcopy(toy[0])
    blk = model.blocks[0]
    blk.attn.proj.w_quantizer.sym = True                                          # a symmetric quantiser
    blk.mlp.fc1.w_quantizer.init_training()                                       # one in training mode
    wq = blk.attn.qkv.w_quantizer                                                 # n_V = 3 with one (scale, zero point) per V block:
    assert blk.attn.qkv.n_V == 3                                                  # neither one pair nor one pair per row
    wq.scale = torch.nn.Parameter(wq.scale.data[:, :1].clone())
    wq.zero_point = torch.nn.Parameter(wq.zero_point.data[:, :1].clone())
    model.head.w_quantizer.n_bits = 9
    obj = P.packed_state_dict(model)
    kept = obj["meta"]["kept_fp32"]
    assert set(kept) == {"blocks.0.attn.proj", "blocks.0.mlp.fc1", "blocks.0.attn.qkv", "head"}
    assert all(isinstance(v, str) and v for v in kept.values())
    assert "symmetric" in kept["blocks.0.attn.proj"] and "training" in kept["blocks.0.mlp.fc1"] and "3 scales" in kept["blocks.0.attn.qkv"]
    for name in kept:
        assert name not in obj["meta"]["packed"] and name + ".weight_packed" not in obj["state"]
        w = obj["state"][name + ".weight"]
        assert w.dtype == torch.float32 and torch.equal(w, dict(model.named_modules())[name].weight.data)
    assert sorted(obj["meta"]["packed"]) == ["blocks.0.mlp.fc2", "patch_embed.proj"]
    assert _packed_bytes(obj["state"]) == _formula_bytes(obj["meta"])


def test_save_and_load_round_trip(toy, tmp_path):
    from adalog_amd.utils import packed as P
    from adalog_amd.utils.wrap_net import wrap_modules_in_net
    model, x, y = toy
    path = str(tmp_path / "toy_packed.pth")
    obj = P.save_packed(model, path)
    assert os.path.exists(path) and obj["format"] == "adalog-packed-v1"
    on_disk = torch.load(path, map_location="cpu")
    assert _packed_bytes(on_disk["state"]) == _formula_bytes(on_disk["meta"])
    fresh = wrap_modules_in_net(_fresh(), _cfg(), reparam=False)
    for p in fresh.parameters():
        p.data.add_(1.0)                                                          # nothing of the fresh model may survive the load
    loaded = P.load_packed(fresh, path, "cpu")
    assert loaded is fresh and not loaded.training
    src = dict(model.named_modules())
    for name, m in loaded.named_modules():
        if hasattr(m, "mode"):
            assert m.mode == "quant_forward" and m.calibrated
        if name in LAYERS:
            with torch.no_grad():
                want = src[name].quant_weight_bias()[0]
            assert torch.equal(m.weight.data, want), name                         # every weight is w_quantizer(weight) of the source
            assert "_wp_cache" not in m.__dict__
    with torch.no_grad():
        assert torch.equal(loaded(x), y)


def test_unknown_format_is_refused(toy, tmp_path):
    from adalog_amd.utils import packed as P
    from adalog_amd.utils.wrap_net import wrap_modules_in_net
    model = toy[0]
    obj = P.packed_state_dict(model)
    obj["format"] = "adalog-packed-v2"
    p2, p3 = str(tmp_path / "v2.pth"), str(tmp_path / "plain.pth")
    torch.save(obj, p2)
    torch.save(model.state_dict(), p3)
    fresh = wrap_modules_in_net(_fresh(), _cfg(), reparam=False)
    with pytest.raises(ValueError, match="adalog-packed-v1"):
        P.load_packed(fresh, p2, "cpu")
    with pytest.raises(ValueError, match="adalog-packed-v1"):
        P.load_packed(fresh, p3, "cpu")
