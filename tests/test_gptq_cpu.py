"""GPTQ without a device: the numpy reference of the column sweep (tests/gptq_reference.py) -- round-to-nearest when U = I, the
kernel's blocked order equal to the column order bit for bit, the objective below round-to-nearest's on the issue's inputs --, the
argument checks of the two C entry points, and the host logic of adalog_amd/utils/gptq.py on a depth-1 toy model with a stand-in
backend (tests/gptq_cpu_backend.py)."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from adalog_amd import backend
from tests import cpu_backend
from tests import gptq_reference as GR
from tests.gptq_cpu_backend import GptqCpuBackend
from tests.test_packed_cpu import LAYERS, _cfg, _fresh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("bits", [2, 3, 4, 8])
@pytest.mark.parametrize("per_row", [0, 1])
def test_identity_factor_is_round_to_nearest_of_the_oracle(bits, per_row):
    rng = np.random.default_rng(10 * bits + per_row)
    R, K = 9, 64
    W = rng.standard_normal((R, K)).astype(np.float32)
    s, z = GR.minmax_params(W, bits)
    s = s * np.float32(0.8)                                                     # both clamps are hit
    if not per_row:
        s, z = s[:1], z[:1]
    what, codes, obj = GR.sweep(W, s, z, bits, np.eye(K))
    n = R if per_row else 1
    y, q = cpu_backend.uniform_fake_quant(torch.from_numpy(W), torch.from_numpy(s).view(n, 1), torch.from_numpy(z).view(n, 1), bits,
                                          want_bins=True)
    assert np.array_equal(codes, q.numpy()) and (codes == 0).any() and (codes == 2 ** bits - 1).any()
    assert np.array_equal(what.view(np.int32), y.numpy().view(np.int32))
    w_rtn, c_rtn = GR.rtn(W, s, z, bits)
    assert np.array_equal(c_rtn, codes) and np.array_equal(w_rtn.view(np.int32), what.view(np.int32))
    # U = I: e = w - q, the objective is the squared rounding error
    np.testing.assert_allclose(obj, ((W.astype(np.float64) - what.astype(np.float64)) ** 2).sum(1), rtol=1e-13)


@pytest.mark.parametrize("R,K", [(3, 32), (5, 160), (4, 192), (2, 448)])
def test_blocked_order_equals_the_column_order_bit_for_bit(R, K):
    X, W = GR.inputs("correlated", 2 * K, K, R, seed=K)
    U, _ = GR.factor(X.T @ X)
    s, z = GR.minmax_params(W, 3)
    a, b = GR.sweep(W, s, z, 3, U), GR.sweep_blocked(W, s, z, 3, U)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2].view(np.int64), b[2].view(np.int64))
    assert not np.array_equal(a[1], GR.rtn(W, s, z, 3)[1])                      # (the sweep did move codes)


def test_factor_inverts_the_damped_hessian():
    X, _ = GR.inputs("correlated", 150, 96, 1, seed=3)
    X[:, 17] = 0.0                                                              # a dead column
    H = X.T @ X
    U, Hd = GR.factor(H)
    assert Hd[17, 17] == 1.0 + 0.01 * np.diagonal(GR.damp(H, 0.0)).mean() and np.allclose(np.tril(U, -1), 0.0)
    np.testing.assert_allclose(U.T @ U @ Hd, np.eye(96), atol=1e-8)
    from adalog_amd.utils.gptq import damped_factor
    Ut, Hdt = damped_factor(torch.from_numpy(H), 0.01)                          # the product's factor: the same matrices
    np.testing.assert_allclose(Hdt.numpy(), Hd, rtol=1e-14)
    np.testing.assert_allclose(Ut.numpy(), U, rtol=1e-7, atol=1e-10)


@pytest.mark.parametrize("kind", ["iid", "correlated"])
@pytest.mark.parametrize("T,K,R", [(200, 64, 48), (400, 192, 64)])
@pytest.mark.parametrize("bits", [3, 4])
def test_total_objective_is_below_round_to_nearest(kind, T, K, R, bits):
    """The issue's outcome table (measured there in fp64 on three seeds each: 0.82-0.87, 0.75-0.77 for iid X, 0.31-0.44 for correlated
    X).  Asserted: < 1 on the TOTAL; single rows may be a few percent worse, which is GPTQ's nature."""
    for seed in (0, 1, 2):
        X, W = GR.inputs(kind, T, K, R, seed)
        U, Hd = GR.factor(X.T @ X)
        s, z = GR.minmax_params(W, bits)
        what, _, obj = GR.sweep(W, s, z, bits, U)
        after = GR.quadratic(W.astype(np.float64) - what, Hd)
        np.testing.assert_allclose(obj, after, rtol=1e-8)                       # sum e^2 IS the quadratic form under the damped H
        before = GR.quadratic(W.astype(np.float64) - GR.rtn(W, s, z, bits)[0], Hd)
        ratio = after.sum() / before.sum()
        print(f"{kind} T,K,R={T},{K},{R} {bits}b seed {seed}: GPTQ / RTN objective {ratio:.3f}")
        assert ratio < 1.0


# ------------------------------------------------------------------------------------------------ C ABI, no device
def _lib():
    from adalog_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def test_sweep_entry_points_reject_bad_arguments_without_a_device():
    lib = _lib()
    for R, K, ok in ((1, 32, 1), (7, 4096, 1), (65, 160, 1), (1, 0, 0), (0, 64, 0), (4, 48, 0), (4, 16, 0), (4, 4128, 0), (4, 8192, 0)):
        assert lib.adalog_gptq_sweep_ok(R, K) == ok, (R, K)
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)                                                   # a valid host address: a rejected call never reads it
    err = lambda: lib.adalog_last_error().decode()
    for w, s, z, u, o in ((None, a, a, a, a), (a, None, a, a, a), (a, a, None, a, a), (a, a, a, None, a), (a, a, a, a, None)):
        assert lib.adalog_gptq_sweep_f32(w, 2, 32, 32, s, z, 0, 4, u, 32, o, None, None, None) == -1 and "gptq_sweep" in err() and "null" in err()
    for nb in (1, 9):
        assert lib.adalog_gptq_sweep_f32(a, 2, 32, 32, a, a, 0, nb, a, 32, a, None, None, None) == -1 and "n_bits" in err()
    for K in (48, 4128, 16):
        assert lib.adalog_gptq_sweep_f32(a, 2, K, K, a, a, 0, 4, a, K, a, None, None, None) == -1 and "unsupported sizes" in err()
    assert lib.adalog_gptq_sweep_f32(a, 2, 64, 63, a, a, 0, 4, a, 64, a, None, None, None) == -1 and "ldw" in err()
    assert lib.adalog_gptq_sweep_f32(a, 2, 64, 64, a, a, 0, 4, a, 32, a, None, None, None) == -1 and "ldu" in err()
    assert lib.adalog_gptq_sweep_f32(a, 2, 64, 64, a, a, 2, 4, a, 64, a, None, None, None) == -1 and "per_row" in err()


# ------------------------------------------------------------------------------------------------ gptq_model, host logic
@pytest.fixture(scope="module")
def be():
    impl = GptqCpuBackend()
    backend.set_backend(impl)
    yield impl
    backend.set_backend(None)


@pytest.fixture(scope="module")
def toy(be):
    """a calibrated depth-1 model (W6A6) and its input, as tests/test_packed_cpu.py builds it"""
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    model = wrap_modules_in_net(_fresh(), _cfg(), reparam=True)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    QuantCalibrator(model, [(x[:2], None), (x[2:], None)]).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model)
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    return model, x


LINEAR = [n for n in LAYERS if n != "patch_embed.proj"]


def test_gptq_model_host_logic(toy, be):
    from adalog_amd.utils.gptq import CONV_REASON, gptq_model
    model = copy.deepcopy(toy[0])
    x = toy[1]
    mods = dict(model.named_modules())
    with torch.no_grad():
        model(x)                                                                # quant_forward once
    for n in LINEAR:
        mods[n].__dict__["_wp_cache"] = ("stale", None)                         # what a warm packed-weight cache would leave
        mods[n].w_quantizer.__dict__["_codes_fit"] = "stale"
    mods["head"].w_quantizer.n_bits = 9                                         # not eligible: listed, untouched
    before = {n: mods[n].weight.data.clone() for n in LAYERS}
    hooks = {n: len(m._forward_hooks) for n, m in mods.items()}
    modes = {n: m.mode for n, m in mods.items() if hasattr(m, "mode")}
    assert set(modes.values()) == {"quant_forward"}
    be.sweeps.clear()
    res = gptq_model(model, x, damp=0.01, batch_size=3)                         # two batches: 3 + 1 images

    swept = [n for n in LINEAR if n != "head"]
    assert list(res["layers"]) == swept and res["images"] == 4 and res["damp"] == 0.01
    assert set(res["skipped"]) == {"patch_embed.proj", "head"}
    assert res["skipped"]["patch_embed.proj"] == CONV_REASON and "n_bits 9" in res["skipped"]["head"]
    assert set(res["seconds"]) == {"capture", "factor", "sweep"} and all(v >= 0 for v in res["seconds"].values())
    assert be.sweeps == [(mods[n].out_features, mods[n].in_features, 6) for n in swept]
    assert {n: len(m._forward_hooks) for n, m in mods.items()} == hooks        # hooks removed
    assert {n: m.mode for n, m in mods.items() if hasattr(m, "mode")} == modes  # modes restored
    for n in ("patch_embed.proj", "head"):
        assert torch.equal(mods[n].weight.data, before[n])
    total_before = total_after = 0.0
    for n in swept:
        m, e = mods[n], res["layers"][n]
        assert (e["R"], e["K"], e["n_bits"]) == (m.out_features, m.in_features, 6) and e["seconds"] >= 0
        assert "_wp_cache" not in m.__dict__ and "_codes_fit" not in m.w_quantizer.__dict__    # caches invalidated
        assert not torch.equal(m.weight.data, before[n])
        with torch.no_grad():
            assert torch.equal(m.quant_weight_bias()[0], m.weight.data), n      # the weight re-quantises to itself
        total_before += e["objective_before"]
        total_after += e["objective_after"]
    assert 0 < total_after < total_before
    # the committed weight is the reference's sweep under the Hessian of quant_input(x) of the FP model
    m = mods["blocks.0.mlp.fc2"]
    src = copy.deepcopy(toy[0])
    for mm in src.modules():
        if hasattr(mm, "mode"):
            mm.mode = "raw"
    got = []
    h = dict(src.named_modules())["blocks.0.mlp.fc2"].register_forward_hook(
        lambda mod, args, out: got.append(mod.quant_input(args[0]).reshape(-1, mod.in_features).double()))
    with torch.no_grad():
        src(x)
    h.remove()
    U, Hd = GR.factor((got[0].t() @ got[0]).numpy())
    wq = m.w_quantizer
    want, _, obj = GR.sweep(before["blocks.0.mlp.fc2"].numpy(), wq.scale.data.reshape(-1).numpy(), wq.zero_point.data.reshape(-1).numpy(), 6, U)
    assert np.mean(want == m.weight.data.numpy()) > 0.99                        # (two factor routines: U agrees to rounding, not bit for bit)
    np.testing.assert_allclose(res["layers"]["blocks.0.mlp.fc2"]["objective_after"], obj.sum(), rtol=1e-6)
    with torch.no_grad():
        assert torch.isfinite(model(x)).all()


def test_command_line_writes_plain_and_packed_checkpoints(toy, be, tmp_path):
    from adalog_amd.utils import gptq as G
    from adalog_amd.utils import packed as P
    from adalog_amd.utils.wrap_net import wrap_modules_in_net
    model = toy[0]
    plain = str(tmp_path / "plain.pth")
    torch.save(model.state_dict(), plain)

    def build_wrapped(name, config, device, img_size=None, depth=None):
        return wrap_modules_in_net(_fresh(), _cfg(), reparam=False)
    real = P.build_wrapped
    P.build_wrapped = build_wrapped
    try:
        outs = {}
        for flag in ([], ["--packed"]):
            out = str(tmp_path / ("gptq" + "_packed" * bool(flag) + ".pth"))
            assert G.main(["--model", "toy", "--config", "unused", "--checkpoint", plain, "--out", out, "--images", "4", "--img-size", "32",
                           "--batch-size", "2", "--device", "cpu"] + flag) == 0
            outs[bool(flag)] = out
        a = P.load_plain(build_wrapped(None, None, "cpu"), outs[False], "cpu")
        b = P.load_packed(build_wrapped(None, None, "cpu"), outs[True], "cpu")
    finally:
        P.build_wrapped = real
    x = toy[1]
    with torch.no_grad():
        ya, yb = a(x), b(x)
    assert torch.equal(ya, yb) and torch.isfinite(ya).all()
    src = dict(model.named_modules())
    for n, m in a.named_modules():
        if n in LINEAR:
            assert not torch.equal(m.weight.data, src[n].weight.data), n
            assert torch.equal(m.weight.data, dict(b.named_modules())[n].weight.data), n
