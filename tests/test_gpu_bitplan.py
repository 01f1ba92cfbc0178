"""`-m gpu`: the Hessian bit-cost kernel (csrc/bitcost.hip, ops.bit_cost) against the numpy restatement of its specification
(tests/bitplan_reference.py) under the derived bound (2K + 8) 2^-53 A, and utils/bitplan.py / cfg.w_bit_plan end to end on a depth-2
deit_tiny: the plan of the GPU kernel equals the plan of the CPU stand-in fed the same Hessians, and a mixed-width model calibrates,
runs fused, packs, loads and reports."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import bitplan_reference as BR
from tests import gptq_reference as GR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

SHAPES = [(1, 32), (17, 64), (16, 96), (130, 160), (5, 4096), (48, 1088)]
BITS = [(0, 3, 4, 6), (0, 2, 3, 4, 5, 6, 7, 8), (4,)]


def _ops():
    from adalog_amd import backend, ops
    backend.set_backend(None)
    return ops


def _last_kernel():
    from adalog_amd import _lib
    return _lib.load().adalog_last_kernel().decode()


_INPUTS, _REFS = {}, {}


def _inputs(R, K):
    """(W fp32 [R, K], H fp64 [K, K]): the correlated seeded X of tests/gptq_reference.inputs with ONE zero column (a dead row and
    column of H), H = (G + G^T) / 2 of G = X^T X"""
    if (R, K) not in _INPUTS:
        X, W = GR.inputs("correlated", 64, K, R, seed=R + K)
        X[:, K // 3] = 0.0
        G = X.T @ X
        _INPUTS[(R, K)] = (W, np.ascontiguousarray((G + G.T) * 0.5))
    return _INPUTS[(R, K)]


def _case(R, K, bits, per_row):
    """(W, scales, zero points, H) and the reference's (cost, A) -- computed once per case.  Per-row scales: row R // 2 has its scale
    multiplied by 0.25 at every width (clamped codes, large errors); single scales: the quantiser of the whole tensor's min / max."""
    key = (R, K, bits, per_row)
    if key not in _REFS:
        W, H = _inputs(R, K)
        if per_row:
            S, Z = BR.minmax_params(W, bits)
            S[:, R // 2] *= np.float32(0.25)
        else:
            S, Z = BR.minmax_params(W.reshape(1, -1), bits)
        _REFS[key] = (W, S, Z, H, BR.bit_cost(W, S, Z, bits, H))
    return _REFS[key]


def _run(ops, W, S, Z, bits, H):
    cost = ops.bit_cost(torch.from_numpy(W).to(DEV), torch.from_numpy(S).to(DEV), torch.from_numpy(Z).to(DEV), bits,
                        torch.from_numpy(H).to(DEV))
    assert _last_kernel() == "k_bit_cost"
    assert cost.dtype == torch.float64 and tuple(cost.shape) == (len(bits), W.shape[0]) and cost.is_cuda
    return cost.cpu().numpy()


def _assert_within_bound(got, ref, A, K, what):
    """|got - ref| <= (2K + 8) 2^-53 A per element: a length-K inner product nested in a length-K inner product, any summation order"""
    bound = (2 * K + 8) * 2.0 ** -53 * A
    err = np.abs(got - ref)
    ratio = np.where(A > 0, err / np.where(A > 0, A, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"{what}: max |got - ref| / A = {ratio.max():.3e}  (bound {(2 * K + 8) * 2.0 ** -53:.3e})")
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float(ratio.max()))


@pytest.mark.parametrize("per_row", [1, 0])
@pytest.mark.parametrize("bits", BITS, ids=lambda b: "b" + "".join(map(str, b)))
@pytest.mark.parametrize("R,K", SHAPES)
def test_bit_cost_matches_the_reference(R, K, bits, per_row):
    ops = _ops()
    W, S, Z, H, (ref, A) = _case(R, K, bits, per_row)
    got = _run(ops, W, S, Z, bits, H)
    _assert_within_bound(got, ref, A, K, f"[{R}, {K}] bits {bits} per_row {per_row}")
    again = _run(ops, W, S, Z, bits, H)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))             # two calls: the same bits
    if bits[0] == 0:                                                            # the signal row is w H w^T
        Wd = W.astype(np.float64)
        aW = np.abs(Wd)
        _assert_within_bound(got[0], ((Wd @ H) * Wd).sum(axis=1), ((aW @ np.abs(H)) * aW).sum(axis=1), K, "signal row")
    if per_row and R > 1:                                                       # the narrowed row clamps: its error is the largest
        i = 1 if bits[0] == 0 else 0
        d, c = BR.diff(W, S[i], Z[i], bits[i])
        assert (c[R // 2] == 0).any() and (c[R // 2] == 2 ** bits[i] - 1).any()


def test_bit_cost_rejects_what_it_does_not_take():
    """K = 48, K = 4128, nine widths, a width of 1 or 9: an error from the host-side checks, no launch"""
    from adalog_amd import _lib
    ops = _ops()
    lib = _lib.load()

    def args(R, K, nw):
        return (torch.zeros(R, K, device=DEV), torch.ones(nw, R, device=DEV), torch.zeros(nw, R, device=DEV),
                torch.eye(K, dtype=torch.float64, device=DEV))
    assert ops.bit_cost_ok(4, 64, 8) and not ops.bit_cost_ok(4, 48, 4) and not ops.bit_cost_ok(4, 4128, 4) and not ops.bit_cost_ok(4, 64, 9)
    # something else launches first, so that the label shows whether a rejected call launched
    ops.pack_codes(torch.zeros(4, 64, device=DEV), torch.ones(1, device=DEV), torch.zeros(1, device=DEV), 4)
    before = _last_kernel()
    assert before != "k_bit_cost"
    for R, K, bits in ((4, 48, (0, 3, 4, 6)), (4, 4128, (0, 3, 4, 6)), (4, 64, (0, 2, 3, 4, 5, 6, 7, 8, 4))):
        w, s, z, H = args(R, K, len(bits))
        with pytest.raises(_lib.AdalogHipError):
            ops.bit_cost(w, s, z, bits, H)
        arr = (ctypes.c_int * len(bits))(*bits)
        rc = lib.adalog_bit_cost_f32(w.data_ptr(), R, K, K, s.data_ptr(), z.data_ptr(), 1, ctypes.cast(arr, ctypes.c_void_p), len(bits),
                                     H.data_ptr(), K, w.data_ptr(), None, 0, None)
        assert rc == -1 and "unsupported sizes" in lib.adalog_last_error().decode()
    for bad in (1, 9):
        w, s, z, H = args(4, 64, 2)
        with pytest.raises(ValueError):
            ops.bit_cost(w, s, z, (0, bad), H)
        arr = (ctypes.c_int * 2)(0, bad)
        out = torch.zeros(2, 4, dtype=torch.float64, device=DEV)
        rc = lib.adalog_bit_cost_f32(w.data_ptr(), 4, 64, 64, s.data_ptr(), z.data_ptr(), 1, ctypes.cast(arr, ctypes.c_void_p), 2,
                                     H.data_ptr(), 64, out.data_ptr(), None, 0, None)
        assert rc == -1 and "width" in lib.adalog_last_error().decode()
    torch.cuda.synchronize()
    assert _last_kernel() == before


# ------------------------------------------------------------------------------------------------ whole models
PLAN = {"blocks.0.attn.qkv": 3, "blocks.0.attn.proj": 6, "blocks.0.mlp.fc1": 4, "blocks.0.mlp.fc2": 6,
        "blocks.1.attn.qkv": 6, "blocks.1.attn.proj": 4, "blocks.1.mlp.fc1": 6, "blocks.1.mlp.fc2": 3, "head": 6}


def test_gpu_plan_equals_the_cpu_stand_in_plan_on_the_same_hessians():
    """plan_bits with the kernel and with the numpy stand-in, both fed the Hessians the GPU captured: the same plan, and costs that
    agree far inside what could move an allocation"""
    from adalog_amd import backend
    from adalog_amd.utils.bitplan import plan_bits
    from adalog_amd.utils.gptq import capture_hessians
    from adalog_amd.utils.models import create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net
    from tests.bitplan_cpu_backend import BitplanCpuBackend
    from tests.test_gpu_packed import _cfg
    _ops()
    torch.manual_seed(11)
    model = wrap_modules_in_net(create_model("deit_tiny", depth=2).eval().to(DEV), _cfg(4), reparam=False).to(DEV).eval()
    x = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(11)).to(DEV)
    layers = [(n, m) for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and hasattr(m, "w_quantizer")]
    hess = capture_hessians(model, [m for _, m in layers], x, 8, lambda m, args: args[0].reshape(-1, m.in_features))
    H = {n: hess[id(m)] for n, m in layers}
    for avg in (4.0, 3.5):
        gpu = plan_bits(model, x, widths=(3, 4, 6), avg_bits=avg, hessians=H)
        assert _last_kernel() == "k_bit_cost"
        try:
            backend.set_backend(BitplanCpuBackend())
            cpu = plan_bits(model, x, widths=(3, 4, 6), avg_bits=avg, hessians=H)
        finally:
            backend.set_backend(None)
        assert list(gpu["plan"]) == [n for n, _ in layers] and gpu["plan"] == cpu["plan"], (avg, gpu["plan"], cpu["plan"])
        assert gpu["avg_bits"] == cpu["avg_bits"] <= avg and set(gpu["skipped"]) == {"patch_embed.proj"}
        for n in gpu["plan"]:
            for b in (3, 4, 6):
                np.testing.assert_allclose(gpu["layers"][n]["cost"][b], cpu["layers"][n]["cost"][b], rtol=1e-10)
    own = plan_bits(model, x, widths=(3, 4, 6), avg_bits=4.0, batch_size=4)     # its own capture pass, in two batches
    assert list(own["plan"]) == [n for n, _ in layers] and own["avg_bits"] <= 4.0


_MIXED = {}


def _mixed():
    """a depth-2 deit_tiny wrapped with PLAN the way quant_mixed.py wraps it, calibrated on 32 images; its input and logits"""
    if not _MIXED:
        import quant_mixed
        from adalog_amd.utils.calibrator import QuantCalibrator
        from adalog_amd.utils.models import create_model
        from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
        from tests.test_gpu_packed import _cfg, _logits
        _ops()
        torch.manual_seed(5)
        cfg = _cfg(4)
        wrap = quant_mixed.with_plan(wrap_modules_in_net, PLAN)
        model = wrap(create_model("deit_tiny", depth=2).eval().to(DEV), cfg, reparam=True).to(DEV)
        assert cfg.w_bit_plan == PLAN
        x = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(5)).to(DEV)
        QuantCalibrator(model, [(x, None)]).batching_quant_calib()
        model = wrap_reparamed_modules_in_net(model).to(DEV).eval()
        for m in model.modules():
            if hasattr(m, "reparam_bias"):
                m.reparam_bias()
        _MIXED["v"] = (model, x[:4].contiguous(), _logits(model, x[:4].contiguous()))
    return _MIXED["v"]


def test_mixed_width_model_calibrates_and_runs_fused():
    ops = _ops()
    model, x, (fused, unfused) = _mixed()
    mods = dict(model.named_modules())
    assert int(mods["patch_embed.proj"].w_quantizer.n_bits) == 4               # not in the plan: the config's width
    for n, b in PLAN.items():
        m = mods[n]
        wq = m.w_quantizer
        assert int(wq.n_bits) == b and type(m).__name__ in ("AsymmetricallyBatchingQuantLinear", "PostGeluLogBasedBatchingQuantLinear"), n
        w2 = m.weight.data.reshape(m.weight.shape[0], -1)
        nch = wq.scale.numel()
        _, codes = ops.uniform_fake_quant(w2, wq.scale.data.reshape(nch, 1), wq.zero_point.data.reshape(nch, 1), b, want_bins=True)
        assert int(codes.min()) >= 0 and int(codes.max()) <= 2 ** b - 1 and len(torch.unique(codes)) > 2 ** (b - 1), n
    assert torch.isfinite(fused).all() and torch.equal(fused, unfused), (fused - unfused).abs().max().item()


def test_mixed_width_model_packs_loads_and_reports(tmp_path):
    from adalog_amd.utils import packed as P
    from adalog_amd.utils.report import format_table, quant_report
    from tests.test_gpu_packed import _assert_same_logits, _cfg_path, _logits
    model, x, want = _mixed()
    path = str(tmp_path / "mixed_packed.pth")
    obj = P.save_packed(model, path)
    assert {n: obj["meta"]["packed"][n]["n_bits"] for n in PLAN} == PLAN and obj["meta"]["packed"]["patch_embed.proj"]["n_bits"] == 4
    loaded = P.load_packed(P.build_wrapped("deit_tiny", _cfg_path(4), DEV, depth=2, bit_plan=PLAN), path, DEV)
    assert {n: int(m.w_quantizer.n_bits) for n, m in loaded.named_modules() if n in PLAN} == PLAN
    _assert_same_logits(_logits(loaded, x), want)
    with pytest.raises(ValueError, match="bits"):                               # the same file without the plan: the width check
        P.load_packed(P.build_wrapped("deit_tiny", _cfg_path(4), DEV, depth=2), path, DEV)
    rep = quant_report(model, x)
    assert {n: rep["modules"][n]["quantizers"]["w_quantizer"]["n_bits"] for n in PLAN} == PLAN
    table = format_table(rep)
    assert all(f"{b}b" in table for b in (3, 4, 6))
