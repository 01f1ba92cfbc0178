"""Bias correction without a device: the host logic of adalog_amd/utils/bias_correct.py on a calibrated depth-2 toy model with a stand-in
backend (tests/biascorr_cpu_backend.py) -- the layer-by-layer recurrence against its fp64 restatement (tests/biascorr_reference.py) for
one chunk and for three uneven ones, eligibility, restoring on every exit, gptq_model's default --, the restatement of ops.mean_err
itself, and the argument checks of the two C entry points."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from adalog_amd import backend
from tests import biascorr_reference as BR
from tests.biascorr_cpu_backend import BiasCorrCpuBackend
from tests.test_packed_cpu import _cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement of ops.mean_err
def test_exact_moments_on_a_case_done_by_hand():
    a = np.array([1.0, 2.0, 3.0, 4.0, 5.0, -6.0], np.float32)
    b = np.array([0.5, 2.0, 1.0, 5.0, 5.0, 0.0], np.float32)
    ex = BR.exact_moments(a, b, 3, 1)                                           # rows of [c0, c1, c2]: channels (1, 4), (2, 5), (3, -6)
    assert ex["n_c"] == 2
    assert ex["sum_d"].tolist() == [-0.5, 0.0, -4.0] and ex["sum_d2"].tolist() == [1.25, 0.0, 40.0]
    assert ex["sum_abs_d"].tolist() == [1.5, 0.0, 8.0] and ex["max_a"].tolist() == [4.0, 5.0, 6.0]
    ex = BR.exact_moments(a, b, 2, 3)                                           # one row of two channels of three
    assert ex["sum_d"].tolist() == [2.5, -7.0] and ex["max_a"].tolist() == [3.0, 6.0]
    p, e = BR._two_square(np.array([1.0 + 2.0 ** -30]))                         # (1 + h)^2 = 1 + 2h + h^2: h^2 = 2^-60 is the residue
    assert p[0] == 1.0 + 2.0 ** -29 and e[0] == 2.0 ** -60


def test_cancellation_case_separates_fp64_from_fp32():
    """The issue's case: d alternates +-1e4 around a mean of 1e-3.  A plain fp64 running sum stays inside the bound with a wide
    margin; an fp32 subtraction or an fp32 running sum does not."""
    a, b = BR.cancellation_case(1 << 16, 2)
    ex = BR.exact_moments(a, b, 2, 1)
    bd, bd2 = BR.sum_bounds(ex)
    A, B = BR.channel_rows(a, 2, 1), BR.channel_rows(b, 2, 1)
    D = A.astype(np.float64) - B.astype(np.float64)
    for c in range(2):
        assert abs(ex["sum_d"][c] / ex["n_c"] - 1e-3) < 1e-4                    # (the mean the case was built around)
        run = float(np.cumsum(D[c])[-1])                                        # a sequential fp64 sum: the worst order there is
        run2 = float(np.cumsum(D[c] * D[c])[-1])
        assert abs(run - ex["sum_d"][c]) <= 1e-3 * bd[c] and abs(run2 - ex["sum_d2"][c]) <= 1e-1 * bd2[c]
        sub32 = float(np.cumsum((A[c] - B[c]).astype(np.float64))[-1])          # a - b rounded to fp32, summed in fp64
        acc32 = float(np.cumsum(D[c].astype(np.float32), dtype=np.float32)[-1])  # fp32 accumulation
        assert abs(sub32 - ex["sum_d"][c]) > bd[c] and abs(acc32 - ex["sum_d"][c]) > bd[c]


# ------------------------------------------------------------------------------------------------ C ABI, no device
def test_mean_err_entry_points_reject_bad_arguments_without_a_device():
    from adalog_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    assert lib.adalog_mean_err_workspace_bytes(0, 3, 1) == 0 and lib.adalog_mean_err_workspace_bytes(10, 3, 1) == -1
    assert lib.adalog_mean_err_workspace_bytes(12, 3, 1) == 3 * 3 * 8           # one part of three doubles per channel
    assert lib.adalog_mean_err_workspace_bytes(12, 3, 1) * 4 == lib.adalog_err_stats_workspace_bytes(12, 3, 1) * 3
    assert lib.adalog_mean_err_workspace_bytes(64, 1, 1) == lib.adalog_mean_err_workspace_bytes(64, 1, 64) == 3 * 8
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)                                                   # a valid host address: a rejected call never reads it
    err = lambda: lib.adalog_last_error().decode()
    assert lib.adalog_mean_err_f32(a, a, 10, 3, 1, a, a, 512, None) == -1 and "mean_err: bad sizes" in err()
    assert lib.adalog_mean_err_f32(a, a, 12, 3, 1, None, a, 512, None) == -1 and "out" in err()
    assert lib.adalog_mean_err_f32(None, a, 12, 3, 1, a, a, 512, None) == -1 and "4-byte aligned" in err()
    assert lib.adalog_mean_err_f32(a, a + 2, 12, 3, 1, a, a, 512, None) == -1 and "4-byte aligned" in err()
    assert lib.adalog_mean_err_f32(a, a, 12, 3, 1, a, None, 512, None) == -1 and "workspace" in err()
    assert lib.adalog_mean_err_f32(a, a, 12, 3, 1, a, a, 71, None) == -1 and "workspace" in err()


# ------------------------------------------------------------------------------------------------ the host module
@pytest.fixture(scope="module")
def be():
    impl = BiasCorrCpuBackend()
    backend.set_backend(impl)
    yield impl
    backend.set_backend(None)


@pytest.fixture(scope="module")
def toy(be):
    """a calibrated depth-2 model (W6A6) and eight images"""
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.models import VisionTransformer
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    torch.manual_seed(7)
    model = VisionTransformer(img_size=32, patch_size=8, embed_dim=32, depth=2, num_heads=2, num_classes=10).eval()
    for p in model.parameters():
        p.data.mul_(8.0)
    for m in model.modules():                                                   # (the initialisation zeroes every bias)
        if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d)) and m.bias is not None:
            m.bias.data.normal_(0.0, 0.5)
    model = wrap_modules_in_net(model, _cfg(), reparam=True)
    x = torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(2))
    QuantCalibrator(model, [(x[:2], None), (x[2:4], None)]).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model)
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    return model, x


LAYERS = ["patch_embed.proj"] + [f"blocks.{i}.{n}" for i in (0, 1) for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")] + ["head"]
MATMULS = [f"blocks.{i}.attn.matmul{j}" for i in (0, 1) for j in (1, 2)]


def _state(model):
    return {k: v.clone() for k, v in model.state_dict().items()}


def test_recurrence_for_one_chunk_and_three_uneven_chunks(toy, be):
    """Biases against the fp64 restatement on whole forward passes: the product's means are chunk sums of exactly rounded sums (the
    stand-in's math.fsum), the restatement's one exactly rounded sum, so the two differ by the additions over the chunks -- within
    the summation bound n u sum |d| / T -- and float32(m) by at most one fp32 unit where that difference straddles a rounding boundary.
    The same holds between the two chunkings: the CPU forward is row for row independent of the batch it runs in as long as no chunk
    is a single image (the head's product over one cls token takes a matrix-vector routine with other last bits), hence 3 + 3 + 2."""
    from adalog_amd.utils.bias_correct import bias_correct_model, measure_bias_error
    model, x = toy
    results = {}
    for step in (8, 3):                                                         # one chunk; 3 + 3 + 2 images
        chunks = [x[s:s + step] for s in range(0, 8, step)]
        mine = copy.deepcopy(model)
        before = _state(mine)
        be.mean_errs.clear()
        res = bias_correct_model(mine, x, batch_size=step)
        assert list(res["layers"]) == LAYERS and sorted(res["skipped"]) == MATMULS and res["images"] == 8 and res["seconds"] >= 0
        assert len(be.mean_errs) == len(LAYERS) * len(chunks)
        assert be.mean_errs[0][1:] == (32, 16) and all(c[2] == 1 for c in be.mean_errs[len(chunks):])   # the CPU convolution: [B, C, H W]
        want, means = BR.recurrence(model, chunks)
        mods, ref = dict(mine.named_modules()), dict(want.named_modules())
        for n in LAYERS:
            e, b, r = res["layers"][n], mods[n].bias.data, ref[n].bias.data
            T = e["T"]
            assert (e["C"], T) == (b.numel(), 8 * (16 if n == "patch_embed.proj" else 1 if n == "head" else 17))
            assert e["max_delta"] > 0 and not torch.equal(b, before[n + ".bias"])
            ulp = torch.maximum(b.abs(), r.abs()) * 2.0 ** -23
            assert bool(((b - r).abs() <= ulp).all()), (step, n, (b - r).abs().max())
            np.testing.assert_allclose(e["mean_abs_before"], float(means[n].abs().mean()), rtol=1e-9)
            assert 0 <= e["sq_err_after_predicted"] <= e["sq_err_before"]
        now = mine.state_dict()
        for k, v in before.items():                                            # weights, scales, zero points, everything but the biases
            if k[:-len(".bias")] not in LAYERS or not k.endswith(".bias"):
                assert torch.equal(now[k], v), k
        # read-only measurement of the corrected model: the means are gone to rounding, sum d^2 is the predicted one
        state = _state(mine)
        after = measure_bias_error(mine, x, batch_size=step, quant_max=True)
        assert all(torch.equal(v, state[k]) for k, v in mine.state_dict().items())
        for n in LAYERS:
            a, e = after["layers"][n], res["layers"][n]
            bound = 4 * 2.0 ** -24 * (a["max_abs_fp"] + a["max_abs_q"] + mods[n].bias.data.double().abs())
            assert bool((a["mean"].abs() <= bound).all()), (step, n)
            slack = 2 * a["T"] * float((bound * (a["sq_err"] / a["T"]).sqrt()).sum()) + 1e-12 * e["sq_err_before"]
            assert abs(float(a["sq_err"].sum()) - e["sq_err_after_predicted"]) <= slack, (step, n)
        results[step] = mine
    a, b = (dict(results[s].named_modules()) for s in (8, 3))
    for n in LAYERS:
        d = (a[n].bias.data - b[n].bias.data).abs()
        assert bool((d <= a[n].bias.data.abs() * 2.0 ** -23).all()), (n, d.max())


def test_eligibility_and_untouched_tensors(toy, be):
    from adalog_amd.utils.bias_correct import bias_correct_model
    model = copy.deepcopy(toy[0])
    mods = dict(model.named_modules())
    mods["blocks.1.attn.proj"].bias = None                                      # a bias-free layer
    mods["head"].calibrated, mods["head"].mode = False, "raw"                   # an uncalibrated one (it cannot run quant_forward)
    before = _state(model)
    res = bias_correct_model(model, toy[1], batch_size=3)
    left = ["blocks.1.attn.proj", "head"]
    assert list(res["layers"]) == [n for n in LAYERS if n not in left]
    assert sorted(res["skipped"]) == sorted(MATMULS + left)
    assert res["skipped"]["blocks.1.attn.proj"] == "no bias" and res["skipped"]["head"] == "not calibrated"
    assert all("product of two activations" in res["skipped"][n] for n in MATMULS)
    assert mods["head"].mode == "raw" and mods["blocks.1.attn.proj"].bias is None
    now = model.state_dict()
    changed = [k for k, v in before.items() if not torch.equal(now[k], v)]
    assert sorted(changed) == sorted(n + ".bias" for n in res["layers"])        # nothing but the corrected biases moved


def test_modes_switches_and_hooks_are_restored_on_every_exit(toy, be):
    from adalog_amd.utils import models as M
    from adalog_amd.utils.bias_correct import bias_correct_model, measure_bias_error
    model = copy.deepcopy(toy[0])
    mods = dict(model.named_modules())
    mods["blocks.0.mlp.fc1"].mode = "debug_only_quant_weight"                   # a mode of its own: listed, and put back as it was
    modes = {n: m.mode for n, m in mods.items() if hasattr(m, "mode")}
    hooks = {n: len(m._forward_hooks) for n, m in mods.items()}
    ptrs = {n: m.bias.data_ptr() for n, m in mods.items() if n in LAYERS}
    saved = (M.QF_FUSED, M.QF_ATTN_CORE, M.QF_LONG)

    def check():
        assert (M.QF_FUSED, M.QF_ATTN_CORE, M.QF_LONG) == (True, True, True)
        assert {n: m.mode for n, m in mods.items() if hasattr(m, "mode")} == modes
        assert {n: m.bias.data_ptr() for n, m in mods.items() if n in LAYERS} == ptrs      # the FP biases are out again
    try:
        M.QF_FUSED = M.QF_ATTN_CORE = M.QF_LONG = True
        res = bias_correct_model(model, toy[1], batch_size=2)
        assert "debug_only_quant_weight" in res["skipped"]["blocks.0.mlp.fc1"]
        check()
        assert {n: len(m._forward_hooks) for n, m in mods.items()} == hooks
        measure_bias_error(model, toy[1], batch_size=8)
        check()

        def boom(mod, args, out):
            raise RuntimeError("raised inside a hook")
        h = mods["blocks.1.mlp.fc1"].register_forward_hook(boom)
        for fn in (bias_correct_model, measure_bias_error):
            with pytest.raises(RuntimeError, match="raised inside a hook"):
                fn(model, toy[1], batch_size=2)
            check()
            assert {n: len(m._forward_hooks) for n, m in mods.items()} == {**hooks, "blocks.1.mlp.fc1": 1}
        h.remove()
    finally:
        M.QF_FUSED, M.QF_ATTN_CORE, M.QF_LONG = saved


def test_fp_side_keeps_the_uncorrected_biases_and_drops_the_shift_fold(toy, be):
    """What makes the correction converge: raw mode shares the bias with quant_forward, so the FP side runs on the biases kept from
    before the correction; fc2's is the bias without the fold of reparam_bias, i.e. (to one rounding) the bias before reparam_bias."""
    from adalog_amd.utils.bias_correct import bias_correct_model, remember_fp_biases
    model = copy.deepcopy(toy[0])
    mods = dict(model.named_modules())
    assert not any("_bc_fp_bias" in m.__dict__ for m in mods.values())
    remember_fp_biases(model)
    fc2 = mods["blocks.0.mlp.fc2"]
    assert bool(fc2.a_quantizer.bias_reparamed)
    s = fc2.w_quantizer.scale.data.view(-1)
    rowsum = torch.round(fc2.quant_weight_bias()[0].detach() / s.view(-1, 1)).sum(1)
    fold = -(fc2.a_quantizer.shift.data * (s * rowsum))
    assert float(fold.abs().max()) > 0.1
    assert torch.equal(fc2.__dict__["_bc_fp_bias"], fc2.bias.data - fold)
    assert torch.equal(mods["blocks.0.attn.qkv"].__dict__["_bc_fp_bias"], mods["blocks.0.attn.qkv"].bias.data)
    kept = {n: mods[n].__dict__["_bc_fp_bias"].clone() for n in LAYERS}
    first = bias_correct_model(model, toy[1], batch_size=8)
    second = bias_correct_model(model, toy[1], batch_size=8)                    # the second call finds nothing left to correct
    for n in LAYERS:
        assert torch.equal(mods[n].__dict__["_bc_fp_bias"], kept[n])
        assert second["layers"][n]["max_delta"] <= 1e-5 * max(first["layers"][n]["max_delta"], 1e-3), n


def test_gptq_default_is_unchanged_and_the_flag_corrects_after_the_sweep(toy, be):
    from adalog_amd.utils.gptq import gptq_model
    x = toy[1]
    runs = {}
    for key, kw in (("default", {}), ("off", {"bias_correct": False}), ("on", {"bias_correct": True})):
        m = copy.deepcopy(toy[0])
        runs[key] = (m, gptq_model(m, x, damp=0.01, batch_size=3, **kw))
    for key in ("default", "off"):
        m, res = runs[key]
        assert set(res) == {"images", "damp", "layers", "skipped", "seconds"}
        assert not any("_bc_fp_bias" in mod.__dict__ for mod in m.modules())
    sd = {k: r[0].state_dict() for k, r in runs.items()}
    assert all(torch.equal(v, sd["off"][k]) for k, v in sd["default"].items())
    for k in ("layers", "skipped", "images", "damp"):
        strip = lambda d: {n: {a: b for a, b in e.items() if a != "seconds"} for n, e in d.items()} if k == "layers" else d
        assert strip(runs["default"][1][k]) == strip(runs["off"][1][k])
    on = runs["on"][1]
    assert list(on["bias_correct"]["layers"]) == LAYERS
    for k, v in sd["on"].items():                                               # the sweep is the same; only biases moved
        assert torch.equal(v, sd["off"][k]) != (k.endswith(".bias") and k[:-5] in LAYERS), k
    with torch.no_grad():
        assert torch.isfinite(runs["on"][0](x)).all()


def test_command_line_writes_plain_and_packed_checkpoints(toy, be, tmp_path, capsys):
    from adalog_amd.utils import bias_correct as BC
    from adalog_amd.utils import packed as P
    from adalog_amd.utils.models import VisionTransformer
    from adalog_amd.utils.wrap_net import wrap_modules_in_net
    model, x = toy
    plain = str(tmp_path / "plain.pth")
    torch.save(model.state_dict(), plain)

    def build_wrapped(name, config, device, img_size=None, depth=None):
        net = VisionTransformer(img_size=32, patch_size=8, embed_dim=32, depth=2, num_heads=2, num_classes=10).eval()
        return wrap_modules_in_net(net, _cfg(), reparam=False)
    real = P.build_wrapped
    P.build_wrapped = build_wrapped
    try:
        outs = {}
        for flag in ([], ["--packed"]):
            out = str(tmp_path / ("bc" + "_packed" * bool(flag) + ".pth"))
            assert BC.main(["--model", "toy", "--config", "unused", "--checkpoint", plain, "--out", out, "--images", "8", "--img-size", "32",
                            "--batch-size", "2", "--seed", "2", "--device", "cpu"] + flag) == 0
            outs[bool(flag)] = out
        line = capsys.readouterr().out
        assert f"{len(LAYERS)} layers corrected, {len(MATMULS)} left as they were" in line and "->" in line
        a = P.load_plain(build_wrapped(None, None, "cpu"), outs[False], "cpu")
        b = P.load_packed(build_wrapped(None, None, "cpu"), outs[True], "cpu")
    finally:
        P.build_wrapped = real
    mine = copy.deepcopy(model)
    BC.bias_correct_model(mine, x, batch_size=2)                                # (--seed 2 draws the fixture's images)
    with torch.no_grad():
        ya, yb, ym = a(x), b(x), mine(x)
    assert torch.equal(ya, yb) and torch.equal(ya, ym) and torch.isfinite(ya).all()
    src = dict(mine.named_modules())
    for n, m in a.named_modules():
        if n in LAYERS:
            assert torch.equal(m.bias.data, src[n].bias.data), n
