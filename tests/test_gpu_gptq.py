"""`-m gpu`: the GPTQ column sweep (csrc/gptq.hip, ops.gptq_sweep) against the numpy reference of its specification
(tests/gptq_reference.py) -- codes and weights bit for bit, the objective to 1e-12 --, ops.gptq_hessian_add against fp64, and
utils/gptq.py end to end on a calibrated depth-2 deit_tiny."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gptq_reference as GR
from tests.test_gpu_packed import _assert_same_logits, _cfg, _cfg_path, _logits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _ops():
    from adalog_amd import backend, ops
    backend.set_backend(None)
    return ops


def _last_kernel():
    from adalog_amd import _lib
    return _lib.load().adalog_last_kernel().decode()


_FACTORS = {}


def _factor(K, dead=None):
    """U (fp64, host) factored from a seeded correlated X [2K or 256 rows, K]; ``dead``: a column of X that is zero (H_jj = 0)"""
    key = (K, dead)
    if key not in _FACTORS:
        from adalog_amd.utils.gptq import damped_factor
        rng = np.random.default_rng(K)
        T = min(2 * K, 256)
        X = rng.standard_normal((T, K)) @ (0.3 * np.eye(K) + rng.standard_normal((K, K)) / np.sqrt(K)) + 0.5
        if dead is not None:
            X[:, dead] = 0.0
        U, _ = damped_factor(torch.from_numpy(X.T @ X), 0.01)
        _FACTORS[key] = U.numpy()
    return _FACTORS[key]


_REFS = {}


def _case(R, K, bits, per_row, clip=False, dead=None):
    """(W, s, z, U) as numpy and the reference's (What, codes, objective) -- computed once per case"""
    key = (R, K, bits, per_row, clip, dead)
    if key not in _REFS:
        rng = np.random.default_rng(1000 * bits + R + K + per_row)
        W = rng.standard_normal((R, K)).astype(np.float32)
        s, z = GR.minmax_params(W, bits)
        if clip:
            s[R // 2] *= np.float32(0.25)                    # this row's grid covers a quarter of its range: clamped codes, large errors
        if not per_row:
            s, z = s[:1].copy(), z[:1].copy()
            if clip:
                s *= np.float32(0.25)
        U = _factor(K, dead)
        _REFS[key] = (W, s, z, U, GR.sweep(W, s, z, bits, U))
    return _REFS[key]


def _run(ops, W, s, z, bits, U):
    what, codes, obj = ops.gptq_sweep(torch.from_numpy(W).to(DEV), torch.from_numpy(s).to(DEV), torch.from_numpy(z).to(DEV), bits,
                                      torch.from_numpy(U).to(DEV), want_codes=True, want_objective=True)
    assert _last_kernel() == "k_gptq_sweep"
    return what.cpu().numpy(), codes.cpu().numpy(), obj.cpu().numpy()


def _assert_equal(got, want, what):
    assert got[1].dtype == np.uint8 and np.array_equal(got[1], want[1]), (what, "codes", int((got[1] != want[1]).sum()))
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), (what, "What")
    rel = np.abs(got[2] - want[2]).max() / np.abs(want[2]).max()
    print(f"{what}: objective relative difference {rel:.3e}")
    assert rel <= 1e-12, (what, rel)


# (1, 32): one row, one column group per lane; (5, 64); (65, 160): K no multiple of 64; (48, 192); (7, 4096): 64 slots per lane.
# (3, 320), (2, 544), (3, 1088): the other slot-count instantiations; (1030, 32): four waves per workgroup; (2049, 96), (2050, 544): two
# rows per wave (R > 2048), the last wave with one row / with two
SHAPES = [(1, 32), (5, 64), (65, 160), (48, 192), (7, 4096), (3, 320), (2, 544), (3, 1088), (1030, 32), (2049, 96), (2050, 544)]


@pytest.mark.parametrize("R,K", SHAPES)
def test_sweep_equals_the_reference_bit_for_bit(R, K):
    ops = _ops()
    W, s, z, U, want = _case(R, K, 4, 1)
    got = _run(ops, W, s, z, 4, U)
    _assert_equal(got, want, (R, K))
    again = _run(ops, W, s, z, 4, U)                                            # the same call twice: the same bits
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again))
    assert not np.array_equal(want[1], GR.rtn(W, s, z, 4)[1]) or K == 32       # (the sweep is not round-to-nearest)


@pytest.mark.parametrize("per_row", [0, 1])
@pytest.mark.parametrize("bits", [2, 3, 4, 8])
def test_sweep_bits_and_parameter_layouts(bits, per_row):
    ops = _ops()
    W, s, z, U, want = _case(48, 192, bits, per_row)
    _assert_equal(_run(ops, W, s, z, bits, U), want, (bits, per_row))


@pytest.mark.parametrize("per_row", [0, 1])
def test_sweep_with_a_clipping_scale(per_row):
    ops = _ops()
    W, s, z, U, want = _case(48, 192, 3, per_row, clip=True)
    rows = want[1][24] if per_row else want[1]
    assert ((rows == 0).mean() + (rows == 7).mean()) > 0.3                      # clamped codes feed large errors forward
    _assert_equal(_run(ops, W, s, z, 3, U), want, ("clip", per_row))


def test_sweep_with_a_dead_column():
    ops = _ops()
    W, s, z, U, want = _case(48, 192, 4, 1, dead=70)
    _assert_equal(_run(ops, W, s, z, 4, U), want, "dead column")


def test_sweep_wrapper_copies_views_and_rejects_what_the_kernel_cannot_take():
    ops = _ops()
    from adalog_amd._lib import AdalogHipError
    W, s, z, U, want = _case(48, 192, 4, 1)
    wt = torch.from_numpy(np.ascontiguousarray(W.T)).to(DEV).t()                # [48, 192] with strides (1, 48): copied, as the other ops do
    ut = torch.from_numpy(np.ascontiguousarray(U.T)).to(DEV).t()
    assert not wt.is_contiguous() and not ut.is_contiguous()
    sd, zd = torch.from_numpy(s).to(DEV), torch.from_numpy(z).to(DEV)
    what = ops.gptq_sweep(wt, sd, zd, 4, ut)
    assert isinstance(what, torch.Tensor) and np.array_equal(what.cpu().numpy().view(np.int32), want[0].view(np.int32))
    w, u = wt.contiguous(), ut.contiguous()
    assert ops.gptq_sweep_ok(48, 192) and not ops.gptq_sweep_ok(48, 200) and not ops.gptq_sweep_ok(4, 4128)
    with pytest.raises(AdalogHipError, match="unsupported shape"):
        ops.gptq_sweep(w[:, :48].contiguous(), sd, zd, 4, u[:48, :48].contiguous())
    with pytest.raises(ValueError):
        ops.gptq_sweep(w, sd, zd, 4, u.float())
    with pytest.raises(ValueError):
        ops.gptq_sweep(w, sd, zd, 4, u[:160, :160].contiguous())
    with pytest.raises(ValueError):
        ops.gptq_sweep(w, sd[:5], zd[:5], 4, u)
    with pytest.raises(ValueError):
        ops.gptq_sweep(w, sd, zd, 9, u)
    with pytest.raises(AdalogHipError):
        ops.gptq_sweep(w.cpu(), sd, zd, 4, u)


def test_hessian_add_against_fp64():
    """T = 394, K = 96 in two chunks; measure and bar of the three-term gemm_f32x3 product in tests/test_gpu_kernels.py: the largest
    difference over the largest reference entry, <= 2e-6 (measured: 2.1e-12, the build is exact to 2^-31 of the largest input)."""
    ops = _ops()
    x = torch.randn(394, 96, generator=torch.Generator().manual_seed(11)).to(DEV) * 3.0 + 0.5
    H = torch.zeros(96, 96, dtype=torch.float64, device=DEV)
    assert ops.gptq_hessian_add(H, x[:197]) is H
    assert _last_kernel().startswith("bq_gemm<")
    ops.gptq_hessian_add(H, x[197:])
    ref = x.double().t() @ x.double()
    err = ((H - ref).abs().max() / ref.abs().max()).item()
    print(f"gptq_hessian_add: relative error {err:.3e}")
    assert err <= 2e-6
    H2 = torch.zeros_like(H)
    ops.gptq_hessian_add(H2, x, chunk=100)                                      # four chunks inside one call
    assert ((H2 - ref).abs().max() / ref.abs().max()).item() <= 2e-6
    H3 = torch.zeros_like(H)
    ops.gptq_hessian_add(H3, x * 1e-20)                                         # the slices follow the chunk's own magnitude
    assert ((H3 * 1e40 - ref).abs().max() / ref.abs().max()).item() <= 2e-6
    with pytest.raises(ValueError):
        ops.gptq_hessian_add(H.float(), x)
    with pytest.raises(ValueError):
        ops.gptq_hessian_add(H, x, chunk=513)                                   # a longer chunk's slice products are not exact in fp32


# ------------------------------------------------------------------------------------------------ end to end
def _calibrated(bits):
    """a depth-2 deit_tiny with seeded random weights, calibrated on 8 synthetic images (as tests/test_gpu_packed.py builds its model)"""
    _ops()
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.models import create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    torch.manual_seed(5)
    model = wrap_modules_in_net(create_model("deit_tiny", depth=2).eval().to(DEV), _cfg(bits), reparam=True).to(DEV)
    x = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(5)).to(DEV)
    QuantCalibrator(model, [(x, None)]).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model).to(DEV).eval()
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    return model, x


def _fp_logits(model, x):
    mods = [m for m in model.modules() if hasattr(m, "mode")]
    saved = [m.mode for m in mods]
    for m in mods:
        m.mode = "raw"
    try:
        with torch.no_grad():
            return model(x).clone()
    finally:
        for m, mode in zip(mods, saved):
            m.mode = mode


def _fresh_hessians(model, names, x, batch):
    """fp64 torch Hessians of quant_input(x) of the FP model, from hooks of this test's own.  The images go through in the batches
    gptq_model uses: the FP forward's last bits depend on the batch shape, and a last bit in front of a quantiser's rounding moves a
    code of quant_input(x) by a whole step (measured: 1e-6 .. 5e-6 of a layer's objective between batches of 8 and of 3)."""
    mods = dict(model.named_modules())
    H, handles = {}, []
    for n in names:
        def hook(m, args, out, n=n):
            xq = m.quant_input(args[0]).reshape(-1, m.in_features).double()
            H[n] = H.get(n, 0) + xq.t() @ xq
        handles.append(mods[n].register_forward_hook(hook))
    for i in range(0, x.shape[0], batch):
        _fp_logits(model, x[i:i + batch])
    for h in handles:
        h.remove()
    return H


def _sqnr_db(ref, y):
    return float(10 * torch.log10(ref.double().pow(2).sum() / (ref.double() - y.double()).pow(2).sum()))


@pytest.mark.parametrize("bits", [4, 3])
def test_gptq_model_end_to_end(bits, tmp_path):
    """Assertions 1-6 of the feature's specification; the bar of assertion 1 (returned objective against an fp64 recomputation from a
    fresh capture: 1e-6 relative) is the specification's.  Measured on an MI355X with the exact sliced Hessian build of
    ops.gptq_hessian_add: 7e-12 .. 6e-9 on the block layers, 1.7e-8 (W4) and 7.9e-9 (W3) on the head, whose Hessian has 8 tokens.
    (A plain fp32-accumulating product per batch gave 2e-6 .. 5e-6, one per 32 tokens 1.03e-6 on the W4 head: the swept error lives in
    the low-curvature directions of H, which amplify H's error.)  The agreement is asserted last, so that a miss still shows the
    other five."""
    ops = _ops()
    from adalog_amd.utils import packed as P
    from adalog_amd.utils.gptq import CONV_REASON, damped_factor, gptq_model
    model, x = _calibrated(bits)
    plain_before = str(tmp_path / "calibrated.pth")
    torch.save(model.state_dict(), plain_before)
    fp = _fp_logits(model, x)
    logits_before = _logits(model, x)                                           # every packed-weight cache is warm now
    layers = [(n, m) for n, m in model.named_modules() if hasattr(m, "w_quantizer")]
    w0 = {n: m.weight.data.clone() for n, m in layers}
    other = {k: v.clone() for k, v in model.state_dict().items() if not any(k == n + ".weight" for n, _ in layers)}
    swept = [n for n, m in layers if isinstance(m, torch.nn.Linear)]
    H = _fresh_hessians(model, swept, x, 3)                                      # of the FP model: before any weight is committed

    res = gptq_model(model, x, damp=0.01, batch_size=3)
    assert list(res["layers"]) == swept and len(swept) == 9
    assert res["skipped"] == {"patch_embed.proj": CONV_REASON}
    assert all(m.mode == "quant_forward" for m in model.modules() if hasattr(m, "mode"))
    mods = dict(model.named_modules())

    # 1. the objective, recomputed in fp64 torch from a fresh capture, is below round-to-nearest's and is the returned one
    tot_after = tot_rtn = 0.0
    misses = []
    for n in swept:
        m, e = mods[n], res["layers"][n]
        R, K = m.out_features, m.in_features
        assert (e["R"], e["K"], e["n_bits"]) == (R, K, bits)
        Hd = damped_factor(H[n], 0.01)[1].to(DEV)
        wq = m.w_quantizer
        w_rtn = ops.uniform_fake_quant(w0[n], wq.scale.data.view(R, 1), wq.zero_point.data.view(R, 1), bits)
        d_after, d_rtn = (w0[n] - m.weight.data).double(), (w0[n] - w_rtn).double()
        after, rtn = float(((d_after @ Hd) * d_after).sum()), float(((d_rtn @ Hd) * d_rtn).sum())
        print(f"W{bits} {n}: objective rtn {rtn:.6g} gptq {after:.6g} (returned {e['objective_after']:.6g}, before {e['objective_before']:.6g}) "
              f"ratio {after / rtn:.3f}  rel. difference to returned {abs(after - e['objective_after']) / after:.2e}")
        for got, want, which in ((e["objective_after"], after, "after"), (e["objective_before"], rtn, "before")):
            if abs(want - got) > 1e-6 * want:
                misses.append((n, which, abs(want - got) / want))              # (asserted at the end: the other assertions run first)
        tot_after, tot_rtn = tot_after + after, tot_rtn + rtn
        # 2. the committed weight lies on the quantiser's grid
        with torch.no_grad():
            assert torch.equal(m.quant_weight_bias()[0].view(torch.int32), m.weight.data.view(torch.int32)), n
        assert not torch.equal(m.weight.data, w0[n])
    assert tot_after < tot_rtn

    # 5. everything else is untouched, tensor for tensor
    assert torch.equal(mods["patch_embed.proj"].weight.data, w0["patch_embed.proj"])
    now = model.state_dict()
    for k, v in other.items():
        assert torch.equal(now[k], v), k

    # 3. no stale cache: the logits are those of a freshly wrapped model loaded from this model's state_dict, on both routes
    logits_after = _logits(model, x)
    plain = str(tmp_path / "gptq_plain.pth")
    torch.save(model.state_dict(), plain)
    fresh = P.load_plain(P.build_wrapped("deit_tiny", _cfg_path(bits), DEV, depth=2), plain, DEV)
    _assert_same_logits(logits_after, _logits(fresh, x))
    assert not torch.equal(logits_after[0], logits_before[0])

    # 4. the packed export round-trips
    packed = str(tmp_path / "gptq_packed.pth")
    obj = P.save_packed(model, packed)
    assert obj["meta"]["kept_fp32"] == {}
    loaded = P.load_packed(P.build_wrapped("deit_tiny", _cfg_path(bits), DEV, depth=2), packed, DEV)
    _assert_same_logits(_logits(loaded, x), logits_after)

    # recorded, not asserted: random weights say nothing about a trained network
    print(f"W{bits}A{bits} depth-2 deit_tiny, random weights: logit SQNR against the FP model {_sqnr_db(fp, logits_before[0]):.2f} dB before, "
          f"{_sqnr_db(fp, logits_after[0]):.2f} dB after GPTQ; total objective GPTQ / RTN {tot_after / tot_rtn:.3f}")

    # 6. the command line, from the calibrated checkpoint and the same seeded images, writes a checkpoint with the same logits
    if bits == 3:
        out = str(tmp_path / "gptq_cli.pth")
        r = subprocess.run([sys.executable, "-m", "adalog_amd.utils.gptq", "--model", "deit_tiny", "--depth", "2", "--config", _cfg_path(3),
                            "--checkpoint", plain_before, "--out", out, "--images", "8", "--seed", "5", "--batch-size", "3"],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "9 layers swept, 1 left" in r.stdout, r.stdout
        cli = P.load_plain(P.build_wrapped("deit_tiny", _cfg_path(3), DEV, depth=2), out, DEV)
        _assert_same_logits(_logits(cli, x), logits_after)
    assert not misses, f"returned objective against the fp64 recomputation, bar 1e-6 relative: {misses}"
