"""`-m gpu`: the signed error-moments kernel (csrc/report.hip, ops.mean_err) against exactly rounded sums (tests/biascorr_reference.py:
math.fsum) within the rounding bounds of an fp64 summation, and utils/bias_correct.py end to end on a calibrated depth-2 deit_tiny."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import biascorr_reference as BR
from tests.test_gpu_gptq import _calibrated, _fp_logits, _sqnr_db
from tests.test_gpu_packed import _assert_same_logits, _cfg_path, _logits

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


def _pair(n, seed, offset=(0, 0)):
    """(a, b) fp32 device tensors of n elements whose base pointers sit ``offset`` elements behind a 16-byte boundary; b = a + noise,
    with a few large and a few equal elements"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, generator=g) * 3.0 + 0.25
    b = a + torch.randn(n, generator=g) * 0.1 + 0.01
    if n > 8:
        a[n // 3], b[n // 2] = 4.0e3, -2.5e3
        b[n // 5] = a[n // 5]
    out = []
    for t, off in ((a, offset[0]), (b, offset[1])):
        buf = torch.empty(n + 8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + n]
        v.copy_(t)
        out.append(v)
    return out


def _check(ops, a, b, n_ch, inner, what):
    """ops.mean_err(a, b) inside the derived bounds: |sum d - exact| <= n_c u sum |d|, |sum d^2 - exact| <= (n_c + 1) u sum d^2,
    max |a| exact (u = 2^-53); and two calls give the same bits"""
    got = ops.mean_err(a, b, n_ch, inner)
    assert _last_kernel() == "k_mean_err"
    again = ops.mean_err(a, b, n_ch, inner)
    assert got.dtype == torch.float64 and tuple(got.shape) == (n_ch, 3)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64)), what
    got = got.cpu().numpy()
    ex = BR.exact_moments(a.cpu().numpy(), b.cpu().numpy(), n_ch, inner)
    bd, bd2 = BR.sum_bounds(ex)
    e1, e2 = np.abs(got[:, 0] - ex["sum_d"]), np.abs(got[:, 1] - ex["sum_d2"])
    print(f"{what}: n_c {ex['n_c']}  |sum d - exact| / bound {np.max(e1 / np.maximum(bd, 1e-300)):.3g}  "
          f"|sum d^2 - exact| / bound {np.max(e2 / np.maximum(bd2, 1e-300)):.3g}")
    assert (e1 <= bd).all(), (what, "sum d", e1.max(), bd.min())
    assert (e2 <= bd2).all(), (what, "sum d^2", e2.max(), bd2.min())
    assert np.array_equal(got[:, 2], ex["max_a"]), (what, "max |a|")
    return got


@pytest.mark.parametrize("C", [1, 3, 65, 384])
def test_mean_err_linear_layout(C):
    """inner = 1, [rows, C]: a thread per channel (C = 1: one contiguous run, float4 loads with a scalar tail)"""
    ops = _ops()
    for rows in (1, 63, 394):
        a, b = _pair(rows * C, 1000 * C + rows)
        _check(ops, a, b, C, 1, (rows, C))


@pytest.mark.parametrize("shape", [(2, 5, 49), (2, 6, 196), (4, 2, 8192)])
def test_mean_err_conv_layout(shape):
    """inner > 1, [B, C, H W]: rows of 49 (unaligned, scalar), of 196 (float4), and 4 rows of 8192 per channel (8 blocks per channel)"""
    ops = _ops()
    B, C, inner = shape
    a, b = _pair(B * C * inner, inner)
    _check(ops, a, b, C, inner, shape)
    if inner == 196:                                                            # rows that hold whole float4s behind a misaligned base: scalar
        a, b = _pair(B * C * inner, inner + 1, offset=(1, 1))
        _check(ops, a, b, C, inner, shape + ("offset",))


@pytest.mark.parametrize("n,offset", [(1003, (0, 0)), (1003, (1, 1)), (1002, (1, 2)), (5, (3, 3)), (2, (1, 1)), (3 * 4096 + 5, (1, 1))])
def test_mean_err_heads_and_tails(n, offset):
    """one channel, n no multiple of 4, base pointers one element (and differently) off: the scalar head and tail, the all-scalar form
    of two differently aligned inputs, runs shorter than a float4, and four blocks' partials in the finish kernel"""
    ops = _ops()
    a, b = _pair(n, n + offset[1], offset)
    assert a.data_ptr() % 16 == 4 * offset[0] and b.data_ptr() % 16 == 4 * offset[1]
    _check(ops, a, b, 1, None, (n, offset))
    _check(ops, a, b, 1, 1, (n, offset, "inner 1"))


def test_mean_err_many_parts():
    """[16500, 3]: 258 partials per channel -- more than the finish kernel's 256 threads, so a thread adds two; and [2^20 + 3] in one
    channel: 257 blocks"""
    ops = _ops()
    a, b = _pair(16500 * 3, 9)
    _check(ops, a, b, 3, 1, "cols, 258 parts")
    a, b = _pair((1 << 20) + 4096 + 3, 10)
    _check(ops, a, b, 1, None, "stream, 258 parts")


def test_mean_err_cancellation():
    """d alternates +-1e4 around a mean of 1e-3 over 2^16 elements per channel: sum |d| is 1e7 |sum d|.  The same bound holds; an fp32
    accumulation or an fp32 a - b misses it (shown on the host, together with the fp64 reference's own margin)."""
    ops = _ops()
    a, b = BR.cancellation_case(1 << 16, 2)
    ex = BR.exact_moments(a, b, 2, 1)
    bd, _ = BR.sum_bounds(ex)
    A, B = BR.channel_rows(a, 2, 1), BR.channel_rows(b, 2, 1)
    D = A.astype(np.float64) - B.astype(np.float64)
    for c in range(2):
        assert abs(float(np.cumsum(D[c])[-1]) - ex["sum_d"][c]) <= 1e-3 * bd[c]                     # a sequential fp64 sum: wide margin
        assert abs(float(np.cumsum((A[c] - B[c]).astype(np.float64))[-1]) - ex["sum_d"][c]) > bd[c]   # fp32 a - b
        assert abs(float(np.cumsum(D[c].astype(np.float32), dtype=np.float32)[-1]) - ex["sum_d"][c]) > bd[c]
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = _check(ops, ta, tb, 2, 1, "cancellation, cols")
    assert np.all(np.abs(got[:, 0] / (1 << 16) - 1e-3) < 1e-4)
    _check(ops, ta[:, 0].contiguous(), tb[:, 0].contiguous(), 1, None, "cancellation, one run")
    _check(ops, ta.t().contiguous(), tb.t().contiguous(), 2, 1 << 16, "cancellation, rows")


def test_mean_err_wrapper_rejects_bad_arguments():
    ops = _ops()
    from adalog_amd._lib import AdalogHipError
    a = torch.zeros(10, device=DEV)
    with pytest.raises(ValueError):
        ops.mean_err(a, a, 3)
    with pytest.raises(ValueError):
        ops.mean_err(a, torch.zeros(9, device=DEV))
    with pytest.raises(AdalogHipError):
        ops.mean_err(a.cpu(), a)
    z = ops.mean_err(a[:0], a[:0], 2, 1)
    assert tuple(z.shape) == (2, 3) and float(z.abs().sum()) == 0.0
    same = ops.mean_err(a + 2.0, a + 2.0, 5, 1)
    assert same[:, :2].abs().sum().item() == 0.0 and bool((same[:, 2] == 2.0).all())


# ------------------------------------------------------------------------------------------------ end to end
BATCH = 8


@pytest.fixture(scope="module")
def corrected(tmp_path_factory):
    """deit_tiny, depth 2, W4A4, calibrated on 8 seeded images (the model of tests/test_gpu_gptq.py); a HIP graph of its forward captured
    BEFORE the correction; then bias_correct_model"""
    _ops()
    from adalog_amd.utils.bias_correct import bias_correct_model, measure_bias_error
    from adalog_amd.utils.graph_forward import GraphedForward
    model, x = _calibrated(4)
    tmp = tmp_path_factory.mktemp("biascorr")
    plain = str(tmp / "calibrated.pth")
    torch.save(model.state_dict(), plain)
    fp = _fp_logits(model, x)
    logits_before = _logits(model, x)
    graph = GraphedForward(model)
    assert torch.equal(graph(x), logits_before[0])
    state = {k: v.clone() for k, v in model.state_dict().items()}
    before = measure_bias_error(model, x, batch_size=BATCH)
    res = bias_correct_model(model, x, batch_size=BATCH)
    return dict(model=model, x=x, tmp=tmp, plain=plain, fp=fp, logits_before=logits_before, graph=graph, state=state, before=before, res=res)


def _bounds(model, after):
    """per layer, per channel: 4 * 2^-24 * (max |y_fp| + max |y_q| + |b_c|) -- one fp32 rounding of the bias and one per output element"""
    mods = dict(model.named_modules())
    return {n: 4 * 2.0 ** -24 * (a["max_abs_fp"] + a["max_abs_q"] + mods[n].bias.data.double().abs().cpu()) for n, a in after["layers"].items()}


def test_bias_correct_end_to_end(corrected):
    from adalog_amd.utils.bias_correct import bias_correct_model, measure_bias_error
    c = corrected
    model, x, res = c["model"], c["x"], c["res"]
    mods = dict(model.named_modules())
    layers = list(res["layers"])
    assert len(layers) == 10 and layers[0] == "patch_embed.proj" and layers[-1] == "head"
    assert sorted(res["skipped"]) == [f"blocks.{i}.attn.matmul{j}" for i in (0, 1) for j in (1, 2)]
    assert all(m.mode == "quant_forward" for m in model.modules() if hasattr(m, "mode"))
    now = model.state_dict()
    changed = sorted(k for k, v in c["state"].items() if not torch.equal(now[k], v))
    assert changed == sorted(n + ".bias" for n in layers)                      # weights, scales and zero points: bit-unchanged
    # the first layer has no corrected layer in front of it: its entry is what a read-only measurement saw before
    e0, b0 = res["layers"][layers[0]], c["before"]["layers"][layers[0]]
    # (the same 192 numbers, summed over channels by two host routines: 192 u)
    assert e0["sq_err_before"] == pytest.approx(float(b0["sq_err"].sum()), rel=1e-13)
    assert e0["mean_abs_before"] == pytest.approx(float(b0["mean"].abs().mean()), rel=1e-13)

    after = measure_bias_error(model, x, batch_size=BATCH, quant_max=True)
    bounds = _bounds(model, after)
    misses = []
    for n in layers:
        a, e, bd = after["layers"][n], res["layers"][n], bounds[n]
        T = a["T"]
        worst = float((a["mean"].abs() / bd).max())
        rest = float(a["sq_err"].sum())
        # d' = d - delta + eps with |eps| <= bound per element: sum d'^2 - sum (d - delta)^2 = sum 2 (d - delta) eps + eps^2
        slack = float((2 * bd * (T * a["sq_err"]).sqrt() + T * bd * bd).sum()) + 1e-12 * e["sq_err_before"]
        print(f"{n}: C {a['C']} T {T}  mean |m| before {e['mean_abs_before']:.4g}  max |m| after / bound {worst:.3g}  "
              f"sum d^2 {e['sq_err_before']:.6g} -> predicted {e['sq_err_after_predicted']:.6g}, measured {rest:.6g} (slack {slack:.3g})")
        if worst > 1.0:
            misses.append((n, "mean after", worst))
        if abs(rest - e["sq_err_after_predicted"]) > slack:
            misses.append((n, "sum d^2", rest, e["sq_err_after_predicted"], slack))
        if rest > e["sq_err_before"]:
            misses.append((n, "sum d^2 grew", rest, e["sq_err_before"]))
    logits_after = _logits(model, x)
    print(f"W4A4 depth-2 deit_tiny, random weights: logit SQNR against the FP model {_sqnr_db(c['fp'], c['logits_before'][0]):.2f} dB before, "
          f"{_sqnr_db(c['fp'], logits_after[0]):.2f} dB after bias correction (recorded, not asserted)")
    assert not misses, misses

    # a second call finds nothing to correct: every bias moves by no more than the bound
    biases = {n: mods[n].bias.data.clone() for n in layers}
    bias_correct_model(model, x, batch_size=BATCH)
    moved = {n: float(((mods[n].bias.data - biases[n]).double().abs().cpu() / bounds[n]).max()) for n in layers}
    print("second call, largest |bias change| / bound per layer:", {n: round(v, 3) for n, v in moved.items()})
    for n in layers:                                                            # (put back: the tests below use the first correction)
        mods[n].bias.data.copy_(biases[n])
    assert all(v <= 1.0 for v in moved.values()), moved


def test_routes_and_captured_graph_agree_after_correction(corrected):
    c = corrected
    model, x = c["model"], c["x"]
    fused, module_route = _logits(model, x)
    assert torch.isfinite(fused).all() and torch.equal(fused, module_route)
    assert not torch.equal(fused, c["logits_before"][0])
    assert torch.equal(c["graph"](x), fused)                                    # captured before the correction, replayed after it


def test_corrected_model_round_trips_through_checkpoints(corrected):
    from adalog_amd.utils import packed as P
    c = corrected
    model, x, tmp = c["model"], c["x"], c["tmp"]
    want = _logits(model, x)
    packed, plain = str(tmp / "bc_packed.pth"), str(tmp / "bc_plain.pth")
    P.save_packed(model, packed)
    loaded = P.load_packed(P.build_wrapped("deit_tiny", _cfg_path(4), DEV, depth=2), packed, DEV)
    _assert_same_logits(_logits(loaded, x), want)
    torch.save(model.state_dict(), plain)
    fresh = P.load_plain(P.build_wrapped("deit_tiny", _cfg_path(4), DEV, depth=2), plain, DEV)
    _assert_same_logits(_logits(fresh, x), want)


def test_command_line_in_a_child_process(corrected):
    c = corrected
    out = str(c["tmp"] / "bc_cli.pth")
    r = subprocess.run([sys.executable, "-m", "adalog_amd.utils.bias_correct", "--model", "deit_tiny", "--depth", "2", "--config", _cfg_path(4),
                        "--checkpoint", c["plain"], "--out", out, "--images", "8", "--seed", "5", "--batch-size", str(BATCH)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "10 layers corrected, 4 left as they were" in r.stdout, r.stdout
    sd = torch.load(out, map_location=DEV)
    now = c["model"].state_dict()
    assert set(sd) == set(now)
    for k, v in now.items():
        assert torch.equal(sd[k], v), k
