"""`-m gpu`: the measurement kernels of the quantisation report (csrc/report.hip: ops.err_stats, ops.uniform_code_hist,
ops.log_code_hist) against the plain-torch reference (tests/report_reference.py) and the existing fake-quant kernels, and
quant_report end to end on the tiny ViT and Swin of tests/test_report_cpu.py, calibrated on the device."""
import pytest
import torch

from tests import report_reference as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from adalog_amd import backend, ops
    backend.set_backend(None)
    return ops


def _last_kernel():
    from adalog_amd import _lib
    return _lib.load().adalog_last_kernel().decode()


def _rel(a, b):
    return ((a - b).abs() / torch.maximum(a.abs(), b.abs()).clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------------------------------------ err_stats
def _pair(n, seed):
    """a, b with exact zeros, -0.0, a stretch where they are equal, and magnitudes near 1e18 and 1e-18 (fp32 squares would overflow
    / vanish; fp64 ones do not)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, generator=g)
    b = a + 0.05 * torch.randn(n, generator=g)
    for i, (va, vb) in enumerate(((0.0, 0.0), (-0.0, 0.0), (1.5e18, -1.25e18), (3e-18, 1e-18), (0.0, -0.0), (2.0, 2.0), (-7e18, -7e18))):
        if i * 3 < n:
            a[i * 3], b[i * 3] = va, vb
    if n > 40:
        b[20:40] = a[20:40]
    return a, b


# (n, n_channels, inner)
ERR_LAYOUTS = [(n, 1, None) for n in (1, 63, 64, 65, 4097, 2 ** 20 + 3)] + \
              [(3 * k, 3, 1) for k in (1, 21, 1366)] + [(15, 3, 5), (105, 3, 5), (192, 3, 64), (576, 3, 64)] + \
              [(3 * 197 * 64, 3, 197 * 64), (2 * 3 * 197 * 64, 3, 197 * 64), (384 * 50, 384, 1)]


@pytest.mark.parametrize("n,n_ch,inner", ERR_LAYOUTS)
def test_err_stats_matches_fp64(n, n_ch, inner):
    ops = _ops()
    a, b = _pair(n, n)
    a, b = a.to(DEV), b.to(DEV)
    got = ops.err_stats(a, b, n_ch, inner)
    assert _last_kernel() == "k_err_stats"
    want = RR.err_stats(a, b, n_ch, inner)
    assert got.dtype == torch.float64 and tuple(got.shape) == (n_ch, 4)
    assert torch.isfinite(got).all()
    assert _rel(got[:, :3], want[:, :3]) <= 1e-12, (got, want)
    assert torch.equal(got[:, 3], want[:, 3])
    again = ops.err_stats(a, b, n_ch, inner)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))            # bit for bit


@pytest.mark.parametrize("n", [1, 65, 4097, 2 ** 20 + 3])
def test_err_stats_unaligned_and_equal_inputs(n):
    ops = _ops()
    a0, b0 = _pair(n + 1, 7 * n)
    a0, b0 = a0.to(DEV), b0.to(DEV)
    a, b = a0[1:], b0[1:]                                                       # both start 4 bytes past an aligned address
    assert a.data_ptr() % 16 == 4 and a.is_contiguous()
    want = RR.err_stats(a, b)
    got = ops.err_stats(a, b)
    assert _rel(got[:, :3], want[:, :3]) <= 1e-12 and torch.equal(got[:, 3], want[:, 3])
    b2 = b.clone()                                                               # a unaligned, b aligned: no common 16-byte phase
    assert b2.data_ptr() % 16 == 0
    got2 = ops.err_stats(a, b2)
    assert _rel(got2[:, :3], want[:, :3]) <= 1e-12 and torch.equal(got2[:, 3], want[:, 3])
    if n >= 6:
        got3 = ops.err_stats(a[: n - n % 3], b[: n - n % 3], 3, 1 if n < 100 else None)
        want3 = RR.err_stats(a[: n - n % 3], b[: n - n % 3], 3, 1 if n < 100 else None)
        assert _rel(got3[:, :3], want3[:, :3]) <= 1e-12 and torch.equal(got3[:, 3], want3[:, 3])
    same = ops.err_stats(a, a.clone())                                           # equal tensors: no noise at all
    assert same[0, 0].item() == 0.0 and same[0, 3].item() == 0.0 and same[0, 1].item() == same[0, 2].item()
    assert _rel(same[:, 1:2], want[:, 1:2]) <= 1e-12


def test_err_stats_rejects_bad_layouts():
    ops = _ops()
    a = torch.zeros(10, device=DEV)
    with pytest.raises(ValueError):
        ops.err_stats(a, a, 3)
    with pytest.raises(ValueError):
        ops.err_stats(a, torch.zeros(9, device=DEV))
    z = ops.err_stats(a[:0], a[:0], 2, 1)
    assert tuple(z.shape) == (2, 4) and not z.any()


# ------------------------------------------------------------------------------------------------ uniform_code_hist
UNI_LAYOUTS = [((1,), (1,)), ((63,), (1,)), ((4097,), (1,)), ((2 ** 18 + 3,), (1,)), ((3, 64), (3, 1)), ((3, 65), (3, 1)),
               ((3, 384), (3, 1)), ((2, 3, 5, 16), (1, 3, 1, 1))]


def _uniform_case(shape, p_shape, bits, seed, pow2):
    """x, scale, zero point with planted values: rounding ties x / s = k + 0.5 (even and odd k, exact for power-of-two scales), one
    step and far beyond either clamp, exact zeros; zero points with fraction .5 (rne(z) is part of the code)"""
    from adalog_amd.ops import broadcast_layout
    g = torch.Generator().manual_seed(seed)
    n_ch = max(p_shape)
    qmax = 2 ** bits - 1
    zpool = [0.5, 1.5, 2.5, qmax / 2.0, float(qmax), 0.0]
    z = torch.tensor([zpool[(seed + c) % len(zpool)] for c in range(n_ch)])
    s = torch.tensor([2.0 ** -(1 + (seed + c) % 4) for c in range(n_ch)]) if pow2 else 0.01 + 0.05 * torch.rand(n_ch, generator=g)
    _, inner = broadcast_layout(shape, p_shape)
    n = 1
    for d in shape:
        n *= d
    rows = n // (n_ch * inner)
    sv, zv = s.view(1, n_ch, 1), torch.round(z).view(1, n_ch, 1)
    t = torch.rand(rows, n_ch, inner, generator=g) * (1.6 * qmax) - 0.3 * qmax          # the code before the clamp, both clamps hit
    x = (t - zv) * sv
    plant = [0.5, 1.5, 2.5, qmax - 0.5, qmax - 1.5, -1.0, qmax + 1.0, -1e6, 1e6, -0.5, qmax + 0.5]   # codes (before rounding)
    for c in range(n_ch):
        for j, code in enumerate(plant):
            if j < inner:
                x[0, c, j] = (code - zv[0, c, 0]) * sv[0, c, 0]
        if inner > len(plant) + 1:
            x[0, c, len(plant)], x[0, c, len(plant) + 1] = 0.0, -0.0
    return x.reshape(shape).to(DEV), s.reshape(p_shape).to(DEV), z.reshape(p_shape).to(DEV), n_ch, inner


@pytest.mark.parametrize("pow2", [True, False])
@pytest.mark.parametrize("bits", [2, 3, 4, 6, 8])
def test_uniform_code_hist_equals_reference_and_the_fake_quant_bins(bits, pow2):
    ops = _ops()
    hit_below = hit_above = 0
    for i, (shape, p_shape) in enumerate(UNI_LAYOUTS):
        x, s, z, n_ch, inner = _uniform_case(shape, p_shape, bits, 10 * bits + i, pow2)
        got = ops.uniform_code_hist(x, s, z, bits, n_ch, inner)
        assert _last_kernel() == "k_code_hist_uniform"
        levels = 2 ** bits
        assert got.dtype == torch.int64 and tuple(got.shape) == (n_ch, levels + 2)
        want = RR.uniform_code_hist(x, s, z, bits, n_ch, inner)
        assert torch.equal(got, want), (shape, got, want)
        assert int(got.sum()) == x.numel() and bool((got.sum(1) == x.numel() // n_ch).all())
        # in-range elements: the codes the fake-quant kernel writes
        bins = ops.uniform_fake_quant(x, s, z, bits, want_bins=True, want_y=False)[1]
        c = RR.uniform_codes(x, s, z, n_ch, inner)
        inside = (c >= 0) & (c <= levels - 1)
        idx = bins.reshape(c.shape).long() + torch.arange(n_ch, device=DEV).view(1, n_ch, 1) * levels
        assert torch.equal(torch.bincount(idx[inside], minlength=n_ch * levels).view(n_ch, levels), got[:, :levels]), shape
        hit_below, hit_above = hit_below + int(got[:, levels].sum()), hit_above + int(got[:, levels + 1].sum())
        again = ops.uniform_code_hist(x, s, z, bits, n_ch, inner)
        assert torch.equal(got, again)
    assert hit_below > 0 and hit_above > 0


def test_uniform_code_hist_unaligned_view():
    ops = _ops()
    x, s, z, _, _ = _uniform_case((4098,), (1,), 4, 3, True)
    v = x[1:]
    assert v.data_ptr() % 16 == 4
    assert torch.equal(ops.uniform_code_hist(v, s, z, 4), RR.uniform_code_hist(v, s, z, 4))


def test_uniform_code_hist_rejects_short_rows():
    from adalog_amd._lib import AdalogHipError
    ops = _ops()
    x = torch.randn(8, 3, 63, device=DEV)
    s, z = torch.full((3,), 0.1, device=DEV), torch.full((3,), 3.0, device=DEV)
    with pytest.raises(AdalogHipError, match="inner >= 64"):
        ops.uniform_code_hist(x, s, z, 4, 3, 63)
    with pytest.raises(AdalogHipError, match="inner >= 64"):
        ops.uniform_code_hist(x, torch.full((63,), 0.1, device=DEV), torch.full((63,), 3.0, device=DEV), 4, 63, 1)
    with pytest.raises(ValueError):
        ops.uniform_code_hist(x, s, z, 9, 3, 63)
    assert int(ops.uniform_code_hist(x, s[:1], z[:1], 4).sum()) == x.numel()


# ------------------------------------------------------------------------------------------------ log_code_hist
def _log_quantiser(bits, qv, with_shift):
    from adalog_amd.quantizers.logarithm import AdaLogQuantizer, ShiftAdaLogQuantizer
    q = (ShiftAdaLogQuantizer if with_shift else AdaLogQuantizer)(n_bits=bits)
    q.scale = torch.nn.Parameter(torch.tensor([0.83]))
    if with_shift:
        q.shift.data.fill_(0.16997124254703522)
    q.q.fill_(qv)
    q.update_table(qv)
    q.inited = True
    return q.to(DEV)


@pytest.mark.parametrize("with_shift", [False, True])
@pytest.mark.parametrize("qv", [10, 37, 137])
@pytest.mark.parametrize("bits", [3, 4, 6])
def test_log_code_hist_equals_the_bins_of_the_fake_quantiser(bits, qv, with_shift):
    ops = _ops()
    q = _log_quantiser(bits, qv, with_shift)
    g = torch.Generator().manual_seed(bits * 1000 + qv)
    masked = 0
    for n in (1, 65, 4097, 2 ** 17 + 3):
        # softmax-like magnitudes over many octaves, some u > 1, some non-positive x + shift, exact zeros
        x = torch.exp2(-24.0 * torch.rand(n + 1, generator=g)) * 1.3
        x[::7] = -x[::7] * 0.4
        x[::11] = 0.0
        x = x.to(DEV)
        for v in (x[:n], x[1:]):                                                 # aligned, and 4 bytes past an aligned address
            shift, _ = q._shift_args()
            got = ops.log_code_hist(v, q.scale.data, q.q, bits, shift=None if shift is None else shift.data)
            assert _last_kernel() == "k_code_hist_log"
            want = RR.log_code_hist_from_bins(q.bins(v), bits)
            assert got.dtype == torch.int64 and tuple(got.shape) == (2 ** bits + 1,)
            assert torch.equal(got, want), (n, got, want)
            assert int(got.sum()) == n
            masked += int(got[-1])
    # the masked code needs a bin index of 2^bits or more; the lower clamp u >= 1e-15 (what the exact zeros hit) ends at rne(49.83 * 37 / q)
    assert (masked > 0) == (round(49.82892142331043 * 37 / qv) >= 2 ** bits)


def test_log_code_hist_pre_gelu():
    """the GELU of the _pre entry points comes with the shared bin function: counted like the bins of log_fake_quant(pre_gelu=True)"""
    ops = _ops()
    q = _log_quantiser(4, 41, True)
    x = torch.randn(4097, generator=torch.Generator().manual_seed(3)).to(DEV) * 2
    shift, sub = q._shift_args()
    bins = ops.log_fake_quant(x, q.scale.data, q.q, q.table1, q.table2, 4, shift=shift.data, sub_shift=sub, want_bins=True,
                              want_y=False, pre_gelu=True)[1]
    got = ops.log_code_hist(x, q.scale.data, q.q, 4, shift=shift.data, pre_gelu=True)
    assert torch.equal(got, RR.log_code_hist_from_bins(bins, 4))


# ------------------------------------------------------------------------------------------------ the whole report
_MODELS = {}


def _calibrated(kind):
    if kind not in _MODELS:
        _ops()
        from tests.test_report_cpu import MAKERS, calibrate
        make, size = MAKERS[kind]
        torch.manual_seed(5)
        x = torch.randn(4, 3, size, size, generator=torch.Generator().manual_seed(1)).to(DEV)
        _MODELS[kind] = (calibrate(make(), x, DEV), x)
    return _MODELS[kind]


@pytest.mark.parametrize("kind", ["vit", "swin"])
def test_quant_report_end_to_end(kind):
    from adalog_amd.utils.report import quant_report
    model, x = _calibrated(kind)
    keep = {}
    rep = quant_report(model, x, tensors=keep)
    mods = [(n, m) for n, m in model.named_modules() if hasattr(m, "mode")]
    assert list(rep["modules"]) == [n for n, _ in mods]
    assert all(m.mode == "quant_forward" for _, m in mods)
    with torch.no_grad():
        y = model(x)                                                             # the switches at their defaults
    assert torch.equal(keep["logits_quant"], y)
    want = RR.recompute(model, x)
    close = lambda v, w: v == w or abs(v - w) <= 1e-9 * max(abs(v), abs(w))
    counted = 0
    for name, m in mods:
        e, w = rep["modules"][name], want["modules"][name]
        for which in ("cumulative", "local"):
            noise, signal, quant, mx = w[which].tolist()
            assert close(e[which]["noise"], noise) and close(e[which]["signal"], signal) and close(e[which]["quant_energy"], quant)
            assert e[which]["max_err"] == mx, (name, which)
        for attr, qe in e["quantizers"].items():
            ref = w["quantizers"][attr]
            if ref is None:
                assert qe is None and e["skipped"][attr]
                continue
            counted += 1
            hist, row = ref
            assert qe is not None, (name, attr, e["skipped"])
            assert qe["hist"] == hist.tolist(), (name, attr)
            assert close(qe["noise"], float(row[0])) and close(qe["signal"], float(row[1])) and qe["max_err"] == float(row[3])
    assert counted >= 12
    lb = want["logits"]["batch"].tolist()
    assert close(rep["logits"]["batch"]["noise"], lb[0]) and close(rep["logits"]["batch"]["signal"], lb[1])
    for got, row in zip(rep["logits"]["per_image"], want["logits"]["per_image"].tolist()):
        assert close(got["noise"], row[0]) and close(got["signal"], row[1]) and got["max_err"] == row[3]
