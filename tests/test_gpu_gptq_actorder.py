"""`-m gpu`: the act-order GPTQ sweep (csrc/gptq.hip: adalog_gptq_sweep_perm_f32) against the numpy restatement of its specification
run on explicitly permuted inputs (tests/gptq_perm_cpu_backend.py over tests/gptq_reference.py) -- weights, codes AND objective bit for
bit --, against the natural-order entry point under the identity order, adalog_permute_sym_f64 against torch indexing, the refusal of
an array that is no permutation, and gptq_model(act_order=True, sweep_conv=True) end to end on a calibrated depth-1 deit_tiny."""
import numpy as np
import pytest
import torch

from tests import gptq_reference as GR
from tests.gptq_perm_cpu_backend import sweep_perm
from tests.test_gpu_packed import _assert_same_logits, _cfg, _cfg_path, _logits

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from adalog_amd import backend, ops
    backend.set_backend(None)
    return ops


def _lib():
    from adalog_amd import _lib as L
    return L.load()


def _last_kernel():
    return _lib().adalog_last_kernel().decode()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _perm(kind, K):
    if kind == "identity":
        return np.arange(K, dtype=np.int32)
    if kind == "reversed":
        return np.arange(K - 1, -1, -1, dtype=np.int32)
    return np.random.default_rng(100 + K).permutation(K).astype(np.int32)


_HESS, _FACTORS, _REFS = {}, {}, {}


def _hessian(K):
    """a seeded correlated Hessian with unequal column energies (fp64, host)"""
    if K not in _HESS:
        rng = np.random.default_rng(K)
        T = min(2 * K, 256)
        X = (rng.standard_normal((T, K)) @ (0.3 * np.eye(K) + rng.standard_normal((K, K)) / np.sqrt(K)) + 0.5) * rng.uniform(0.5, 2.0, K)
        _HESS[K] = X.T @ X
    return _HESS[K]


def _factor(K, kind):
    """U (fp64, host) of the PERMUTED damped Hessian, by the product's own factor routine -- once per (K, order)"""
    if (K, kind) not in _FACTORS:
        from adalog_amd.utils.gptq import damped_factor
        p = _perm(kind, K).astype(np.int64)
        _FACTORS[K, kind] = damped_factor(torch.from_numpy(_hessian(K)[p][:, p]), 0.01)[0].numpy()
    return _FACTORS[K, kind]


def _case(R, K, bits, per_row, kind):
    """(W, s, z, U, perm) as numpy and the restatement's (What, codes, objective) in natural order -- computed once per case"""
    key = (R, K, bits, per_row, kind)
    if key not in _REFS:
        rng = np.random.default_rng(1000 * bits + R + K + per_row)
        W = rng.standard_normal((R, K)).astype(np.float32)
        s, z = GR.minmax_params(W, bits)
        if not per_row:
            s, z = s[:1].copy(), z[:1].copy()
        U, p = _factor(K, kind), _perm(kind, K)
        _REFS[key] = (W, s, z, U, p, sweep_perm(W, s, z, bits, U, p))
    return _REFS[key]


SENTINEL_F, SENTINEL_B, SENTINEL_D = -77.25, 0xA5, -3.0e300


def _run_raw(W, s, z, bits, U, p, pad_w=0, pad_u=0, perm_dev=None):
    """adalog_gptq_sweep_perm_f32 through the C ABI, with rows of w pad_w (of U pad_u) elements longer than K and every output
    prefilled with a sentinel -> (rc, What, codes, objective) as numpy"""
    R, K = W.shape
    w = torch.full((R, K + pad_w), 1.0e30, dtype=torch.float32)
    w[:, :K] = torch.from_numpy(W)
    u = torch.full((K, K + pad_u), 1.0e300, dtype=torch.float64)
    u[:, :K] = torch.from_numpy(U)
    w, u, sd, zd = w.to(DEV), u.to(DEV), torch.from_numpy(s).to(DEV), torch.from_numpy(z).to(DEV)
    pd = torch.from_numpy(p).to(DEV) if perm_dev is None else perm_dev
    what = torch.full((R, K), SENTINEL_F, dtype=torch.float32, device=DEV)
    codes = torch.full((R, K), SENTINEL_B, dtype=torch.uint8, device=DEV)
    obj = torch.full((R,), SENTINEL_D, dtype=torch.float64, device=DEV)
    rc = _lib().adalog_gptq_sweep_perm_f32(w.data_ptr(), R, K, K + pad_w, sd.data_ptr(), zd.data_ptr(), int(s.size == R and R > 1), bits,
                                          u.data_ptr(), K + pad_u, pd.data_ptr(), what.data_ptr(), codes.data_ptr(), obj.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, what.cpu().numpy(), codes.cpu().numpy(), obj.cpu().numpy()


def _assert_bits(got, want, what):
    assert got[1].dtype == np.uint8 and np.array_equal(got[1], want[1]), (what, "codes", int((got[1] != want[1]).sum()))
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), (what, "What")
    assert np.array_equal(got[2].view(np.int64), want[2].view(np.int64)), (what, "objective", np.abs(got[2] - want[2]).max())


# K = 32: half a slot; 64: one slot; 4096: 64 slots per lane.  R = 1; 3; 65: more than one workgroup.  K = 4096 with R = 3 only.
SHAPES = [(1, 32), (3, 32), (65, 32), (1, 64), (3, 64), (65, 64), (3, 4096)]
ORDERS = ["identity", "reversed", "random"]


@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("R,K", SHAPES)
def test_permuted_sweep_equals_the_restatement_bit_for_bit(R, K, kind):
    """every shape in every order, rows of w (and of U) longer than K: 4 bits, one quantiser per row"""
    W, s, z, U, p, want = _case(R, K, 4, 1, kind)
    rc, *got = _run_raw(W, s, z, 4, U, p, pad_w=5, pad_u=2)
    assert rc == 0 and _last_kernel() == "k_gptq_sweep_perm"
    _assert_bits(got, want, (R, K, kind))
    if kind != "identity" and K > 32:
        assert not np.array_equal(want[1], _case(R, K, 4, 1, "identity")[5][1])  # (the order does change the result)


@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("per_row", [0, 1])
@pytest.mark.parametrize("bits", [2, 4, 8])
def test_permuted_sweep_bits_and_parameter_layouts(bits, per_row, kind):
    W, s, z, U, p, want = _case(65, 64, bits, per_row, kind)
    rc, *got = _run_raw(W, s, z, bits, U, p, pad_w=0 if per_row else 3)
    assert rc == 0
    _assert_bits(got, want, (bits, per_row, kind))


@pytest.mark.parametrize("bits,per_row", [(2, 0), (8, 0)])
def test_permuted_sweep_of_4096_columns_at_other_widths(bits, per_row):
    W, s, z, U, p, want = _case(3, 4096, bits, per_row, "random")
    rc, *got = _run_raw(W, s, z, bits, U, p, pad_w=1)
    assert rc == 0
    _assert_bits(got, want, (bits, per_row))


@pytest.mark.parametrize("R,K", SHAPES)
def test_identity_order_equals_the_natural_order_entry_point(R, K):
    ops = _ops()
    W, s, z, U, p, _ = _case(R, K, 4, 1, "identity")
    args = (torch.from_numpy(W).to(DEV), torch.from_numpy(s).to(DEV), torch.from_numpy(z).to(DEV), 4, torch.from_numpy(U).to(DEV))
    nat = ops.gptq_sweep(*args, want_codes=True, want_objective=True)
    assert _last_kernel() == "k_gptq_sweep"
    got = ops.gptq_sweep(*args, want_codes=True, want_objective=True, perm=torch.from_numpy(p).to(DEV))
    assert _last_kernel() == "k_gptq_sweep_perm"
    for a, b in zip(got, nat):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_sweep_wrapper_takes_perm_and_rejects_what_it_cannot_take():
    ops = _ops()
    from adalog_amd._lib import AdalogHipError
    W, s, z, U, p, want = _case(65, 64, 4, 1, "random")
    w, sd, zd, u = (torch.from_numpy(a).to(DEV) for a in (W, s, z, U))
    pd = torch.from_numpy(p).to(DEV)
    what = ops.gptq_sweep(w, sd, zd, 4, u, perm=pd)
    assert isinstance(what, torch.Tensor) and np.array_equal(what.cpu().numpy().view(np.int32), want[0].view(np.int32))
    doubled = torch.stack([pd, pd], 1)[:, 0]                                     # a strided view: copied, as the other operands are
    assert not doubled.is_contiguous()
    assert torch.equal(ops.gptq_sweep(w, sd, zd, 4, u, perm=doubled), what)
    for bad in (pd.long(), pd[:32], pd.cpu(), p):
        with pytest.raises(ValueError, match="perm must be an int32"):
            ops.gptq_sweep(w, sd, zd, 4, u, perm=bad)
    twice = pd.clone()
    twice[3] = twice[9]
    with pytest.raises(AdalogHipError, match="not a permutation"):
        ops.gptq_sweep(w, sd, zd, 4, u, perm=twice)
    with pytest.raises(AdalogHipError, match="not a permutation"):
        ops.permute_sym(u, twice)
    with pytest.raises(ValueError):
        ops.permute_sym(u.float(), pd)
    with pytest.raises(ValueError):
        ops.permute_sym(u[:, :32], pd)


@pytest.mark.parametrize("K", [32, 4096])
def test_permute_sym_equals_torch_indexing(K):
    ops = _ops()
    g = torch.Generator().manual_seed(K)
    H = torch.randn(K, K + 3, generator=g, dtype=torch.float64)                  # rows of H three elements longer than K
    p = torch.from_numpy(_perm("random", K))
    want = H[:, :K][p.long()][:, p.long()]
    Hd, pd = H.to(DEV), p.to(DEV)
    out = torch.full((K, K + 1), SENTINEL_D, dtype=torch.float64, device=DEV)
    assert _lib().adalog_permute_sym_f64(Hd.data_ptr(), K, K + 3, pd.data_ptr(), out.data_ptr(), K + 1, _stream()) == 0
    assert _last_kernel() == "k_permute_sym"
    got = out.cpu()
    assert torch.equal(got[:, :K], want) and bool((got[:, K] == SENTINEL_D).all())
    if K == 32:                                                                 # the wrapper: a new contiguous tensor, the input untouched
        Hc = Hd[:, :K].contiguous()
        assert torch.equal(ops.permute_sym(Hc, pd).cpu(), want) and torch.equal(Hc.cpu(), H[:, :K])
        assert torch.equal(ops.permute_sym(Hd[:, :K], pd).cpu(), want)          # a strided view is copied
        ident = torch.arange(K, dtype=torch.int32, device=DEV)
        assert torch.equal(ops.permute_sym(Hc, ident), Hc)


@pytest.mark.parametrize("how", ["duplicate", "too large", "negative"])
def test_an_array_that_is_no_permutation_is_refused_before_any_kernel_indexes_with_it(how):
    """return -1, a message, every output as it was, and no kernel but the check"""
    lib = _lib()
    W, s, z, U, p, _ = _case(3, 64, 4, 1, "random")
    bad = p.copy()
    bad[17] = {"duplicate": bad[40], "too large": 64, "negative": -1}[how]
    rc, what, codes, obj = _run_raw(W, s, z, 4, U, bad)
    assert rc == -1 and "not a permutation" in lib.adalog_last_error().decode() and "gptq_sweep_perm" in lib.adalog_last_error().decode()
    assert _last_kernel() == "k_perm_check"
    assert (what == np.float32(SENTINEL_F)).all() and (codes == SENTINEL_B).all() and (obj == SENTINEL_D).all()
    H = torch.randn(64, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = torch.full((64, 64), SENTINEL_D, dtype=torch.float64, device=DEV)
    bd = torch.from_numpy(bad).to(DEV)
    assert lib.adalog_permute_sym_f64(H.data_ptr(), 64, 64, bd.data_ptr(), out.data_ptr(), 64, _stream()) == -1
    assert "not a permutation" in lib.adalog_last_error().decode() and "permute_sym" in lib.adalog_last_error().decode()
    assert _last_kernel() == "k_perm_check"
    torch.cuda.synchronize()
    assert bool((out == SENTINEL_D).all())
    rc, *got = _run_raw(W, s, z, 4, U, p)                                        # the next valid call is served
    assert rc == 0
    _assert_bits(got, _case(3, 64, 4, 1, "random")[5], "after a refusal")


# ------------------------------------------------------------------------------------------------ end to end
def _calibrated(bits, depth=1):
    """a depth-1 deit_tiny with seeded random weights, calibrated on 8 synthetic images (as tests/test_gpu_gptq.py builds its model)"""
    _ops()
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.models import create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    torch.manual_seed(5)
    model = wrap_modules_in_net(create_model("deit_tiny", depth=depth).eval().to(DEV), _cfg(bits), reparam=True).to(DEV)
    x = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(5)).to(DEV)
    QuantCalibrator(model, [(x, None)]).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model).to(DEV).eval()
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    return model, x


def _fresh_hessians(model, names, x):
    """fp64 torch Hessians of the layers' GEMM rows in the FP model, from hooks of this test's own, in ONE batch as gptq_model is called"""
    from adalog_amd.utils.gptq import _gemm_rows
    mods = dict(model.named_modules())
    moded = [m for m in model.modules() if hasattr(m, "mode")]
    saved = [m.mode for m in moded]
    H, handles = {}, []
    for n in names:
        def hook(m, args, out, n=n):
            r = _gemm_rows(m, args[0]).double()
            H[n] = r.t() @ r
        handles.append(mods[n].register_forward_hook(hook))
    try:
        for m in moded:
            m.mode = "raw"
        with torch.no_grad():
            model(x)
    finally:
        for h in handles:
            h.remove()
        for m, mode in zip(moded, saved):
            m.mode = mode
    return H


def test_gptq_model_act_order_with_the_convolution_end_to_end(tmp_path):
    """Per swept layer, the quadratic error tr((W - What) Hd (W - What)^T) in fp64 (Hd: the damped Hessian of a fresh capture, natural
    column order) is no larger than round-to-nearest's with the same scale and zero point; the figures are printed before the
    assertion.  Then the packed export round-trips to the same quant_forward logits."""
    ops = _ops()
    from adalog_amd.utils import packed as P
    from adalog_amd.utils.gptq import _quadratic, _rows_cols, damped_factor, gptq_model
    model, x = _calibrated(4)
    layers = [(n, m) for n, m in model.named_modules() if hasattr(m, "w_quantizer")]
    names = [n for n, _ in layers]
    assert names[0] == "patch_embed.proj" and len(names) == 6
    w0 = {n: m.weight.data.clone() for n, m in layers}
    params = {n: (m.w_quantizer.scale.data.clone(), m.w_quantizer.zero_point.data.clone()) for n, m in layers}
    H = _fresh_hessians(model, names, x)                                         # of the FP model: before any weight is committed
    logits_before = _logits(model, x)

    res = gptq_model(model, x, damp=0.01, batch_size=8, act_order=True, sweep_conv=True)
    assert list(res["layers"]) == names and res["skipped"] == {}                 # the convolution is swept
    assert all(e["act_order"] is True for e in res["layers"].values())
    conv = res["layers"]["patch_embed.proj"]
    assert (conv["R"], conv["K"], conv["n_bits"]) == (192, 768, 4)
    assert all(m.mode == "quant_forward" for m in model.modules() if hasattr(m, "mode"))
    worse = []
    for n, m in layers:
        R, K = _rows_cols(m)
        wq = m.w_quantizer
        assert torch.equal(wq.scale.data, params[n][0]) and torch.equal(wq.zero_point.data, params[n][1]), n
        Hd = damped_factor(H[n], 0.01)[1].to(DEV)
        w2 = w0[n].reshape(R, K)
        w_rtn = ops.uniform_fake_quant(w2, wq.scale.data.view(R, 1), wq.zero_point.data.view(R, 1), 4)
        after, rtn = _quadratic(w2 - m.weight.data.reshape(R, K), Hd), _quadratic(w2 - w_rtn, Hd)
        e = res["layers"][n]
        print(f"W4 act-order {n} [{R}, {K}]: quadratic error rtn {rtn:.6g} gptq {after:.6g} ratio {after / rtn:.4f} "
              f"(returned {e['objective_before']:.6g} -> {e['objective_after']:.6g})")
        if not after <= rtn:
            worse.append((n, after, rtn))
        with torch.no_grad():                                                   # the committed weight lies on the quantiser's grid
            assert torch.equal(m.quant_weight_bias()[0].view(torch.int32), m.weight.data.view(torch.int32)), n
        assert not torch.equal(m.weight.data, w0[n])
    assert not worse, f"layers whose quadratic error exceeds round-to-nearest's: {worse}"

    logits_after = _logits(model, x)
    assert not torch.equal(logits_after[0], logits_before[0])
    packed = str(tmp_path / "gptq_actorder_packed.pth")
    obj = P.save_packed(model, packed)
    assert obj["meta"]["kept_fp32"] == {}
    loaded = P.load_packed(P.build_wrapped("deit_tiny", _cfg_path(4), DEV, depth=1), packed, DEV)
    _assert_same_logits(_logits(loaded, x), logits_after)
