"""`-m gpu`: the trimmed-K form of the softmax.v weight search (rows of 208 instead of 256 elements; csrc k_gemm_grpk8t,
ADALOG_AV_KTRIM) against the 256-element path it replaces.  The launch leaves out only K positions that are zero padding in both
operands and keeps the order of every other operation, so nothing here has a tolerance: scores, packed bytes and the committed
search parameters are compared for equality."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
IMGS, H, D, P = 2, 6, 64, 128                     # G = 12 groups (image x head), head dim 64, 128 candidates


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import backend
    backend.set_backend(None)
    return backend.get()


def _last_kernel():
    from adalog_amd import _lib
    return _lib.load().adalog_last_kernel().decode()


def _case(M, K, bits, seed=0):
    """probabilities A [IMGS, H, M, K], values v [IMGS, H, K, D] with entries planted on rounding ties of two candidates, the
    per-head candidate grid (scale, zero point) [P, H]"""
    gen = torch.Generator().manual_seed(7000 + 13 * M + K + bits + seed)
    A = torch.softmax(4.0 * torch.randn(IMGS, H, M, K, generator=gen), dim=-1)
    v = torch.randn(IMGS, H, K, D, generator=gen) * 1.3 + 0.4
    qmax = 2 ** bits - 1
    lo, hi = v.amin(), v.amax()
    sc = ((hi - lo) / qmax) * torch.linspace(0.5, 1.1, P).view(P, 1) * torch.linspace(0.9, 1.1, H).view(1, H)
    zp = torch.round(-lo / sc).clamp(0, qmax)
    v[:, :, 3, 5] = (sc[17, 0] * 2.5).item()       # exact ties of candidate 17 / head 0, near-ties of its neighbours
    v[:, :, 7, 20] = (sc[90, H - 1] * -1.5).item()
    v[:, :, K - 1, 9] = (sc[40, 2] * 1.5).item()   # ... and one in the last key (the ragged end of the row)
    return A, v, sc.contiguous(), zp.contiguous()


def _layer(A, v, bits, steps=6):
    from adalog_amd import quant_layers as Q
    lay = Q.PostSoftmaxAsymmetricallyBatchingQuantMatMul(A_bit=bits, B_bit=bits, mode="raw", calib_batch_size=IMGS, search_round=1,
                                                         eq_n=P, head_channel_wise=True, num_heads=H, fpcs=True, steps=steps,
                                                         quantizer="adalog").to(DEV)
    Ad, vd = A.to(DEV), v.to(DEV)
    lay.raw_input, lay.raw_out = [Ad, vd], Ad @ vd
    return lay


def _scores(monkeypatch, trim, A, v, sc, zp, bits):
    """the B (v) search's scoring call as hyperparameter_searching makes it -> ([P, H] scores, kernel label, row length)"""
    from adalog_amd import search
    from adalog_amd.ops import BF16, BF16_FP8, Strided
    from adalog_amd.quant_layers import matmul as MM
    monkeypatch.setattr(MM, "AV_KTRIM", trim)
    lay = _layer(A, v, bits)
    lay._initialize_calib_parameters()
    aq = lay.A_quantizer
    a_q = 29
    aq.q.data.fill_(a_q)
    lay._q_host = a_q
    with torch.no_grad():
        qv = search.const_tensor([float(a_q)], torch.device(DEV))
        mixed = lay._mixed_B_search()
        ap = lay._pack_A_adalog(lay._a3(lay.raw_input[0]), qv, aq.scale.data.view(-1), 1, True,
                                k_align=lay._mixed_kalign()[1] if mixed else lay._kalign())
        got = lay._score("B", ap, sc.to(DEV), zp.to(DEV), BF16_FP8 if mixed else BF16, fixed_sa=Strided(aq.scale.data.view(-1)),
                         sa_mul=lay._ts32())
    torch.cuda.synchronize()
    return got.cpu(), _last_kernel(), ap.shape[-1]


OLD = "k_gemm_grpk8<bf16xfp8>"
# (M rows, K keys) -> kernel of the new path.  K <= 200: 13 MFMAs per block; 201..208: 14 (the 14th holds K = 200..207); K = 209 and
# the shapes outside the mixed 197-token family (K = 129, M = 33) run what they ran before
SHAPES = [(197, 197, "k_gemm_grpk8t<13,bf16xfp8>"), (197, 193, "k_gemm_grpk8t<13,bf16xfp8>"), (197, 207, "k_gemm_grpk8t<14,bf16xfp8>"),
          (197, 208, "k_gemm_grpk8t<14,bf16xfp8>"), (197, 129, None), (197, 209, OLD), (33, 197, None),
          (224, 197, "k_gemm_grpk8t<13,bf16xfp8>")]


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("M,K,label", SHAPES, ids=[f"M{m}-K{k}" for m, k, _ in SHAPES])
def test_scores_bit_identical(ops, monkeypatch, M, K, label, bits):
    A, v, sc, zp = _case(M, K, bits)
    want, k_old, kp_old = _scores(monkeypatch, False, A, v, sc, zp, bits)
    got, k_new, kp_new = _scores(monkeypatch, True, A, v, sc, zp, bits)
    print(f"M={M} K={K} bits={bits}: old {k_old} Kp={kp_old}, new {k_new} Kp={kp_new}, "
          f"max |diff| {(got - want).abs().max().item():.3e}, differing {int((got != want).sum())}/{got.numel()}")
    assert got.shape == want.shape == (P, H)
    assert torch.isfinite(want).all() and want.abs().max() > 0
    if label is None:                              # not a shape of the mixed 197-token family: one path
        assert k_new == k_old and kp_new == kp_old
    else:
        assert k_old == OLD and kp_old == 256
        assert k_new == label and kp_new == (256 if label == OLD else 208)
    assert torch.equal(got, want)


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("K", [197, 207, 208])
def test_packed_operands_are_the_old_ones_without_the_tail(ops, K, bits):
    """fp8 candidate columns (K-contiguous source: the fast packer, ragged last quad for K % 4 != 0; transposed view: the general
    one) and the fixed bf16 rows: the first 208 elements of every 256-element row, whose remaining 48 are zero."""
    from adalog_amd import search
    from adalog_amd.ops import FP8
    A, v, sc, zp = _case(197, K, bits, seed=1)
    G = IMGS * H
    d = lambda t: t.to(DEV)
    vt_view = d(v).reshape(G, K, D).transpose(1, 2)                    # [G, D, K], K stride D
    for src in (vt_view.contiguous(), vt_view):
        new = ops.pack_uniform(src, d(sc), d(zp), P, H, H, 1, 0, bits, FP8, c_inner=True, k_align=16)
        old = ops.pack_uniform(src, d(sc), d(zp), P, H, H, 1, 0, bits, FP8, c_inner=True, k_align=256)
        assert new.shape == (1, G, D * P, 208) and old.shape == (1, G, D * P, 256) and new.k_valid == old.k_valid == K
        nb, ob = new.view(torch.uint8), old.view(torch.uint8)
        assert torch.equal(nb, ob[..., :208])
        assert not ob[..., 208:].any() and not nb[..., K:].any()
        assert nb[..., :K].any()
    lay = _layer(A, v, bits)
    qv = search.const_tensor([29.0], torch.device(DEV))
    a3 = lay._a3(lay.raw_input[0])
    new = lay._pack_A_adalog(a3, qv, lay.A_quantizer.scale.data.view(-1), 1, True, k_align=32)
    old = lay._pack_A_adalog(a3, qv, lay.A_quantizer.scale.data.view(-1), 1, True, k_align=512)
    assert new.shape[-1] == 208 and old.shape[-1] == 256
    assert torch.equal(new.view(torch.int16), old.view(torch.int16)[..., :208])
    assert not old.view(torch.int16)[..., 208:].any() and new.view(torch.int16)[..., :K].any()


@pytest.mark.parametrize("bits", [3, 4])
def test_search_commits_identical_parameters(ops, monkeypatch, bits):
    """one hyperparameter_searching() of a 2-image softmax.v module: same log base, scale and zero point with the switch on and off"""
    from adalog_amd.quant_layers import matmul as MM
    A, v, _, _ = _case(197, 197, bits, seed=2)
    out = {}
    for trim in (False, True):
        monkeypatch.setattr(MM, "AV_KTRIM", trim)
        lay = _layer(A, v, bits)
        with torch.no_grad():
            lay.hyperparameter_searching()
        torch.cuda.synchronize()
        out[trim] = (lay.B_quantizer.scale.data.clone().cpu(), lay.B_quantizer.zero_point.data.clone().cpu(),
                     lay.A_quantizer.q.data.clone().cpu())
    for a, b in zip(out[False], out[True]):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a, b)
