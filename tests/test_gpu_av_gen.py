"""`-m gpu`: the softmax.v weight search with its candidates generated inside the scoring kernel (csrc k_gemm_avw_gen,
ops.gemm_score_avw, ADALOG_AV_GEN) against the route the search takes without it: pack_uniform + gemm_score, i.e. the mixed
bf16 x fp8 launch (k_gemm_grpk8t) where that takes the shape and the all-bf16 launch otherwise.  The generated operand is the
packed one value for value and the kernel keeps k_gemm_grpk8t's items, MFMA and summation order: against that launch the [P, H]
scores are compared for equality.  Where the search ran the all-bf16 launch (fewer than 8 groups, 128 rows or fewer) there is no
packed mixed launch to equal; those shapes are held against an fp64 evaluation of the objective, no worse than the route they had."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
H = 2
NEW = "k_gemm_avw_gen<13,bf16>"


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import backend
    backend.set_backend(None)
    return backend.get()


def _last_kernel():
    from adalog_amd import _lib
    return _lib.load().adalog_last_kernel().decode()


def _case(imgs, S, Sp, P, bits, headwise, seed=0):
    """probabilities A [imgs, H, S, S], values v [imgs, H, S, Sp], the candidate grid (scale, zero point) [P, H] or [P, 1].  Planted
    in v: exact rounding ties x / s = n + 0.5 of several candidates and their fp32 neighbours (the tie zone), values far beyond both
    clamp ends, +0 and -0, and one all-zero key row."""
    gen = torch.Generator().manual_seed(9000 + 17 * S + Sp + P + bits + 5 * imgs + seed)
    A = torch.softmax(4.0 * torch.randn(imgs, H, S, S, generator=gen), dim=-1)
    v = torch.randn(imgs, H, S, Sp, generator=gen) * 1.3 + 0.4
    qmax = 2 ** bits - 1
    lo, hi = v.amin(), v.amax()
    nh = H if headwise else 1
    sc = ((hi - lo) / qmax) * torch.linspace(0.5, 1.1, P).view(P, 1) * torch.linspace(0.9, 1.1, nh).view(1, nh)
    sc = sc.float().contiguous()
    zp = torch.round(-lo / sc).clamp(0, qmax).contiguous()
    k = lambda i: i % S                                                   # key rows, whatever S is
    for j, (c, h, n) in enumerate([(1, 0, 2.5), (P // 2, nh - 1, -1.5), (P - 1, 0, 0.5), (7 % P, nh - 1, -0.5)]):
        t = (sc[c, h] * n).float()                                        # x / s = n (a tie) in fp32
        v[:, :, k(3 + 2 * j), 5 + j] = t
        v[:, :, k(4 + 2 * j), 5 + j] = torch.nextafter(t, t * 2)          # ... and the values right beside it
        v[:, :, k(4 + 2 * j), 6 + j] = torch.nextafter(t, t * 0)
    v[:, :, S - 1, 9] = (sc[P // 3, 0] * 1.5).float()                     # a tie in the last key (the ragged end of the row)
    v[:, :, k(1), 0] = 1.0e4                                               # clamps at both ends
    v[:, :, k(2), 1] = -1.0e4
    v[:, :, k(0), 2] = 0.0
    v[:, :, k(1), 3] = -0.0
    v[:, :, k(11), :] = 0.0                                                # a zero row
    return A, v, sc, zp


def _layer(A, v, P, bits, headwise):
    from adalog_amd import quant_layers as Q
    lay = Q.PostSoftmaxAsymmetricallyBatchingQuantMatMul(A_bit=bits, B_bit=bits, mode="raw", calib_batch_size=A.shape[0], search_round=1,
                                                         eq_n=P, head_channel_wise=headwise, num_heads=H, fpcs=True, steps=6,
                                                         quantizer="adalog").to(DEV)
    Ad, vd = A.to(DEV), v.to(DEV)
    lay.raw_input, lay.raw_out = [Ad, vd], Ad @ vd
    return lay


def _scores(ops, gen, A, v, sc, zp, P, bits, headwise):
    """the B (v) search's scoring call -> ([P, H | 1] scores, kernel label).  gen = False: operands and dtype as the search picks them
    without the generated form; gen = True: the search's request for it, with the fixed operand in the trimmed rows (16-element
    granularity) the kernel reads wherever ops.gemm_score_avw_ok takes the shape."""
    from adalog_amd import search
    from adalog_amd.ops import BF16, BF16_FP8, Strided
    lay = _layer(A, v, P, bits, headwise)
    lay._initialize_calib_parameters()
    aq = lay.A_quantizer
    a_q = 29
    aq.q.data.fill_(a_q)
    lay._q_host = a_q
    G, S, K, Sp = lay._dims()
    with torch.no_grad():
        qv = search.const_tensor([float(a_q)], torch.device(DEV))
        mixed = lay._mixed_B_search()
        takes = gen and bool(ops.gemm_score_avw_ok(S, Sp, G, lay._heads(), P, K, (K + 15) // 16 * 16, bits))
        if takes:
            al, dt = 32, BF16_FP8
        else:
            al, dt = (lay._mixed_kalign()[1], BF16_FP8) if mixed else (lay._kalign(), BF16)
        ap = lay._pack_A_adalog(lay._a3(lay.raw_input[0]), qv, aq.scale.data.view(-1), 1, True, k_align=al)
        got = lay._score("B", ap, sc.to(DEV), zp.to(DEV), dt, fixed_sa=Strided(aq.scale.data.view(-1)), sa_mul=lay._ts32(), gen=gen)
    torch.cuda.synchronize()
    return got.cpu(), _last_kernel()


def _compare(ops, imgs, S, Sp, P, bits, headwise, new_label):
    A, v, sc, zp = _case(imgs, S, Sp, P, bits, headwise)
    want, k_old = _scores(ops, False, A, v, sc, zp, P, bits, headwise)
    got, k_new = _scores(ops, True, A, v, sc, zp, P, bits, headwise)
    print(f"imgs={imgs} S=K={S} Sp={Sp} P={P} bits={bits} headwise={headwise}: old {k_old}, new {k_new}, "
          f"max |diff| {(got - want).abs().max().item():.3e}, max rel {((got - want).abs() / want.abs()).max().item():.3e}, "
          f"differing {int((got != want).sum())}/{got.numel()}")
    assert got.shape == want.shape == (P, H if headwise else 1)
    assert torch.isfinite(want).all() and want.abs().max() > 0
    assert "avw" not in k_old
    if new_label is None:
        assert k_new == k_old                       # declined: the route of before
    else:
        assert k_new == new_label
    assert torch.equal(got, want)


def _fp64_scores(A, v, raw_out, sc, zp, bits, headwise, a_q=29):
    """the reference's objective (quant_layers/matmul.py:173-201) with the operands of the oracle's fake-quantisers -- bins decided
    in fp32 as the reference decides them -- and everything behind them (dequantisation, product, squared error, means) in fp64"""
    from oracle import adalog_oracle as O
    Aq = O.adalog_fake_quant(A, torch.ones(1, 1, 1, 1), a_q, bits)[0].double().to(DEV)           # [n, H, S, S]
    ro = raw_out.double()
    P = sc.shape[0]
    out = torch.empty(P, sc.shape[1], dtype=torch.float64)
    for c in range(P):
        s_c, z_c = sc[c].view(1, -1, 1, 1), zp[c].view(1, -1, 1, 1)
        bins = O.uniform_fake_quant(v, s_c, z_c, bits)[1]
        Vq = ((bins - torch.round(z_c)).double() * s_c.double()).to(DEV)
        err = -((ro - Aq @ Vq) ** 2)
        out[c] = (err.mean(dim=(2, 3)) if headwise else err.mean(dim=(1, 2, 3)).unsqueeze(1)).sum(0).cpu()
    return out


# (images, Sp, head-wise candidate parameters): every value of the three axes with either value of the others
COMBOS = [(2, 32, True), (3, 64, True), (2, 64, False), (3, 32, False)]
SMALL = [(S, n, sp, hw, bits) for S in (197, 16, 17, 33, 200) for n, sp, hw in COMBOS for bits in (3, 4)]


@pytest.fixture(scope="module")
def small_cases(ops):
    """every small case once: scores of both routes, their kernels, and their largest relative error against fp64"""
    res = {}
    for S, imgs, Sp, headwise, bits in SMALL:
        A, v, sc, zp = _case(imgs, S, Sp, 128, bits, headwise)
        want, k_old = _scores(ops, False, A, v, sc, zp, 128, bits, headwise)
        got, k_new = _scores(ops, True, A, v, sc, zp, 128, bits, headwise)
        ref = _fp64_scores(A, v, (A.to(DEV) @ v.to(DEV)), sc, zp, bits, headwise)
        rel = lambda t: ((t.double() - ref).abs() / ref.abs()).max().item()
        res[(S, imgs, Sp, headwise, bits)] = dict(want=want, got=got, k_old=k_old, k_new=k_new, e_old=rel(want), e_new=rel(got))
    return res


@pytest.mark.parametrize("S,imgs,Sp,headwise,bits", SMALL,
                         ids=[f"S{S}-n{n}-Sp{sp}-{'head' if hw else 'shared'}-b{b}" for S, n, sp, hw, b in SMALL])
def test_small_shapes_against_current_route(small_cases, S, imgs, Sp, headwise, bits):
    """G = 4 / 6 groups of 16 .. 200 keys: the kernel takes them all.  Without it the search runs pack_uniform(bf16) + the all-bf16
    streaming launch here (the packed mixed launch needs >= 8 groups of 129 .. 224 rows) -- another kernel, whose fp32 sums run
    over 64-row tiles in another order -- so the scores cannot be equal bit for bit (measured: up to 89 of 256 scores differ, by at
    most 1.4e-7 relative); equality is asserted where the packed mixed launch exists (test_scores_equal_packed_mixed_launch).  Here
    both routes are held against the fp64 evaluation of the reference's objective: the kernel's largest relative error may exceed
    the current route's on the same inputs by no more than the current route's own spread over these cases.
    Measured (MI355X, these 40 cases): largest relative error against fp64 of the current route 7.1e-8 .. 1.85e-7 (spread 1.14e-7),
    of the kernel 8.5e-8 .. 2.08e-7; the kernel's largest excess over the current route on the same inputs 5.8e-8 (33 keys, 3 bit);
    between the two routes 15 .. 126 of the 128 / 256 scores differ."""
    r = small_cases[(S, imgs, Sp, headwise, bits)]
    e_old = [c["e_old"] for c in small_cases.values()]
    spread = max(e_old) - min(e_old)
    print(f"S=K={S} imgs={imgs} Sp={Sp} headwise={headwise} bits={bits}: old {r['k_old']} rel err {r['e_old']:.3e}, new {r['k_new']} "
          f"rel err {r['e_new']:.3e}; old route over all cases [{min(e_old):.3e}, {max(e_old):.3e}], "
          f"differing {int((r['got'] != r['want']).sum())}/{r['got'].numel()}")
    assert r["got"].shape == r["want"].shape == (128, H if headwise else 1)
    assert torch.isfinite(r["want"]).all() and r["want"].abs().max() > 0
    assert "avw" not in r["k_old"] and r["k_new"] == NEW
    if "bf16xfp8" in r["k_old"]:
        assert torch.equal(r["got"], r["want"])
    else:
        assert r["e_new"] <= r["e_old"] + spread


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("S,Sp,headwise,P", [(197, 64, True, 128), (200, 32, True, 128), (197, 32, False, 128), (193, 64, True, 128),
                                             (197, 64, True, 64), (200, 32, False, 64), (197, 64, True, 256), (193, 32, False, 256)])
def test_scores_equal_packed_mixed_launch(ops, S, Sp, headwise, P, bits):
    """G = 8 groups, 193..200 keys: the route without the generated form is pack_uniform(fp8) + k_gemm_grpk8t<13>, the launch whose
    items, MFMA order and sums the kernel reproduces -- with 64, 128 and 256 candidates (2, 4 and 8 waves per workgroup)."""
    A, v, sc, zp = _case(4, S, Sp, P, bits, headwise, seed=3)
    want, k_old = _scores(ops, False, A, v, sc, zp, P, bits, headwise)
    got, k_new = _scores(ops, True, A, v, sc, zp, P, bits, headwise)
    print(f"S=K={S} Sp={Sp} P={P} bits={bits} headwise={headwise}: old {k_old}, new {k_new}, differing {int((got != want).sum())}/{got.numel()}")
    assert got.shape == (P, H if headwise else 1) and torch.isfinite(want).all() and want.abs().max() > 0
    assert k_old == "k_gemm_grpk8t<13,bf16xfp8>" and k_new == NEW
    assert torch.equal(got, want)


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("S,Sp,P", [(201, 64, 128), (197, 48, 128), (197, 32, 32), (197, 64, 32)],
                         ids=["K201", "Sp48", "P32-Sp32", "P32-Sp64"])
def test_declined_shapes_fall_back(ops, S, Sp, P, bits):
    """more than 200 keys, a head dim that is no multiple of 32, 32 candidates: the predicate declines, the request is ignored"""
    assert not ops.gemm_score_avw_ok(S, Sp, 8, H, P, S, (S + 15) // 16 * 16, bits)
    _compare(ops, 4, S, Sp, P, bits, True, None)


def test_predicate(ops):
    ok = lambda M, N, G, gmod, P, K, Kp, bits: bool(ops.gemm_score_avw_ok(M, N, G, gmod, P, K, Kp, bits))
    assert ok(197, 64, 192, 6, 128, 197, 208, 4) and ok(197, 64, 96, 3, 128, 197, 208, 4) and ok(16, 32, 4, 2, 128, 16, 16, 3)
    assert ok(200, 64, 8, 2, 64, 200, 208, 4) and ok(224, 64, 8, 2, 256, 197, 256, 2)
    assert not ok(197, 64, 192, 6, 128, 197, 208, 5)           # more than 4 bits: the codes leave the exact range
    assert not ok(197, 48, 192, 6, 128, 197, 208, 4)           # Sp no multiple of 32
    assert not ok(201, 64, 192, 6, 128, 201, 208, 4)           # K > 200: a fourteenth MFMA
    assert not ok(197, 64, 192, 6, 32, 197, 208, 4) and not ok(197, 64, 192, 6, 96, 197, 208, 4)
    assert not ok(225, 64, 192, 6, 128, 197, 208, 4)           # more than 7 row blocks
    assert not ok(197, 64, 192, 6, 128, 197, 196, 4) and not ok(197, 64, 192, 6, 128, 197, 204, 4)   # rows shorter than K / not 16-byte slots
    assert not ok(197, 64, 192, 5, 128, 197, 208, 4)           # groups no multiple of the heads


@pytest.mark.parametrize("bits", [3, 4])
def test_search_commits_identical_parameters(ops, monkeypatch, bits):
    """one hyperparameter_searching() of a 4-image softmax.v module: same log base, scale and zero point with the switch on and off,
    and the switch decides the kernel of the search's last scoring call"""
    from adalog_amd.quant_layers import matmul as MM
    A, v, _, _ = _case(4, 197, 64, 128, bits, True, seed=2)
    out, seen = {}, {}
    for gen in (False, True):
        monkeypatch.setattr(MM, "AV_GEN", gen)
        lay = _layer(A, v, 128, bits, True)
        calls = []
        orig = lay._score
        lay._score = lambda *a, **kw: (orig(*a, **kw), calls.append(_last_kernel()))[0]
        with torch.no_grad():
            lay.hyperparameter_searching()
        torch.cuda.synchronize()
        seen[gen] = set(calls)
        out[gen] = (lay.B_quantizer.scale.data.clone().cpu(), lay.B_quantizer.zero_point.data.clone().cpu(),
                    lay.A_quantizer.q.data.clone().cpu())
    assert seen[False] == {"k_gemm_grpk8t<13,bf16xfp8>"} and seen[True] == {NEW}
    for a, b in zip(out[False], out[True]):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a, b)


def test_window_search_keeps_its_kernel(ops):
    """windows of a Swin (49 x 49 probabilities, 32 head-dim columns, 256 groups): the kernel could take the shape, but the search
    asks for the generated form only above 64 keys -- its mixed launch here is the window kernel, and stays"""
    assert ops.gemm_score_avw_ok(49, 32, 256, H, 128, 49, 64, 3)
    A, v, _, _ = _case(128, 49, 32, 128, 3, True, seed=4)
    lay = _layer(A, v, 128, 3, True)
    assert lay._mixed_B_search()
    calls = []
    orig = lay._score
    lay._score = lambda *a, **kw: (orig(*a, **kw), calls.append(_last_kernel()))[0]
    with torch.no_grad():
        lay.hyperparameter_searching()
    torch.cuda.synchronize()
    assert calls and set(calls) == {"k_gemm_winb<bf16xfp8>"}
