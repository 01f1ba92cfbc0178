"""`-m gpu`: the per-launch timing records of adalog_amd.ops (``GEMM_EVENTS``, read by bench.py) -- one row per site that records
one, driven once at the smallest shape at which the site's own test drives it (the row names that test), on whichever route
(torch.ops / ctypes) the environment takes.  With ``GEMM_EVENTS`` a list the call appends exactly one tuple
(dtype, M, N, K, C_or_P, G, start event, end event, label); with ``GEMM_EVENTS = None`` it creates no event and appends nothing.
The expected fields are written out below; the two Gram builds record a fixed label, every other site adalog_last_kernel()."""
import pytest
import torch

from tests import gram_cases as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
I8, BF16, F32, FP8, BF16_FP8 = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import backend
    backend.set_backend(None)
    return backend.get()


def d(t):
    return None if t is None else t.to(DEV).contiguous()


def g(seed):
    return torch.Generator().manual_seed(seed)


def _linear_case(rows, T_, K, P, bits, seed):
    """x [T, K], W [rows, K], bias, raw_out and per-row weight parameters of a uniformly quantised Linear layer"""
    gen = g(seed)
    x = torch.randn(T_, K, generator=gen) * 1.3 + 0.2
    W = torch.randn(rows, K, generator=gen) * 0.05
    b = torch.randn(rows, generator=gen) * 0.1
    qmax = 2 ** bits - 1
    w_lo, w_hi = W.min(1).values, W.max(1).values
    w_s = (w_hi - w_lo) / qmax
    w_z = torch.round(-w_lo / w_s).clamp(0, qmax)
    return x, W, b, torch.nn.functional.linear(x, W, b), w_s, w_z, qmax, gen


# ---- the sites: each returns a zero-argument callable that makes ONE call of the site (everything else is done before)
def _gemm_score(ops):
    """test_gpu_gemm_routes.py::test_stream_route, first row (keep_n, no row vectors)"""
    M, Ncols, K, P, G = 197, 5, 40, 64, 3
    gen = g(4100 + M + K)
    Kp = ops.pad_k(K, F32)
    A = torch.zeros(1, G, M, Kp); B = torch.zeros(1, G, Ncols * P, Kp)
    A[..., :K] = torch.randint(-15, 16, (1, G, M, K), generator=gen).float() * 0.25
    B[..., :K] = torch.randint(-15, 16, (1, G, Ncols * P, K), generator=gen).float()
    ref = d(torch.randn(G, Ncols, M, generator=gen) * 3)
    sa = ops.Strided(d(torch.rand(1, generator=gen) * 0.002 + 0.001))
    sb = ops.Strided(d(torch.rand(P, Ncols, generator=gen) * 0.5 + 0.5), c=Ncols, n=1)
    bias = ops.Strided(d(torch.randn(P, Ncols, generator=gen)), c=Ncols, n=1)
    Ad, Bd = A.to(DEV), B.to(DEV)
    Ad.k_valid = K; Bd.k_valid = K
    return lambda: ops.gemm_score(F32, Ad, Bd, M, Ncols, P, G, 1, ref, sa, sb, bias, False, True, 0.01, sa_mul=0.5, ref_div=P, order=2,
                                  ref_transposed=True)


def _gemm_score_gen(ops):
    """test_gpu_kernels.py::test_gemm_score_gen_matches_packed_path, ("win", 512, 8, 49, 32, 32), 4-bit fp8"""
    G, H, S, K, al, bits, P = 512, 8, 49, 32, 32, 4, 128
    gen = g(9100 + bits + G + S)
    qmax = 2 ** bits - 1
    src = torch.randn(G, S, K, generator=gen) * 1.3 + 0.4
    fix = torch.randn(G, S, K, generator=gen)
    lo, hi = src.amin(), src.amax()
    sc = ((hi - lo) / qmax) * torch.linspace(0.5, 1.1, P).view(P, 1) * torch.linspace(0.9, 1.1, H).view(1, H)
    zp = torch.round(-lo / sc).clamp(0, qmax)
    f_s = torch.full((H,), fix.abs().max().item() * 2 / qmax)
    f_z = torch.full((H,), float(2 ** (bits - 1)))
    ref = d(torch.einsum("gsk,gtk->gst", src, fix))
    fp = ops.pack_uniform(d(fix), d(f_s), d(f_z), 1, 0, H, 1, 0, bits, FP8, k_align=al)
    assert ops.gemm_score_gen_ok(FP8, S, S, G, H, P, K, fp.shape[-1])
    sa, sb, srcd, zpd = ops.Strided(d(f_s), g=1), ops.Strided(d(sc), c=H, g=1), d(src), d(zp)
    return lambda: ops.gemm_score_gen(FP8, fp, srcd, zpd, bits, S, S, P, G, H, ref, sa, sb, True, 1.0 / (S * S))


def _gemm_score_avq(ops):
    """test_gpu_kernels.py::test_gemm_score_avq_matches_packed_path, ("win16", 512, 16, 49, 32), 4 bits"""
    G, H, S, D, bits, P = 512, 16, 49, 32, 4, 128
    gen = g(9300 + bits + G + S)
    A = torch.softmax(4.0 * torch.randn(G, S, S, generator=gen), dim=-1)
    v = torch.randn(G, S, D, generator=gen)
    b_s = torch.full((H,), v.abs().max().item() * 2 / (2 ** bits - 1))
    b_z = torch.full((H,), float(2 ** (bits - 1)))
    ref = d(torch.einsum("gsk,gkd->gsd", A, v))
    q_all = d(torch.arange(10, 10 + P).float())
    mant = torch.round(torch.tensor([2 ** (-j / 37.0) for j in range(37)]) * (4 * 2 ** (bits - 1) - 2))
    bp = ops.pack_uniform(d(v.transpose(1, 2)), d(b_s), d(b_z), 1, 0, H, 1, 0, bits, BF16, k_align=64)
    assert ops.gemm_score_avq_ok(D, S, G, H, P, S, bp.shape[-1], bits)
    lut = ops.adalog_value_lut(q_all, bits, d(mant))
    sa, sb, Ad = ops.Strided(d(b_s), g=1), ops.Strided(d(torch.ones(P)), c=1), d(A)
    ts = 1.0 / (4 * 2 ** (bits - 1) - 2)
    return lambda: ops.gemm_score_avq(bp, Ad, q_all, lut, bits, D, S, P, G, H, ref, sa, sb, 1.0 / (S * D), sa_mul=ts)


def _gemm_score_avw(ops):
    """test_gpu_av_gen.py::test_small_shapes_against_current_route, S = K = 16, 2 images x 2 heads, Sp = 32, head-wise, 3 bits: the
    search's own scoring call (MatMul._score with gen=True)"""
    from tests.test_gpu_av_gen import _case, _scores
    A, v, sc, zp = _case(2, 16, 32, 128, 3, True)
    return lambda: _scores(ops, True, A, v, sc, zp, 128, 3, True)


def _score_act_fused(ops):
    """test_gpu_kernels.py::test_score_act_fused_matches_packed_path, (256, 96, 31, 2, 4, 0.0, True): the search's own scoring call"""
    from tests.test_gpu_kernels import _postgelu_layer
    I, Oc, T_, N, bits = 256, 96, 31, 2, 4
    lay, scs, qs = _postgelu_layer(I, Oc, T_, N, bits, 1234 + I + T_, 0.0, True)
    with torch.no_grad():
        wp, rowsum = lay._pack_w_fixed(BF16, want_rowsum=True)
        fold = ops.shift_fold(rowsum.view(1, -1), lay.w_quantizer.scale.data.view(1, -1), lay.a_quantizer.shift.data, lay.bias.data).view(-1)
        assert ops.score_act_fused_ok(Oc, N * T_, I, wp.shape[-1], 128, bits)
        lay._log2_x()                                   # (memoised per captured tensor: not part of the scoring call)

    def call():
        with torch.no_grad():
            return lay._score_scale_logbase(wp, fold, scs, qs)
    return call


def _score_act_gen(ops):
    """test_gpu_kernels.py::test_score_act_gen_matches_packed_path, (384, 591, 384, 128, 3, "fp8")"""
    M, T_, K, P, bits = 384, 591, 384, 128, 3
    x, W, b, ref, w_s, w_z, qmax, gen = _linear_case(M, T_, K, P, bits, 4000 + M + T_ + K + P)
    s = d((x.abs().max() * 2 / qmax) * (0.4 + 1.2 * torch.rand(P, 1, generator=gen)))
    z = d(torch.randint(0, qmax + 1, (P, 1), generator=gen).float())
    wp = ops.pack_uniform(d(W).unsqueeze(0), d(w_s), d(w_z), 1, 0, 1, 0, 1, bits, FP8)
    assert ops.score_act_gen_ok(FP8, M, T_, K, wp.shape[-1], P)
    xd, refd, wsd, bd = d(x), d(ref), d(w_s), d(b)
    return lambda: ops.score_act_gen(FP8, wp, xd, s, z, bits, refd, wsd, bd, 1.0 / (197 * M))


def _score_w_gen(ops):
    """test_gpu_kernels.py::test_score_w_gen_matches_packed_path, (1568, 768, 768), 4-bit fp8"""
    T_, O, K, P, bits = 1568, 768, 768, 128, 4
    x, W, b, ref, w_s, w_z, qmax, gen = _linear_case(O, T_, K, P, bits, 8000 + bits + T_ + O)
    sc = d(w_s.view(1, O) * torch.linspace(0.6, 1.2, P).view(P, 1))
    zp = d(torch.round(w_z.view(1, O) / torch.linspace(0.6, 1.2, P).view(P, 1)).clamp(0, qmax))
    a_s, a_z = d(torch.tensor([x.abs().max().item() * 2 / qmax])), d(torch.tensor([float(2 ** (bits - 1))]))
    xp = ops.pack_uniform(d(x).unsqueeze(0), a_s, a_z, 1, 0, 1, 0, 0, bits, FP8)
    assert ops.score_w_gen_ok(FP8, T_, O, K, xp.shape[-1], P)
    Wd, ref_t, bd = d(W), d(ref.t()), d(b)
    return lambda: ops.score_w_gen(FP8, xp, Wd, sc, zp, bits, ref_t, a_s, bd, 1.0 / 197)


W_CASE, A_CASE = T.W_CASES[0], T.A_CASES[0]             # test_gpu_gram_edges.py: K32 T1 O1 P32 a4w4 / K32 T1 O3 P1 a4w4


def _gram_build(ops):
    i = T.weight_inputs(W_CASE)
    x, sa, za, ref_t, b = d(i["x"]), d(i["sa"]), d(i["za"]), d(i["ref"].t()), d(i["bias"])
    return lambda: ops.GramState(x, sa, za, W_CASE.a_bits, ref_t, b)


def _gram_score_w(ops):
    i = T.weight_inputs(W_CASE)
    st = _gram_build(ops)()
    W, sc, zp = d(i["W"]), d(i["sc"]), d(i["zp"])
    return lambda: st.score_w(W, sc, zp, W_CASE.w_bits, i["norm"])


def _gram_act_build(ops):
    i = T.act_inputs(A_CASE)
    prep = ops.GramActPrepared(d(i["x"]))
    ref, b, W, sw, zw = d(i["ref"]), d(i["bias"]), d(i["W"]), d(i["sw"]), d(i["zw"])
    return lambda: ops.GramActState(prep, ref, b, W, sw, zw, A_CASE.w_bits, A_CASE.a_bits, A_CASE.P)


def _gram_act_score(ops):
    i = T.act_inputs(A_CASE)
    st = _gram_act_build(ops)()
    sc, zp = d(i["sc"]).view(A_CASE.P, 1), d(i["zp"]).view(A_CASE.P, 1)
    return lambda: st.score(sc, zp, i["norm"])


# (site, (dtype, M, N, K, C_or_P, G), label)
SITES = [
    (_gemm_score, (F32, 197, 5, 40, 64, 3), "k_gemm_stream<f32>"),
    (_gemm_score_gen, (FP8, 49, 49, 32, 128, 512), "k_gemm_win_gen<fp8>"),
    (_gemm_score_avq, (BF16, 32, 49, 49, 128, 512), "k_gemm_avq<4,bf16>"),
    (_gemm_score_avw, (BF16_FP8, 16, 32, 16, 128, 4), "k_gemm_avw_gen<13,bf16>"),
    (_score_act_fused, (BF16, 96, 62, 256, 128, 1), "k_act_fused_asm<4,4,bf16>"),
    (_score_act_gen, (FP8, 384, 591, 384, 128, 1), "k_gemm_slab_gen<fp8>"),
    (_score_w_gen, (FP8, 1568, 768, 768, 128, 1), "k_gemm_slab128_wgen<fp8>"),
    (_gram_build, (I8, 1, 32 + 4 * 1, 32, 1, 1), "k_gram_build"),                # K + 4 O columns
    (_gram_score_w, (I8, 2 * 32 + 32, 1, 32, 32, 1), "k_gram_score<i8>"),        # two limbs (T = 1, 4 bits) x K + the 32-row panel
    (_gram_act_build, (I8, 4 * 1, 32, 3, 1, 1), "k_gram_act_build"),             # four limbs x T
    (_gram_act_score, (I8, 1, 32, 32, 1, 1), "k_gram_act<i8>"),                  # one 32 x 32 block of the triangle
]


@pytest.mark.parametrize("site,meta,label", SITES, ids=[s[0].__name__.lstrip("_") for s in SITES])
def test_site_records_one_event(ops, monkeypatch, site, meta, label):
    call = site(ops)
    made = []
    event = torch.cuda.Event
    monkeypatch.setattr(torch.cuda, "Event", lambda *a, **k: made.append(1) or event(*a, **k))
    assert ops.GEMM_EVENTS is None
    call()
    assert ops.GEMM_EVENTS is None and not made         # not timed: no event object, nothing appended
    ops.GEMM_EVENTS = []
    try:
        call()
        rec = ops.GEMM_EVENTS
    finally:
        ops.GEMM_EVENTS = None
    torch.cuda.synchronize()
    print(site.__name__, [r[:6] + r[8:] for r in rec], len(made))
    assert len(rec) == 1 and len(rec[0]) == 9 and len(made) == 2
    assert rec[0][:6] == meta
    assert rec[0][6].elapsed_time(rec[0][7]) >= 0
    assert rec[0][8] == label
