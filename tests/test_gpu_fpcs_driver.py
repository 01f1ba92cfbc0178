"""`-m gpu`: every tail route of the FPCS search driver (adalog_amd.search.fpcs) on the device, held to the independent replay of
tests/fpcs_reference.py.  The scoring kernels are pinned call by call elsewhere; this file pins what joins them: the grids the
driver's tails generate from the device's own scores, the spacing chain in the driver's private buffer, the commit into the
quantiser's parameter storage, the read-only memo, and ADALOG_FUSED_TAIL on / off.

Every case is one search of 128 candidates driven through a Spy over hand-built scorers on ``ops`` objects, so that the route is known:

    plain             plain scores -> search.honour_tail -> k_topk_next              (score_w_self; a NaN, ties and the clamp planted)
    sorted_*          score_self_sorted(..., tail=): rows of a weight, per-tensor, channel-wise
    gram_w_*          GramState.score_w(..., tail=)
    gram_a_*          GramActState.score(..., tail=)
    pend_w            PendingScores of gemm_score -> finish_topk_next, per-column partials (a block ranks its own columns)
    pend_a            PendingScores of score_act_gen -> finish_topk_next, per-workgroup accumulators (the last block ranks)
    pend_mm           PendingScores of the per-head q . k^T search (cols = H = 3) -> finish_topk_next (per-workgroup accumulators)
    postgelu          zp = None, a third plane (the log base), width 32: the fused AdaLog scorer's plain scores -> k_topk_next

Shapes of the pend_* layers: (I, Oc, T, N) = (128, 96, 50, 4) for the weight search -- the smallest the issue names; gemm_score
defers it with candidate-innermost per-column partials (mode 1) -- and (128, 256, 50, 4) for score_act_gen, which refuses fewer
than 256 output rows (adalog_score_act_gen_ok).

The clamp edge.  clamp_min = 1e-4 decides a grid value only where a survivor lies within half a spacing of it.  The product's
activation grids are clamped themselves (a grid below the clamp has spacing 0 and never moves again), and the MSE optimum of real data
lies inside its grid, so the cases that pass the clamp put it there: the data are scaled until the first grid starts at 1.03e-4, and the
scorer is then given the same data scaled once more so that its optimum falls just below the grid's first scale (the objectives are
covariant: data * r moves the optimum to scale * r).  The lowest scale survives, its lower neighbours fall below 1e-4, and every case
with a clamp asserts from the recorded steps that the clamp changed values (_clamp_hits).

The fp64 ranking check: at every step, for every candidate the device left out of its top-k, the fp64 objective must not exceed the
k-th survivor's by more than 2 * tol * |score|, with tol the relative tolerance the scorer's own kernel test asserts:
    score_w_self        1e-5   tests/test_gpu_kernels.py:508
    score_self_sorted   1e-5   tests/test_gpu_kernels.py:537 (weight rows), 2e-5 tests/test_gpu_kernels.py:555 (activation layouts)
    k_gram_score        2e-7   tests/test_gpu_kernels.py:1776
    k_gram_act          3e-6   tests/test_gpu_kernels.py:1848
    gemm_score          2e-6   tests/test_gpu_kernels.py:424
    score_act_gen       1e-4   tests/test_gpu_kernels.py:610 (its only comparison with a specification; 2e-6 at :605 is kernel vs kernel)
    score_act_fused     3.5e-6 measured, see _case_postgelu
"""
import pytest
import torch

from tests import cpu_backend as CB
from tests import fpcs_reference as FR

pytestmark = pytest.mark.gpu

DEV = "cuda"
P = 128


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import backend
    backend.set_backend(None)
    return backend.get()          # raises loudly if the HIP library or the device is missing


def _last_kernel():
    from adalog_amd import _lib
    return _lib.load().adalog_last_kernel().decode()


def g(seed):
    return torch.Generator().manual_seed(seed)


def d(t):
    return t.to(DEV).contiguous()


class Case:
    """one search: the grid it starts from, a factory of its scorer, the fp64 objective of its candidates"""
    width, clamp, third, nan_at, kernel, pend_mode, route = 16, None, None, None, None, None, "fused"      # route: fused | pend | topk

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ------------------------------------------------------------------------------------------------ fp64 objectives
def _fq_int(x, s, z, bits):
    """q - z of the uniform quantiser: the rounding decision in fp32 like the kernels (x / s, round half to even), the result exact"""
    z = torch.round(z)
    return ((torch.round(x / s) + z).clamp(0, 2 ** bits - 1) - z).double()


def _self_mse64(seg, bits, norm):
    """-norm * sum over segment c of (x - fq_p(x))^2 for the candidates of the checked columns"""
    def f(scale, zp, third, cols):
        out = []
        for c in cols:
            x = seg[c].view(1, -1)
            s, z = scale[:, c].view(-1, 1), zp[:, c].view(-1, 1)
            e = x.double() - _fq_int(x, s, z, bits) * s.double()
            out.append(-norm * (e * e).sum(1))
        return torch.stack(out, 1)
    return f


def _plant_tie(scale, zp, f64, cols, width=16):
    """make a candidate outside the top-k a copy of the k-th best of one column: an exact tie across the k boundary -> (a, b, col).
    Of `cols` the column is taken whose k-th best is furthest (in fp64, relative) from its neighbours in the order, so that the
    fp32 scores of the device put the same candidate on the boundary."""
    s64 = f64(scale.cpu(), zp.cpu(), None, cols)
    srt, order = torch.sort(s64, dim=0, descending=True, stable=True)
    room = torch.minimum(srt[width - 2] - srt[width - 1], srt[width - 1] - srt[width]) / srt[width - 1].abs()
    j = int(room.argmax())
    col, a, b = cols[j], int(order[width - 1, j]), int(order[60, j])
    scale[b, col], zp[b, col] = scale[a, col], zp[a, col]
    return a, b, col


CLAMP = 1e-4


def _edge_factors(grid_of, f64_of, col):
    """the two data factors of the clamp edge (file docstring): f puts the first scale of column `col` of the data's own grid at
    1.03e-4; r then moves the optimum of the scored data to 0.97 of that scale.  grid_of(f) -> (scale, zp, delta) of data * f;
    f64_of(f) -> the fp64 objective of data * f."""
    f = 1.03e-4 / float(grid_of(1.0)[0][0, col])
    scale, zp, delta = grid_of(f)
    assert float(scale[:, col].min()) >= CLAMP and float(delta[col]) > 0          # the grid itself is not clamped
    s64 = f64_of(f)(scale.cpu(), zp.cpu(), None, [col])[:, 0]
    r = 0.97 * float(scale[0, col]) / float(scale[int(s64.argmax()), col])
    return f, r, (scale, zp, delta)


def _clamp_hits(steps, delta0, width, clamp, col):
    """how many recorded grid values of column `col` equal the clamp where the reference's unclamped scale + (lin - 0.5) * delta lies below it"""
    dd, hits = delta0.detach().cpu().clone(), 0
    for cur, nxt in zip(steps[:-1], steps[1:]):
        (raw, _, _), dd = FR.next_grid(cur.scale, cur.zp, cur.third, FR.rank(cur.scores, width), dd, P // width, None)
        hits += int(((raw[:, col] < clamp) & (nxt.scale[:, col] == clamp)).sum())
    return hits


# ------------------------------------------------------------------------------------------------ the cases
def _case_plain(ops):
    """honour_tail -> topk_next on [100, 70] weight rows; clamp 1e-4 (row 5 lies below it: 128 equal scales after the first expansion),
    a tie across the k boundary in one of columns 6 .. 39, one NaN score at step 2"""
    from adalog_amd import search
    bits = 4
    W = torch.randn(100, 70, generator=g(1)) * 0.1
    W[5] *= 1e-4
    w2 = d(W)
    scale, zp, delta = search.weight_grid(w2, bits, P)
    scale, zp = scale.clone(), zp.clone()
    f64 = _self_mse64(W, bits, 1.0 / 70)
    tie = _plant_tie(scale, zp, f64, list(range(6, 40)))

    def make():
        n = [0]

        def fn(s, z, t, tail=None):
            sc = ops.score_w_self(w2, s, z, bits)
            if n[0] == 2:
                sc[37, 3] = float("nan")
            n[0] += 1
            return search.honour_tail(sc, tail)
        fn.fused_tail = True
        return fn
    return Case(make=make, scale=scale, zp=zp, delta=delta, clamp=CLAMP, f64=f64, tol=1e-5, cols=sorted({0, 3, 5, tie[2], 50, 99}),
                nan_at=(2, 37, 3), tie=tie, clamp_col=5)


def _case_sorted(ops, layout):
    from adalog_amd import search
    bits = 4
    tie_cols = clamp_col = None
    if layout == "rows":                                   # a segment per weight row: S = 100, n = 70
        W = torch.randn(100, 70, generator=g(2)) * 0.1
        w2 = d(W)
        seg, norm, clamp, tol = W, 1.0 / 70, None, 1e-5
        scale, zp, delta = search.weight_grid(w2, bits, P)
        cols, tie_cols = [0, 33, 99], list(range(6, 40))
    else:
        x = torch.randn(4, 50, 96, generator=g(3)) * torch.linspace(0.3, 2, 96) + 0.2
        cw = layout == "channel"
        clamp, tol = CLAMP, 2e-5
        clamp_col = 5 if cw else 0                         # channel 5 | the one segment: scaled to the clamp edge

        def scaled(f):
            xs = x.clone()
            if cw:
                xs[..., 5] *= f
            else:
                xs *= f
            return xs
        if cw:                                             # a segment per channel: S = 96, n = 200
            segs, norm = lambda xs: xs.reshape(-1, 96).t().contiguous(), 1.0 / 50
            cols, tie_cols = [0, 5, 40, 95], list(range(6, 40))
        else:                                              # one segment: S = 1, n = 4 * 50 * 96
            segs, norm = lambda xs: xs.reshape(1, -1), 1.0 / (50 * 96)
            cols = [0]
        f, r, (scale, zp, delta) = _edge_factors(lambda f_: search.activation_grid(d(scaled(f_)), bits, P, cw),
                                                 lambda f_: _self_mse64(segs(scaled(f_)), bits, norm), clamp_col)
        seg = segs(scaled(f * r))
    sp = ops.sorted_prefix(d(seg))
    assert ops.sorted_prefix_ok(sp.S, sp.n, bits)
    scale, zp = scale.clone(), zp.clone()
    f64 = _self_mse64(seg, bits, norm)
    tie = _plant_tie(scale, zp, f64, tie_cols) if tie_cols else None
    if tie:
        cols = sorted(set(cols) | {tie[2]})

    def make():
        fn = lambda s, z, t, tail=None: ops.score_self_sorted(sp, s, z, bits, norm, tail=tail)
        fn.fused_tail = True
        return fn
    return Case(make=make, scale=scale, zp=zp, delta=delta, clamp=clamp, f64=f64, tol=tol, cols=cols, tie=tie, clamp_col=clamp_col)


def _gram_inputs(T, O, K, bits):
    gen = g(12000 + bits + T + O + K)
    x = torch.randn(T, K, generator=gen)
    x[:, : max(1, K // 8)] *= 3.0
    W = torch.randn(O, K, generator=gen) * 0.05
    b = torch.randn(O, generator=gen) * 0.1 if K != 96 else None
    ref = torch.nn.functional.linear(x, W, b)
    return x, W, b, ref


def _case_gram_w(ops, T, O, K, bits):
    from adalog_amd import search
    x, W, b, ref = _gram_inputs(T, O, K, bits)
    qmax = 2 ** bits - 1
    a_s = torch.tensor([x.abs().max().item() * 1.2 / qmax])
    a_z = torch.tensor([float(2 ** (bits - 1) - 1)])
    tok = 49 if K == 64 else 125
    norm = 1.0 / tok
    assert ops._lib.load().adalog_gram_supported(T, O, K, bits, bits, P)
    Wd = d(W)
    scale, zp, delta = search.weight_grid(Wd, bits, P)
    st = ops.GramState(d(x), d(a_s), d(a_z), bits, d(ref.t()), None if b is None else d(b))
    spec = CB.GramState(x, a_s, a_z, bits, ref.t().contiguous(), b)

    def make():
        fn = lambda s, z, t, tail=None: st.score_w(Wd, s, z, bits, norm, tail=tail)
        fn.fused_tail = True
        fn.global_scores = True                            # (as quant_layers/linear.py sets it for the Gram form)
        return fn
    f64 = lambda s, z, t, cols: spec.score_w(W, s, z, bits, norm).double()[:, cols]
    return Case(make=make, scale=scale, zp=zp, delta=delta, f64=f64, tol=2e-7, cols=[0, 1, 3, O // 2, O - 1], kernel="k_gram_score<i8>")


def _case_gram_a(ops, T, O, K, bits):
    from adalog_amd import search
    x, W, b, _ = _gram_inputs(T, O, K, bits)
    qmax = 2 ** bits - 1
    tok = 49 if K == 64 else 125
    norm = 1.0 / (tok * O)
    assert ops._lib.load().adalog_gram_act_supported(T, O, K, bits, bits, P)

    def problem(f, device=True):
        """the search of x * f against W / f (same outputs): -> (scorer factory, fp64 objective)"""
        xs, Ws = x * f, W / f
        ref = torch.nn.functional.linear(xs, Ws, b)
        w_lo, w_hi = Ws.min(1).values, Ws.max(1).values
        sw = (w_hi - w_lo) / qmax
        zw = torch.round(-w_lo / sw).clamp(0, qmax)
        spec = CB.GramActState(CB.GramActPrepared(xs), ref, b, Ws, sw, zw, bits, bits, P)
        f64 = lambda s, z, t, cols: spec.score(s.reshape(-1), z.reshape(-1), norm).double()
        if not device:
            return None, f64
        st = ops.GramActState(ops.GramActPrepared(d(xs)), d(ref), None if b is None else d(b), d(Ws), d(sw), d(zw), bits, bits, P)

        def make():
            fn = lambda s, z, t, tail=None: st.score(s, z, norm, tail=tail)
            fn.fused_tail = True
            return fn
        return make, f64
    f, r, (scale, zp, delta) = _edge_factors(lambda f_: search.activation_grid(d(x * f_).view(T // tok, tok, K), bits, P, False),
                                             lambda f_: problem(f_, device=False)[1], 0)
    make, f64 = problem(f * r)
    return Case(make=make, scale=scale, zp=zp, delta=delta, clamp=CLAMP, f64=f64, tol=3e-6, cols=[0], kernel="k_gram_act<i8>", clamp_col=0)


def _linear_layer(I, Oc, T, N, bits, seed, x_mul=1.0):
    """a Linear layer with captured tensors and both quantisers set, as test_finish_topk_next_fused_equals_two_launches builds it;
    x_mul: the input times x_mul against the weight over x_mul (same outputs)"""
    from adalog_amd import quant_layers as Q
    gen = g(seed)
    x = torch.randn(N, T, I, generator=gen) * 1.3 * x_mul
    W = torch.randn(Oc, I, generator=gen) * 0.05 / x_mul
    b = torch.randn(Oc, generator=gen) * 0.1
    lay = Q.AsymmetricallyBatchingQuantLinear(I, Oc, True, "raw", bits, bits, calib_batch_size=N, search_round=1, eq_n=P, n_V=1,
                                              fpcs=True, steps=6).to(DEV)
    lay.weight.data.copy_(W)
    lay.bias.data.copy_(b)
    lay.raw_input = x.to(DEV)
    lay.raw_out = torch.nn.functional.linear(lay.raw_input, lay.weight.data, lay.bias.data)
    qmax = 2 ** bits - 1
    a_s = torch.tensor([x.abs().max().item() * 2 / qmax])
    a_z = torch.tensor([float(2 ** (bits - 1))])
    w_lo, w_hi = W.min(1).values, W.max(1).values
    w_s = (w_hi - w_lo) / qmax
    w_z = torch.round(-w_lo / w_s).clamp(0, qmax)
    for q, sc, zp_ in ((lay.a_quantizer, a_s, a_z), (lay.w_quantizer, w_s, w_z)):
        q.scale.data.copy_(sc.reshape(q.scale.shape))
        q.zero_point.data.copy_(zp_.reshape(q.zero_point.shape))
        q.inited = True
        q._zp_on_grid = True
    return lay, x.reshape(-1, I), W, b, lay.raw_out.reshape(-1, Oc).cpu(), (a_s, a_z, w_s, w_z)


def _case_pend_w(ops):
    """output-MSE weight search through gemm_score(defer=True): [128, 96] scores from per-column partials"""
    from adalog_amd import search
    I, Oc, T, N, bits = 128, 96, 50, 4, 4
    lay, x2, W, b, ref, (a_s, a_z, _, _) = _linear_layer(I, Oc, T, N, bits, 31)
    with torch.no_grad():
        fixed = lay._pack_x_fixed()
    scale, zp, delta = search.weight_grid(lay._w2(), bits, P)
    xq = _fq_int(x2, a_s, a_z, bits)                                                     # [tokens, I]
    r = (ref - b.view(1, -1)).double()

    def f64(s, z, t, cols):
        out = []
        for c in cols:
            wq = _fq_int(W[c].view(1, -1), s[:, c].view(-1, 1), z[:, c].view(-1, 1), bits)       # [P, I]
            sim = (xq @ wq.t()) * (s[:, c].double() * a_s.double()).view(1, -1)                      # [tokens, P]
            out.append(-(1.0 / T) * ((r[:, c].view(-1, 1) - sim) ** 2).sum(0))
        return torch.stack(out, 1)

    def make():
        def fn(s, z, t):
            with torch.no_grad():
                return lay._score_w(fixed, s, z, defer=True)
        return fn
    return Case(make=make, scale=scale, zp=zp, delta=delta, f64=f64, tol=2e-6, cols=[0, 1, 47, 95], pend_mode=(1,), route="pend", keep=lay)


def _case_pend_a(ops):
    """per-tensor output-MSE activation search through score_act_gen(defer=True): per-workgroup accumulators, the last block ranks"""
    from adalog_amd import search
    I, Oc, T, N, bits = 128, 256, 50, 4, 4

    def problem(f):
        lay, x2, W, b, ref, (_, _, w_s, w_z) = _linear_layer(I, Oc, T, N, bits, 32, x_mul=f)
        wq = _fq_int(W, w_s.view(-1, 1), w_z.view(-1, 1), bits) * w_s.double().view(-1, 1)            # [Oc, I]
        r_ = (ref - b.view(1, -1)).double()

        def f64(s, z, t, cols):
            out = []
            for p_ in range(s.shape[0]):
                sim = (_fq_int(x2, s[p_, 0], z[p_, 0], bits) @ wq.t()) * float(s[p_, 0])
                out.append(-(1.0 / (T * Oc)) * ((r_ - sim) ** 2).sum())
            return torch.stack(out).view(-1, 1)
        return lay, f64
    f, r, (scale, zp, delta) = _edge_factors(lambda f_: search.activation_grid(problem(f_)[0].raw_input, bits, P, False),
                                             lambda f_: problem(f_)[1], 0)
    lay, f64 = problem(f * r)
    with torch.no_grad():
        dt = lay._int_dt(N * T, prefer_fp8=True)
        wp = lay._pack_w_fixed(dt)
        wp.int_dt = dt
    assert ops.score_act_gen_ok(dt, Oc, N * T, I, wp.shape[-1], P)

    def make():
        def fn(s, z, t):
            with torch.no_grad():
                return lay._score_a(wp, s, z, defer=True)
        return fn
    return Case(make=make, scale=scale, zp=zp, delta=delta, clamp=CLAMP, f64=f64, tol=1e-4, cols=[0], pend_mode=(2,), route="pend", keep=lay,
                kernel=("k_gemm_slab_gen<", "k_gemm_slab128_gen<"), clamp_col=0)


def _case_pend_mm(ops):
    """per-head q . k^T search of the A operand (cols = H = 3) at (N, H, S, D) = (4, 3, 50, 32): PendingScores from the attention scorer"""
    from adalog_amd import quant_layers as Q, search
    from adalog_amd.ops import I8, pad_k
    N, H, S, D, bits = 4, 3, 50, 32, 4
    gen = g(33)
    A = torch.randn(N, H, S, D, generator=gen) * (0.5 + torch.rand(1, H, 1, 1, generator=gen))
    Bt = torch.randn(N, H, S, D, generator=gen)
    mm = Q.AsymmetricallyBatchingQuantMatMul(A_bit=bits, B_bit=bits, mode="raw", calib_batch_size=N, search_round=1, eq_n=P,
                                             head_channel_wise=True, num_heads=H, fpcs=True, steps=6).to(DEV)
    Bd = Bt.to(DEV).transpose(-2, -1)
    mm.raw_input, mm.raw_out = [A.to(DEV), Bd], A.to(DEV) @ Bd
    mm._initialize_calib_parameters()
    qmax = 2 ** bits - 1
    sA, sB = A.abs().amax((0, 2, 3)) * 2 / qmax, Bt.abs().amax((0, 2, 3)) * 2 / qmax
    z8 = torch.full((H,), float(2 ** (bits - 1)))
    for q, sc in ((mm.A_quantizer, sA), (mm.B_quantizer, sB)):
        q.scale.data.copy_(sc.reshape(q.scale.shape).to(DEV))
        q.zero_point.data.copy_(z8.reshape(q.zero_point.shape).to(DEV))
        q.inited = True
        q._zp_on_grid = True
    with torch.no_grad():
        # (the operand storage type the layer's own search picks: matmul.py's hyperparameter_searching)
        G_, S_, K_, Sp_ = mm._dims()
        dtm = search.int_operand_dtype(bits, bits, mm._cand_chunk(G_ * max(S_, Sp_) * pad_k(K_, I8)), prefer_fp8=K_ <= 64)
        fixed_b = mm._pack_fixed("B", dtm)
    scale, zp, delta = search.matmul_grid(mm.raw_input[0], bits, P, True)
    ref = mm.raw_out.cpu().double()                                                                   # [N, H, S, S]
    bq = _fq_int(Bt, sB.view(1, H, 1, 1), z8.view(1, H, 1, 1), bits) * sB.double().view(1, H, 1, 1)   # [N, H, S', D]

    def f64(s, z, t, cols):
        out = []
        for h in cols:
            col = []
            for p_ in range(s.shape[0]):
                aq = _fq_int(A[:, h], s[p_, h], z[p_, h], bits) * float(s[p_, h])                     # [N, S, D]
                col.append(-(1.0 / (S * S)) * ((ref[:, h] - aq @ bq[:, h].transpose(-2, -1)) ** 2).sum())
            out.append(torch.stack(col))
        return torch.stack(out, 1)

    def make():
        def fn(s, z, t):
            with torch.no_grad():
                return mm._score("A", fixed_b, s, z, dtm, defer=True)
        return fn
    return Case(make=make, scale=scale, zp=zp, delta=delta, f64=f64, tol=2e-6, cols=[0, 1, 2], pend_mode=(2,), route="pend", keep=mm)


def _case_postgelu(ops):
    """the post-GELU form: search.fpcs(scale, None, qv, ...) with width 32 (4 neighbours) and the fused AdaLog activation scorer at
    (I, Oc, T, N) = (256, 96, 31, 2); plain scores, so every step ends in k_topk_next with a third plane and no zero point.
    tol: no kernel test compares score_act_fused with a specification (tests/test_gpu_kernels.py:1184 is kernel against kernel), so
    it is twice the largest relative gap between oracle.score_postgelu evaluated in fp64 and in fp32 on this input's first grid,
    measured on the CPU: 1.74e-6 -> 3.5e-6."""
    from oracle import adalog_oracle as O
    from adalog_amd import backend
    from adalog_amd.ops import BF16
    from adalog_amd import quant_layers as Q
    I, Oc, T, N, bits = 256, 96, 31, 2, 4
    gen = g(77)
    x = torch.nn.functional.gelu(2.0 * torch.randn(N, T, I, generator=gen))
    W = torch.randn(Oc, I, generator=gen) * 0.03
    b = torch.randn(Oc, generator=gen) * 0.1
    lay = Q.PostGeluLogBasedBatchingQuantLinear(I, Oc, True, "raw", bits, bits, calib_batch_size=N, search_round=1, eq_n=P, n_V=1,
                                                quantizer="adalog", fpcs=True, steps=6).to(DEV)
    lay.weight.data.copy_(W)
    lay.bias.data.copy_(b)
    lay.raw_input, lay.raw_out = x.to(DEV), torch.nn.functional.linear(x, W, b).to(DEV)
    lay.w_quantizer.scale.data.fill_(float(W.abs().max()) / 7.0)
    lay.w_quantizer.zero_point.data.fill_(float(2 ** (bits - 1)))
    lay.w_quantizer.inited = True
    # the first grid as activation_fpcs lays it out: 16 scales x 8 log bases
    hi = float(x.max()) + float(torch.tensor(0.16997124254703522, dtype=torch.float32))
    scs = d(torch.linspace(0.55 * hi, hi, 16).repeat(8).view(-1, 1))
    qs = d(torch.tensor([13., 23., 31., 37., 45., 60., 90., 137.]).repeat_interleave(16).view(-1, 1))
    be = backend.get()
    aq = lay.a_quantizer
    with torch.no_grad():
        wp, rowsum = lay._pack_w_fixed(BF16, want_rowsum=True)
        fold = be.shift_fold(rowsum.view(1, -1), lay.w_quantizer.scale.data.view(1, -1), aq.shift.data, lay.bias.data).view(-1)
    assert be.score_act_fused_ok(Oc, N * T, I, wp.shape[-1], P, bits)
    delta = (scs[1] - scs[0]).view(1).contiguous()
    x, W, b = lay.raw_input.cpu().double(), lay.weight.data.cpu(), lay.bias.data.cpu().double()
    w_q = O.uniform_fake_quant(W, lay.w_quantizer.scale.data.cpu().view(-1)[0], lay.w_quantizer.zero_point.data.cpu().view(-1)[0], bits)[0].double()
    ref, shift, table = lay.raw_out.cpu().double(), float(aq.shift.data.reshape(-1)[0]), O.search_table(bits).double()
    f64 = lambda s, z, t, cols: O.score_postgelu(x, w_q, b, ref, s.double().view(1, -1), t.double().view(1, -1), shift, bits, table).reshape(-1, 1)

    def make():
        def fn(s, z, t):
            with torch.no_grad():
                return lay._score_scale_logbase(wp, fold, s, t, defer=True)
        return fn
    return Case(make=make, scale=scs, zp=None, third=qs, delta=delta, width=32, f64=f64, tol=3.5e-6, cols=[0], route="topk", keep=lay)


GRAM = [(1568, 100, 64), (1000, 200, 96)]
CASES = {"plain": _case_plain, "sorted_rows": lambda o: _case_sorted(o, "rows"), "sorted_tensor": lambda o: _case_sorted(o, "tensor"),
         "sorted_channel": lambda o: _case_sorted(o, "channel"), "pend_w": _case_pend_w, "pend_a": _case_pend_a, "pend_mm": _case_pend_mm, "postgelu": _case_postgelu}
for _T, _O, _K in GRAM:
    for _b in (3, 4, 6):
        CASES["gram_w_%dx%dx%d_b%d" % (_T, _O, _K, _b)] = lambda o, a=(_T, _O, _K, _b): _case_gram_w(o, *a)
        CASES["gram_a_%dx%dx%d_b%d" % (_T, _O, _K, _b)] = lambda o, a=(_T, _O, _K, _b): _case_gram_a(o, *a)


# ------------------------------------------------------------------------------------------------ the checks
class _Run:
    """one search.fpcs call with everything around it recorded"""

    def __init__(self, ops, monkeypatch, case, steps=6, fused=True, commit="params", spy=True):
        from adalog_amd import search
        cols = case.scale.shape[1]
        log = self.tails = []

        class RecTail(ops.FpcsTail):                       # the driver takes the class from the backend at every call
            def __init__(self, scale, zp, third, k, new_cnt, lin, delta_in, delta_out, clamp_min, out=None):
                super().__init__(scale, zp, third, k, new_cnt, lin, delta_in, delta_out, clamp_min, out=out)
                log.append((new_cnt, None if delta_in is None else delta_in.data_ptr(), None if delta_out is None else delta_out.data_ptr(), out))
        calls = self.calls = {"topk_next": 0, "finish_topk_next": 0}

        def counted(name, f):
            def w(*a, **kw):
                calls[name] += 1
                return f(*a, **kw)
            return w
        mk = lambda have: None if have is None else torch.nn.Parameter(torch.full((cols,), -7.0, device=DEV))
        if commit == "strided":
            # storage the last kernel cannot write: every other element of a buffer; with one column (where any view is contiguous) fp64
            mk = lambda have: None if have is None else torch.nn.Parameter(
                torch.full((cols, 2), -7.0, device=DEV)[:, 0] if cols > 1 else torch.full((1,), -7.0, device=DEV, dtype=torch.float64))
        self.params = (mk(case.scale), mk(case.zp), mk(case.third))
        self.targets = search.commit_targets(*self.params) if commit != "fresh" else None
        fn = case.make()
        self.spy = FR.Spy(fn) if spy else None
        self.kernels = []
        if spy and case.kernel:
            inner = self.spy.fn

            def noting(*a, **kw):
                r = inner(*a, **kw)
                self.kernels.append(_last_kernel())
                return r
            self.spy.fn = noting
        with monkeypatch.context() as mp:
            mp.setattr(ops, "FpcsTail", RecTail)
            mp.setattr(ops, "topk_next", counted("topk_next", ops.topk_next))
            mp.setattr(ops, "finish_topk_next", counted("finish_topk_next", ops.finish_topk_next))
            mp.setattr(search, "FUSED_TAIL", fused)
            self.res = search.fpcs(case.scale, case.zp, case.third, case.delta, self.spy or fn, steps, case.width, P, case.clamp,
                                   commit_to=self.targets)
            torch.cuda.synchronize()

    def replay(self, case):
        return FR.replay(self.spy.steps, case.delta, case.width, P, case.clamp, self.res, first=(case.scale, case.zp, case.third))


def _same_steps(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for name in ("scale", "zp", "third", "scores"):
            assert FR.bits_equal(getattr(x, name), getattr(y, name)), "call %d: %s differs" % (i, name)


def _same_commit(a, b):
    for x, y in zip(a, b):
        assert FR.bits_equal(x, y)


def _check_ranking(case, steps):
    """item 6 of the file's docstring: the device's survivors are the best candidates of the fp64 objective, within the scorer's tolerance"""
    for i, st in enumerate(steps):
        k = 1 if i == len(steps) - 1 else case.width
        top = FR.rank(st.scores, k)
        ref = case.f64(st.scale, st.zp, st.third, case.cols)                     # [P, len(cols)] fp64
        for j, c in enumerate(case.cols):
            kth = ref[top[k - 1, c], j]
            out = torch.ones(P, dtype=torch.bool)
            out[top[:, c]] = False
            worst = ref[out, j].max()
            gap, margin = float(worst - kth), 2 * case.tol * abs(float(kth))
            print("step %d col %d: best left out - k-th survivor = %.3e (margin %.3e, score %.6e)" % (i, c, gap, margin, float(kth)))
            assert gap <= margin, (i, c, gap, margin)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fpcs_route(ops, monkeypatch, name):
    from adalog_amd import search
    case = CASES[name](ops)
    cols = case.scale.shape[1]
    before = [None if t is None else t.clone() for t in (case.delta, case.scale, case.zp, case.third)]
    d_ptr = case.delta.data_ptr()

    # 1. replay: grids, copied planes, spacing chain, committed winner -- bit for bit
    run = _Run(ops, monkeypatch, case)
    want = run.replay(case)
    assert len(run.spy.steps) == 6
    # the route that ran
    if case.route == "fused":
        assert all(t is not None for t in [st.delta_in for st in run.spy.steps[:-1]])          # every call was handed its tail
        assert run.calls["finish_topk_next"] == 0
        assert run.calls["topk_next"] == (6 if name == "plain" else 0)                        # (honour_tail's launch | the scorer's own)
    elif case.route == "pend":
        assert all(isinstance(r, ops.PendingScores) and r.mode in case.pend_mode for r in run.spy.returned), [r.mode for r in run.spy.returned]
        assert run.calls == {"topk_next": 0, "finish_topk_next": 6}
    else:
        assert all(torch.is_tensor(r) for r in run.spy.returned) and run.calls == {"topk_next": 6, "finish_topk_next": 0}
    if case.kernel:
        assert run.kernels and all(k_.startswith(case.kernel) for k_ in run.kernels), run.kernels
    # the planted edges occurred
    if getattr(case, "tie", None):
        a, b, c = case.tie
        s0 = run.spy.steps[0].scores
        assert FR.bits_equal(s0[a, c].view(1), s0[b, c].view(1))
        top0 = FR.rank(s0, case.width)[:, c].tolist()
        assert (a in top0) != (b in top0) and min(a, b) in top0, (a, b, top0)          # the tie straddles the boundary: lower index in
    if case.clamp is not None:
        assert _clamp_hits(run.spy.steps, case.delta, case.width, case.clamp, case.clamp_col) > 0
    if case.nan_at:
        i, r, c = case.nan_at
        assert torch.isnan(run.spy.steps[i].scores[r, c]) and bool((run.spy.steps[i + 1].zp[:8, c] == run.spy.steps[i].zp[r, c]).all())
    # the spacing: read from the caller's tensor once, then narrowed in ONE private buffer that is delta_in and delta_out
    exp, last = run.tails[:-1], run.tails[-1]
    assert len(run.tails) == 6 and [t[0] for t in exp] == [P // case.width] * 5 and last[0] == 0
    assert exp[0][1] == d_ptr and all(t[1] == exp[0][2] for t in exp[1:]) and all(t[2] == exp[0][2] != d_ptr for t in exp)
    assert last[3] is run.targets and run.targets is not None

    # 4a. commit_to: the winner is IN the parameters' storage
    for r_, p_, w_ in zip(run.res, run.params, want):
        assert (r_ is None) == (p_ is None)
        if r_ is not None:
            assert r_.data_ptr() == p_.data_ptr() and FR.bits_equal(p_.data, w_)

    # 2. the switch, and 4b. commit_to=None: fresh tensors, same bits; 3. a second search from the same tensors
    off = _Run(ops, monkeypatch, case, fused=False, commit="fresh")
    _same_steps(run.spy.steps, off.spy.steps)
    _same_commit(run.res, off.res)
    assert off.calls["topk_next"] + off.calls["finish_topk_next"] == 6
    assert all(r_ is None or r_.data_ptr() not in [p_.data_ptr() for p_ in off.params if p_ is not None] for r_ in off.res)
    assert all(p_ is None or bool((p_.data == -7.0).all()) for p_ in off.params)
    # 4c. a non-contiguous parameter: no in-place commit, commit_param copies
    nc = _Run(ops, monkeypatch, case, commit="strided", spy=False)
    assert nc.targets is None
    for r_, p_, w_ in zip(nc.res, nc.params, want):
        if r_ is not None:
            assert bool((p_.data == -7.0).all())
            search.commit_param(p_, r_)
            assert FR.bits_equal(p_.data.float().contiguous(), w_)

    # 3. nothing the caller passed in was written
    for t, b in zip((case.delta, case.scale, case.zp, case.third), before):
        assert FR.bits_equal(t, b)

    # 5. steps
    one = _Run(ops, monkeypatch, case, steps=1)
    assert one.res is None and len(one.spy.steps) == 1 and one.tails == []
    assert all(p_ is None or bool((p_.data == -7.0).all()) for p_ in one.params)
    two = _Run(ops, monkeypatch, case, steps=2)
    assert len(two.spy.steps) == 2 and [t[0] for t in two.tails] == [P // case.width, 0]
    assert [t[1] for t in two.tails].count(d_ptr) == 1 and two.tails[0][2] != d_ptr
    two.replay(case)
    _same_steps(two.spy.steps, run.spy.steps[:2])
    four = _Run(ops, monkeypatch, case, steps=4)                                    # the conv form
    assert len(four.spy.steps) == 4
    four.replay(case)
    for t, b in zip((case.delta, case.scale, case.zp, case.third), before):
        assert FR.bits_equal(t, b)

    # 6. the ranking is right in high precision
    _check_ranking(case, run.spy.steps)
