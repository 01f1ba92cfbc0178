"""Host code that decides which scoring kernel a layer search runs (quant_layers/linear.py, matmul.py, conv.py and the part of
search.py they talk to), on the stand-in kernels of tests/cpu_backend.py and the smallest layer shapes of tests/layer_cases.py:

* search.search_scope: a search that raises in the middle of hyperparameter_searching leaves no memo entry, no round snapshot and no
  address-keyed cache behind, and neither marks the module calibrated nor drops its captures;
* the chunked pack-and-score loop (score_chunks) at each of its six sites: 128 candidates in chunks of 48, 48 and a ragged 32 score
  bit for bit what one launch scores, and never defer their partial sums;
* search.Scorer: what _w_scorer() / _a_scorer() return, and the fields search.fpcs reads from the Gram and self-MSE scorers.
"""
import pytest
import torch

from adalog_amd import backend, search
from adalog_amd import quant_layers as Q
from adalog_amd.quant_layers import conv as CV, linear as LN, matmul as MM
from tests import cpu_backend as CB

P = 128


@pytest.fixture(autouse=True)
def _cpu_backend():
    backend.set_backend(CB)
    yield
    backend.set_backend(None)


def _rand(*shape, seed=0, mul=1.0, add=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * mul + add


def _linear(cls=Q.AsymmetricallyBatchingQuantLinear, dims=(6, 5, 24, 16), **kw):
    """layer_cases' linear_w4a4_ragged shape (postgelu: its postgelu_w4a4 shape), captures in place"""
    N, T, I, O = dims
    lay = cls(I, O, True, "raw", 4, 4, calib_batch_size=2, search_round=2, eq_n=P, n_V=1, fpcs=True, steps=2, **kw)
    x = _rand(N, T, I, seed=1)
    if cls is Q.PostGeluLogBasedBatchingQuantLinear:
        x = torch.nn.functional.gelu(x)
    with torch.no_grad():
        lay.raw_input, lay.raw_out = x, lay(x)
    return lay


def _postgelu():
    return _linear(Q.PostGeluLogBasedBatchingQuantLinear, (4, 7, 40, 24), quantizer="adalog")


def _matmul(cls=Q.AsymmetricallyBatchingQuantMatMul, S=7, **kw):
    """layer_cases' matmul_a4b4 (q.k^T: B is a transposed view) / postsoftmax_a4b4 shapes"""
    N, H, C = 4, 2, 8
    lay = cls(A_bit=4, B_bit=4, mode="raw", calib_batch_size=2, search_round=2, eq_n=P, head_channel_wise=True, num_heads=H,
              fpcs=True, steps=2, **kw)
    if cls is Q.PostSoftmaxAsymmetricallyBatchingQuantMatMul:
        A, B = _rand(N, H, S, S, seed=2).softmax(-1), _rand(N, H, S, C, seed=3)
    else:
        A, B = _rand(N, H, S, C, seed=2, mul=1.7), _rand(N, H, S, C, seed=3, mul=0.9, add=0.2).transpose(-2, -1)
    with torch.no_grad():
        lay.raw_input, lay.raw_out = [A, B], lay(A, B)
    return lay


def _postsoftmax():
    return _matmul(Q.PostSoftmaxAsymmetricallyBatchingQuantMatMul, S=9, quantizer="adalog")


def _conv():
    lay = Q.AsymmetricallyBatchingQuantConv2d(in_channels=3, out_channels=12, kernel_size=(4, 4), stride=(4, 4), mode="raw", w_bit=4,
                                              a_bit=8, calib_batch_size=2, search_round=2, eq_n=P, fpcs=True, steps=2)
    x = _rand(4, 3, 16, 16, seed=4)
    with torch.no_grad():
        lay.raw_input, lay.raw_out = x, lay(x)
    return lay


def _init_linear(lay):
    """both quantisers at candidate [-2] of their percentile grids (not committed FPCS winners: the token-form routes serve them)"""
    ws, wz, _ = search.weight_grid(lay._w2(), lay.w_quantizer.n_bits, P)
    lay.w_quantizer.scale.data.copy_(ws[-2].view(lay.w_quantizer.scale.shape))
    lay.w_quantizer.zero_point.data.copy_(wz[-2].view(lay.w_quantizer.zero_point.shape))
    lay.w_quantizer.inited = True
    aq = lay.a_quantizer
    if hasattr(aq, "zero_point"):
        s, z, _ = search.activation_grid(lay.raw_input, aq.n_bits, P, False)
        aq.scale.data.copy_(s[-2].view(aq.scale.shape))
        aq.zero_point.data.copy_(z[-2].view(aq.zero_point.shape))
    else:
        aq.scale.data.copy_(lay.calculate_percentile_activation_candidates()[1][:, -2])
    aq.inited = True
    return ws, wz


# ------------------------------------------------------------------------------------------------ search scope
class Boom(Exception):
    pass


def _fail_at(monkeypatch, lay, n_fail):
    """the n_fail-th scoring call that search.fpcs makes raises Boom; -> what was cached at that moment"""
    real, n, seen = search.fpcs, [0], {}

    def fpcs(scale, zp, third, delta, score_fn, *a, **k):
        def fn(*sa, **sk):
            n[0] += 1
            if n[0] == n_fail:
                seen.update(memo=len(search._memo_dict()), rounds=len(lay.__dict__["_round_inputs"]))
                raise Boom()
            return score_fn(*sa, **sk)
        for attr in ("fused_tail", "global_scores"):
            if hasattr(score_fn, attr):
                setattr(fn, attr, getattr(score_fn, attr))
        return real(scale, zp, third, delta, fn, *a, **k)
    monkeypatch.setattr(search, "fpcs", fpcs)
    return seen


# (class, scoring call that raises -- with steps = 2 every fpcs call scores twice --, the address-keyed caches of the class)
SCOPE_CASES = {
    "linear": (_linear, 6, ("_ref_t", "_ref_t_key")),                               # in the activation search of round 1
    "postgelu": (_postgelu, 6, ("_ref_t", "_ref_t_key", "_lx", "_lx_key")),         # in the weight search of round 1
    "matmul": (_matmul, 4, ("_ref_t", "_ref_t_key", "_bt_c", "_bt_key")),           # in the B search of round 1
    "postsoftmax": (_postsoftmax, 2, ("_ref_t", "_ref_t_key", "_bt_c", "_bt_key")),  # in the B search of round 1
}


@pytest.mark.parametrize("name", list(SCOPE_CASES))
def test_search_that_raises_leaves_no_cache_behind(monkeypatch, name):
    make, n_fail, caches = SCOPE_CASES[name]
    lay = make()
    raw_input, raw_out = lay.raw_input, lay.raw_out
    seen = _fail_at(monkeypatch, lay, n_fail)
    with torch.no_grad(), pytest.raises(Boom):
        lay.hyperparameter_searching()
    assert seen["memo"] > 0 and seen["rounds"] > 0                 # (the search had cached something when it raised)
    assert len(search._memo_dict()) == 0
    assert lay.__dict__["_round_inputs"] == {}
    for c in caches:
        assert getattr(lay, c, None) is None, c
    assert lay.calibrated is False
    assert lay.raw_input is raw_input and lay.raw_out is raw_out


def test_search_that_ends_calibrates_and_releases_the_captures():
    lay = _linear()
    with torch.no_grad():
        lay.hyperparameter_searching()
    assert lay.calibrated is True and not hasattr(lay, "raw_input") and not hasattr(lay, "raw_out")
    assert len(search._memo_dict()) == 0 and lay.__dict__["_round_inputs"] == {} and lay._ref_t is None and lay._ref_t_key is None


# ------------------------------------------------------------------------------------------------ chunk loop
def _site_linear_w(lay=None):
    lay = lay or _linear()
    ws, wz = _init_linear(lay)
    return LN, lambda defer: lay._score_w(lay._pack_x_fixed(), ws, wz, defer=defer)


def _site_linear_w_shifted():
    return _site_linear_w(_postgelu())                                # (the bf16 activation image and the folded shift)


def _site_linear_a():
    lay = _linear()
    _init_linear(lay)
    s, z, _ = search.activation_grid(lay.raw_input, lay.a_quantizer.n_bits, P, False)
    return LN, lambda defer: lay._score_a(lay._pack_w_fixed(), s, z, defer=defer)


def _site_postgelu():
    lay = _postgelu()
    _init_linear(lay)
    wp, rowsum = lay._pack_w_fixed(LN.BF16, want_rowsum=True)
    fold = CB.shift_fold(rowsum.view(1, -1), lay.w_quantizer.scale.data.view(1, -1), lay.a_quantizer.shift.data, lay.bias.data).view(-1)
    s = lay.calculate_percentile_activation_candidates()[1].reshape(-1, 1).contiguous()
    q = torch.arange(10, 10 + P, dtype=torch.float32).view(-1, 1)
    return LN, lambda defer: lay._score_scale_logbase(wp, fold, s, q, defer=defer)


def _site_matmul(which):
    def site():
        lay = _matmul()
        lay._init_from_grid("A")
        lay._init_from_grid("B")
        s, z, _ = search.matmul_grid(lay.raw_input[0 if which == "A" else 1], 4, P, True)
        # (the fixed operand is packed inside: its row padding follows the chunking, _kalign)
        return MM, lambda defer: lay._score(which, lay._pack_fixed("B" if which == "A" else "A"), s, z, defer=defer)
    return site


def _site_postsoftmax():
    lay = _postsoftmax()
    lay._init_from_grid("B")
    return MM, lambda defer: lay._score_A_log_base()[1]


def _site_conv():
    lay = _conv()
    patches, gh, gw = lay._patches(lay.raw_input)
    M = patches.shape[0]
    xp = lay._pack_x(patches)
    ref = lay.raw_out.permute(1, 0, 2, 3).reshape(1, lay.out_channels, M).contiguous()
    s, z, _ = search.weight_grid(lay._w2(), 4, P, conv=True)
    return CV, lambda defer: lay._score_w(xp, ref, M, gh * gw, s, z, defer=defer)


CHUNK_SITES = {"Linear._score_w": _site_linear_w, "Linear._score_w[shift]": _site_linear_w_shifted, "Linear._score_a": _site_linear_a,
               "PostGelu._score_scale_logbase": _site_postgelu, "MatMul._score[A]": _site_matmul("A"),
               "MatMul._score[B]": _site_matmul("B"), "PostSoftmax._score_A_log_base": _site_postsoftmax, "Conv._score_w": _site_conv}


def _budget_for_chunk(monkeypatch, mod, call, want):
    """the smallest MAX_PACK_BYTES at which the site's own chunk-size formula gives ``want`` candidates per launch (the formula is
    monotone in the budget; the scoring itself is skipped while bisecting)"""
    class Stop(Exception):
        pass

    def probe(P_, chunk, *a):
        raise Stop(chunk)

    def chunk_at(budget):
        with monkeypatch.context() as m:
            m.setattr(mod, "MAX_PACK_BYTES", budget)
            m.setattr(mod, "score_chunks", probe)
            try:
                call(False)
            except Stop as e:
                return e.args[0]
    lo, hi = 1, 1 << 30
    assert chunk_at(lo) < want <= chunk_at(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if chunk_at(mid) < want else (lo, mid)
    return hi


@pytest.mark.parametrize("name", list(CHUNK_SITES))
def test_chunked_scores_equal_one_launch(monkeypatch, name):
    # the routes that generate their candidates inside the kernel take whole calls only: the packed loop is what is under test
    monkeypatch.setattr(LN, "GEN_W_SEARCH", False)
    monkeypatch.setattr(LN, "GEN_ACT_SEARCH", False)
    monkeypatch.setattr(MM, "GEN_MM", "0")
    monkeypatch.setattr(MM, "GEN_AVQ", False)
    mod, call = CHUNK_SITES[name]()
    want = call(False)
    assert isinstance(want, torch.Tensor) and want.shape[0] == P
    real, launches = mod.score_chunks, []

    def spy(P_, chunk, defer, planes, score):
        def counted(n, d, *pl):
            launches.append((n, d))
            return score(n, d, *pl)
        return real(P_, chunk, defer, planes, counted)
    monkeypatch.setattr(mod, "MAX_PACK_BYTES", _budget_for_chunk(monkeypatch, mod, call, 48))
    monkeypatch.setattr(mod, "score_chunks", spy)
    got = call(True)
    assert launches == [(48, False), (48, False), (32, False)]              # ragged last chunk, nothing deferred
    assert isinstance(got, torch.Tensor) and not isinstance(got, CB.PendingScores)
    assert got.shape == want.shape and torch.equal(got, want)
    # ... and one launch that takes all candidates defers where it is asked to (the sites with a ``defer``)
    monkeypatch.setattr(mod, "MAX_PACK_BYTES", 1 << 40)
    del launches[:]
    whole = call(True)
    assert launches == [(P, name != "PostSoftmax._score_A_log_base")]
    assert torch.equal(whole.finish() if isinstance(whole, CB.PendingScores) else whole, want)


def test_mixed_softmax_v_search_refuses_chunks(monkeypatch):
    lay = _postsoftmax()
    lay._init_from_grid("B")
    s, z, _ = search.matmul_grid(lay.raw_input[1], 4, P, True)
    ap = lay._pack_A_adalog(lay._a3(lay.raw_input[0]), search.const_tensor([37.0], s.device), lay.A_quantizer.scale.data.view(-1), 1, True,
                            k_align=64)
    monkeypatch.setattr(MM, "MAX_PACK_BYTES", 1 << 10)
    with pytest.raises(RuntimeError):
        lay._score("B", ap, s, z, MM.BF16_FP8)


# ------------------------------------------------------------------------------------------------ scorers
def test_w_scorer_and_a_scorer_are_the_packed_scoring_calls():
    lay = _linear()
    ws, wz = _init_linear(lay)
    score = lay._w_scorer()
    assert isinstance(score, search.Scorer) and score.fused_tail is False and score.global_scores is False
    assert torch.equal(score(ws, wz), lay._score_w(lay._pack_x_fixed(), ws, wz))
    s, z, _ = search.activation_grid(lay.raw_input, lay.a_quantizer.n_bits, P, False)
    score = lay._a_scorer()
    assert isinstance(score, search.Scorer) and score.fused_tail is False and score.global_scores is False
    assert torch.equal(score(s, z), lay._score_a(lay._pack_w_fixed(), s, z))
    pend = lay._w_scorer(defer=True)(ws, wz)
    assert isinstance(pend, CB.PendingScores) and torch.equal(pend.finish(), lay._w_scorer()(ws, wz))


@pytest.mark.parametrize("tails", [False, True])
def test_gram_scorers_are_fused_where_the_backend_has_tails(monkeypatch, tails):
    if tails:
        monkeypatch.setattr(CB, "FpcsTail", object, raising=False)
    lay = _linear(dims=(4, 7, 32, 48))                       # (K a multiple of 32: both Gram forms take the shape)
    _init_linear(lay)
    lay.w_quantizer._zp_on_grid = lay.a_quantizer._zp_on_grid = True
    w = lay._w_scorer(defer=True)
    assert isinstance(w, search.Scorer) and w.fused_tail is tails and w.global_scores is True
    a = lay._a_scorer(defer=True)
    assert isinstance(a, search.Scorer) and a.fused_tail is tails and a.global_scores is False

    class LocalState(CB.GramState):                           # (global_scores is the state's field, not a constant)
        def __init__(self, *args):
            super().__init__(*args)
            self.global_scores = False
    monkeypatch.setattr(CB, "GramState", LocalState)
    w = lay._w_scorer()
    assert w.fused_tail is tails and w.global_scores is False


def test_self_mse_scorers_are_always_fused(monkeypatch):
    lay = _linear()
    _init_linear(lay)
    got = []
    monkeypatch.setattr(search, "fpcs", lambda scale, zp, third, delta, fn, *a, **k: got.append(fn))
    lay.weight_fpcs(steps=2, search_strategy="self")
    lay.activation_fpcs(steps=2, search_strategy="self")
    lay.weight_fpcs(steps=2, search_strategy="output")
    lay.activation_fpcs(steps=2, search_strategy="output")
    assert [type(f) for f in got] == [search.Scorer] * 4
    assert [(f.fused_tail, f.global_scores) for f in got] == [(True, False), (True, False), (False, False), (False, False)]
    ws, wz, _ = search.weight_grid(lay._w2(), 4, P)
    assert got[0](ws, wz).shape == (P, lay.out_features)      # no tail given: none passed on to a backend that has none
