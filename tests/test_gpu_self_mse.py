"""`-m gpu`: the three device scorers of the self-MSE searches -- k_score_sorted behind the prefix build (csrc/sorted_score.hip),
k_score_w_self and k_score_a_self (csrc/search_ops.hip) -- against the long-double reference of tests/self_mse_reference.py on the
case table of tests/self_mse_cases.py.  EVERY SCORE is compared on its own, |got - ref| <= bar(case, candidate, segment); the bars
and their derivations are self_mse_reference.sorted_bar / onepass_bar (the latter never wider than the fp32-accumulation bars act_bar
/ weight_bar, which tests/test_self_mse_cpu.py proves on the CPU stand-ins).  No route is another's reference: where two routes take a case both are held to the reference.

Every case prints its worst err / bar per route (`-s`) and writes it to self_mse_parity.jsonl next to the suite's other parity logs;
DESIGN.md section 2 records the figures.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import self_mse_cases as T
from tests import self_mse_reference as R
from tests.test_gpu_golden_forward import LOG as _GOLDEN_LOG

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOG = os.path.join(os.path.dirname(_GOLDEN_LOG), "self_mse_parity.jsonl")
_log_started = []


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import backend
    backend.set_backend(None)
    return backend.get()


def d(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _log(**row):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a" if _log_started else "w") as f:
        f.write(json.dumps(row) + "\n")
    _log_started.append(1)


def _judge(route, case, got, ref, bar):
    got = got.detach().cpu().double().numpy()
    assert got.shape == ref.score.shape, (route, case.id, got.shape)
    assert np.isfinite(ref.score).all() and np.isfinite(got).all(), (route, case.id)
    err = np.abs(got - ref.score)
    ratio = err / bar
    k = int(ratio.argmax())
    p, seg = divmod(k, got.shape[1])
    worst = dict(ratio=float(ratio.flat[k]), err=float(err.flat[k]), bar=float(bar.flat[k]), ref=float(ref.score.flat[k]), p=p, seg=seg)
    _log(route=route, case=case.id, **worst)
    print(f"{route:7s} {case.id}: worst err / bar {worst['ratio']:.3f} (err {worst['err']:.3e}, bar {worst['bar']:.3e}, score "
          f"{worst['ref']:.3e}) at candidate {p}, segment {seg} [{case.pattern_of(seg)}]")
    return worst


def _run_sorted(ops, case, x, scale, zp):
    sp = ops.sorted_prefix(d(x))
    return sp, ops.score_self_sorted(sp, d(scale), d(zp), case.bits, case.norm)


def _run_act(ops, case, x, scale, zp):
    return ops.score_a_self(d(T.act_view(case, x)), d(scale), d(zp), case.layout == "cw", case.bits, case.norm)


def _run_w(ops, case, x, scale, zp):
    return ops.score_w_self(d(x), d(scale), d(zp), case.bits)


# ------------------------------------------------------------------------------------------------ 4a / 4c: every score, every route
@pytest.mark.parametrize("case", T.ALL_SMALL, ids=repr)
def test_every_score_of_every_route(ops, case):
    x, scale, zp = T.inputs(case)
    ref = T.reference(case)
    assert ops.sorted_prefix_ok(case.S, case.n, case.bits)
    sp, got = _run_sorted(ops, case, x, scale, zp)
    assert np.array_equal(sp.sorted.cpu().numpy(), np.sort(x, axis=1))                     # by value: -0.0 == +0.0
    worst = {"sorted": _judge("sorted", case, got, ref, R.sorted_bar(ref, case.norm))}
    if T.accepts("act", case):
        assert (R.onepass_bar(ref, case.n) <= R.act_bar(ref, case.norm, case.rows, zp, case.n)).all()
        worst["act"] = _judge("act", case, _run_act(ops, case, x, scale, zp), ref, R.onepass_bar(ref, case.n))
    if T.accepts("w", case):
        assert (R.onepass_bar(ref, case.n) <= R.weight_bar(ref, case.n)).all()
        worst["w"] = _judge("w", case, _run_w(ops, case, x, scale, zp), ref, R.onepass_bar(ref, case.n))
    bad = {r: w for r, w in worst.items() if not w["ratio"] <= 1.0}
    assert not bad, (case.id, "worst err / bar per route", {r: round(w["ratio"], 3) for r, w in worst.items()}, bad)


@pytest.mark.parametrize("case", T.SORTED_BIG, ids=repr)
def test_sorted_route_large_segments_and_many_segments(ops, case):
    """one launch each: 258 prefix blocks per segment (two chunks of the block scan's carry loop, a ragged last block), gaussian and
    large-offset; 514 blocks (a third chunk, the first whose carry adds two chunk totals); and as many segments as the entry point
    takes"""
    x, scale, zp = T.inputs(case)
    ref = T.reference(case)
    assert ops.sorted_prefix_ok(case.S, case.n, case.bits)
    _, got = _run_sorted(ops, case, x, scale, zp)
    w = _judge("sorted", case, got, ref, R.sorted_bar(ref, case.norm))
    assert w["ratio"] <= 1.0, (case.id, w)


def test_sorted_route_refuses_one_segment_too_many(ops):
    assert ops.sorted_prefix_ok(T.MAX_SEGMENTS, 8, 3) and not ops.sorted_prefix_ok(T.MAX_SEGMENTS + 1, 8, 3)


def test_weight_route_refusals_are_host_visible(ops):
    """more than 256 candidates, and a row one element past the LDS staging limit: an error the caller sees, no launch"""
    w = torch.zeros(2, 8, device=DEV)
    with pytest.raises(RuntimeError):
        ops.score_w_self(w, torch.ones(T.W_REFUSED_P, 2, device=DEV), torch.zeros(T.W_REFUSED_P, 2, device=DEV), 4)
    w = torch.zeros(1, T.W_REFUSED_I, device=DEV)
    with pytest.raises(RuntimeError):
        ops.score_w_self(w, torch.ones(2, 1, device=DEV), torch.zeros(2, 1, device=DEV), 4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4b: the prefix build on its own
@pytest.mark.parametrize("n", [c.n for c in T.SORTED_N] + [T.SORTED_CARRY.n, T.SORTED_CARRY3.n])
def test_prefix_entries_and_totals(ops, n):
    """sorted == torch.sort bit for bit; every prefix entry, the totals at index n included, within prefix_bar of the exact prefix;
    entry 0 exactly (0, 0).  Segments: gaussian and the large offset (sum x ~ 1000 n, sum x^2 ~ 1e6 n)."""
    rng = np.random.default_rng(n)
    x = np.stack([T.pattern("gauss", n, 4, rng), T.pattern("offset", n, 4, rng)])
    sp = ops.sorted_prefix(d(x))
    want_sorted, want, mass = R.exact_prefix(x)
    got_sorted = sp.sorted.cpu()
    assert torch.equal(got_sorted.view(torch.int32), torch.from_numpy(x).sort(dim=1).values.view(torch.int32))
    assert np.array_equal(got_sorted.numpy(), want_sorted)
    pf = sp.prefix.cpu().numpy()
    assert pf.shape == (2, n + 1, 2) and (pf[:, 0, :] == 0.0).all()
    err, bar = np.abs(pf - want), R.prefix_bar(n, mass)
    ok = err <= bar
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0)
    _log(route="prefix", case=f"n{n}", ratio=float(ratio.max()), totals_ratio=float(ratio[:, n].max()))
    print(f"prefix  n={n}: worst err / bar {ratio.max():.3f}, totals entry {ratio[:, n].max():.3f}")
    assert ok.all(), (n, np.argwhere(~ok)[:4].tolist(), float(ratio.max()))


# ------------------------------------------------------------------------------------------------ NaN
def _nan_case(case, row):
    x, scale, zp = T.inputs(case)
    bad = x.copy()
    seg = 0 if case.layout == "pt" else T.NAN_SEG
    bad[seg, row * case.I + 1 if case.layout == "pt" else row] = np.nan
    return x, bad, scale, zp, seg


@pytest.mark.parametrize("row", T.NAN_ROWS, ids=("full_slab", "partial_slab"))
@pytest.mark.parametrize("case", (T.NAN_ACT, T.NAN_PT, T.NAN_W), ids=repr)
def test_nan_poisons_its_segment_and_no_other(ops, case, row):
    """one NaN in one segment / channel / row: that segment's scores are NaN on every route that takes the case -- in the one-pass
    activation kernel whether the NaN's row lies in a full slab or in the partial last one -- and every other segment's scores are
    bit for bit those of the run without it"""
    x, bad, scale, zp, seg = _nan_case(case, row)
    keep = [s for s in range(case.S) if s != seg]
    routes = {"sorted": lambda a: _run_sorted(ops, case, a, scale, zp)[1]}
    if T.accepts("act", case):
        routes["act"] = lambda a: _run_act(ops, case, a, scale, zp)
    if T.accepts("w", case):
        routes["w"] = lambda a: _run_w(ops, case, a, scale, zp)
    for name, run in routes.items():
        clean, got = run(x).cpu(), run(bad).cpu()
        assert bool(torch.isfinite(clean).all()), name
        assert bool(torch.isnan(got[:, seg]).all()), (name, case.id, row, got[:, seg])
        assert torch.equal(got[:, keep], clean[:, keep]), (name, case.id, row)


# ------------------------------------------------------------------------------------------------ 4d: the tail form
def test_tail_form_leaves_the_scores_untouched(ops):
    from adalog_amd.ops import FpcsTail
    case = T.SORTED_PAIRS[2]                                       # P = 128, S = 1, 4 bits
    x, scale, zp = T.inputs(case)
    sp = ops.sorted_prefix(d(x))
    sc, z = d(scale), d(zp)
    plain = ops.score_self_sorted(sp, sc, z, case.bits, case.norm)
    delta = torch.full((case.S,), 0.01, device=DEV)
    tail = FpcsTail(sc, z, None, 16, 8, torch.linspace(0, 1, 8, device=DEV), delta, torch.empty_like(delta), 1e-4)
    with_tail = ops.score_self_sorted(sp, sc, z, case.bits, case.norm, tail=tail)
    assert torch.equal(plain, with_tail)
    o_s, o_z, _ = tail.result()
    assert o_s.shape == (128, case.S) and bool(torch.isfinite(o_s).all()) and bool(torch.isfinite(o_z).all())


# ------------------------------------------------------------------------------------------------ 4e: determinism
def test_two_runs_give_the_same_bits(ops):
    for case, run in ((T.SORTED_BITS[5], lambda c, *a: _run_sorted(ops, c, *a)[1]), (T.ACT_CASES[-1], lambda c, *a: _run_act(ops, c, *a)),
                      (T.W_CASES[5], lambda c, *a: _run_w(ops, c, *a))):
        args = T.inputs(case)
        assert torch.equal(run(case, *args), run(case, *args)), case.id
    sp1, sp2 = ops.sorted_prefix(d(args[0])), ops.sorted_prefix(d(args[0]))
    assert torch.equal(sp1.prefix, sp2.prefix) and torch.equal(sp1.sorted, sp2.sorted)


# ------------------------------------------------------------------------------------------------ 4f: the routes the layer picks
def _layer(cls_name, I, Oc, x, W, bits):
    from adalog_amd import quant_layers as Q
    lay = getattr(Q, cls_name)(I, Oc, True, "raw", bits, bits, calib_batch_size=x.shape[0], search_round=1, eq_n=128, n_V=1,
                               fpcs=True, steps=6).to(DEV)
    lay.weight.data.copy_(W)
    lay.raw_input = x.to(DEV)
    lay.raw_out = torch.nn.functional.linear(lay.raw_input, lay.weight.data, lay.bias.data)
    return lay


@pytest.mark.parametrize("which", ("weight", "act_per_tensor", "act_channel_wise"))
def test_layer_commits_the_same_winner_on_either_route(ops, which):
    """weight_fpcs / activation_fpcs with search_strategy="self" (the reference's _search_best_w_scale_self / _search_best_a_scale_self
    inside FPCS) once from the sorted prefix and once from the one-pass kernels: the same committed (scale, zero point).

    The one-pass kernels accumulate in fp64 for this: around the optimum the last FPCS grids are finer than fp32 sums of fp32 terms
    resolve (with fp32 accumulation 61 of 64 weight rows and 56 of 96 channels committed different winners on the MI355X, whose exact
    scores differed by at most 3.2e-7 and 8.1e-8 of the score)."""
    from adalog_amd import search
    from adalog_amd.quant_layers import linear as LM
    gen = torch.Generator().manual_seed(4100)
    I, Oc = (192, 64) if which == "weight" else (96, 32)
    x = torch.randn(2, 197, I, generator=gen) * torch.linspace(0.3, 2, I)
    W = torch.randn(Oc, I, generator=gen) * 0.1
    cls = "AsymmetricallyChannelWiseBatchingQuantLinear" if which == "act_channel_wise" else "AsymmetricallyBatchingQuantLinear"
    seen, kept = [], LM.SORTED_SELF_SEARCH
    try:
        for flag in (True, False):
            LM.SORTED_SELF_SEARCH = flag
            lay = _layer(cls, I, Oc, x, W, 4)
            search.forget_grids()
            lay._initialize_calib_parameters()
            search.begin_rounds(lay)
            with torch.no_grad():
                if which == "weight":
                    lay.weight_fpcs(steps=6, search_strategy="self")
                    q = lay.w_quantizer
                else:
                    lay.activation_fpcs(steps=6, search_strategy="self")
                    q = lay.a_quantizer
            from adalog_amd import _lib
            last = _lib.load().adalog_last_kernel().decode()
            seen.append((q.scale.data.clone().cpu(), q.zero_point.data.clone().cpu(), last))
            search.begin_rounds(lay)
            search.forget_grids()
    finally:
        LM.SORTED_SELF_SEARCH = kept
    (s1, z1, _), (s0, z0, _) = seen
    assert bool((s1 > 0).all()) and s1.numel() == {"weight": Oc, "act_per_tensor": 1, "act_channel_wise": I}[which]
    # what the two winners are worth: the reference's score of each, per column, against the fp32 resolution of a score
    seg = {"weight": W, "act_per_tensor": x.reshape(1, -1), "act_channel_wise": x.reshape(-1, I).t()}[which].contiguous().numpy()
    par = np.stack([t.reshape(-1).numpy() for t in (s1, s0)]), np.stack([t.reshape(-1).numpy() for t in (z1, z0)])
    ref = R.score_segments(seg, par[0], par[1], 4, 1.0, stats=False).score                    # [2, columns]
    differ = (par[0][0] != par[0][1]) | (par[1][0] != par[1][1])
    gap = np.abs(ref[0] - ref[1]) / np.abs(ref).max(axis=0)
    print(f"layer {which}: {int(differ.sum())} of {differ.size} columns commit different winners; their reference scores differ by at "
          f"most {gap.max():.3e} of the score (one fp32 rounding of a score: {R.U32:.3e}); scale differs by at most "
          f"{float(((s1 - s0).abs() / s0).max()):.3e} relative")
    _log(route="layer", case=which, differ=int(differ.sum()), columns=int(differ.size), score_gap=float(gap.max()))
    assert torch.equal(s1, s0) and torch.equal(z1, z0), (which, int(differ.sum()), float(gap.max()))
