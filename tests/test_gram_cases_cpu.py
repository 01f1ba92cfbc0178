"""CPU tier of the Gram-form edge tests: the case tables of tests/gram_cases.py and the references of tests/gram_reference.py, which
tests/test_gpu_gram_edges.py holds the kernels of csrc/gram.hip and csrc/gram_act.hip to.

  * the specification cpu_backend.GramState is unchanged by the extension that returns its terms, and agrees with the plain fp64
    token-form sum on every weight case within the bound of ONE rounding of r to 2^-30 of its column maximum
    (gram_reference.weight_selfcheck_bound);
  * the activation reference's terms recombine to its direct fp64 sum, which is cpu_backend.GramActState's;
  * the tables honour adalog_gram_supported / adalog_gram_act_supported, restated in Python (and equal to the library's where it is
    built), reach the launches they claim, and the limb-switch token counts follow from the g_limbs formula.
A ``big`` case is evaluated on a slice of its candidates here (the GPU tier evaluates all of them on the device).
"""
import os

import pytest
import torch

from tests import cpu_backend as CB
from tests import gram_cases as T
from tests import gram_reference as R


def _slice(case, i):
    n = 32 if case.big else case.P
    return i["sc"][:n], i["zp"][:n]


def _weight_ref(case):
    i = T.weight_inputs(case)
    return i, R.WeightRef(i["x"], i["sa"], i["za"], case.a_bits, i["ref"].t().contiguous(), i["bias"])


@pytest.mark.parametrize("case", T.W_CASES, ids=lambda c: c.id)
def test_weight_spec_terms_and_token_form(case):
    i, ref = _weight_ref(case)
    sc, zp = _slice(case, i)
    t = ref.terms(i["W"], sc, zp, case.w_bits, i["norm"])
    spec = CB.GramState(i["x"], i["sa"], i["za"], case.a_bits, i["ref"].t().contiguous(), i["bias"]).score_w(i["W"], sc, zp, case.w_bits,
                                                                                                             i["norm"])
    # the extension holds the specification's own state and scores (its fp64 sum over K may be ordered otherwise: 4 roundings)
    st = CB.GramState(i["x"], i["sa"], i["za"], case.a_bits, i["ref"].t().contiguous(), i["bias"])
    assert torch.equal(st.G, ref.G.to(torch.int64)) and torch.equal(st.c, ref.c.to(torch.int64)) and torch.equal(st.S0, ref.S0)
    assert bool(((t["score"] - spec.double()).abs() <= R.weight_bar(t, i["norm"], c=4)).all())
    assert bool(torch.isfinite(t["score"]).all())
    assert float(t["quad_int_abs"].max()) < 2.0 ** 53, "weight_bar counts the additions of w^T G w as exact"
    tok, tok_abs = ref.token_form(i["W"], sc, zp, case.w_bits, i["norm"])
    bound = R.weight_selfcheck_bound(ref, t, tok, tok_abs, i["norm"])
    worst = float(((t["score"] - tok).abs() / bound.clamp(min=1e-300)).max())
    assert worst <= 1.0, (case.id, worst)
    # ... and that bound is the fixed-point rounding's, not a loose one: 2^-28 of the terms' sum at the most
    assert bool((bound <= 2.0 ** -28 * i["norm"] * (t["S0"] + t["lin2"] + t["quad"] + tok_abs) + 1e-300).all())


def test_expo_columns_are_what_they_claim():
    for case in T.W_EXPO:
        i, ref = _weight_ref(case)
        am = ref.am
        assert float(am[0]) == 8.0 and float(am[1]) == 8.0 - 2.0 ** -21 and float(am[2]) == 2.0 ** -126 and float(am[3]) == 2.0 ** -140
        assert float(am[4]) == 0.0 and float(am[6]) > 2.0 ** 40
        assert [float(ref.e[j]) for j in (0, 1, 2, 3, 4)] == [26.0, 27.0, 155.0, 169.0, 0.0]
        r5 = ref.rb[5].abs()
        assert float(r5.max()) == 3.0 and float(r5.sort().values[-2]) <= 3.0 * 2.0 ** -20
        assert int(ref.v[5].abs().sort().values[-2]) < 2 ** 11          # ... so they live in the two low limbs
        assert float(ref.S0[4]) == 0.0 and not ref.c[4].any()


@pytest.mark.parametrize("case", T.W_SAT + T.W_LIMBS, ids=lambda c: c.id)
def test_saturated_operands(case):
    i, ref = _weight_ref(case)
    qa = 2 ** case.a_bits - 1
    assert bool((ref.X == qa).all()) and bool((ref.G == case.T * qa * qa).all())
    if case.kind == "satx":
        return
    assert case.T == 128 and case.a_bits == 7 and int(ref.G[0, 0]) == 0x1F8080 and (0x1F8080 & 0xFF) == 0x80      # lowest limb -128
    qw = 2 ** case.w_bits - 1
    wq = ref._wq(i["W"], i["sc"], i["zp"], case.w_bits)
    assert set(wq.unique().tolist()) == {float(v) for v in (qw, -qw, 0, qw - (qw + 1) // 2, -((qw + 1) // 2))}
    if case.kind == "sat":
        assert bool((wq[0, 0] == qw).all()) and bool((wq[1, 1] == -qw).all())        # whole rows at +qmax and at -qmax
    else:
        assert bool((wq[2, 0, 0::2] * wq[2, 0, 1::2] < 0).all())                     # the sign alternates along K
    # the largest K the predicate admits for this width
    nxt = [k for k in (32 * n for n in R.NJ_OK) if k > case.K]
    assert all(not R.gram_supported(case.T, case.O, k, case.a_bits, case.w_bits, case.P) for k in nxt)


def test_limb_switches_follow_the_formula():
    want = {2: [(14, 15), (3626, 3627)], 4: [(145, 146), (37136, 37137)], 7: [(2, 3), (518, 519)]}
    for a, pairs in want.items():
        assert R.limb_switches(a, 40000) == pairs
        for lo, hi in pairs:
            assert R.g_limbs(hi, a) == R.g_limbs(lo, a) + 1
            assert lo * (2 ** a - 1) ** 2 <= 127 * (256 ** R.g_limbs(lo, a) - 1) // 255 < hi * (2 ** a - 1) ** 2
    assert sorted({(c.a_bits, c.T) for c in T.W_LIMBS}) == sorted((a, t_) for a, pairs in want.items() for pr in pairs for t_ in pr)
    assert R.g_limbs(6304, 4) == 3 and R.g_limbs(6304, 6) == 4                        # (tests/test_gpu_kernels.py asks the library the same)


def _lib_or_none():
    from adalog_amd import _lib
    return _lib.load() if os.path.exists(_lib.LIB_PATH) else None


def test_tables_honour_the_predicates():
    lib = _lib_or_none()
    for c in T.W_CASES + [T.shard_case(s) for s in T.S_CASES]:
        assert R.gram_supported(c.T, c.O, c.K, c.a_bits, c.w_bits, c.P), c.id
    for args in T.W_REJECTED:
        assert not R.gram_supported(*args), args
    for c in T.A_CASES:
        assert R.gram_act_supported(c.T, c.O, c.K, c.a_bits, c.w_bits, c.P), c.id
    if lib is not None:                                      # (host code: no device is touched)
        for c in T.W_CASES:
            assert lib.adalog_gram_supported(c.T, c.O, c.K, c.a_bits, c.w_bits, c.P), c.id
            assert lib.adalog_gram_limbs(c.T, c.a_bits) == R.g_limbs(c.T, c.a_bits)
        for args in T.W_REJECTED:
            assert not lib.adalog_gram_supported(*args), args
        for K in (32 * n for n in range(1, 33)):
            for w in range(1, 9):
                for a in (1, 2, 4, 7, 8):
                    for P in (31, 32, 96):
                        assert bool(lib.adalog_gram_supported(128, 4, K, a, w, P)) == R.gram_supported(128, 4, K, a, w, P), (K, a, w, P)


def test_weight_table_reaches_the_launches_it_claims():
    """on 256 CUs: every NJ with both row-dot group sizes; 1, 2, 3, 4 blocks; workgroups of 4 CB - 1, 4 CB and 4 CB + 1 blocks; a
    cooperative thin tail of 1 and of 2 blocks at NJ = 8, 12, 24; every T of the issue; both bias settings"""
    shapes = T.W_SHAPES + T.W_BITS
    for K in (32, 64, 96, 128, 192, 256, 384, 512, 768):
        assert {c.w_bits > 4 for c in shapes if c.K == K} == {True, False}, K
        assert {c.bias for c in T.W_CASES if c.K == K} == {True, False}, K
    assert {1, 2, 3, 4} <= {T.weight_blocks(c)[0] for c in shapes}
    assert {1, 49, 127, 128, 129, 1000} <= {c.T for c in shapes} and any(c.T > 8192 and c.K == 32 and c.O == 8 for c in shapes)
    assert {32, 64, 96, 128, 256} <= {c.P for c in shapes}
    per_wg = {}
    for c in shapes:
        nblk, wgs = T.weight_blocks(c)
        per_wg.setdefault(c.K, set()).update({nblk // wgs, -(-nblk // wgs)})
    for K, cb in ((32, 4), (256, 2), (768, 2)):
        assert {4 * cb - 1, 4 * cb, 4 * cb + 1} <= per_wg[K], (K, per_wg[K])
    for K in (256, 384, 768):
        assert {1, 2} <= per_wg[K]
    assert {(c.a_bits, c.w_bits) for c in T.W_BITS} == {(2, 2), (2, 7), (7, 2), (3, 5), (5, 3), (7, 7), (6, 6)}
    assert len({c.id for c in T.W_CASES}) == len(T.W_CASES) and len({c.id for c in T.A_CASES}) == len(T.A_CASES)


@pytest.mark.parametrize("case", T.A_CASES, ids=lambda c: c.id)
def test_act_reference_terms(case):
    i = T.act_inputs(case)
    ref = R.ActRef(i["x"], i["ref"], i["bias"], i["W"], i["sw"], i["zw"], case.w_bits, case.a_bits)
    n = 4 if case.big else min(case.P, 16)
    sub = torch.linspace(0, case.P - 1, n).round().long().unique()
    t = ref.terms(i["sc"][sub], i["zp"][sub], i["norm"])
    assert bool(torch.isfinite(t["score"]).all())
    err = (t["gram"] - t["score"]).abs()
    assert bool((err <= R.act_gram_vs_direct_bound(ref, t, i["norm"])).all()), float(err.max())
    spec = CB.GramActState(CB.GramActPrepared(i["x"]), i["ref"], i["bias"], i["W"], i["sw"], i["zw"], case.w_bits, case.a_bits,
                           case.P).score(i["sc"][sub], i["zp"][sub], i["norm"]).view(-1)
    assert bool(((t["score"] - spec.double()).abs() <= 2.0 ** -23 * spec.abs().double() + R.TINY32).all())
    # the derived bound stays a bound on fp32-level effects: far below the score's own terms
    assert bool((R.act_bound(ref, t, i["norm"]) <= 2.0 ** -20 * i["norm"] * (t["S0"] + t["lin_abs"] + t["quad_abs"]) + R.TINY32).all())


def test_act_edge_inputs_are_what_they_claim():
    by = {c.kind: c for c in T.A_CASES if c.kind != "rand"}
    qa = lambda c: 2 ** c.a_bits - 1
    i = T.act_inputs(by["runs"]); assert i["x"].unique().numel() == 5
    i = T.act_inputs(by["const"]); assert i["x"].unique().numel() == 1
    i = T.act_inputs(by["zeros"]); z = i["x"][i["x"] == 0]
    assert bool(torch.signbit(z).any()) and bool((~torch.signbit(z)).any())
    for kind, end in (("clamp", "hi"), ("clamp_neg", "lo")):
        c = by[kind]; i = T.act_inputs(c); third = c.P // 3
        for p in (0, third - 1, third, 2 * third - 1):
            zq = torch.round(i["zp"][p])
            xq = (torch.round(i["x"] / i["sc"][p]) + zq).clamp(0, qa(c)) - zq
            want = (qa(c) - zq if end == "hi" else -zq) if p < third else 0.0
            assert bool((xq == want).all()), (kind, p)
    c = by["ties"]; i = T.act_inputs(c)
    frac = (i["x"].view(-1, 1) / i["sc"][:: max(1, c.P // 8)].view(1, -1))
    assert int(((frac - torch.floor(frac)) == 0.5).sum()) >= 20
    c = by["wsat"]; i = T.act_inputs(c); qw = 2 ** c.w_bits - 1
    zq = torch.round(i["zw"]).view(-1, 1)
    wq = (torch.round(i["W"] / i["sw"].view(-1, 1)) + zq).clamp(0, qw)
    assert bool(((wq == 0) | (wq == qw)).all())
    i = T.act_inputs(by["wzero"]); assert not i["W"][3].any()
    c = by["rowbias"]; i = T.act_inputs(c); assert torch.equal(i["ref"][c.T // 2], i["bias"])
    assert {c.P for c in T.A_CASES} >= {1, 2, 33, 100, 128, 256} and {c.K for c in T.A_CASES} == {32 * n for n in R.NJ_OK}
    assert {c.T for c in T.A_CASES} >= {1, 31, 32, 33, 127, 128, 129}
    assert {2, 7} <= {c.a_bits for c in T.A_CASES} and {2, 7} <= {c.w_bits for c in T.A_CASES} and any(c.a_bits != c.w_bits for c in T.A_CASES)
    for K in (512, 768):
        assert any(c.K == K and c.O < 2 * K for c in T.A_CASES) and any(c.K == K and c.O > 2 * K for c in T.A_CASES)
