"""The self-MSE scorers' case table (tests/self_mse_cases.py) and fp64 reference (tests/self_mse_reference.py), proved on the CPU:
the reference against the oracle, the CPU stand-ins of tests/cpu_backend.py against the reference PER SCORE with the bars the GPU
tier uses, and the table's claims about what it covers.  tests/test_gpu_self_mse.py then runs the same table on the kernels."""
import numpy as np
import pytest
import torch

from oracle import adalog_oracle as O
from tests import cpu_backend as CB
from tests import self_mse_cases as T
from tests import self_mse_reference as R


def _t(a):
    return torch.from_numpy(np.array(a, order="C"))


def _assert_within(got, ref_score, bar, what):
    got = np.asarray(got, np.float64)
    assert got.shape == ref_score.shape, (what, got.shape, ref_score.shape)
    nan = np.isnan(ref_score)
    assert np.array_equal(np.isnan(got), nan), what
    err = np.abs(got - ref_score)[~nan]
    ratio = err / bar[~nan]
    k = int(ratio.argmax()) if ratio.size else 0
    assert (err <= bar[~nan]).all(), (what, "worst err / bar", float(ratio[k]), "at", k, float(err[k]), float(bar[~nan][k]))


# ------------------------------------------------------------------------------------------------ 3a: reference against the oracle
# The oracle evaluates the same three fp32 operations for c, so c agrees bit for bit.  It then rounds x - c (relative u on the
# difference, 2 u on its square), the square (u), and sums in fp32 with ATen's cascade sum: a term passes through at most 16
# sequential adds on each of the 4 cascade levels, the folds of the vector lanes and of the 4 accumulator chains (<= 5 + 2), the
# division(s) of torch.mean (<= 2) and, for activations, the sum over images (1 here): 3 + 64 + 7 + 3 = 77 roundings, all on
# non-negative terms, hence relative to the score.
ORACLE_ROUNDINGS = 77


@pytest.mark.parametrize("case", T.GRID_CASES, ids=repr)
def test_reference_agrees_with_oracle_on_search_grids(case):
    x, scale, zp = T.inputs(case)
    if case.layout == "w":
        w3 = _t(x).view(1, case.S, case.n)
        got = O.score_w_self(w3, _t(scale).view(-1, 1, case.S, 1), _t(zp).view(-1, 1, case.S, 1), case.bits).reshape(case.P, case.S)
        norm = 1.0 / case.n
    else:
        cw = case.layout == "cw"
        x3 = _t(T.act_view(case, x)).unsqueeze(0)
        got = O.score_a_self(x3, _t(scale).t().contiguous(), _t(zp).t().contiguous(), case.bits, cw).t()
        norm = 1.0 / case.rows if cw else 1.0 / (case.rows * case.I)
    ref = R.score_segments(x, scale, zp, case.bits, norm, stats=False)
    bar = R._rel(ORACLE_ROUNDINGS) * np.abs(ref.score) + 2 * R.TINY32
    _assert_within(got.double().numpy(), ref.score, bar, case.id)
    # the table's reference is this one at the case's own norm
    assert np.allclose(T.reference(case).score * (norm / case.norm), ref.score, rtol=4 * R.U64, atol=0)


# ------------------------------------------------------------------------------------------------ 3b: the CPU stand-ins, per score
def _cpu_bar(ref, norm, n_terms):
    """cpu_backend.score_a_self / score_self_sorted: x - c in fp32 (2 u on the square), the square and the sum in fp64, one fp32
    rounding of the result: 3 u on non-negative terms, plus the underflow floor of the result"""
    return R._rel(3) * np.abs(ref.score) + R.TINY32 * (1 + abs(norm) * n_terms)


@pytest.mark.parametrize("case", T.ALL_SMALL + T.SORTED_BIG, ids=repr)
def test_cpu_backend_matches_reference_per_score(case):
    x, scale, zp = T.inputs(case)
    ref = T.reference(case)
    got = CB.score_self_sorted(CB.sorted_prefix(_t(x)), _t(scale), _t(zp), case.bits, case.norm)
    _assert_within(got.numpy(), ref.score, _cpu_bar(ref, case.norm, case.n), (case.id, "score_self_sorted"))
    if T.accepts("act", case):
        cw = case.layout == "cw"
        got = CB.score_a_self(_t(T.act_view(case, x)), _t(scale), _t(zp), cw, case.bits, case.norm)
        _assert_within(got.numpy(), ref.score, _cpu_bar(ref, case.norm, case.n), (case.id, "score_a_self"))
        # and the GPU tier's own bar holds the stand-in as well: it is never tighter than what fp32 terms allow
        assert (R.act_bar(ref, case.norm, case.rows, zp, case.n) >= _cpu_bar(ref, case.norm, case.n) * (1 - 1e-12)).all()
    if T.accepts("w", case):
        got = CB.score_w_self(_t(x), _t(scale), _t(zp), case.bits)
        _assert_within(got.numpy(), ref.score, R.weight_bar(ref, case.n), (case.id, "score_w_self"))


@pytest.mark.parametrize("case", (T.NAN_ACT, T.NAN_PT, T.NAN_W), ids=repr)
@pytest.mark.parametrize("row", T.NAN_ROWS)
def test_cpu_backend_nan_stays_in_its_segment(case, row):
    x, scale, zp = T.inputs(case)
    bad = x.copy()
    seg = 0 if case.layout == "pt" else T.NAN_SEG
    bad[seg, row * case.I + 1 if case.layout == "pt" else row] = np.nan
    clean, ref = T.reference(case), R.score_segments(bad, scale, zp, case.bits, case.norm, stats=False)
    assert np.isnan(ref.score[:, seg]).all()
    keep = [s for s in range(case.S) if s != seg]
    assert np.array_equal(ref.score[:, keep], clean.score[:, keep])
    got = CB.score_self_sorted(CB.sorted_prefix(_t(bad)), _t(scale), _t(zp), case.bits, case.norm).numpy()
    base = CB.score_self_sorted(CB.sorted_prefix(_t(x)), _t(scale), _t(zp), case.bits, case.norm).numpy()
    assert np.isnan(got[:, seg]).all() and np.array_equal(got[:, keep], base[:, keep])


# ------------------------------------------------------------------------------------------------ 3c: the table covers what it claims
@pytest.mark.parametrize("case", T.SORTED_BITS, ids=repr)
def test_sorted_cases_reach_every_kind_of_run(case):
    ref = T.reference(case)
    assert (ref.low & ref.high).any(), "no (candidate, segment) with both clamped runs occupied"
    assert (ref.low & ~ref.high).any() and (~ref.low & ref.high).any() and (~ref.low & ~ref.high).any()
    assert ref.hole.any(), "no empty unclamped run"
    assert ref.dup_edge.any(), "no run boundary next to a block of equal elements"
    assert (ref.runs == 1).any(), "no candidate that puts a whole segment into one run"
    if case.bits >= 2:
        assert (ref.runs >= min(2 ** case.bits, 8)).any()
    x, scale, zp = T.inputs(case)
    with np.errstate(all="ignore"):
        q = x[None] / scale[:, :, None]
    assert np.isinf(q).any(), "no candidate whose quotient overflows"
    assert (np.rint(zp) != zp).any() and (np.rint(zp) == zp).any() and (zp < 0).any() and (zp > 2 ** case.bits - 1).any()
    all_zero = np.rint(q) == 0
    assert all_zero.all(axis=2).any(), "no candidate that puts every element on level 0"


def test_sorted_cases_leave_dead_groups_and_full_workgroups():
    """groups per workgroup = 256 / 2^bits: the table holds products P * S off a multiple of it (a last workgroup with dead groups)
    at every width below 8 bits, and on one"""
    for bits in range(1, 8):
        gpb = 256 >> bits
        pairs = [c.P * c.S for c in T.SORTED_CASES if c.bits == bits]
        assert any(p % gpb for p in pairs), bits
    for bits in (4, 7):
        assert any(c.P * c.S % (256 >> bits) == 0 for c in T.SORTED_CASES if c.bits == bits)
    assert {c.bits for c in T.SORTED_BITS} == set(range(1, 9))
    assert any(c.P > 256 for c in T.SORTED_CASES) and any(c.P == 1 for c in T.SORTED_CASES)
    assert {c.n for c in T.SORTED_N} == {1, 3, 4, 5, 1023, 1024, 1025, 4096}
    nb = -(-T.SORTED_CARRY.n // R.PB)
    assert nb == 258 and T.SORTED_CARRY.n % R.PB not in (0, 1023) and T.SORTED_CARRY.S == 2


def test_one_pass_cases_split_every_path():
    rows = {c.rows for c in T.ACT_CASES}
    chans = {c.I for c in T.ACT_CASES}
    assert rows >= {1, 127, 128, 129, 256, 385} and chans >= {1, 63, 64, 65, 130}
    assert any(c.layout == "pt" and c.I > 64 for c in T.ACT_CASES)
    for layout in ("cw", "pt"):
        assert {c.zmode for c in T.ACT_CASES if c.layout == layout} == {"int", "frac", "mixed"}
    assert {1, 2, 128} <= {c.P for c in T.ACT_CASES}
    for c in T.ACT_CASES:
        _, _, zp = T.inputs(c)
        integral = np.rint(zp) == zp
        assert {"int": integral.all(), "frac": (~integral).all(), "mixed": c.P == 1 or (integral.any() and (~integral).any())}[c.zmode], c.id
    assert {(c.rows, c.I) for c in T.W_CASES} == {(r, i) for r in (1, 7) for i in (1, 5, 192, 4096)}
    assert {c.P for c in T.W_CASES} == {1, 255, 256}
    # the tie case: whole slabs, integral zero points, and planted values whose exact quotient by a candidate's scale is k + 0.5
    x, scale, zp = T.inputs(T.ACT_CASES[-4])
    assert T.ACT_CASES[-4].id.startswith("cw_ties_r256") and T.ACT_CASES[-4].rows % R.SLAB_ROWS == 0 and (np.rint(zp) == zp).all()
    with np.errstate(all="ignore"):
        q = x[None] / scale[:, :, None]
        tie = np.abs(q - np.floor(q)) == 0.5
        lvl = np.rint(q) + zp[:, :, None]
    assert (tie & (lvl < 0)).any() and (tie & (lvl > 255)).any() and (tie & (lvl > 0) & (lvl < 255)).any()


def test_bars_are_what_their_derivations_say():
    assert R.prefix_depth(1) == 36 and R.prefix_depth(262144) == 36 and R.prefix_depth(262144 + 1025) == 37
    assert R.kappa(4096) == 72
    assert list(R.act_chain(256, np.array([3.0, 3.5]))) == [20, 35] and list(R.act_chain(129, np.array([3.0]))) == [35]
    assert abs(R._rel(39) / (39 * R.U32) - 1) < 1e-5


def test_tie_grid_case_has_no_clamped_element_and_quotients_on_both_sides_of_the_tie():
    case = T.ACT_CASES[-3]
    assert case.id.startswith("cw_ties_in") and case.rows % R.SLAB_ROWS == 0
    x, scale, zp = T.inputs(case)
    ref = T.reference(case)
    assert (zp == 0).all() and not ref.low.any() and not ref.high.any()
    q = x[None].astype(np.float32) / scale[:, :, None]
    frac = q - np.floor(q)
    assert (frac == 0.5).any() and (frac < 0.5).any() and (frac > 0.5).any()
    assert (np.abs(frac - 0.5) <= 7 * 2.0 ** -23 * 255.5).all()                  # six ulps of the scale and one of the element
    assert (np.abs(frac - 0.5)[6] < 1e-4).all()                                   # the base scales: inside the kernel's tie zone


def test_third_carry_chunk_is_reached():
    assert -(-T.SORTED_CARRY3.n // R.PB) == 514 and R.prefix_depth(T.SORTED_CARRY3.n) == 38
