"""tests/fpcs_reference.replay IS the reference's progressive search: it accepts the oracle's loop and the CPU-tier run of
adalog_amd.search.fpcs (the driver's no-FpcsTail branch, which is also what several ranks run), and it rejects four planted faults.
The device routes of the same driver are held to the same replay in tests/test_gpu_fpcs_driver.py."""
import pytest
import torch

from adalog_amd import backend, search
from oracle import adalog_oracle as O
from tests import cpu_backend
from tests import fpcs_reference as FR


@pytest.fixture(autouse=True)
def _cpu_backend():
    backend.set_backend(cpu_backend)
    yield
    backend.set_backend(None)


def _grid(cols, seed, third=False):
    """128 distinct (scale, zp) pairs per column.  Rows 0 and 1 are one spacing apart (the oracle takes its delta from them) and
    carry different zero points; every other row is 1.3 spacings from its neighbour.  On the product's own grids neighbours ARE one
    spacing apart, and s + 0.5 d and (s + d) - 0.5 d of two surviving neighbours then meet in the first expansion: exact duplicate
    candidates, which a tie-free scorer must not be given."""
    gen = torch.Generator().manual_seed(seed)
    a = 0.02 + 0.05 * torch.rand(cols, generator=gen)
    d = a * (0.05 + 0.05 * torch.rand(cols, generator=gen))       # (the sixth grid's spacing, d / 22 148, is still > 30 ulps of a)
    j = torch.arange(128, dtype=torch.float32).view(-1, 1)
    scale = (a + torch.where(j < 2, j * d, d + (j - 1) * (1.3 * d))).contiguous()
    zp = (torch.arange(128) % 8).float().view(-1, 1).repeat(1, cols).contiguous()
    delta = (scale[1] - scale[0]).contiguous()
    # the optimum: strictly inside the grid, off every grid point and off every integer zero point
    s_opt = scale[20] + (scale[100] - scale[20]) * torch.rand(cols, generator=gen)
    z_opt = 0.3 + 6.4 * torch.rand(cols, generator=gen)
    c = 0.01 + 0.04 * torch.rand(cols, generator=gen)
    t = (10.0 + torch.arange(128, dtype=torch.float32)).view(-1, 1).repeat(1, cols).contiguous() if third else None
    return scale, zp, t, delta, (s_opt, z_opt, c)


def _scorer(opt, distinct=True):
    """-(s - s*)^2 (1 + c (z - z*)^2) per column in fp64, rounded once to fp32 -- the product form of -(s - s*)^2 - c (z - z*)^2: in the
    last steps (s - s*)^2 is ~1e-9 of its first-step size, and a sum would round the scale term away.  Asserts that the fp32 scores
    of a column are all distinct."""
    s_opt, z_opt, c = (t.double() for t in opt)
    # off the fp32 lattice: the last grids are a few ulps wide, and s* - n ulp and s* + n ulp would score the same
    s_opt = s_opt * (1.0 + 1.2345e-9)

    def fn(scale, zp, third=None):
        z = zp if zp is not None else third
        sc = (-(scale.double() - s_opt) ** 2 * (1.0 + c * (z.double() - z_opt) ** 2)).float()
        if distinct:
            for col in range(sc.shape[1]):
                assert sc[:, col].unique().numel() == sc.shape[0], "the synthetic scorer tied in column %d" % col
        return sc
    return fn


def _tie_free_grid(cols, seed, steps=6):
    """_grid with s*, z* and c chosen per column so that the search never meets two equal scores: the expansions of neighbouring
    survivors overlap, and in some columns two of them land on the same fp32 scale.  Three times the columns are tried (one
    oracle run), the first `cols` tie-free ones are kept; the callers' scorers assert that the choice holds."""
    scale, zp, _, delta, opt = _grid(3 * cols + 8, seed)
    ok = torch.ones(scale.shape[1], dtype=torch.bool)

    def fn(sc, z):
        s = _scorer(opt, distinct=False)(sc, z)
        for col in range(s.shape[1]):
            ok[col] &= s[:, col].unique().numel() == s.shape[0]
        return s
    O.fpcs(scale, zp, fn, 0, steps=steps, width=16, eq_n=128, clamp_min=None)
    keep = ok.nonzero().flatten()[:cols]
    assert keep.numel() == cols
    return (scale[:, keep].contiguous(), zp[:, keep].contiguous(), None, delta[keep].contiguous(),
            tuple(o[keep].contiguous() for o in opt))


def _oracle_run(scale, zp, fn, steps):
    calls = []

    def spy(sc, z):
        s = fn(sc, z)
        calls.append(FR.Step(sc.clone(), z.clone(), None, s.clone(), None))
        return s
    top_s, top_z = O.fpcs(scale, zp, spy, 0, steps=steps, width=16, eq_n=128, clamp_min=None)
    return calls, (top_s.reshape(-1), top_z.reshape(-1), None)


@pytest.mark.parametrize("steps", [2, 4, 6])
@pytest.mark.parametrize("cols", [1, 7, 200])
def test_replay_accepts_the_oracle_and_the_cpu_driver(cols, steps):
    scale, zp, _, delta, opt = _tie_free_grid(cols, 100 * cols + steps, steps)
    fn = _scorer(opt)
    calls, committed = _oracle_run(scale, zp, fn, steps)
    assert len(calls) == steps
    FR.replay(calls, delta, 16, 128, None, committed, first=(scale, zp, None))
    # the product's driver, CPU tier: same scorer, same trajectory, same commit
    spy = FR.Spy(lambda s, z, t: fn(s, z))
    d_before = delta.clone()
    got = search.fpcs(scale, zp, None, delta, spy, steps, 16, 128, None)
    assert len(spy.steps) == steps
    FR.replay(spy.steps, delta, 16, 128, None, got, first=(scale, zp, None))
    for a, b in zip(spy.steps, calls):
        assert FR.bits_equal(a.scale, b.scale) and FR.bits_equal(a.zp, b.zp) and FR.bits_equal(a.scores, b.scores)
    assert FR.bits_equal(got[0], committed[0]) and FR.bits_equal(got[1], committed[1]) and got[2] is None
    assert FR.bits_equal(delta, d_before)                  # the caller's spacing is only read


def test_cpu_driver_with_the_clamp_exact_ties_and_a_nan():
    """clamp_min = 1e-4 with scales that reach it: the first expansion of column 0 lies below the clamp (128 identical scales, at
    most 16 distinct zero points -> exact ties decided by the candidate index), column 1 straddles it; one score of step 2 is NaN and
    must survive as the best of its column."""
    cols = 5
    scale, zp, _, delta, opt = _grid(cols, 7)
    f = torch.tensor([1e-5, 1e-4 / float(opt[0][1]), 1, 1, 1])         # column 0: all below the clamp; column 1: optimum AT the clamp
    scale = (scale * f).contiguous()
    delta = (scale[1] - scale[0]).contiguous()
    opt = (opt[0] * f, opt[1], opt[2])
    base = _scorer(opt, distinct=False)
    n_call = [0]

    def fn(s, z, t):
        sc = base(s, z)
        if n_call[0] == 2:
            sc[77, 3] = float("nan")
        n_call[0] += 1
        return sc
    spy = FR.Spy(fn)
    got = search.fpcs(scale, zp, None, delta, spy, 6, 16, 128, 1e-4)
    FR.replay(spy.steps, delta, 16, 128, 1e-4, got, first=(scale, zp, None))
    s1, s2 = spy.steps[1], spy.steps[2]
    assert bool((s1.scale[:, 0] == 1e-4).all()) and s1.scores[:, 0].unique().numel() <= 16   # the clamp was reached: exact ties
    # (around a clamped survivor the upper half of the neighbours lies above the clamp again)
    assert all(int((st.scale[:, 0] == 1e-4).sum()) >= 64 for st in spy.steps[2:])
    assert 0 < int((spy.steps[1].scale[:, 1] == 1e-4).sum()) < 128
    # the NaN candidate is the first survivor of its column: the next grid's first 8 rows surround it
    assert torch.isnan(s2.scores[77, 3]) and FR.rank(s2.scores, 16)[0, 3] == 77
    assert bool((spy.steps[3].zp[:8, 3] == s2.zp[77, 3]).all())


def test_cpu_driver_post_gelu_form():
    """zp = None, a third plane (the log base), width 32, 4 neighbours"""
    scale, _, third, delta, opt = _grid(3, 11, third=True)
    opt = (opt[0], 10.3 + 100.0 * opt[1] / 6.7, opt[2] * 1e-3)        # (the third plane holds 10 .. 137)
    fn = _scorer(opt, distinct=False)
    spy = FR.Spy(lambda s, z, t: fn(s, z, t))
    got = search.fpcs(scale, None, third, delta, spy, 6, 32, 128, None)
    assert got[1] is None and got[2] is not None
    assert all(st.zp is None and st.scale.shape == (128, 3) for st in spy.steps)
    FR.replay(spy.steps, delta, 32, 128, None, got, first=(scale, None, third))


def test_one_step_scores_once_and_commits_nothing():
    scale, zp, _, delta, opt = _grid(7, 3)
    spy = FR.Spy(lambda s, z, t: _scorer(opt)(s, z))
    assert search.fpcs(scale, zp, None, delta, spy, 1, 16, 128, None) is None
    assert len(spy.steps) == 1 and FR.bits_equal(spy.steps[0].scale, scale)
    with pytest.raises(FR.Mismatch):
        FR.replay(spy.steps, delta, 16, 128, None, None)


def test_rank_order():
    nan, inf = float("nan"), float("inf")
    s = torch.tensor([[1.0, 0.0], [nan, -0.0], [3.0, 0.0], [3.0, nan], [inf, nan], [-inf, 1.0]])
    assert FR.rank(s, 6).t().tolist() == [[1, 4, 2, 3, 0, 5], [3, 4, 5, 0, 1, 2]]
    assert FR.rank(s, 2).shape == (2, 2)


# ------------------------------------------------------------------------------------------------ the replay can fail
def _good_run(clamp=None):
    scale, zp, _, delta, opt = _tie_free_grid(7, 42)
    spy = FR.Spy(lambda s, z, t: _scorer(opt)(s, z))
    got = search.fpcs(scale, zp, None, delta, spy, 6, 16, 128, clamp)
    FR.replay(spy.steps, delta, 16, 128, clamp, got)
    return spy.steps, delta, got


def _regrid(steps, i, idx, delta_i):
    """steps with call i+1's grid rebuilt around the survivors idx of call i"""
    cur = steps[i]
    (s, z, t), _ = FR.next_grid(cur.scale, cur.zp, cur.third, idx, delta_i, 8, None)
    out = list(steps)
    out[i + 1] = out[i + 1]._replace(scale=s, zp=z, third=t)
    return out


def test_mutation_a_survivor_swapped_with_the_17th_candidate():
    steps, delta, got = _good_run()
    order = FR.rank(steps[0].scores, 17)
    idx = order[:16].clone()
    idx[15, 2] = order[16, 2]                                  # column 2: the 16th survivor dropped for the 17th candidate
    with pytest.raises(FR.Mismatch, match="call 0 -> 1"):
        FR.replay(_regrid(steps, 0, idx, delta), delta, 16, 128, None, got)


def test_mutation_the_runner_up_is_committed():
    steps, delta, got = _good_run()
    last = steps[-1]
    second = FR.rank(last.scores, 2)[1]
    bad_s, bad_z = got[0].clone(), got[1].clone()
    bad_s[4], bad_z[4] = last.scale[second[4], 4], last.zp[second[4], 4]
    assert not FR.bits_equal(bad_s, got[0])
    with pytest.raises(FR.Mismatch, match="commit"):
        FR.replay(steps, delta, 16, 128, None, (bad_s, bad_z, None))


def test_mutation_delta_narrowed_twice_in_one_step():
    steps, delta, got = _good_run()
    d2 = delta / 7.5 / 7.5                                     # call 1 -> 2 should use delta / 7.5
    with pytest.raises(FR.Mismatch, match="call 1 -> 2"):
        FR.replay(_regrid(steps, 1, FR.rank(steps[1].scores, 16), d2), delta, 16, 128, None, got)
    # ... and a spy that saw the tail's spacing reports it directly
    chain = [delta]
    for _ in steps:
        chain.append(chain[-1] / 7.5)
    seen = [st._replace(delta_in=chain[i]) for i, st in enumerate(steps)]
    FR.replay(seen, delta, 16, 128, None, got)
    seen[3] = seen[3]._replace(delta_in=chain[4])
    with pytest.raises(FR.Mismatch, match="call 3: the spacing"):
        FR.replay(seen, delta, 16, 128, None, got)


def test_mutation_a_grid_value_off_by_one_ulp():
    steps, delta, got = _good_run()
    s = steps[3].scale.clone()
    s[50, 6] = torch.nextafter(s[50, 6], torch.tensor(float("inf")))
    bad = list(steps)
    bad[3] = bad[3]._replace(scale=s)
    with pytest.raises(FR.Mismatch, match=r"call 2 -> 3: the scale plane.*first at \[row 50, col 6\]"):
        FR.replay(bad, delta, 16, 128, None, got)
