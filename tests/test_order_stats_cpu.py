"""The order-statistic case table (tests/order_stats_cases.py) against the CPU specification of the radix select: proves that the row
builders, the edge ranks and the exact reference agree before tests/test_gpu_order_stats.py holds the kernels to them."""
import numpy as np
import pytest
import torch

from tests import cpu_backend as CB
from tests import order_stats_cases as OC

CPU_MAX = 10 ** 6                                            # the specification walks every row in Python


def _spec_values(x, S, ranks8):
    sel = CB.ShardedSelect(torch.from_numpy(x), S, OC.MAXR, 0, S, 0, ranks=torch.from_numpy(ranks8))
    for p in range(4):
        sel.hist_pass(p)
        sel.pick(p)
    return sel.values().numpy()                              # [8, S]


def test_key_round_trip_and_order():
    x = np.array([-np.inf, -OC.FLT_MAX, -1.0, -OC.DENORM, -0.0, 0.0, OC.DENORM, 1.0, OC.FLT_MAX, np.inf], np.float32)
    k = OC.f2key(x)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert OC.key2f(k).view(np.uint32).tolist() == x.view(np.uint32).tolist()
    probe = np.array([OC.DENORM, 1e-38, 1.0, 1.5, 2.0, 1.7e38], np.float32)
    assert (OC.ulp32(probe) == np.spacing(probe)).all() and OC.ulp32(OC.FLT_MAX) == 2.0 ** 104
    for top in (OC.TOP_POS, OC.TOP_NEG, OC.TOP_BIG, OC.TOP_NBIG):
        assert np.isfinite(OC.key2f((np.uint32(top) << np.uint32(8)) | np.arange(256, dtype=np.uint32))).all()


@pytest.mark.parametrize("n", [1, 2, 255, 257, 4097, 16385])
def test_builders_put_ranks_on_edges(n):
    """deep rows are finite, carry ranks 0 and n - 1, and hold a pair e - 1 | e across every change of their deciding byte"""
    for spec in OC.DEEP:
        x, ranks = OC.build_row(spec, n, seed=5)
        assert x.shape == (n,) and np.isfinite(x).all() and ranks[0] == 0 and ranks[-1] == n - 1
        bits = OC._SPEC[spec][1]
        ks = np.sort(OC.f2key(x))
        if n >= 20:
            hi = ks >> np.uint32(24 - bits)
            straddle = [r for r in ranks[:-1] if r + 1 in ranks and hi[r] != hi[r + 1]]
            assert len(straddle) >= len(OC.POP) - 1, (spec, n, straddle)


@pytest.mark.parametrize("S,n,mbs,route,only", [s for s in OC.ROUTE_SHAPES if s[0] * s[1] <= CPU_MAX], ids=lambda v: str(v)[:12])
def test_spec_select_matches_sort(S, n, mbs, route, only):
    for inf in (False, True):
        for case in OC.cases(S, n, inf, only):
            for b, ranks8 in enumerate(case.ranks):
                assert np.array_equal(_spec_values(case.x, S, ranks8), case.want[:, b].T), (case, ranks8)


@pytest.mark.parametrize("n", [256, 4097, 65537])
def test_diverging_ranks_split_in_pass_two(n):
    for spec in ("deep16+", "deep16-"):
        ranks = OC.diverging_ranks(n, spec)
        keys = np.sort(OC.f2key(OC.build_row(spec, n, seed=9)[0]))[ranks]
        assert len(set((keys >> np.uint32(16)).tolist())) == 1 and len(set((keys >> np.uint32(8)).tolist())) == OC.MAXR
    case = [c for c in OC.cases(3, n) if "deep16+" in c.specs][0]
    assert OC.diverging_ranks(n, "deep16+") in case.ranks.tolist() and OC.diverging_ranks(n, "deep16-") in case.ranks.tolist()


@pytest.mark.parametrize("mbs", [1, 2, 4])
@pytest.mark.parametrize("n", [300, 16385])
def test_spec_quantiles_within_bound(n, mbs):
    from adalog_amd.search import _pct_lists
    for qs in (_pct_lists(), [0.37]):
        for case in OC.cases(8, n, False, OC.QUANTILE_FAMILIES):
            got = CB.quantile_rows(torch.from_numpy(case.x), qs, mbs).numpy()
            OC.assert_quantiles(got, OC.quantile_reference(case, qs, mbs), (case, qs))


def test_count_rounding_above_two_pow_24_in_the_specification():
    """The `rk >= total` branch of the specification's pick on a synthetic pass-0 histogram (a row of 2**24 + 3 elements is past what
    the specification can walk): fp32(2**24 + 1) = 2**24 -> rank count - 2; fp32(2**24 + 3) = 2**24 + 4 -> one past the end -> 0."""
    for cnt, rem in (((1 << 24) + 1, ((1 << 24) - 1, (1 << 23) - 1, 0)), ((1 << 24) + 3, (-1, (1 << 23) + 1, 0))):
        sel = CB.ShardedSelect(torch.ones(1, 1), 1, 3, 0, 1, 0, qfrac=list(OC.ROUNDING_QS))
        sel.hist.view(1, 3, 256)[0, :, 0xBF] = cnt
        sel.pick(0)
        assert sel.remaining[0].tolist() == list(rem) and sel.prefix[0].tolist() == [0 if r < 0 else 0xBF for r in rem]
        assert (sel.values()[:, 0] == 0).tolist() == [r < 0 for r in rem]


@pytest.mark.parametrize("S,n", [(3, 20000), (300, 4000)])
def test_positive_oracle_matches_reference(S, n):
    x = OC.positive_rows(S, n)
    got = CB.positive_percentile_rows(torch.from_numpy(x), list(OC.PP_QS)).numpy()
    assert np.array_equal(got, OC.positive_reference(x, OC.PP_QS))
    want = OC.positive_reference(x, OC.PP_QS)
    kinds = [OC.PP_KINDS[s % len(OC.PP_KINDS)] for s in range(S)]
    assert (want[:, [k == "none" for k in kinds]] == 0).all() and (want[:, [k == "one" for k in kinds]] == 0.75).all()
    assert np.isinf(want[1, [k == "nan_inf" for k in kinds]]).all()          # q = 1.0: +inf is the largest positive, NaNs are none
    sel = CB.ShardedSelect(torch.from_numpy(x), S, len(OC.PP_QS), 0, S, 0, qfrac=list(OC.PP_QS))
    for p in range(4):
        sel.hist_pass(p)
        sel.pick(p)
    assert np.array_equal(sel.values().numpy(), want)
