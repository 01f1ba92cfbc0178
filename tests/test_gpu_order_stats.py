"""`-m gpu`: the radix select of csrc/select.hip held to exact order statistics on every route -- the one-block kernel, the fused
multi-block kernel (agent-scope atomics, last-block ticket) and the separate count / pick launches of ShardedSelect -- at the rows
and ranks of tests/order_stats_cases.py (cumulative-count edges, lane boundaries of the pick, late-diverging ranks, heavy ties,
denormals / +-0 / +-FLT_MAX / +-inf) and at the sizes where run_select changes route or grid.  The reference is numpy.sort at the
rank and the assertion is equality; tests/test_order_stats_cpu.py proves the same table against the CPU specification."""
import numpy as np
import pytest
import torch

from tests import cpu_backend as CB
from tests import order_stats_cases as OC

pytestmark = pytest.mark.gpu

DEV = "cuda"
R = OC.MAXR


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import backend
    backend.set_backend(None)
    return backend.get()          # raises loudly if the HIP library or the device is missing


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ the three routes
def separate_values(ops, xd, S, ranks8, layout=None):
    """k_sel_hist + k_sel_pick, four rounds, then the raw values [8, S]"""
    sel = ops.ShardedSelect(xd, S, R, *(layout or (0, S, 0)), ranks=_dev(ranks8))
    for p in range(4):
        sel.hist_pass(p)
        sel.pick(p)
    return sel.values()


_W4 = (0.25, 0.5, 0.75, 0.0)                                   # arbitrary: lerp(a, a, w) is a


def raw_quantile_launch(ops, xd, ranks4_dev, w_dev, mbs=1):
    """adalog_quantile_rows with ranks_lo_hi = (r0, r0, r1, r1, r2, r2, r3, r3): d = a - a = 0 and fma(w, 0, a) = a, so the output
    [4, S / mbs] is the raw order statistic (its chunk mean for mbs > 1) with all eight states live.  One-block or fused multi-block,
    as one_block_ok decides.  -> (out, workspace); nothing here waits for the device."""
    lib = ops._lib.load()
    S, n = xd.shape
    nb = lib.adalog_select_workspace_bytes(S, R)
    ws = torch.empty(nb, dtype=torch.uint8, device=xd.device)
    out = torch.empty((R // 2, S // mbs), dtype=torch.float32, device=xd.device)
    rc = lib.adalog_quantile_rows(xd.data_ptr(), S, n, R // 2, ranks4_dev.data_ptr(), w_dev.data_ptr(), int(mbs), out.data_ptr(),
                                  ws.data_ptr(), nb, ops._stream())
    ops._lib.check(rc, "adalog_quantile_rows")
    return out, ws


def quantile_route_values(ops, xd, ranks8, mbs=1):
    """two launches of four ranks each -> (out [8, S / mbs], the two workspaces)"""
    w = _dev(np.asarray(_W4, np.float32))
    outs, wss = [], []
    for h in range(2):
        o, ws = raw_quantile_launch(ops, xd, _dev(np.repeat(ranks8[4 * h:4 * h + 4], 2)), w, mbs)
        outs.append(o)
        wss.append(ws)
    return torch.cat(outs, 0), wss


def state_values(ws, S):
    """The per-row values the multi-block route descended to, read from its workspace before any mean: [S][R] states of
    {uint32 prefix; int64 remaining} behind the [S][R][256] uint32 histograms (ws_state in select.hip) -> [4, S] (even states)."""
    assert ws.numel() == S * R * (4 * 256 + 16) + 256, "the workspace is no longer [S][R][256] uint32 + [S][R] 16-byte states"
    off = (4 * S * R * 256 + 15) // 16 * 16
    st = ws[off:off + 16 * S * R].cpu().numpy().view(np.uint32).reshape(S, R, 4)
    return OC.key2f(st[:, 0::2, 0]).T


def _check_case_on_routes(ops, case, mbs):
    """every batch on every route; all routes are tried before the case fails, so that the message names each one that is wrong"""
    xd = _dev(case.x)
    bad = []
    for b, ranks8 in enumerate(case.ranks):
        want = case.want[:, b].T                                                       # [8, S]
        if not np.array_equal(separate_values(ops, xd, case.S, ranks8).cpu().numpy(), want):
            bad.append(("separate launches", ranks8.tolist()))
        if case.has_inf:
            continue
        out, wss = quantile_route_values(ops, xd, ranks8, mbs)
        if mbs == 1:
            if not np.array_equal(out.cpu().numpy(), want):
                bad.append(("quantile route", ranks8.tolist()))
        else:                                                                          # per row first, then the fp32 chunk mean
            if not np.array_equal(np.concatenate([state_values(ws, case.S) for ws in wss], 0), want):
                bad.append(("fused, per row", ranks8.tolist()))
            acc = np.zeros((R, case.S // mbs), np.float32)
            with np.errstate(over="ignore", invalid="ignore"):
                for m in range(mbs):
                    acc = acc + want[:, m::mbs]
                acc = acc / np.float32(mbs)
            if not np.array_equal(out.cpu().numpy(), acc, equal_nan=True):
                bad.append(("fused, chunk mean", ranks8.tolist()))
    assert not bad, (case, bad[:6])


@pytest.mark.parametrize("S,n,mbs,route,only", OC.ROUTE_SHAPES, ids=lambda v: str(v)[:10])
def test_raw_order_statistics_on_every_route(ops, S, n, mbs, route, only):
    for case in OC.cases(S, n, False, only) + OC.cases(S, n, True, only if only is None else ("inf+-",)):
        _check_case_on_routes(ops, case, mbs)


def test_cases_run_on_the_route_they_name(ops):
    """one case per route under the profiler: a later change of one_block_ok must not move the table off a route silently"""
    from torch.profiler import ProfilerActivity, profile

    def names(fn):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.key for e in prof.key_averages()]

    for S, n, mbs, route, only in OC.ROUTE_SHAPES:
        if (S, n) not in ((3, 16384), (3, 16385), (256, 65536), (256, 65537), (4, 300)):
            continue
        case = OC.cases(S, n, False, only)[0]
        xd = _dev(case.x)
        got = names(lambda: quantile_route_values(ops, xd, case.ranks[0], mbs))
        other = OC.FUSED if route == OC.ONE_BLOCK else OC.ONE_BLOCK
        assert any(route in k for k in got) and not any(other in k for k in got), (S, n, mbs, got)
        assert not any("k_sel_hist(" in k or "k_sel_pick" in k for k in got), got
    case = OC.cases(3, 257)[0]
    xd = _dev(case.x)
    got = names(lambda: separate_values(ops, xd, 3, case.ranks[0]))
    assert any("k_sel_pick" in k for k in got) and any("k_sel_hist" in k and "k_sel_hist_pick" not in k for k in got), got
    assert not any(OC.ONE_BLOCK in k or OC.FUSED in k for k in got), got


# ------------------------------------------------------------------------------------------------ interpolated quantiles
@pytest.mark.parametrize("mbs", [1, 2, 4])
@pytest.mark.parametrize("n", [300, 16385])
def test_quantile_rows_within_three_ulp(ops, n, mbs):
    """ops.quantile_rows with the product's percentile list and with nq = 1: a, b exact, so what is left is the lerp (3 ulp of
    max(|a|, |b|)) and one rounding of the chunk mean -- see order_stats_cases.quantile_reference.  S / mbs = 8, 4, 2.  Where the
    fp32 chunk sum of values next to +-FLT_MAX overflows, the result must be that same non-finite value."""
    from adalog_amd.search import _pct_lists
    for qs in (_pct_lists(), [0.37]):
        for case in OC.cases(8, n, False, OC.QUANTILE_FAMILIES):
            got = ops.quantile_rows(_dev(case.x), qs, mbs).cpu().numpy()
            OC.assert_quantiles(got, OC.quantile_reference(case, qs, mbs), (case, qs))


# ------------------------------------------------------------------------------------------------ positive percentile
@pytest.mark.parametrize("S,n", [(3, 20000), (300, 20000), (300, 4000)])
def test_positive_percentile_several_rows(ops, S, n):
    """qfrac[r] and out[r][S] with several rows: multi-block (n > 16384) and one-block (n = 4000), against the oracle by equality"""
    x = OC.positive_rows(S, n)
    want = CB.positive_percentile_rows(torch.from_numpy(x), list(OC.PP_QS))
    got = ops.positive_percentile_rows(_dev(x), list(OC.PP_QS)).cpu()
    assert torch.equal(got, want), (got - want).abs().max()


@pytest.mark.parametrize("which", [0, 1], ids=["2pow24+1", "2pow24+3"])
def test_positive_percentile_count_rounds_in_fp32(ops, which):
    """Above 2**24 positives counts.float() rounds to even (order_stats_cases.rounding_row): rank count - 2 for 2**24 + 1 positives,
    and for 2**24 + 3 a rank one past the last positive value, which gives 0.  Equality with the exact reference and with the oracle."""
    x = OC.rounding_row(which)
    want = OC.positive_reference(x, OC.ROUNDING_QS)
    assert want[0, 0] == (150.0, 0.0)[which] and want[1, 0] > 0 and want[2, 0] == x[x > 0].min()
    xt = torch.from_numpy(x)
    got = ops.positive_percentile_rows(xt.to(DEV), list(OC.ROUNDING_QS)).cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(CB.positive_percentile_rows(xt, list(OC.ROUNDING_QS)).numpy(), want)


# ------------------------------------------------------------------------------------------------ sharded
def _emulated(ops, shards, S, layouts, ranks=None, qfrac=None):
    """ShardedSelect on several emulated ranks in one process: the all-reduce is the sum of their histograms"""
    Rr = R if ranks is not None else len(qfrac)
    sels = [ops.ShardedSelect(_dev(x2), S, Rr, *lay, ranks=None if ranks is None else ranks, qfrac=qfrac)
            for x2, lay in zip(shards, layouts)]
    for p in range(4):
        for s in sels:
            s.hist_pass(p)
        total = sum(s.hist.clone() for s in sels)
        for s in sels:
            s.hist.copy_(total)
            s.pick(p)
    return sels


def _dealt_rows(specs, n, cuts, seed):
    """Rows whose deciding block lies wholly in columns >= cuts[0]: -> full [S, n] and the column shards (the first holds filler only)"""
    rows = []
    for s, spec in enumerate(specs):
        blk, fill = OC.row_parts(spec, n, seed + s)
        rest = np.concatenate([blk, fill[cuts[0]:]])
        OC._rng(seed, s, 5).shuffle(rest)
        rows.append(np.concatenate([fill[:cuts[0]], rest]))
    full = np.stack(rows)
    return full, [np.ascontiguousarray(p) for p in np.split(full, cuts, axis=1)]


@pytest.mark.parametrize("layout", ["columns", "spread_chunks", "whole_chunks"])
def test_sharded_quantiles_three_uneven_ranks(ops, layout):
    """The (first, inner, outer) layouts of search._sharded_quantiles with S_local > 1 on three ranks of unequal size -- against the
    exact reference, not against the fused kernel.
      columns:       (0, S, 0), per-channel: every rank holds a column slice of all S segments; rank 0 holds none of the deciding block.
      spread_chunks: (chunk, 1, mbs) of _flat_layout with mbs <= ranks: 2 heads x 2 chunks; chunk 0 of both heads is spread over ranks 0
                     and 1 (rank 0 again without the deciding block), chunk 1 lies on rank 2; local row h counts into slot chunk + 2 h.
      whole_chunks:  (first chunk, per, mbs) of _flat_layout with mbs > ranks: 2 heads x 4 chunks, ranks hold 1, 2 and 1 chunks per head."""
    from adalog_amd.search import _pct_lists
    qs = _pct_lists()
    specs = ("deep24+", "deep16-", "deep24+-", "deep8+")
    if layout == "whole_chunks":
        n, S, mbs = 5000, 8, 4
        case = OC.Case("chunks", specs, S, n, seed=41)
        x = case.x.reshape(2, 4, n)
        shards = [x[:, 0:1].reshape(-1, n), x[:, 1:3].reshape(-1, n), x[:, 3:4].reshape(-1, n)]
        layouts = [(0, 1, 4), (1, 2, 4), (3, 1, 4)]
    else:
        n, S = 20000, 4
        full, cols = _dealt_rows(specs, n, [137, 9000], seed=43)
        case = OC.Rows(full)
        assert not np.isin(full[:, :137], np.concatenate([OC.row_parts(sp, n, 43 + i)[0] for i, sp in enumerate(specs)])).any()
        if layout == "columns":
            mbs, shards, layouts = 1, cols, [(0, S, 0)] * 3
        else:                                          # global segment = 2 * head + chunk
            mbs, shards = 2, [full[0::2, :137], full[0::2, 137:], full[1::2]]
            layouts = [(0, 1, 2), (0, 1, 2), (1, 1, 2)]
    lohi, w = ops.quantile_ranks(qs, n)
    sels = _emulated(ops, shards, S, layouts, ranks=lohi.to(DEV))
    ref = OC.quantile_reference(case, qs, mbs)
    for sel in sels:                                   # every rank descends identically
        OC.assert_quantiles(sel.quantiles(w, mbs).cpu().numpy(), ref, layout)
    raw = sels[0].values().cpu().numpy()               # and the states themselves, exactly
    assert np.array_equal(raw, case.sorted[:, lohi.numpy()].T)


def test_sharded_positive_percentile_two_segments(ops):
    x = OC.positive_rows(7, 9000, seed=3)[[3, 6]]                                      # 1000 positives; NaNs and +inf among them
    shards = [np.ascontiguousarray(p) for p in np.split(x, [137, 5000], axis=1)]
    sels = _emulated(ops, shards, 2, [(0, 2, 0)] * 3, qfrac=list(OC.PP_QS))
    want = CB.positive_percentile_rows(torch.from_numpy(x), list(OC.PP_QS))
    assert np.array_equal(want.numpy(), OC.positive_reference(x, OC.PP_QS))
    for sel in sels:
        assert torch.equal(sel.values().cpu(), want)


# ------------------------------------------------------------------------------------------------ back to back
def test_fused_selects_back_to_back_on_one_stream(ops):
    """Five multi-block selects queued without a wait in between, S = 1, 7, 3, 7, 1: the ticket words are shared and each pass relies
    on the last block of the pass before having cleared the histogram and put the ticket back."""
    n = 16385
    cs = [OC.Case(f"b2b{i}", OC.DEEP[i:] + OC.TIES, S, n, seed=70 + i) for i, S in enumerate((1, 7, 3, 7, 1))]
    w = _dev(np.asarray(_W4, np.float32))
    xs = [_dev(c.x) for c in cs]
    rk = [[_dev(np.repeat(c.ranks[b % len(c.ranks)][4 * h:4 * h + 4], 2)) for h in range(2)] for b, c in enumerate(cs)]
    torch.cuda.synchronize()
    outs = [[raw_quantile_launch(ops, xd, r, w)[0] for r in rr] for xd, rr in zip(xs, rk)]       # workspaces freed and reused at once
    torch.cuda.synchronize()
    for b, (c, oo) in enumerate(zip(cs, outs)):
        got = torch.cat(oo, 0).cpu().numpy()
        assert np.array_equal(got, c.want[:, b % len(c.ranks)].T), c


# ------------------------------------------------------------------------------------------------ sorted prefix
@pytest.mark.parametrize("n", [8192, 8193, 100352])
def test_sorted_prefix_both_columns(ops, n):
    """SortedPrefix.prefix[s, i] = (sum of the i smallest x, sum of their x^2) in fp64, against a long-double running sum of the
    sorted row."""
    case = OC.Case("prefix", ("deep24+-", "plain"), 2, n, seed=90)
    sp = ops.sorted_prefix(_dev(case.x))
    srt = np.sort(case.x, axis=1)
    assert np.array_equal(sp.sorted.cpu().numpy(), srt)
    pf = sp.prefix.cpu()
    assert pf.shape == (2, n + 1, 2)
    ld = srt.astype(np.longdouble)
    for col, v in ((0, ld), (1, ld * ld)):
        ref = np.concatenate([np.zeros((2, 1), np.longdouble), np.cumsum(v, axis=1)], 1).astype(np.float64)
        torch.testing.assert_close(pf[..., col], torch.from_numpy(ref), rtol=1e-13, atol=1e-13)
