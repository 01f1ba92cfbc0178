"""`-m gpu`: k_gemm_stream<bf16xfp8> (csrc/gemm_k_stream.inc, MX form: bf16 rows x fp8 candidate columns, the fc2 weight search) at the
smallest shapes that take every path of its main-loop schedule.  The schedule of that loop (where the fragment reads, the fp8 -> bf16
conversions and the DMA requests sit among the MFMAs) may change; the scores may not: every accumulator sees the same MFMAs in the
same K order and the epilogue is the same arithmetic.  Two comparisons per case, through ops.gemm_score with the kernel label asserted:

  1. bit equality with tests/golden/stream_mx_parent_scores.npz -- the scores of the commit before the schedule was first changed,
     recorded on an MI355X with the very inputs of this file (tests/gemm_cases.inputs, seeded by the case id);
  2. per score against fp64: |got - score| <= gemm_reference.bar, the analytic bar of tests/test_gpu_gemm_edges.py (imported, not
     edited), so that the test does not rest on the recording alone.

Shapes.  The route decision (gemm_score.hip: route_of, pick_wide, adalog_gemm_mixed_ok) sends a launch here only with more than 256
valid K elements, M >= 192 and no row scale (the entry point refuses bf16 x fp8 operands otherwise), so of the shapes one would list
for a streaming kernel these do not reach it, and stand-ins do:
  M = 1                    not a wide shape; M = 192 is the smallest (one full 192-row tile, RI = 3)
  K = 64, 128 (nk = 1, 2)  K <= 256 runs on the group kernels; nk = 5 (K = 257 in rows of 320, and K = 320) is the shallowest and wraps
                           the 3-stage ring with a remainder of 2, nk = 6 (K = 321 in rows of 384) a whole number of times, nk = 8
                           (K = 449 in rows of 512) with a remainder of 2 after two turns
  row scale                refused by the entry point for these operands: all cases are without
What is covered: M = 192 (RI = 3, full tile), 193 (RI = 4, 63 rows masked), 256 (RI = 4, full), 257 (RI = 3: 192 + 65), 449 (RI = 4:
256 + 193), 513 (RI = 3: two full tiles and 129 rows); 64 x 3 and 128 x 5 candidate columns (one ragged 256-column tile; two full and a
half); the column bias shared by the candidates (staged with the reference) and per candidate (applied in the epilogue), and none;
per-column partials and per-workgroup accumulators (column axis summed); one and two groups; and two launches with more tiles than the
256 workgroups of a launch (262 and 258), where a workgroup's DMA ring runs on from one tile into the next -- with fewer tiles every
workgroup has exactly one.  A: integers 1 .. 15 (spread, hit) or the AdaLog values 30 x 2^-t, t = 0 .. 15 -- 16 binades -- (ext), B:
fp8-exact integers in [-15, 15].
"""
import os

import numpy as np
import pytest
import torch

from tests import gemm_cases as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROUTE = "k_gemm_stream<bf16xfp8>"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_mx_parent_scores.npz")


def _case(M, ncols, P, kv, K, G, keep_n, bias, kind):
    cid = "mx-M%d-n%d-P%d-K%d.%d-G%d-%s%s-%s" % (M, ncols, P, kv, K, G, "n" if keep_n else "", "" if bias == "none" else "b" + bias, kind)
    return T.Case(cid, ROUTE, T.BF16_FP8, M, ncols, P, K, kv, G, 1, 1, False, keep_n, bias, False, kind, "cols", False)


CASES = [
    _case(192, 3, 64, 257, 320, 1, True, "n", "spread"),
    _case(193, 5, 128, 320, 320, 1, True, "cn", "ext"),
    _case(256, 3, 64, 321, 384, 2, False, "none", "hit"),
    _case(257, 5, 128, 257, 320, 1, True, "n", "ext"),
    _case(257, 3, 64, 449, 512, 2, True, "cn", "spread"),
    _case(449, 3, 64, 449, 512, 1, True, "cn", "hit"),
    _case(449, 5, 128, 321, 384, 1, False, "n", "ext"),
    _case(513, 5, 128, 257, 320, 1, True, "none", "spread"),
    _case(513, 3, 64, 320, 320, 2, False, "cn", "ext"),
    # more tiles than workgroups: 2 row tiles x 131 column tiles (the last one half full), 1 x 258
    _case(257, 261, 128, 257, 320, 1, False, "n", "spread"),
    _case(193, 1029, 64, 257, 320, 1, True, "n", "ext"),
]


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import backend
    backend.set_backend(None)
    return backend.get()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def run_case(ops, case, i):
    """one ops.gemm_score call of the case -> (scores, kernel label)"""
    Ad, Bd = i["A"].to(DEV), i["B"].to(DEV)
    Ad.k_valid = case.k_valid; Bd.k_valid = case.k_valid
    args, kw = T.call_args(case, i, ops, A=Ad, B=Bd, move=lambda t: t.to(DEV))
    ops.GEMM_EVENTS = []
    try:
        got = ops.gemm_score(*args, **kw)
        label = ops.GEMM_EVENTS[-1][-1]
    finally:
        ops.GEMM_EVENTS = None
    return got, label


def test_case_table_reaches_every_path():
    """(no kernel runs) the table holds what the docstring says it does"""
    assert len({c.id for c in CASES}) == len(CASES)
    assert {c.M for c in CASES} == {192, 193, 256, 257, 449, 513}
    assert {-(-c.k_valid // 64) for c in CASES} == {5, 6, 8} and {c.K for c in CASES} == {320, 384, 512}
    assert {(c.P, c.ncols) for c in CASES} >= {(64, 3), (128, 5)}
    for M in (193, 257):                                     # both row-tile heights with both column bias forms and without
        assert {c.bias for c in CASES if c.M == M} >= {"n", "cn"}
    assert {c.bias for c in CASES} == {"none", "n", "cn"} and {c.keep_n for c in CASES} == {True, False} and {c.G for c in CASES} == {1, 2}
    tiles = lambda c: -(-c.M // (256 if c.M in (193, 256, 449) else 192)) * -(-c.ncols * c.P // 256) * c.G
    assert sorted(tiles(c) for c in CASES if tiles(c) > 256) == [258, 262] and not any(c.rows for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_scores_equal_parent_and_fp64(ops, golden, case):
    c = case
    assert ops.gemm_mixed_ok(c.M, c.ncols, c.G, c.gmod, c.P, c.k_valid)
    i = T.inputs(c)
    t = i["terms"]
    got, label = run_case(ops, c, i)
    assert label == ROUTE
    want = t["score"]
    assert got.shape == want.shape and got.dtype == torch.float32
    g32 = got.detach().cpu()
    # 1. the parent's bits
    assert c.id in golden, c.id
    assert torch.equal(g32.view(torch.int32), golden[c.id].view(torch.int32)), (c.id, int((g32 != golden[c.id]).sum()))
    # 2. fp64, per score
    g = g32.double()
    assert bool(torch.isfinite(g).all())
    bar = T.case_bar(c, t)
    err = (g - want).abs()
    ratio = err / bar
    k = int(ratio.argmax())
    worst = dict(err=float(err.view(-1)[k]), bar=float(bar.view(-1)[k]), ratio=float(ratio.view(-1)[k]), score=float(want.view(-1)[k]))
    print(f"{c.id}: err {worst['err']:.3e}, bar {worst['bar']:.3e}, err / bar {worst['ratio']:.3f} at score {worst['score']:.3e}")
    assert bool((err <= bar).all()), (c.id, worst, divmod(k, g.shape[1]))
    if c.kind == "hit":
        assert torch.equal(g.argmax(0), want.argmax(0)) and torch.equal(g.argmax(0), i["planted"])
