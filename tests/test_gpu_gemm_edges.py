"""`-m gpu`: the packed-candidate scoring kernels behind adalog_gemm_score (csrc/gemm_score.hip: route_of, and the gemm_k_*.inc
families) against the fp64 reference of tests/gemm_reference.py on the case table of tests/gemm_cases.py.  Every comparison is PER
SCORE: |got - score| <= gemm_reference.bar, an analytic bound from the roundings counted in the kernel source (bar's docstring);
nothing is normalised across candidates, columns or heads, and the kernel's output never sets a bar.

Per case: one ops.gemm_score call, the exact kernel label, shape; every score within its bar; ``hit``: the argmax over the candidates
is the planted one, as in the reference; ``nan``: the set of NaN scores equals the reference's exactly and every other score is within
its bar; a second identical call returns the same bits.

Each case's worst err, bar and err / bar are printed with `-s` and written to gemm_edges_parity.jsonl next to the suite's other
parity logs.  Worst row of each route on an MI355X (records, not bars):
  k_gemm_cand_glds            cand_glds-i8-M65-n3-P128-K1100-G1.1-n-ext                  err 2.42e+01   bar 3.14e+02   err / bar 0.077
  k_gemm_grpk8<bf16xfp8>      grpk8.bf16xfp8-bf16xfp8-M129-n1-P128-K256-G8.1--hit        err 1.47e-05   bar 6.11e-04   err / bar 0.024
  k_gemm_grpk8t<13,bf16xfp8>  grpk8t.13,bf16xfp8-bf16xfp8-M129-n1-P128-K193-G8.1--hit    err 1.78e-05   bar 6.44e-04   err / bar 0.028
  k_gemm_grpk8t<14,bf16xfp8>  grpk8t.14,bf16xfp8-bf16xfp8-M129-n1-P128-K208-G8.1--hit    err 2.28e-05   bar 7.56e-04   err / bar 0.030
  k_gemm_grpk<bf16>           grpk.bf16-bf16-M224-n1-P128-K224-G8.1--hit                 err 7.91e-05   bar 2.52e-03   err / bar 0.031
  k_gemm_grpw<fp8>            grpw.fp8-fp8-M129-n1-P64-K1-G8.1--hit                      err 1.04e-02   bar 2.04e-01   err / bar 0.051
  k_gemm_grpw<i8>             grpw.i8-i8-M129-n1-P64-K1-G8.1--spread                     err 3.80e-08   bar 8.48e-07   err / bar 0.045
  k_gemm_score                score-i8-M33-n17-P2-K1100-G2.1-nbn-ext                     err 2.17e+01   bar 2.73e+02   err / bar 0.079
  k_gemm_slab128<fp8>         slab128.fp8-fp8-M800-n3-P128-K385-G1.1-n-nan               err 2.50e-08   bar 1.33e-06   err / bar 0.019
  k_gemm_slab128<i8>          slab128.i8-i8-M800-n3-P128-K768-G1.1-n-hit                 err 5.31e-01   bar 2.85e+01   err / bar 0.019
  k_gemm_slab<fp8>            slab.fp8-fp8-M800-n1-P64-K65-G1.1-nrbn-hit                 err 7.59e-02   bar 5.08e+00   err / bar 0.015
  k_gemm_slab<i8>             slab.i8-i8-M800-n5-P64-K384-G1.1-rbn-hit                   err 1.31e+01   bar 7.76e+02   err / bar 0.017
  k_gemm_stream<bf16>         stream.bf16-bf16-M127-n1-P256-K1-G4.2-h-spread             err 1.74e-10   bar 2.50e-09   err / bar 0.070
  k_gemm_stream<bf16xfp8>     stream.bf16xfp8-bf16xfp8-M256-n1-P64-K257-G2.1--hit        err 6.55e-05   bar 2.25e-03   err / bar 0.029
  k_gemm_stream<f32>          stream.f32-f32-M1-n5-P128-K1-G4.2-hr-spread                err 1.47e-12   bar 2.71e-11   err / bar 0.054
  k_gemm_stream<fp8>          stream.fp8-fp8-M1-n5-P64-K1-G1.1-rbn-hit                   err 7.52e-06   bar 9.83e-05   err / bar 0.076
  k_gemm_stream<i8>           stream.i8-i8-M1-n1-P64-K65-G1.1-nr-spread                  err 8.35e-11   bar 1.01e-09   err / bar 0.083
  k_gemm_win<fp8>             win.fp8-fp8-M33-n1-P64-K33-G256.32-h-nan                   err 6.65e-07   bar 7.30e-06   err / bar 0.091
  k_gemm_win<i8>              win.i8-i8-M32-n1-P128-K32-G258.3--ext                      err 5.73e-02   bar 7.03e-01   err / bar 0.082
  k_gemm_winb<bf16xfp8>       winb.bf16xfp8-bf16xfp8-M5-n3-P128-K1-G256.4-h-spread       err 9.67e-09   bar 1.55e-07   err / bar 0.063
"""
import json
import os

import pytest
import torch

from tests import gemm_cases as T
from tests.test_gpu_golden_forward import LOG as _GOLDEN_LOG

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOG = os.path.join(os.path.dirname(_GOLDEN_LOG), "gemm_edges_parity.jsonl")
_log_started = []


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import backend
    backend.set_backend(None)
    return backend.get()


def _log(**row):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a" if _log_started else "w") as f:
        f.write(json.dumps(row) + "\n")
    _log_started.append(1)


def _call(ops, case, i, Ad, Bd):
    args, kw = T.call_args(case, i, ops, A=Ad, B=Bd, move=lambda t: t.to(DEV))
    ops.GEMM_EVENTS = []                                    # (reports the kernel behind the launch on either binding)
    try:
        got = ops.gemm_score(*args, **kw)
        label = ops.GEMM_EVENTS[-1][-1]
    finally:
        ops.GEMM_EVENTS = None
    return got, label


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_scores_per_score(ops, case):
    c = case
    if c.route.startswith("k_gemm_win<"):
        assert ops.gemm_win_ok(c.dtype, c.M, c.ncols, c.G, c.gmod, c.P, c.k_valid) == (c.k_valid <= 32) == (c.K == 32)
    if c.dtype == T.BF16_FP8:
        assert ops.gemm_mixed_ok(c.M, c.ncols, c.G, c.gmod, c.P, c.k_valid)
        assert (ops.gemm_mixed_ktrim(c.M, c.ncols, c.G, c.gmod, c.P, c.k_valid) == 208) == (192 < c.k_valid <= 208)
    i = T.inputs(c)
    t = i["terms"]
    Ad, Bd = i["A"].to(DEV), i["B"].to(DEV)
    Ad.k_valid = c.k_valid; Bd.k_valid = c.k_valid
    got, label = _call(ops, c, i, Ad, Bd)
    assert label == c.route
    again, _ = _call(ops, c, i, Ad, Bd)
    want = t["score"]
    assert got.shape == want.shape and got.dtype == torch.float32
    g = got.detach().cpu().double()
    nan_want = torch.isnan(want)
    if c.kind == "nan":
        assert bool(nan_want.any())
        assert torch.equal(torch.isnan(g), nan_want), (c.id, torch.isnan(g).nonzero().tolist()[:8], nan_want.nonzero().tolist()[:8])
    else:
        assert not bool(nan_want.any()) and bool(torch.isfinite(g).all())
    ok = ~nan_want
    bar = T.case_bar(c, t)
    err = (g - want).abs()
    ratio = torch.where(ok, err / bar, torch.zeros_like(err))
    k = int(ratio.argmax())
    worst = dict(err=float(err.view(-1)[k]), bar=float(bar.view(-1)[k]), ratio=float(ratio.view(-1)[k]), score=float(want.view(-1)[k]))
    _log(route=c.route, case=c.id, **worst)
    print(f"{c.route} {c.id}: err {worst['err']:.3e}, bar {worst['bar']:.3e}, err / bar {worst['ratio']:.3f} at score {worst['score']:.3e}")
    assert bool((err[ok] <= bar[ok]).all()), (c.id, worst, divmod(k, g.shape[1]))
    if c.kind == "hit":
        assert torch.equal(g.argmax(0), want.argmax(0)) and torch.equal(g.argmax(0), i["planted"])
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
