"""`-m gpu`: the Gram-form search kernels -- csrc/gram.hip (weight search: adalog_gram_build, the three-call sharded build,
adalog_gram_score_w) and csrc/gram_act.hip (activation search) -- against the fp64 references of tests/gram_reference.py on the case
tables of tests/gram_cases.py.  Every comparison is PER SCORE; nothing is normalised across output columns or candidates.

Weight search: |got - spec| <= gram_reference.weight_bar = 2^-24 |spec| + 2^-150 + 16 x 2^-53 norm (S0 + 2 sigma |lin| + sigma^2 quad)
(the count of fp64 operations is in weight_bar's docstring), spec = the exact-integer specification cpu_backend.GramState extended by
its three terms.  The specification itself is checked against the plain fp64 token form in tests/test_gram_cases_cpu.py and, for the
``big`` cases whose reference runs on the device, here.

Activation search: per candidate, bar = max(gram_reference.act_bound, 4 x the error of the fp32 token-form route against the same
fp64 reference on the same case) -- ops.score_act_gen where it takes the shape (and both widths are equal, as the searches call it),
else the ATen fp32 evaluation of the formula on the device.  The kernel's own output never sets a bar.

Worst case of each group on an MI355X, error and bar as fractions of norm x the sum of the score's terms (the tests print every
case's figures with `-s` and write them to gram_edges_parity.jsonl next to the suite's other parity logs).  The weight figures sit
just under their bars because both are the one fp32 rounding of the score: the fp64 part of the bar is ~2e-15.
  weight  shapes       rand_K32_T127_O1025_P256_a3w6        error 2.70e-09   bar 2.71e-09
          reuse        rand_K256_T129_O192_P128_a4w4_b            1.05e-09       1.05e-09
          bits         bits_K128_T200_O5_P64_a2w2_b               9.09e-09       9.35e-09
          saturation   sat_alt_K768_T128_O4_P96_a7w6_b            5.90e-08       5.96e-08
          limbs        satx_K32_T15_O4_P32_a2w4                   5.75e-08       5.96e-08
          exponent     expo_K64_T100_O12_P32_a4w4_b               4.99e-10       5.15e-10
          strides      rand_K256_T129_O192_P128_a4w4_b            2.45e-09       2.47e-09   (and equal to the contiguous call)
          sharded      shard_K96_T377_O5_P64_a6w6_b               6.19e-10       6.58e-10
  activation (token form: ATen fp32 at every case -- ops.score_act_gen takes none of these small shapes)
          shapes       rand_K32_T1_O3_P1_a4w4               kernel 6.10e-10  token form 2.62e-11  bar 1.64e-09
          candidates   rand_K64_T100_O20_P128_a3w3_b               4.83e-09             5.12e-09      2.70e-08
          bits         rand_K96_T150_O30_P32_a2w2_b                1.30e-08             1.30e-08      5.18e-08
          sort/prefix  clamp_K64_T100_O16_P63_a4w4_b               1.65e-08             1.65e-08      6.60e-08
          weights      wsat_K64_T100_O16_P32_a4w7_b                1.90e-08             1.90e-08      7.59e-08
"""
import json
import os

import pytest
import torch

from tests import cpu_backend as CB
from tests import gram_cases as T
from tests import gram_reference as R
from tests.test_gpu_golden_forward import LOG as _GOLDEN_LOG

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOG = os.path.join(os.path.dirname(_GOLDEN_LOG), "gram_edges_parity.jsonl")
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


def _last_kernel():
    from adalog_amd import _lib
    return _lib.load().adalog_last_kernel().decode()


def d(t):
    return None if t is None else t.to(DEV).contiguous()


def _to(i, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in i.items()}


def _weight_terms(case, i, sc=None):
    """the reference's terms [P, O] (fp64, on the CPU): a big case is evaluated on the device, and its specification checked against
    the token form there (the CPU tier does that on a slice of the candidates)"""
    j = _to(i, DEV) if case.big else i
    ref = R.WeightRef(j["x"], j["sa"], j["za"], case.a_bits, j["ref"].t().contiguous(), j["bias"])
    s = j["sc"] if sc is None else sc.to(j["sc"].device)
    t = ref.terms(j["W"], s, j["zp"], case.w_bits, i["norm"])
    if case.big:
        tok, tok_abs = ref.token_form(j["W"], s, j["zp"], case.w_bits, i["norm"])
        assert bool(((t["score"] - tok).abs() <= R.weight_selfcheck_bound(ref, t, tok, tok_abs, i["norm"])).all())
    return {k: v.cpu() for k, v in t.items()}


def _judge_w(group, case_id, got, t, norm, what="score"):
    got = got.detach().cpu().double()
    assert got.shape == t["score"].shape and bool(torch.isfinite(got).all())
    err, bar = (got - t["score"]).abs(), R.weight_bar(t, norm)
    A = norm * (t["S0"] + t["lin2"] + t["quad"]) + R.TINY32
    k = int((err / bar).argmax())
    worst = dict(err=float((err / A).view(-1)[k]), bar=float((bar / A).view(-1)[k]), ratio=float((err / bar).view(-1)[k]))
    _log(group=group, case=case_id, what=what, **worst)
    print(f"{group} {case_id} {what}: err {worst['err']:.3e}, bar {worst['bar']:.3e} (of the terms' sum), err / bar {worst['ratio']:.3f}")
    assert bool((err <= bar).all()), (group, case_id, what, worst, divmod(k, got.shape[1]))


def _group(case):
    return {"rand": "shapes", "sat": "saturation", "sat_alt": "saturation", "satx": "limbs", "expo": "exponent"}[case.kind] \
        if not case.id.startswith("bits") else "bits"


# ---------------------------------------------------------------------------------------------------------------- weight search
@pytest.mark.parametrize("case", T.W_CASES, ids=lambda c: c.id)
def test_gram_score_w_per_element(ops, case):
    """1a-1e and 1h: every score of [P, O] within weight_bar of the specification."""
    i = T.weight_inputs(case)
    lib = ops._lib.load()
    assert lib.adalog_gram_supported(case.T, case.O, case.K, case.a_bits, case.w_bits, case.P)
    assert lib.adalog_gram_limbs(case.T, case.a_bits) == R.g_limbs(case.T, case.a_bits)
    st = ops.GramState(d(i["x"]), d(i["sa"]), d(i["za"]), case.a_bits, d(i["ref"].t()), d(i["bias"]))
    Wd, scd, zpd = d(i["W"]), d(i["sc"]), d(i["zp"])
    got = st.score_w(Wd, scd, zpd, case.w_bits, i["norm"])
    assert _last_kernel() == "k_gram_score<i8>"
    t = _weight_terms(case, i)
    _judge_w(_group(case), case.id, got, t, i["norm"])
    if case.kind == "expo":
        # raw_out == bias: S0 = c = 0 and the score is -norm sigma^2 w^T G w to fp32 rounding
        want = (-t["quad"][:, 4] * i["norm"])
        assert bool(((got[:, 4].cpu().double() - want).abs() <= 2.0 ** -24 * want.abs() * (1 + 2.0 ** -20)).all())
    if case.reuse:
        # a second step from the same state with another grid, then the first again: bit for bit
        sc2 = i["sc"] * 1.01
        got2 = st.score_w(Wd, d(sc2), zpd, case.w_bits, i["norm"])
        _judge_w("reuse", case.id, got2, _weight_terms(case, i, sc2), i["norm"], "second grid")
        assert torch.equal(got, st.score_w(Wd, scd, zpd, case.w_bits, i["norm"]))


def test_gram_form_rejects_widths_it_cannot_carry(ops):
    lib = ops._lib.load()
    for args in T.W_REJECTED:
        assert not lib.adalog_gram_supported(*args) and not lib.adalog_gram_ok(*args), args
    assert lib.adalog_gram_supported(128, 4, 256, 7, 7, 64)


def test_nan_in_one_column_stays_there(ops):
    """a NaN in one column of raw_out leaves every other column's scores unchanged bit for bit"""
    case = T.W_SHAPES[5]                                    # K = 64, O = 7
    i = T.weight_inputs(case)

    def run(ref):
        st = ops.GramState(d(i["x"]), d(i["sa"]), d(i["za"]), case.a_bits, d(ref.t()), d(i["bias"]))
        return st.score_w(d(i["W"]), d(i["sc"]), d(i["zp"]), case.w_bits, i["norm"]).cpu()

    clean = run(i["ref"])
    bad = i["ref"].clone()
    bad[case.T // 2, 2] = float("nan")
    got = run(bad)
    keep = [o for o in range(case.O) if o != 2]
    assert bool(torch.isfinite(clean).all()) and torch.equal(got[:, keep], clean[:, keep])


def _ws(ops, lib, T_, O, K, a_bits):
    nb = lib.adalog_gram_workspace_bytes(T_, O, K, a_bits)
    assert nb > 0
    return ops._aligned_bytes(nb, DEV), nb


def _score_direct(lib, W, ldw, O, K, sc, zp, P, w_bits, ws, T_, a_bits, sa, norm):
    from adalog_amd.ops import _stream
    out = torch.empty((P, O), dtype=torch.float32, device=DEV)
    rc = lib.adalog_gram_score_w(W.data_ptr(), O, K, ldw, sc.data_ptr(), zp.data_ptr(), P, w_bits, ws.data_ptr(), T_, a_bits, sa.data_ptr(),
                                 float(norm), out.data_ptr(), _stream())
    assert rc == 0, lib.adalog_last_error()
    return out


@pytest.mark.parametrize("case", [T.W_SHAPES[5], T.W_SHAPES[12]], ids=lambda c: c.id)
def test_row_strides_wider_than_k(ops, case):
    """1f: adalog_gram_build / adalog_gram_score_w through the C ABI with ldx > K and ldw > K (multiples of 4, 16-byte aligned bases):
    equal to the contiguous call, whatever lies between the rows."""
    from adalog_amd.ops import _stream
    lib = ops._lib.load()
    i = T.weight_inputs(case)
    Tn, O, K, P = case.T, case.O, case.K, case.P
    sa, za, sc, zp, b, ref_t = d(i["sa"]), d(i["za"]), d(i["sc"]), d(i["zp"]), d(i["bias"]), d(i["ref"].t())
    outs = []
    for ldx, ldw in ((K, K), (K + 12, K + 8)):
        x = torch.full((Tn, ldx), 1.0e30, device=DEV); x[:, :K] = d(i["x"])
        W = torch.full((O, ldw), -1.0e30, device=DEV); W[:, :K] = d(i["W"])
        assert x.data_ptr() % 16 == 0 and W.data_ptr() % 16 == 0
        ws, nb = _ws(ops, lib, Tn, O, K, case.a_bits)
        rc = lib.adalog_gram_build(x.data_ptr(), Tn, K, ldx, sa.data_ptr(), za.data_ptr(), case.a_bits, ref_t.data_ptr(), O,
                                   None if b is None else b.data_ptr(), ws.data_ptr(), nb, _stream())
        assert rc == 0, lib.adalog_last_error()
        outs.append(_score_direct(lib, W, ldw, O, K, sc, zp, P, case.w_bits, ws, Tn, case.a_bits, sa, i["norm"]))
    assert torch.equal(outs[0], outs[1])
    _judge_w("strides", case.id, outs[1], _weight_terms(case, i), i["norm"])


@pytest.mark.parametrize("s", T.S_CASES, ids=lambda s: s.id)
def test_sharded_build_in_one_process(ops, s):
    """1g: adalog_gram_amax / adalog_gram_build_sums per shard, the sums added as the ranks' all-reduce would, then
    adalog_gram_build_from_sums and a score.  G and c are integer sums: the same limbs as the one-call build's.  S0 is an fp64 sum of
    the shards' shares: where the first shard ends on a boundary of k_gram_rfix's 8192-token chunks the shares ARE the one-call build's
    chunk sums, added in the same order, and the scores are equal bit for bit (``equal``); otherwise S0 differs by fp64 rounding and
    the scores meet the per-element bar against the specification, as the one-call build's do."""
    from adalog_amd.ops import _stream
    lib = ops._lib.load()
    case = T.shard_case(s)
    i = T.weight_inputs(case)
    Tn, O, K, P = case.T, case.O, case.K, case.P
    sa, za, b = d(i["sa"]), d(i["za"]), d(i["bias"])
    bounds = [0]
    for n in s.shards:
        bounds.append(bounds[-1] + n)
    parts = []
    for lo, hi in zip(bounds, bounds[1:]):
        parts.append((hi - lo, d(i["x"][lo:hi]), d(i["ref"][lo:hi].t())))
    amax = None
    for n, _, rt in parts:
        am = torch.empty(O, dtype=torch.int32, device=DEV)
        assert lib.adalog_gram_amax(rt.data_ptr(), n, O, b.data_ptr(), am.data_ptr(), _stream()) == 0
        amax = am if amax is None else torch.maximum(amax, am)
    gsum = torch.zeros((K, K), dtype=torch.int64, device=DEV)
    csum = torch.zeros((O, K), dtype=torch.int64, device=DEV)
    s0 = None
    for n, x, rt in parts:
        g1, c1, s1 = torch.empty_like(gsum), torch.empty_like(csum), torch.empty(O, dtype=torch.float64, device=DEV)
        ws, nb = _ws(ops, lib, n, O, K, case.a_bits)
        rc = lib.adalog_gram_build_sums(x.data_ptr(), n, K, K, sa.data_ptr(), za.data_ptr(), case.a_bits, rt.data_ptr(), O, b.data_ptr(),
                                        amax.data_ptr(), g1.data_ptr(), c1.data_ptr(), s1.data_ptr(), ws.data_ptr(), nb, _stream())
        assert rc == 0, lib.adalog_last_error()
        gsum += g1; csum += c1
        s0 = s1 if s0 is None else s0 + s1
    ws, nb = _ws(ops, lib, Tn, O, K, case.a_bits)
    rc = lib.adalog_gram_build_from_sums(gsum.data_ptr(), csum.data_ptr(), s0.data_ptr(), amax.data_ptr(), Tn, O, K, case.a_bits,
                                         ws.data_ptr(), nb, _stream())
    assert rc == 0, lib.adalog_last_error()
    got = _score_direct(lib, d(i["W"]), K, O, K, d(i["sc"]), d(i["zp"]), P, case.w_bits, ws, Tn, case.a_bits, sa, i["norm"])
    assert _last_kernel() == "k_gram_score<i8>"
    if s.id == "limbs_2_2_to_3":
        assert [lib.adalog_gram_limbs(n, case.a_bits) for n in s.shards + (Tn,)] == [2, 2, 3]
    # the integer sums against the specification's
    ref = R.WeightRef(i["x"], i["sa"], i["za"], case.a_bits, i["ref"].t().contiguous(), i["bias"])
    assert torch.equal(gsum.cpu(), ref.G.to(torch.int64)) and torch.equal(csum.cpu(), ref.c.to(torch.int64))
    t = ref.terms(i["W"], i["sc"], i["zp"], case.w_bits, i["norm"])
    _judge_w("sharded", case.id, got, t, i["norm"])
    one = ops.GramState(d(i["x"]), sa, za, case.a_bits, d(i["ref"].t()), b).score_w(d(i["W"]), d(i["sc"]), d(i["zp"]), case.w_bits, i["norm"])
    if s.equal:
        assert torch.equal(got, one)
    else:
        assert bool(((got - one).abs().cpu().double() <= 2 * R.weight_bar(t, i["norm"])).all())


# ---------------------------------------------------------------------------------------------------------------- activation search
def _aten_act(i, case, dev=DEV):
    """the module's formula in fp32 ATen ops on the device, candidate by candidate"""
    x, W, ref = i["x"].to(dev), i["W"].to(dev), i["ref"].to(dev)
    sw, zw = i["sw"].to(dev).view(-1, 1), torch.round(i["zw"].to(dev)).view(-1, 1)
    Wq = ((torch.round(W / sw) + zw).clamp(0, 2 ** case.w_bits - 1) - zw) * sw
    r = ref - (i["bias"].to(dev).view(1, -1) if i["bias"] is not None else 0.0)
    out = []
    for s_, z_ in zip(i["sc"].to(dev), torch.round(i["zp"]).to(dev)):
        xq = (torch.round(x / s_) + z_).clamp(0, 2 ** case.a_bits - 1) - z_
        out.append(-i["norm"] * ((r - (xq @ Wq.t()) * s_) ** 2).sum())
    return torch.stack(out)


def _token_form_act(ops, case, i):
    from adalog_amd.ops import FP8, I8
    if case.a_bits == case.w_bits:
        dt = FP8 if case.w_bits <= 4 else I8
        wp = ops.pack_uniform(d(i["W"]).unsqueeze(0), d(i["sw"]), d(i["zw"]), 1, 0, 1, 0, 1, case.w_bits, dt)
        if ops.score_act_gen_ok(dt, case.O, case.T, case.K, wp.shape[-1], case.P):
            P = case.P
            return "score_act_gen", ops.score_act_gen(dt, wp, d(i["x"]), d(i["sc"]).view(P, 1), d(i["zp"]).view(P, 1), case.a_bits,
                                                      d(i["ref"]), d(i["sw"]), d(i["bias"]), i["norm"]).view(-1)
    return "aten_fp32", _aten_act(i, case)


def _a_group(case):
    k = T.A_CASES.index(case)
    return "shapes" if k < 15 else "candidates" if k < 21 else "bits" if k < 27 else "sort_prefix" if k < 34 else "weights"


@pytest.mark.parametrize("case", T.A_CASES, ids=lambda c: c.id)
def test_gram_act_score_per_candidate(ops, case):
    """2a-2f: every candidate's score within max(act_bound, 4 x the token-form route's error) of the fp64 direct sum; a second score
    call returns the same bits."""
    i = T.act_inputs(case)
    lib = ops._lib.load()
    P = case.P
    assert lib.adalog_gram_act_supported(case.T, case.O, case.K, case.a_bits, case.w_bits, P)
    prep = ops.GramActPrepared(d(i["x"]))
    st = ops.GramActState(prep, d(i["ref"]), d(i["bias"]), d(i["W"]), d(i["sw"]), d(i["zw"]), case.w_bits, case.a_bits, P)
    scd, zpd = d(i["sc"]).view(P, 1), d(i["zp"]).view(P, 1)
    got = st.score(scd, zpd, i["norm"])
    assert _last_kernel() == "k_gram_act<i8>" and got.shape == (P, 1)
    assert torch.equal(got, st.score(scd, zpd, i["norm"]))
    j = _to(i, DEV) if case.big else i
    ref = R.ActRef(j["x"], j["ref"], j["bias"], j["W"], j["sw"], j["zw"], case.w_bits, case.a_bits)
    t = {k: v.cpu() for k, v in ref.terms(j["sc"], j["zp"], i["norm"]).items()}
    route, tok = _token_form_act(ops, case, i)
    got, tok = got.view(-1).cpu().double(), tok.detach().cpu().double()
    assert bool(torch.isfinite(got).all())
    k_err, a_err, bound = (got - t["score"]).abs(), (tok - t["score"]).abs(), R.act_bound(ref, t, i["norm"]).cpu()
    bar = torch.maximum(bound, 4 * a_err)
    A = i["norm"] * (t["S0"] + t["lin_abs"] + t["quad_abs"]) + R.TINY32
    k = int((k_err / bar).argmax())
    worst = dict(kernel_err=float((k_err / A)[k]), token_err=float((a_err / A)[k]), bound=float((bound / A)[k]), bar=float((bar / A)[k]),
                 ratio=float((k_err / bar)[k]))
    _log(group="act_" + _a_group(case), case=case.id, route=route, **worst)
    print(f"act_{_a_group(case)} {case.id} [{route}]: kernel {worst['kernel_err']:.3e}, token form {worst['token_err']:.3e}, "
          f"bound {worst['bound']:.3e}, bar {worst['bar']:.3e} (of the terms' sum), err / bar {worst['ratio']:.3f}")
    assert bool((k_err <= bar).all()), (case.id, k, worst)
