"""The fp64 references of the BRECQ training kernels (tests/brecq_kernel_reference.py) and their case table
(tests/brecq_kernel_cases.py), checked without a GPU:
  1. each reference equals fp64 torch.autograd of the module's formula (the fp32-decided roundings handed in, so that the forward is
     the decided one and differentiable) to 1e-12 of the tensor's largest value;
  2. the fp32 specifications of tests/cpu_backend.py (what the older GPU tests compare with) agree with it to fp32 rounding;
  3. the table's own conditions: every planted value is exactly what it claims, and the ``near`` masks cover at most 1e-4 of a case.
"""
import math

import pytest
import torch

from tests import brecq_kernel_cases as T
from tests import brecq_kernel_reference as R
from tests import cpu_backend as CB

F64 = torch.float64
EPS32 = 2.0 ** -24
NEAR_CAP = 1e-4


def _close(got, ref, tol=1e-12):
    scale = max(float(ref.abs().max()), 1e-300)
    assert float((got - ref).abs().max()) <= tol * scale, (float((got - ref).abs().max()), scale)


def _leaf(t):
    return None if t is None else t.detach().to(F64).requires_grad_(True)


# ------------------------------------------------------------------------------------------------ 1. against fp64 autograd
@pytest.mark.parametrize("case", T.UNIFORM_CASES, ids=lambda c: c.id)
def test_uniform_reference_is_fp64_autograd(case):
    i, ref = T.uniform_inputs(case), T.uniform_reference(case)
    x, s, z = _leaf(i["x"]), _leaf(i["s"]), _leaf(i["z"])
    y = R.uniform_formula(x, s, z, ref["dec"])
    y.backward(i["gy"].to(F64))
    assert torch.equal(x.grad.float(), ref["gx"])
    assert_scaled(s.grad, ref["gs"], ref["gs_abs"] + ref["gs_cond"] + 1e-300)
    if not case.sym:
        assert_scaled(z.grad, ref["gz"], ref["gz_abs"] + 1e-300)


def assert_scaled(got, ref, scale, tol=1e-12):
    assert float(((got - ref).abs() / scale.clamp(min=1e-300)).max()) <= tol


@pytest.mark.parametrize("case", T.LOG_CASES, ids=lambda c: c.id)
def test_log_reference_is_fp64_autograd(case):
    i, ref = T.log_inputs(case), T.log_reference(case)
    x, s = _leaf(i["x"]), _leaf(i["s"])
    y = R.log_formula(x, s.reshape(()), float(i["q"]), case.bits, None if i["shift"] is None else i["shift"].to(F64).reshape(()), case.sub_shift, case.pre_gelu,
                      ref["k_decided"], ref["dec"]["iu"].to(F64))
    y.backward(i["gy"].to(F64))
    _close(x.grad, ref["gx"])
    assert_scaled(s.grad, ref["gs"], ref["gs_abs"])


@pytest.mark.parametrize("soft", [True, False], ids=["soft", "hard"])
@pytest.mark.parametrize("case", T.ADAROUND_CASES, ids=lambda c: c.id)
def test_adaround_reference_is_fp64_autograd(case, soft):
    """Away from the decision points: elements where the fp64 clamps decide as the fp32 ones did (all but ``near`` and the planted
    saturations, where the gradient is 0 on both sides anyway)."""
    i, ref = T.adaround_inputs(case), T.adaround_reference(case, soft)
    a = _leaf(i["alpha"])
    y = R.adaround_formula(i["w"].to(F64), a, i["s"].to(F64), i["z"].to(F64), float(2 ** case.bits - 1), soft, ref["fl"])
    _close(y.detach(), ref["y"])
    if soft:
        y.backward(i["gy"].to(F64))
        keep = ~ref["near"]
        _close(a.grad[keep], ref["ga"][keep])


@pytest.mark.parametrize("b", T.ROUND_LOSS_BS)
@pytest.mark.parametrize("n", T.ROUND_LOSS_NS)
def test_round_loss_reference_is_fp64_autograd(n, b):
    ref = T.round_loss_reference(n, b)
    a = _leaf(T.round_loss_alpha(n))
    loss = R.round_loss_formula(a, b)
    loss.backward()
    assert abs(float(loss) - float(ref["loss"])) <= 1e-12 * max(float(ref["loss_abs"]), 1e-300)
    keep = ~ref["near"] & (T.round_loss_alpha(n) != 0)                   # (|.|'s subgradient at d = 0 is a convention: the reference says 0)
    if keep.any():
        _close(a.grad[keep], ref["grad"][keep])


def test_rec_loss_and_softmax_references_are_fp64_autograd():
    for n in T.REC_LOSS_NS:
        i = T.rec_loss_inputs(n, True)
        p = _leaf(i["pred"])
        loss = ((p - i["tgt"].to(F64)) ** 2).sum() * R.f32(i["scale"])
        (loss * float(i["gmul"].to(F64))).backward()
        assert abs(float(loss) - float(R.rec_loss(i["pred"], i["tgt"], i["scale"])["loss"])) <= 1e-12 * float(loss)
        _close(p.grad, R.rec_loss_backward(i["pred"], i["tgt"], i["scale"], i["gmul"])["gpred"])
    for rows, n in [(5, 65), (4, 197), (3, 1)]:
        i = T.softmax_inputs(rows, n)
        x = _leaf(i["x"])
        y = torch.softmax(x * R.f32(T.SOFTMAX_SCALE), -1)
        _close(y.detach(), R.scaled_softmax(i["x"], T.SOFTMAX_SCALE)["y"])
        y32 = y.detach().float()                                          # the backward kernel is handed the fp32 y
        want = R.scaled_softmax_backward(i["gy"], y32, T.SOFTMAX_SCALE)
        y.backward(i["gy"].to(F64))
        assert float(((x.grad - want["gx"]).abs().amax(-1) / want["row_abs"].clamp(min=1e-300)).max()) <= 4 * EPS32   # y rounded to fp32


def test_adam_reference_is_torch_adam_in_fp64():
    i = T.adam_inputs("mixed", False)
    h = T.ADAM_HYPER
    b1, b2 = R.f32(h["beta1"]), R.f32(h["beta2"])
    for step in T.ADAM_STEPS:
        ps = [p.to(F64).clone().requires_grad_(True) for p in i["p"]]
        opt = torch.optim.Adam(ps, lr=R.f32(h["lr"]), betas=(b1, b2), eps=R.f32(h["eps"]))
        for p_, g_, m_, v_ in zip(ps, i["g"], i["m"], i["v"]):
            p_.grad = g_.to(F64)
            opt.state[p_].update(step=torch.tensor(float(step)), exp_avg=m_.to(F64).clone(), exp_avg_sq=v_.to(F64).clone())
        opt.step()
        ref = R.adam(i["p"], i["g"], i["m"], i["v"], step, **h)
        assert ref["step"] == step + 1
        for p_, rp, rm, rv in zip(ps, ref["p"], ref["m"], ref["v"]):
            _close(p_.detach(), rp); _close(opt.state[p_]["exp_avg"], rm); _close(opt.state[p_]["exp_avg_sq"], rv)


# ------------------------------------------------------------------------------------ 2. the fp32 specifications of cpu_backend
@pytest.mark.parametrize("case", T.UNIFORM_CASES, ids=lambda c: c.id)
def test_cpu_backend_uniform_backward_agrees(case):
    i, ref = T.uniform_inputs(case), T.uniform_reference(case)
    gx, gs, gz = CB.uniform_fake_quant_backward(i["gy"], i["x"], i["s"], i["z"], case.bits, case.sym, True, True)
    # autograd's gy * s / s is gy to an ulp; its sums are fp32 sums of the same terms (pairwise, depth <= 32) of fp32-evaluated pieces
    torch.testing.assert_close(gx, ref["gx"], rtol=4 * EPS32, atol=0)
    assert_scaled(gs.to(F64), ref["gs"], 32 * ref["gs_abs"] + 8 * ref["gs_cond"] + 1e-300, EPS32)
    if not case.sym:
        assert_scaled(gz.to(F64), ref["gz"], 32 * ref["gz_abs"] + 1e-300, EPS32)


@pytest.mark.parametrize("case", [c for c in T.LOG_CASES if not c.pre_gelu], ids=lambda c: c.id)
def test_cpu_backend_log_backward_agrees(case):
    i, ref = T.log_inputs(case), T.log_reference(case)
    gx, gs = CB.log_fake_quant_backward(i["gy"], i["x"], None, i["s"], torch.tensor([i["q"]]), case.bits, i["shift"], case.sub_shift)
    # fp32 forms x + shift with one rounding: relative to xs that is eps (|x| + |shift|) / |xs|, and gx is proportional to 1 / xs
    sh = 0.0 if i["shift"] is None else float(i["shift"])
    xs = (i["x"].to(F64) + sh).abs().clamp(min=1e-300)
    allow = ref["gx"].abs() * (2 * EPS32 * (i["x"].abs().to(F64) + sh) / xs + 64 * EPS32) + 1e-30
    assert bool(((gx.to(F64) - ref["gx"]).abs() <= allow).all())
    assert_scaled(gs.to(F64), ref["gs"], ref["gs_abs"], 64 * EPS32)


@pytest.mark.parametrize("soft", [True, False], ids=["soft", "hard"])
@pytest.mark.parametrize("case", T.ADAROUND_CASES, ids=lambda c: c.id)
def test_cpu_backend_adaround_agrees(case, soft):
    i, ref = T.adaround_inputs(case), T.adaround_reference(case, soft)
    y = CB.adaround(i["w"], i["alpha"], i["s"], i["z"], case.bits, soft)
    _close(y.to(F64), ref["y"], 8 * EPS32)
    ga = CB.adaround(i["w"], i["alpha"], i["s"], i["z"], case.bits, soft, gy=i["gy"]).to(F64)
    err = (ga - ref["ga"]).abs()
    for alt in ref["ga_alts"]:
        err = torch.where(ref["near"], torch.minimum(err, (ga - alt).abs()), err)
    assert float(err.max()) <= 16 * EPS32 * max(float(ref["ga"].abs().max()), 1e-30)


@pytest.mark.parametrize("b", T.ROUND_LOSS_BS)
@pytest.mark.parametrize("n", T.ROUND_LOSS_NS)
def test_cpu_backend_round_loss_agrees(n, b):
    """fp32 pow of |d| with |d| itself 2^-24-accurate: |d|^b moves by b 2^-24 at most (absolute, |d| <= 1); the gradient likewise."""
    ref, alpha = T.round_loss_reference(n, b), T.round_loss_alpha(n)
    ga = torch.zeros_like(alpha)
    loss = CB.round_loss(alpha, b, galpha=ga)
    assert abs(float(loss) - float(ref["loss"])) <= (4 * b * ref["active"] + 32 * float(ref["loss_abs"])) * EPS32
    err = (ga.to(F64) - ref["grad"]).abs()
    err = torch.where(ref["near"], torch.minimum(err, (ga.to(F64) - ref["grad_alts"][0]).abs()), err)
    assert float(err.max()) <= 8 * b * b * EPS32
    val, grads = CB.round_loss_multi([alpha, alpha], b, 0.5)
    assert abs(float(val) - 2 * 0.5 * float(ref["loss"])) <= (4 * b * ref["active"] + 32 * float(ref["loss_abs"])) * EPS32
    assert torch.equal(grads[0], grads[1])


# ---------------------------------------------------------------------------------------------- 3. the table's own conditions
@pytest.mark.parametrize("case", [c for c in T.UNIFORM_CASES if c.planted], ids=lambda c: c.id)
def test_uniform_plants_are_exact(case):
    i, ref = T.uniform_inputs(case), T.uniform_reference(case)
    r32 = ref["dec"]["r32"].reshape(-1)
    L = 2 ** (case.bits - 1)
    qmin, qmax = (-L, L - 1) if case.sym else (0, 2 * L - 1)
    seen_t, ties = set(), set()
    assert i["plants"]
    for idx, r, ch in i["plants"]:
        assert float(r32[idx]) == r, (idx, float(r32[idx]), r)
        zr = 0.0 if i["z"] is None else float(torch.round(i["z"].reshape(-1)[ch]))
        if r == math.floor(r):
            seen_t.add(int(r + zr))
        else:
            ties.add(int(math.floor(r)) % 2)
    assert {qmin - 1, qmin, qmax} <= seen_t
    if _inner(case) >= 8:
        assert qmax + 1 in seen_t and ties == {0, 1}
    if not case.sym and case.z != "int":
        k = torch.floor(i["z"])
        assert bool((i["z"] - k == 0.5).all()) and bool(((k % 2) == (0 if case.z == "half_even" else 1)).all())


def _inner(case):
    return T._layout(case)[1]


@pytest.mark.parametrize("case", T.UNIFORM_INT_CASES, ids=lambda c: c.id)
def test_uniform_int_plants_are_exact_and_match_the_spec(case):
    i = T.uniform_int_inputs(case)
    ref = R.uniform_int(i["x"], i["s"], i["z"], case.bits)
    r32 = ref["dec"]["r32"]
    for j, r in enumerate(i["rs"][:case.n]):
        assert float(r32[(case.n - 1 - j) if j < 3 else j]) == r
    assert torch.equal(CB.uniform_int(i["x"], i["s"], i["z"], case.bits), ref["y"])


@pytest.mark.parametrize("case", T.LOG_CASES, ids=lambda c: c.id)
def test_log_plants_and_near_cap(case):
    i, ref = T.log_inputs(case), T.log_reference(case)
    assert float(ref["near"].float().mean()) <= NEAR_CAP
    if i["plants"]:
        xs = i["x"] if i["shift"] is None else i["x"] + i["shift"]
        ur = xs / i["s"]
        names = i["plants"]
        at = lambda name: names[name]
        assert float(xs[at("nonpos")]) <= 0
        if "tiny" in names:
            assert 0 < float(ur[at("tiny")]) < 1e-15 and 0 < float(i["x"][at("tiny")].double() / i["s"].double()) < 1e-15
        assert float(ur[at("one")]) == 1.0
        assert float(ur[at("above")]) > 1.0
        if (2 ** case.bits + 1) * case.q / 37.0 < 49:                  # (u is clamped at 1e-15 = 2^-49.8: wider tables have no bin past the last)
            assert not bool(ref["dec"]["mask"][at("past")]) and bool(ref["dec"]["iu"][at("past")])
        assert float(ref["gx"][at("nonpos")]) == 0 and float(ref["gx"][at("above")]) == 0 and float(ref["gx"][at("past")]) == 0


@pytest.mark.parametrize("case", T.ADAROUND_CASES, ids=lambda c: c.id)
def test_adaround_plants_and_near_cap(case):
    i, ref = T.adaround_inputs(case), T.adaround_reference(case, True)
    n = case.rows * case.inner
    assert float(ref["near"].float().sum()) <= max(NEAR_CAP * n, 0)
    q = (i["w"] / i["s"].view(-1, 1)).view(-1)
    for idx, want in i["plants"]:
        assert float(q[idx]) == want
    a = i["alpha"].view(-1)
    if n >= 30:
        for v in T.ALPHA_SPECIALS:
            hit = (a == v) & (torch.signbit(a) == (math.copysign(1.0, v) < 0))
            assert bool(hit.any()), v
    sh = R.soft_h(torch.tensor(T.ALPHA_SPECIALS))
    assert sh["lin"].tolist() == [True, True, True, True, False, False, False, False, False, False]
    assert sh["h"].tolist()[4:] == [1.0, 0.0, 1.0, 0.0, 1.0, 0.0]


def test_round_loss_softmax_and_alpha_step_tables():
    for n in T.ROUND_LOSS_NS:
        assert float(T.round_loss_reference(n, 20.0)["near"].float().sum()) <= NEAR_CAP * n
    for a in T.multi_alphas():
        assert float(R.soft_h(a)["near"].float().sum()) <= NEAR_CAP * a.numel()
    assert len(T.MULTI_NS) == 16
    seen = set()
    for n in T.SOFTMAX_NS:
        for rows in T.softmax_rows_for(n):
            seen.add(rows)
            i = T.softmax_inputs(rows, n)
            t = i["x"][torch.isfinite(i["x"])] * T.SOFTMAX_SCALE
            assert float(t.abs().max()) <= 161
    assert seen == set(T.SOFTMAX_ROWS)
    i = T.softmax_inputs(5, 65)
    t = i["x"][4] * T.SOFTMAX_SCALE
    assert i["kinds"][4] == "dominant" and float(t.max()) == 80.0 and float(t.min()) < -100          # exponentials that underflow in fp32
    for case in T.ALPHA_STEP_CASES[:4]:
        inp = T.alpha_step_inputs(case)
        for L in inp["layers"]:
            g = R.alpha_grad(L["w"], L["alpha"], L["gw"], L["s"], L["z"], L["bits"], case.b, inp["weight"], inp["gmul"], inp["gate"])
            assert float(g["near"].float().sum()) <= NEAR_CAP * L["w"].numel()
