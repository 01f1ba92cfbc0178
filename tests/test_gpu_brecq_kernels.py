"""`-m gpu`: the elementwise and reduction kernels of csrc/brecq.hip -- quantiser backward passes, AdaRound, the rounding regulariser,
the reconstruction loss, the scaled softmax and the two one-launch optimiser steps -- through the public ``backend.get()`` entries,
against the fp64 references of tests/brecq_kernel_reference.py on the case table of tests/brecq_kernel_cases.py.

Exact: uniform_int, gx of the uniform backward, AdaRound's hard forward, adaround_t against adaround, the step counters, and every
reduction bit for bit over two launches; the gradients of round_loss and round_loss_multi bit for bit against each other.

Everything else has a bar that is the larger of (a) a bound derived from the kernel's arithmetic and (b) 4 x the error, against the
same fp64 reference, of the ATen fp32 composition of the module's formula on the same device and inputs (tests/cpu_backend.py's
specifications run on the device; the factor 4 as in test_gpu_brecq_grads.py: another summation order is not an error).  The
kernel's own output never sets a bar.  Elementwise outputs are compared element by element, none skipped, the error normalised by
the tensor's (softmax: the row's) natural scale from the reference; an element of the reference's ``near`` mask may equal any of its
admissible values, to the same bar.  Reductions: |got - ref| / sum |term|.  With E = 2^-24 the bounds (a) are:
  uniform gscale   E (18 + 2 sum|gy r| / sum|term|): r = fl(x / s) carries E |r| into (q - z) - r; <= 8 serial adds per thread and row,
                   6 shuffles, 2 adds across waves (then fp64); one rounding of the product.  gzp: 18 E.
  AdaLog gx        200 E: the exponent k q / 37 <= 126 takes E twice (q / 37, the product), i.e. 2 ln2 126 E on 2^-kq/37; hardware exp2
                   and rcp an ulp each; GELU' a few.  On top, per element, the conditioning of xs = fl(v + shift): 6 E (|v| + |shift|) / |xs|
                   of the value (gx is proportional to 1 / xs).  gscale: E (16 + 200) of the sum of the PIECES' magnitudes, plus what the
                   admissible bins of the ``near`` elements move.
  AdaRound y       8 E of max|y| (t = floor + h + z rounded at qmax; h to ~3 E);  d/d alpha 16 E: sigmoid through the fast exp
                   ((1.44 |a| + 3) E, |a| <= 2.4 where the gradient is not 0), 1 - sg amplifies sg's rounding 12-fold at most.
  regulariser      |d|^e by exp2(e log2 |d|): 1.5 x 2^-23 max(u |ln u|) + one rounding, <= 4 E absolute; |d| itself to 8 E, so a term moves by
                   (8 b + 4) E and a gradient, relative to its natural scale 0.6 b, by (8 b + 12) E.  Value: those over the unsaturated
                   elements plus 16 E sum|term| of fp32 summation.
  rec_loss         20 E (three roundings per term, depth <= 16);  its gradient 4 E.
  softmax          E (2 T + 30) per row, T = max |x scale| of the row (fl(x scale) moves the exponent by E T, twice: t_i and the maximum),
                   22 adds, expf and the quotient;  backward E 26 of |scale| sum_j |gy_j y_j|.
  Adam             m, v: 4 E.  The update: E (12 + 4 beta1^t / bc1 + 2 beta2^t / bc2) -- the bias corrections 1 - beta^t are formed in
                   fp32 on the device (t = 2: 1 - 0.998 keeps 9 bits fewer) -- of max|update|, and E |p| for the final rounding of p.
  alpha_step       the Adam bound plus 4 x (regulariser gradient + AdaRound d/d alpha): with sqrt(v) >= sqrt(1 - beta2) |g| the update
                   moves by at most ~3.2 times the relative error of g.
Both routes' figures go, one JSON line per case and quantity, to brecq_kernels_parity.jsonl next to the suite's other parity logs.
"""
import json
import os

import pytest
import torch

from tests import brecq_kernel_cases as T
from tests import brecq_kernel_reference as R
from tests import cpu_backend as CB
from tests.test_gpu_golden_forward import LOG as _GOLDEN_LOG

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOG = os.path.join(os.path.dirname(_GOLDEN_LOG), "brecq_kernels_parity.jsonl")
E = 2.0 ** -24
F64 = torch.float64
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


def dv(t):
    return None if t is None else t.to(DEV)


def c64(t):
    return t.detach().cpu().to(F64)


def _elem(got, ref, scale, alts=(), near=None, allow=None):
    """max over ALL elements of |got - ref| / scale; a ``near`` element takes the smallest distance to its admissible values; ``allow``
    (per element, from the inputs' conditioning) is subtracted first.  scale: a float or a tensor broadcastable to ref."""
    got = c64(got).reshape(ref.shape)
    err = (got - ref).abs()
    for alt in alts:
        err = torch.where(near, torch.minimum(err, (got - alt).abs()), err)
    if allow is not None:
        err = (err - allow).clamp(min=0)
    assert bool(torch.isfinite(got).all())
    return float((err / scale).max())


def _judge(kernel, case, quantity, k_err, a_err, bound):
    bar = max(bound, 4 * a_err)
    _log(kernel=kernel, case=case, quantity=quantity, kernel_err=k_err, aten_err=a_err, bound_a=bound, bar=bar)
    print(f"{kernel} {case} {quantity}: kernel {k_err:.3e}, ATen {a_err:.3e}, (a) {bound:.3e}, bar {bar:.3e}")
    assert k_err <= bar, (kernel, case, quantity, k_err, a_err, bound)


def _max(ref, floor=1e-300):
    return max(float(ref.abs().max()), floor)


# ---------------------------------------------------------------------------------------------------------------- uniform
@pytest.mark.parametrize("case", T.UNIFORM_CASES, ids=lambda c: c.id)
def test_uniform_backward(ops, case):
    i, ref = T.uniform_inputs(case), T.uniform_reference(case)
    args = (dv(i["gy"]), dv(i["x"]), dv(i["s"]), dv(i["z"]), case.bits, case.sym, True, not case.sym)
    gx, gs, gz = ops.uniform_fake_quant_backward(*args)
    gx2, gs2, gz2 = ops.uniform_fake_quant_backward(*args)
    assert torch.equal(gx.cpu(), ref["gx"]), "gx is gy or 0"
    assert torch.equal(gs, gs2) and (gz is None or torch.equal(gz, gz2)), "reductions are reproducible"
    ax, as_, az = CB.uniform_fake_quant_backward(*args)
    if case.gy == "zero":
        assert not gs.any() and not gz.any()
        return
    abs_s = ref["gs_abs"].clamp(min=1e-300)
    bound = float((E * (18 + 2 * ref["gs_cond"] / abs_s)).max())
    _judge("uniform_bwd", case.id, "gscale", _elem(gs, ref["gs"], abs_s), _elem(as_, ref["gs"], abs_s), bound)
    if not case.sym:
        abs_z = ref["gz_abs"].clamp(min=1e-300)
        _judge("uniform_bwd", case.id, "gzp", _elem(gz, ref["gz"], abs_z), _elem(az, ref["gz"], abs_z), 18 * E)


@pytest.mark.parametrize("case", T.UNIFORM_INT_CASES, ids=lambda c: c.id)
def test_uniform_int_is_exact(ops, case):
    i = T.uniform_int_inputs(case)
    got = ops.uniform_int(dv(i["x"]), dv(i["s"]), dv(i["z"]), case.bits)
    assert torch.equal(got.cpu(), R.uniform_int(i["x"], i["s"], i["z"], case.bits)["y"])


# ----------------------------------------------------------------------------------------------------------------- AdaLog
def _aten_log_backward(gy, x, s, q, bits, shift, sub_shift, pre_gelu):
    with torch.enable_grad():
        xl, sl = x.detach().clone().requires_grad_(True), s.detach().clone().requires_grad_(True)
        v = torch.nn.functional.gelu(xl) if pre_gelu else xl
        xs = v if shift is None else v + shift
        u = (xs / sl).clamp(min=1e-15, max=1.0)
        k = CB._ste(-u.log2() * 37.0 / q)
        mask = k < 2 ** bits
        out = 2 ** (-1 * torch.clamp(k, 0, 2 ** bits - 1) * q / 37.0) * sl * mask
        if sub_shift and shift is not None:
            out = out - shift
        return torch.autograd.grad(out, (xl, sl), gy)


@pytest.mark.parametrize("case", T.LOG_CASES, ids=lambda c: c.id)
def test_adalog_backward(ops, case):
    i, ref = T.log_inputs(case), T.log_reference(case)
    x, s, gy, sh = dv(i["x"]), dv(i["s"]), dv(i["gy"]), dv(i["shift"])
    qd = torch.tensor([i["q"]], device=DEV)
    y = ops.log_fake_quant(x, s, qd, None, None, case.bits, shift=sh, sub_shift=case.sub_shift, train_form=True, pre_gelu=case.pre_gelu)
    gx, gs = ops.log_fake_quant_backward(gy, x, y, s, qd, case.bits, sh, case.sub_shift, pre_gelu=case.pre_gelu)
    _, gs2 = ops.log_fake_quant_backward(gy, x, y, s, qd, case.bits, sh, case.sub_shift, pre_gelu=case.pre_gelu)
    assert torch.equal(gs, gs2)
    ax, as_ = _aten_log_backward(gy, x, s, qd, case.bits, sh, case.sub_shift, case.pre_gelu)
    xd = i["x"].to(F64)
    v = R.gelu64(xd) if case.pre_gelu else xd
    shf = 0.0 if i["shift"] is None else float(i["shift"])
    allow = ref["gx"].abs() * 6 * E * (v.abs() + shf) / (v + shf).abs().clamp(min=1e-300)
    kw = dict(alts=ref["gx_alts"], near=ref["near"], allow=allow)
    _judge("adalog_bwd", case.id, "gx", _elem(gx, ref["gx"], _max(ref["gx"]), **kw), _elem(ax, ref["gx"], _max(ref["gx"]), **kw), 200 * E)
    slack = float(ref["gs_slack"] / ref["gs_abs"])
    _judge("adalog_bwd", case.id, "gscale", _elem(gs, ref["gs"], ref["gs_abs"]), _elem(as_, ref["gs"], ref["gs_abs"]), 216 * E + slack)
    for name in ("nonpos", "above", "past"):
        if name in i["plants"]:
            assert float(gx.reshape(-1)[i["plants"][name]]) == 0.0, name


# --------------------------------------------------------------------------------------------------------------- AdaRound
@pytest.mark.parametrize("case", T.ADAROUND_CASES, ids=lambda c: c.id)
def test_adaround_forward_backward_and_transposed(ops, case):
    i = T.adaround_inputs(case)
    w, al, s, z, gy = (dv(i[k]) for k in ("w", "alpha", "s", "z", "gy"))
    for soft in (True, False):
        ref = T.adaround_reference(case, soft)
        y = ops.adaround(w, al, s, z, case.bits, soft)
        yt, yt_t = ops.adaround_t(w, al, s, z, case.bits, soft)
        assert torch.equal(yt, y) and torch.equal(yt_t, y.t().contiguous()), "adaround_t equals adaround in both orientations"
        ga = ops.adaround(w, al, s, z, case.bits, soft, gy=gy)
        if not soft:
            assert torch.equal(y.cpu(), ref["y"].float()) and bool((ref["y"].float().double() == ref["y"]).all()), "hard forward is exact"
            assert not ga.any()
            continue
        ay, aga = CB.adaround(w, al, s, z, case.bits, soft), CB.adaround(w, al, s, z, case.bits, soft, gy=gy)
        _judge("adaround", case.id, "y", _elem(y, ref["y"], _max(ref["y"])), _elem(ay, ref["y"], _max(ref["y"])), 8 * E)
        scale = float((i["gy"].abs() * i["s"].view(-1, 1)).max()) * 0.3            # |gy| s max(dh), from the inputs
        kw = dict(alts=ref["ga_alts"], near=ref["near"])
        _judge("adaround", case.id, "galpha", _elem(ga, ref["ga"], scale, **kw), _elem(aga, ref["ga"], scale, **kw), 16 * E)


# ------------------------------------------------------------------------------------------------------------- round loss
def _loss_bound(ref, b, depth=16):
    return (ref["active"] * (8 * b + 4) + depth * float(ref["loss_abs"])) * E / max(float(ref["loss_abs"]), 1e-300)


@pytest.mark.parametrize("b_dev", [False, True], ids=["b_float", "b_dev"])
@pytest.mark.parametrize("b", T.ROUND_LOSS_BS)
@pytest.mark.parametrize("n", T.ROUND_LOSS_NS)
def test_round_loss(ops, n, b, b_dev):
    alpha, ref = T.round_loss_alpha(n), T.round_loss_reference(n, b)
    al = dv(alpha)
    bb = torch.tensor([b], device=DEV) if b_dev else b
    gscale, gmul = 0.5, torch.tensor([0.37], device=DEV)
    acc0 = torch.randn(n, generator=T.gen(f"acc/{n}"))
    ga = dv(acc0).clone()
    loss = ops.round_loss(al, bb, galpha=ga, gscale=gscale)                                        # accumulate form
    assert torch.equal(loss, ops.round_loss(al, bb))
    ga_ow = torch.full_like(al, 7.0)
    assert ops.round_loss(al, bb, galpha=ga_ow, gscale=gscale, want_loss=False, overwrite=True) is None    # overwrite form
    ga_mul = torch.full_like(al, 7.0)
    ops.round_loss(al, bb, galpha=ga_mul, gscale=gscale, want_loss=False, gmul=gmul, overwrite=True)       # gmul form
    a_ga = torch.zeros_like(al)
    a_loss = CB.round_loss(al, b, galpha=a_ga, gscale=gscale)
    labs = max(float(ref["loss_abs"]), 1e-300)
    tag = f"n{n}_b{b}_{'dev' if b_dev else 'float'}"
    if labs > 1e-300:
        _judge("round_loss", tag, "loss", abs(float(loss) - float(ref["loss"])) / labs, abs(float(a_loss) - float(ref["loss"])) / labs,
               _loss_bound(ref, b))
    else:
        assert float(loss) == 0.0
    scale, kw = 0.6 * b * gscale, dict(near=ref["near"])
    want, alts = gscale * ref["grad"], [gscale * ref["grad_alts"][0]]
    _judge("round_loss", tag, "grad", _elem(ga_ow, want, scale, alts=alts, **kw), _elem(a_ga, want, scale, alts=alts, **kw), (8 * b + 12) * E)
    f = R.f32(0.37)
    k_err = _elem(ga_mul, f * want, scale * f, alts=[f * alts[0]], **kw)
    _judge("round_loss", tag, "grad_gmul", k_err, _elem(a_ga * gmul, f * want, scale * f, alts=[f * alts[0]], **kw), (8 * b + 13) * E)
    # accumulate: galpha + g with one rounding of the sum
    acc = acc0.to(F64)
    k_err = _elem(ga, acc + want, scale, alts=[acc + alts[0]], allow=E * (acc + want).abs() * 2, **kw)
    _judge("round_loss", tag, "grad_accumulate", k_err, 0.0, (8 * b + 12) * E)


@pytest.mark.parametrize("gate", [None, 0.0, 1.0])
@pytest.mark.parametrize("b", [20.0, 7.3, 2.0])
def test_round_loss_multi_sixteen_tensors(ops, b, gate):
    alphas = T.multi_alphas()
    weight = 0.01
    ref = R.round_loss_multi(alphas, b, weight, None if gate is None else torch.tensor([gate]))
    al = [dv(a) for a in alphas]
    gt = None if gate is None else torch.tensor([gate], device=DEV)
    for bb in (b, torch.tensor([b], device=DEV)):
        loss, grads = ops.round_loss_multi(al, bb, weight, gate=gt)
        loss2, none = ops.round_loss_multi(al, bb, weight, want_grads=False, gate=gt)
        assert torch.equal(loss, loss2) and none is None
        a_loss, a_grads = CB.round_loss_multi(al, b, weight, gate=gt)
        tag = f"b{b}_gate{gate}_{'dev' if torch.is_tensor(bb) else 'float'}"
        if gate == 0.0:
            assert float(loss) == 0.0
        else:
            single = {"active": ref["active"], "loss_abs": ref["loss_abs"] / R.f32(weight)}
            _judge("round_loss_multi", tag, "loss", abs(float(loss) - float(ref["loss"])) / float(ref["loss_abs"]),
                   abs(float(a_loss) - float(ref["loss"])) / float(ref["loss_abs"]), _loss_bound(single, b) + 2 * E)
        scale = 0.6 * b * weight
        for t, a_ in enumerate(al):
            kw = dict(alts=ref["grads_alts"][t], near=ref["near"][t])
            _judge("round_loss_multi", tag, f"grad[{t}]", _elem(grads[t], ref["grads"][t], scale, **kw),
                   _elem(a_grads[t], ref["grads"][t], scale, **kw), (8 * b + 13) * E)
            # the regulariser's kernels agree bit for bit on the gradient
            one = torch.empty_like(a_)
            ops.round_loss(a_, bb, galpha=one, gscale=weight, want_loss=False, overwrite=True)
            assert torch.equal(one, grads[t]), t


# --------------------------------------------------------------------------------------------------------------- rec loss
@pytest.mark.parametrize("cancel", [True, False], ids=["cancelling", "independent"])
@pytest.mark.parametrize("n", T.REC_LOSS_NS)
def test_rec_loss_forward_backward(ops, n, cancel):
    i = T.rec_loss_inputs(n, cancel)
    p, t, gm = dv(i["pred"]), dv(i["tgt"]), dv(i["gmul"])
    ref = R.rec_loss(i["pred"], i["tgt"], i["scale"])
    loss = ops.rec_loss(p, t, i["scale"])
    assert torch.equal(loss, ops.rec_loss(p, t, i["scale"]))
    labs = max(float(ref["loss_abs"]), 1e-300)
    tag = f"n{n}_{'cancel' if cancel else 'indep'}"
    _judge("rec_loss", tag, "loss", abs(float(loss) - float(ref["loss"])) / labs,
           abs(float(CB.rec_loss(p, t, i["scale"])) - float(ref["loss"])) / labs, 20 * E)
    rb = R.rec_loss_backward(i["pred"], i["tgt"], i["scale"], i["gmul"])["gpred"]
    _judge("rec_loss", tag, "gpred", _elem(ops.rec_loss_backward(p, t, i["scale"], gm), rb, _max(rb)),
           _elem(CB.rec_loss_backward(p, t, i["scale"], gm), rb, _max(rb)), 4 * E)


# ---------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("n", T.SOFTMAX_NS)
def test_scaled_softmax_forward_backward(ops, n):
    for rows in T.softmax_rows_for(n):
        i = T.softmax_inputs(rows, n)
        x, gy = dv(i["x"]), dv(i["gy"])
        ref = R.scaled_softmax(i["x"], T.SOFTMAX_SCALE)
        y = ops.scaled_softmax(x, T.SOFTMAX_SCALE)
        ay = CB.scaled_softmax(x, T.SOFTMAX_SCALE)
        row_scale = ref["y"].amax(-1, keepdim=True)
        bound = float((E * (2 * ref["tmax"] + 30)).max())
        per_row = lambda got: ((c64(got) - ref["y"]).abs() / row_scale / (E * (2 * ref["tmax"] + 30)).unsqueeze(-1)).max().item() * bound
        assert bool(torch.isfinite(y).all())
        _judge("scaled_softmax", f"{rows}x{n}", "y", per_row(y), per_row(ay), bound)
        rb = R.scaled_softmax_backward(i["gy"], y.cpu(), T.SOFTMAX_SCALE)
        scale = rb["row_abs"].clamp(min=1e-300).unsqueeze(-1)
        gx = ops.scaled_softmax_backward(gy, y, T.SOFTMAX_SCALE)
        _judge("scaled_softmax", f"{rows}x{n}", "gx", _elem(gx, rb["gx"], scale),
               _elem(CB.scaled_softmax_backward(gy, y, T.SOFTMAX_SCALE), rb["gx"], scale), 26 * E)


def test_scaled_softmax_rejects_rows_wider_than_documented(ops):
    """ops.scaled_softmax documents rows of <= 1024 values and has no fallback: a wider row is an error, not a result."""
    from adalog_amd import _lib
    x = torch.zeros(2, T.SOFTMAX_TOO_WIDE, device=DEV)
    with pytest.raises(_lib.AdalogHipError):
        ops.scaled_softmax(x, 1.0)
    with pytest.raises(_lib.AdalogHipError):
        ops.scaled_softmax_backward(x, x, 1.0)


# ------------------------------------------------------------------------------------------------------------------- Adam
def _adam_bound(ref, h):
    b1t, b2t = 1.0 - ref["bc1"], 1.0 - ref["bc2"]
    return E * (12 + 4 * b1t / ref["bc1"] + 2 * b2t / ref["bc2"])


def _p_err(got, ref_p, ref_dp):
    """|p - ref| less the final rounding of p (E |p|), over max |update|."""
    return _elem(got, ref_p, _max(ref_dp, 1e-38), allow=E * ref_p.abs())


@pytest.mark.parametrize("lr_dev", [False, True], ids=["lr_float", "lr_dev"])
@pytest.mark.parametrize("step", T.ADAM_STEPS)
@pytest.mark.parametrize("grads", T.ADAM_GRADS)
def test_adam_multi(ops, grads, step, lr_dev):
    sixteen = step == 999
    i, h = T.adam_inputs(grads, sixteen), T.ADAM_HYPER
    ref = R.adam(i["p"], i["g"], i["m"], i["v"], step, **h)
    run = {k: [dv(t).clone() for t in i[k]] for k in ("p", "g", "m", "v")}
    lib = {k: [dv(t).clone() for t in i[k]] for k in ("p", "g", "m", "v")}
    sd, sl = torch.tensor([float(step)], device=DEV), torch.tensor([float(step)], device=DEV)
    lr = torch.tensor([h["lr"]], device=DEV) if lr_dev else h["lr"]
    ops.adam_multi(run["p"], run["g"], run["m"], run["v"], sd, lr, h["beta1"], h["beta2"], h["eps"])
    CB.adam_multi(lib["p"], lib["g"], lib["m"], lib["v"], sl, R.f32(h["lr"]), R.f32(h["beta1"]), R.f32(h["beta2"]), R.f32(h["eps"]))
    assert float(sd) == step + 1, "the step counter"
    tag = f"{grads}_step{step}_{'dev' if lr_dev else 'float'}"
    worst = {"p": [0.0, 0.0], "m": [0.0, 0.0], "v": [0.0, 0.0]}
    for t in range(len(i["p"])):
        for q_, (k_, a_) in {"m": (run["m"][t], lib["m"][t]), "v": (run["v"][t], lib["v"][t])}.items():
            sc = _max(ref[q_][t], 2.0 ** -126)
            worst[q_] = [max(worst[q_][0], _elem(k_, ref[q_][t], sc)), max(worst[q_][1], _elem(a_, ref[q_][t], sc))]
        worst["p"] = [max(worst["p"][0], _p_err(run["p"][t], ref["p"][t], ref["dp"][t])),
                      max(worst["p"][1], _p_err(lib["p"][t], ref["p"][t], ref["dp"][t]))]
        assert torch.equal(run["g"][t].cpu(), i["g"][t])
    _judge("adam_multi", tag, "m", *worst["m"], 4 * E)
    _judge("adam_multi", tag, "v", *worst["v"], 4 * E)
    _judge("adam_multi", tag, "p", *worst["p"], _adam_bound(ref, h))


# ------------------------------------------------------------------------------------------------------- alpha_step_multi
@pytest.mark.parametrize("case", T.ALPHA_STEP_CASES, ids=lambda c: c.id)
def test_alpha_step_multi(ops, case):
    """The whole alpha update of a captured iteration against fp64: ga + weight grl gmul gate, then Adam -- two consecutive steps (the
    second from the state the first one left on the device, so the stored m, v and the counter are what it reads)."""
    inp = T.alpha_step_inputs(case)
    Ls = inp["layers"]
    hyp = {k: inp[k] for k in ("lr", "beta1", "beta2", "eps")}
    st = {k: [dv(L[k]).clone() for L in Ls] for k in ("alpha", "m", "v")}
    fixed = {k: [dv(L[k]) for L in Ls] for k in ("w", "gw", "s", "z")}
    step = torch.tensor([inp["step0"]], device=DEV)
    b = torch.tensor([case.b], device=DEV) if case.b_dev else case.b
    lr = torch.tensor([inp["lr"]], device=DEV) if case.lr_dev else inp["lr"]
    gmul, gate = dv(inp["gmul"]), dv(inp["gate"])
    for it in range(case.steps):
        before = {k: [t.cpu() for t in st[k]] for k in ("alpha", "m", "v")}
        lib = {k: [t.clone() for t in st[k]] for k in ("alpha", "m", "v")}
        ops.alpha_step_multi(st["alpha"], fixed["w"], fixed["gw"], fixed["s"], fixed["z"], st["m"], st["v"], [L["inner"] for L in Ls],
                             [L["bits"] for L in Ls], step, lr, hyp["beta1"], hyp["beta2"], hyp["eps"], b, inp["weight"], gmul, gate)
        assert float(step) == inp["step0"] + it + 1, "the step counter"
        # the ATen route: the per-layer backward of AdaRound, the regulariser's gradient times its upstream factor, torch's Adam
        f = 0.0 if gmul is None else R.f32(inp["weight"]) * float(gmul) * (1.0 if gate is None else float(gate))
        a_g = []
        for t, L in enumerate(Ls):
            ga = torch.zeros_like(lib["alpha"][t]) if fixed["gw"][t] is None else \
                CB.adaround(fixed["w"][t], lib["alpha"][t], fixed["s"][t], fixed["z"][t], L["bits"], True, gy=fixed["gw"][t])
            grl = torch.zeros_like(ga)
            if f != 0.0:
                CB.round_loss(lib["alpha"][t], case.b, galpha=grl, gscale=f, want_loss=False)
            a_g.append(ga + grl)
        CB.adam_multi(lib["alpha"], a_g, lib["m"], lib["v"], torch.tensor([inp["step0"] + it], device=DEV), R.f32(hyp["lr"]),
                      R.f32(hyp["beta1"]), R.f32(hyp["beta2"]), R.f32(hyp["eps"]))
        worst = [0.0, 0.0]
        bound = None
        for t, L in enumerate(Ls):
            g = R.alpha_grad(L["w"], before["alpha"][t], L["gw"], L["s"], L["z"], L["bits"], case.b, inp["weight"], inp["gmul"], inp["gate"])
            outs = [R.adam([before["alpha"][t]], [gg], [before["m"][t]], [before["v"][t]], inp["step0"] + it, **hyp)
                    for gg in [g["g"]] + (g["g_alts"] if bool(g["near"].any()) else [])]
            ref = outs[0]
            bound = _adam_bound(ref, hyp) + 4 * ((8 * case.b + 12) + 16) * E
            allow = E * ref["p"][0].abs()
            kw = dict(alts=[o["p"][0] for o in outs[1:]], near=g["near"], allow=allow)
            sc = _max(ref["dp"][0], 1e-38)
            worst = [max(worst[0], _elem(st["alpha"][t], ref["p"][0], sc, **kw)), max(worst[1], _elem(lib["alpha"][t], ref["p"][0], sc, **kw))]
            for q_ in ("m", "v"):
                kq = dict(alts=[o[q_][0] for o in outs[1:]], near=g["near"])
                assert _elem(st[q_][t], ref[q_][0], _max(ref[q_][0], 2.0 ** -126), **kq) <= \
                    max(bound, 4 * _elem(lib[q_][t], ref[q_][0], _max(ref[q_][0], 2.0 ** -126), **kq)), (case.id, it, t, q_)
        _judge("alpha_step_multi", case.id, f"alpha_step{it + 1}", worst[0], worst[1], bound)
