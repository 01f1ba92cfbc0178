"""`-m gpu`: the autograd routes of adalog_amd/train_mm.py -- linear, quant_linear, matmul and the attention chain
qkv_split_quant -> matmul -> scaled_softmax -> matmul as utils/models.py composes it -- called through their public entries,
forward and backward with a fixed random gy, against fp64 autograd of the operation each stands for
(tests/brecq_grad_reference.py) on the case table of tests/brecq_grad_cases.py.  Every case runs with the default term counts
(FWD_TERMS = GRAD_TERMS = 2) and with both set to 0 (three terms).

Bars.  Tensors: the project's own for one product of csrc/brecq_gemm.hip against its fp64 specification
(test_gpu_kernels.py: test_gemm_f32x3_every_orientation, test_gemm_f32x3_two_term_operands) -- 2e-6 with three terms, 6e-5 with
two -- on the suite's rel_err (max |got - ref| / max |ref|), every element included.  Scale gradients are sums with
cancellation: their error is normalised by the sum of the terms' magnitudes (from the reference), measured for the library route
as well (the same call with train_mm.ENABLED off: ATen's fp32 GEMMs), and the bar is the larger of the product bar and 4 x the
library route's error (the kernel sums in another order; a smaller factor would test summation order).  Both routes' figures go to
brecq_grads_parity.jsonl in the directory of the suite's other parity logs.

The route is asserted too: where the table says native, the last kernel the library noted is a ``bq_gemm<...>`` after the forward
and after the backward; where it says library route, none was launched.  adalog_last_kernel() is per thread and autograd runs
the backward on a thread of its own, so the backward's answer is read by tensor hooks on that thread: one on the result clears
the note before the route's backward runs, those on the product's leaves read it after.
"""
import ctypes
import json
import os
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from tests import brecq_grad_cases as T
from tests.test_gpu_golden_forward import LOG as _GOLDEN_LOG
from tests.test_gpu_kernels import rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOG = os.path.join(os.path.dirname(_GOLDEN_LOG), "brecq_grads_parity.jsonl")      # next to the suite's other parity logs
PRODUCT_BAR = {2: 6e-5, 0: 2e-6}                       # by term count of train_mm (0 = three terms)
_NO_KERNEL = ctypes.c_char_p(b"(no gemm launch noted)")
_log_started = []


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import backend
    backend.set_backend(None)
    return backend.get()


@pytest.fixture(params=[2, 0], ids=["terms2", "terms3"])
def terms(request, monkeypatch):
    from adalog_amd import train_mm
    monkeypatch.setattr(train_mm, "FWD_TERMS", request.param)
    monkeypatch.setattr(train_mm, "GRAD_TERMS", request.param)
    monkeypatch.setattr(train_mm, "ENABLED", True)
    train_mm.reset_offers()
    return request.param


def _log(**row):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a" if _log_started else "w") as f:
        f.write(json.dumps(row) + "\n")
    _log_started.append(1)


# ------------------------------------------------------------------------------------------------------- running a route
def _lib():
    from adalog_amd import _lib
    lib = _lib.load()
    lib.adalog_note_kernel.argtypes, lib.adalog_note_kernel.restype = [ctypes.c_char_p], None
    return lib


def _clear_note():
    _lib().adalog_note_kernel(_NO_KERNEL)


def _last():
    return _lib().adalog_last_kernel().decode()


def _run(fn, leaves, gy, product_leaves):
    """y = fn(); y.backward(gy).  -> (y, {name: leaf.grad}, kernel noted after the forward, [kernels noted on the backward thread
    when the gradients of ``product_leaves`` arrived])."""
    _clear_note()
    y = fn()
    fwd = _last()
    seen = []
    y.register_hook(lambda g: _clear_note())
    hooks = [leaves[n].register_hook(lambda g: seen.append(_last())) for n in product_leaves
             if leaves.get(n) is not None and leaves[n].requires_grad]
    y.backward(gy.to(y.dtype))
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    return y.detach(), {n: (None if t is None else t.grad) for n, t in leaves.items()}, fwd, seen


def _assert_route(native, fwd, seen, what):
    assert seen, (what, "no product leaf received a gradient")
    if native:
        assert fwd.startswith("bq_gemm<"), (what, "forward", fwd)
        assert all(k.startswith("bq_gemm<") for k in seen), (what, "backward", seen)
    else:
        assert not fwd.startswith("bq_gemm<"), (what, "forward", fwd)
        assert not any(k.startswith("bq_gemm<") for k in seen), (what, "backward", seen)


def _check(got, ref, bar, what):
    assert got is not None, what
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    err = rel_err(got.detach().cpu().double(), ref)
    print(f"{what}: rel_err {err:.3e} (bar {bar:.0e})")
    assert err <= bar, (what, err, bar)


def _scale_err(got, ref, ref_abs):
    return ((got.detach().cpu().double().reshape(ref.shape) - ref).abs() / ref_abs).max().item()


def _check_scale(native_err, library_err, nterms, **row):
    bar = max(PRODUCT_BAR[nterms], 4 * library_err)
    _log(terms=3 if nterms == 0 else 2, native_err=native_err, library_err=library_err, bar=bar, **row)
    print(f"{row}: scale gradient error / sum|term|: native {native_err:.3e}, library route {library_err:.3e}, bar {bar:.3e}")
    assert native_err <= bar, (row, native_err, library_err, bar)


def _dev(t, grad=True):
    return None if t is None else t.to(DEV).requires_grad_(grad)


# ---------------------------------------------------------------------------------------------------------------- linear
def _linear_leaves(case, on=("x", "w", "b", "addend")):
    d = T.linear_inputs(case)
    return {n: _dev(d[n], n in on) for n in ("x", "w", "b", "addend")}, d["gy"].to(DEV)


def _run_linear(case, on=("x", "w", "b", "addend")):
    from adalog_amd import train_mm
    lv, gy = _linear_leaves(case, on)
    return _run(lambda: train_mm.linear(lv["x"], lv["w"], lv["b"], lv["addend"]), lv, gy, ("x", "w"))


@pytest.mark.parametrize("case", T.LINEAR_CASES, ids=lambda c: c.id)
def test_linear_against_fp64_autograd(ops, terms, case):
    ref, bar = T.linear_reference(case), PRODUCT_BAR[terms]
    y, g, fwd, seen = _run_linear(case)
    _assert_route(case.native, fwd, seen, case.id)
    _check(y, ref["y"], bar, "y")
    _check(g["x"], ref["gx"], bar, "gx")
    _check(g["w"], ref["gw"], bar, "gw")
    if case.bias:
        _check(g["b"], ref["gb"], bar, "gb")
    if case.addend:
        _check(g["addend"], ref["gaddend"], bar, "gaddend")


def test_linear_needs_input_grad_arms(ops, terms):
    """Each gradient of _LinearFn asked for alone is, bit for bit, the one of the run that asks for all; the others are not
    produced."""
    case = next(c for c in T.LINEAR_CASES if c.id == "197x64x48_b+add")
    names = ("x", "w", "b", "addend")
    _, full, _, _ = _run_linear(case)
    for name in names:
        _, g, _, _ = _run_linear(case, on=(name,))
        for other in names:
            if other == name:
                assert g[other] is not None and torch.equal(g[other], full[other]), (name, other)
            else:
                assert g[other] is None, (name, other)


# ---------------------------------------------------------------------------------------------------------- quant_linear
def _quantizer(bits, s, z):
    from adalog_amd.quantizers.uniform import UniformQuantizer
    q = UniformQuantizer(n_bits=bits, symmetric=False, channel_wise=False)
    q.scale = nn.Parameter(s.clone().to(DEV))
    q.zero_point = nn.Parameter(z.clone().to(DEV), requires_grad=False)
    q.inited = True
    q.init_training()
    return q


def _run_quant(case, on=("x", "s", "w", "b")):
    from adalog_amd import train_mm
    d = T.quant_inputs(case)
    aq = _quantizer(case.bits, d["s"], d["z"])
    aq.scale.requires_grad_("s" in on)
    lv = {"x": _dev(d["x"], "x" in on), "s": aq.scale, "w": _dev(d["w"], "w" in on), "b": _dev(d["b"], "b" in on)}
    addend = None if d["addend"] is None else d["addend"].to(DEV)
    return _run(lambda: train_mm.quant_linear(lv["x"], aq, lv["w"], lv["b"], addend=addend), lv, d["gy"].to(DEV), ("x", "s", "w"))


@pytest.mark.parametrize("case", T.QUANT_CASES, ids=lambda c: c.id)
def test_quant_linear_against_fp64_autograd(ops, terms, monkeypatch, case):
    from adalog_amd import train_mm
    ref, bar = T.quant_reference(case), PRODUCT_BAR[terms]
    y, g, fwd, seen = _run_quant(case)
    _assert_route(case.native, fwd, seen, case.id)
    _check(y, ref["y"], bar, "y")
    _check(g["x"], ref["gx"], bar, "gx")
    _check(g["w"], ref["gw"], bar, "gw")
    if case.bias:
        _check(g["b"], ref["gb"], bar, "gb")
    native_err = _scale_err(g["s"], ref["gs"], ref["gs_abs"])
    monkeypatch.setattr(train_mm, "ENABLED", False)
    _, g_lib, fwd, seen = _run_quant(case)
    _assert_route(False, fwd, seen, case.id + " (library route)")
    _check_scale(native_err, _scale_err(g_lib["s"], ref["gs"], ref["gs_abs"]), terms, route="quant_linear", case=case.id, grad="s")


@pytest.mark.parametrize("subset", [k for k in T.GRAD_SUBSETS if k != "all"])
def test_quant_linear_needs_input_grad_arms(ops, terms, subset):
    """Every needs_input_grad arm of _QuantLinearFn.backward: the gradients asked for equal, bit for bit, those of the run that
    asks for all of them, and nothing else is produced."""
    case = next(c for c in T.QUANT_CASES if c.id == T.SUBSET_CASE)
    _, full, fwd, seen = _run_quant(case, T.GRAD_SUBSETS["all"])
    _assert_route(True, fwd, seen, case.id)
    on = T.GRAD_SUBSETS[subset]
    _, g, fwd, seen = _run_quant(case, on)
    _assert_route(True, fwd, seen, case.id + " / " + subset)
    for name in ("x", "s", "w", "b"):
        if name in on:
            assert g[name] is not None and torch.equal(g[name], full[name]), (subset, name)
        else:
            assert g[name] is None, (subset, name)


# ---------------------------------------------------------------------------------------------------------------- matmul
def _strided(t):
    """The values of t read through a last-dim stride of 2 (what the kernel cannot read in place); differentiable."""
    return torch.stack([t, torch.zeros_like(t)], -1).flatten(-2)[..., ::2]


def _mm_operands(case, a, b):
    A, B = a, b
    if case.form.startswith("qk"):
        B = b.transpose(-1, -2)
    if case.form == "qk_strided":
        A = _strided(a)
    if case.form == "pv_strided":
        B = _strided(b)
    if case.form == "qk_offset":                           # the same values starting 4 bytes off a 16-byte boundary
        A = torch.cat([a.new_zeros(1), a.flatten()])[1:].view(a.shape)
        assert A.data_ptr() % 16 == 4
    return A, B


def _run_matmul(case):
    from adalog_amd import train_mm
    d = T.matmul_inputs(case)
    lv = {"a": _dev(d["a"]), "b": _dev(d["b"])}
    heads_last = case.form in ("pv_hl", "pv_strided")
    shared = []

    def fn():
        A, B = _mm_operands(case, lv["a"], lv["b"])
        out = train_mm.matmul(A, B, heads_last=heads_last)
        if T.matmul_merges(case):
            b_, h_, n_, d_ = out.shape
            merged = out.transpose(1, 2).reshape(b_, n_, h_ * d_)
            shared.append(merged.data_ptr() == out.data_ptr())
            return merged
        return out
    y, g, fwd, seen = _run(fn, lv, d["gy"].to(DEV), ("a", "b"))
    if T.matmul_merges(case):
        assert shared[0] is heads_last, "heads_last: the merge of the heads is a view of the product's own storage"
    return y, g, fwd, seen


@pytest.mark.parametrize("case", T.MATMUL_CASES, ids=lambda c: c.id)
def test_matmul_against_fp64_autograd(ops, terms, case):
    ref, bar = T.matmul_reference(case), PRODUCT_BAR[terms]
    y, g, fwd, seen = _run_matmul(case)
    _assert_route(case.native, fwd, seen, case.id)
    _check(y, ref["y"], bar, "y")
    _check(g["a"], ref["gA"], bar, "gA")
    _check(g["b"], ref["gB"], bar, "gB")


@pytest.mark.parametrize("case", [c for c in T.MATMUL_CASES if c.form in ("qk", "pv_hl")], ids=lambda c: c.id)
def test_matmul_gradient_orientation(ops, terms, case):
    """The gradient that reaches k through k.transpose(-1, -2), and the one that reaches v through heads_last and the merged view,
    element by element in k's / v's own index order.  N != D in every case, and the same elements in the other orientation
    (the reference's, so nothing is measured from the code under test) are shown to be far outside the bar."""
    ref, bar = T.matmul_reference(case)["gB"], PRODUCT_BAR[terms]
    _, g, _, _ = _run_matmul(case)
    got = g["b"].detach().cpu().double()
    N, D = ref.shape[-2:]
    assert N != D and tuple(got.shape) == tuple(ref.shape)
    tol = bar * ref.abs().max()
    assert bool(((got - ref).abs() <= tol).all())
    swapped = ref.transpose(-1, -2).reshape(ref.shape)     # a gradient laid out in the other orientation over the same storage
    assert not bool(((swapped - ref).abs() <= tol).all())
    assert not bool(((got - swapped).abs() <= tol).all())


# ------------------------------------------------------------------------------------------------------- attention chain
def _run_attention(case):
    from adalog_amd import train_mm
    d = T.attention_inputs(case)
    qs = [_quantizer(b_, s_, z_) for b_, s_, z_ in zip(d["bits"], d["scales"], d["zps"])]
    mm1 = SimpleNamespace(mode="quant_forward", A_quantizer=qs[0], B_quantizer=qs[1])
    mm2 = SimpleNamespace(mode="quant_forward", A_quantizer=None, B_quantizer=qs[2])
    lv = {"x": _dev(d["x"]), "s0": qs[0].scale, "s1": qs[1].scale, "s2": qs[2].scale}
    H, fused_taken = case.H, []

    def fn():                                                # utils/models.py, Attention._forward, without the projections
        x = lv["x"]
        fused = train_mm.qkv_split_quant(x, H, mm1, mm2)
        fused_taken.append(fused is not None)
        if fused is not None:
            q, k, v = fused
            kt = k.transpose(-2, -1)
        else:
            q, k, v = train_mm.split_heads(x, 3, H)
            q, kt, v = mm1.A_quantizer(q), mm1.B_quantizer(k.transpose(-2, -1)), mm2.B_quantizer(v)
        attn = train_mm.scaled_softmax(train_mm.matmul(q, kt), d["mul"])
        out = train_mm.matmul(attn, v, heads_last=True)
        B, _, N, D = out.shape
        return out.transpose(1, 2).reshape(B, N, H * D)
    y, g, fwd, seen = _run(fn, lv, d["gy"].to(DEV), ("x", "s0", "s1", "s2"))
    return y, g, fwd, seen, fused_taken[0]


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.id)
def test_attention_chain_against_fp64_autograd(ops, terms, monkeypatch, case):
    from adalog_amd import train_mm
    ref, bar = T.attention_reference(case), PRODUCT_BAR[terms]
    y, g, fwd, seen, fused = _run_attention(case)
    assert fused, "train_mm.qkv_split_quant did not take the fused route"
    _assert_route(True, fwd, seen, case.id)
    _check(y, ref["y"], bar, "y")
    _check(g["x"], ref["gx"], bar, "gx")
    native = [_scale_err(g[f"s{p}"], ref["gs"][p], ref["gs_abs"][p]) for p in range(3)]
    monkeypatch.setattr(train_mm, "ENABLED", False)
    _, g_lib, fwd, seen, fused = _run_attention(case)
    assert not fused
    _assert_route(False, fwd, seen, case.id + " (library route)")
    for p in range(3):
        assert tuple(g[f"s{p}"].shape) == tuple(ref["gs"][p].shape)
        _check_scale(native[p], _scale_err(g_lib[f"s{p}"], ref["gs"][p], ref["gs_abs"][p]), terms, route="attention", case=case.id,
                     grad=f"s{p}")


# ------------------------------------------------------------------------------------------------- stale K-major offers
def test_stale_offer_is_not_read_on_the_device(ops, terms):
    """An image offered for w, then w overwritten in place: the forward product must read the new values."""
    from adalog_amd import train_mm
    g_ = torch.Generator().manual_seed(41)
    x = torch.randn(197, 64, generator=g_).to(DEV).requires_grad_(True)
    w = torch.randn(48, 64, generator=g_).to(DEV)
    w_new = torch.randn(48, 64, generator=g_).to(DEV)
    train_mm.offer_kmajor(w, w.t().contiguous())
    w.copy_(w_new)
    _clear_note()
    y = train_mm.linear(x, w, None)
    assert _last().startswith("bq_gemm<")
    _check(y, x.detach().cpu().double() @ w_new.cpu().double().t(), PRODUCT_BAR[terms], "y after the overwrite")


def test_adaround_offers_follow_alpha(ops, terms):
    """w_sim of AdaRoundQuantizer in training mode comes with its K-major image; with alpha changed between two forwards -- the
    first image never taken and its tensor freed, the second taken -- every product sees the w_sim it was given."""
    from adalog_amd import train_mm
    from adalog_amd.quantizers.adaround import AdaRoundQuantizer
    from adalog_amd.quantizers.uniform import UniformQuantizer
    g_ = torch.Generator().manual_seed(42)
    x = torch.randn(130, 64, generator=g_).to(DEV).requires_grad_(True)
    w = torch.randn(48, 64, generator=g_).to(DEV)
    uq = UniformQuantizer(n_bits=4, symmetric=False, channel_wise=True)
    uq.scale = (w.abs().amax(1, keepdim=True) / 7).contiguous()
    uq.zero_point = torch.full((48, 1), 8.0, device=DEV)
    uq.inited = True
    aq = AdaRoundQuantizer(uq, w)
    aq.init_training()
    aq.soft_targets = True
    bar = PRODUCT_BAR[terms]
    sims = []
    for step in range(3):
        with torch.no_grad():
            aq.alpha.add_(torch.randn(48, 64, generator=g_).to(DEV) * 2)
        w_sim = aq(w)
        assert len(train_mm._KMAJOR_OFFER) >= 1, "the AdaRound forward made no offer"
        sims.append(w_sim.detach().cpu().double())
        if step == 0:
            del w_sim                                      # never taken: its address is free for the next w_sim
            continue
        _clear_note()
        y = train_mm.linear(x, w_sim, None)
        assert _last().startswith("bq_gemm<")
        assert w_sim.data_ptr() not in train_mm._KMAJOR_OFFER, "the offer was not taken"
        _check(y, x.detach().cpu().double() @ sims[-1].t(), bar, f"y of forward {step}")
    assert rel_err(sims[1], sims[0]) > 1e-3 and rel_err(sims[2], sims[1]) > 1e-3     # alpha really moved w_sim
