"""CPU half of the BRECQ autograd-route tests: the fp64 reference checks itself (closed-form straight-through gradients against
autograd, to 1e-12), the inputs of every quantised case decide every bin alike in fp32 and fp64, the K-major offer table of
adalog_amd/train_mm.py (pure torch: exercised on CPU tensors), and the two dispatch decisions on the shapes of the case table.

Dispatch on the CPU: ``train_mm._usable`` and ``ops.gemm_f32x3_ok`` read nothing of a tensor but its dtype, shape, strides,
address and device flag, so they are handed stand-ins (``_OnDevice``) that report a CPU tensor's real geometry with
``is_cuda = True`` -- a fake device.  ``_usable`` is called itself; the ``fits`` closure of ``train_mm.matmul`` cannot be reached
without launching, so its expression is restated here over ``ops.gemm_f32x3_ok`` and the decision of the real closure is asserted
again on the GPU (tests/test_gpu_brecq_grads.py checks which kernel ran for every case of the same table).
"""
import gc
import weakref

import pytest
import torch

from tests import brecq_grad_cases as T
from tests import brecq_grad_reference as R
from tests import cpu_backend as CB


def rel_err(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


# ----------------------------------------------------------------------------------------------- the reference checks itself
@pytest.mark.parametrize("case", T.QUANT_CASES, ids=lambda c: c.id)
def test_quant_linear_closed_form_equals_autograd(case):
    ref = T.quant_reference(case)
    for name in ("y", "gx", "gw", "gb"):
        if ref[name] is not None:
            assert ref[name].shape == ref["closed"][name].shape
            assert rel_err(ref["closed"][name], ref[name]) <= 1e-12, name
    # the scale gradient is a sum with cancellation: normalised by the sum of its terms' magnitudes
    assert (ref["closed"]["gs"] - ref["gs"]).abs().item() / ref["gs_abs"].item() <= 1e-12
    assert ref["gs_abs"].item() > 0 and ref["gx"].abs().max().item() > 0


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.id)
def test_attention_closed_form_equals_autograd(case):
    ref = T.attention_reference(case)
    assert rel_err(ref["closed"]["gx"], ref["gx"]) <= 1e-12
    for p in range(3):
        assert ref["gs"][p].shape == T.attention_inputs(case)["scales"][p].shape
        assert ((ref["closed"]["gs"][p] - ref["gs"][p]).abs() / ref["gs_abs"][p]).max().item() <= 1e-12, p
        assert ref["gs"][p].abs().min().item() > 0


def _assert_bins(x, k, s, z, bits):
    b32, b64 = R.bins(x, s, z, torch.float32), R.bins(x, s, z, torch.float64)
    assert torch.equal(b32, b64) and torch.equal(b64, k)                 # every element, and the bin the generator aimed at
    r = x.double() / s.double()
    assert ((r - r.round()).abs() <= 0.36).all()                          # |f| <= 0.35 survived the fp32 rounding of x
    qmax = 2 ** bits - 1
    assert (k < 0).any() and (k > qmax).any() and (k == 0).any() and (k == qmax).any()      # both clamp sides, both edges


@pytest.mark.parametrize("case", T.QUANT_CASES, ids=lambda c: c.id)
def test_quant_inputs_are_off_ties(case):
    d = T.quant_inputs(case)
    if d["x"].numel() >= 2048:
        _assert_bins(d["x"], d["k"], d["s"], d["z"], d["bits"])
    else:                                                                 # (the M = 1 case is too small to hold every bin)
        assert torch.equal(R.bins(d["x"], d["s"], d["z"], torch.float32), d["k"])
        assert torch.equal(R.bins(d["x"], d["s"], d["z"], torch.float64), d["k"])


@pytest.mark.parametrize("case", T.ATTN_CASES, ids=lambda c: c.id)
def test_attention_inputs_are_off_ties(case):
    d = T.attention_inputs(case)
    B, N, H, D = case.B, case.N, case.H, case.D
    back = d["x"].reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    for p in range(3):
        assert torch.equal(back[p], d["parts"][p])
        _assert_bins(d["parts"][p], d["k"][p], d["scales"][p], d["zps"][p], d["bits"][p])


def test_reference_orientation_is_not_symmetric():
    """Every matmul case has N != D, so a gradient in the wrong orientation cannot pass by shape."""
    for case in T.MATMUL_CASES:
        assert case.dims[-1] != case.dims[-2]
        ref, d = T.matmul_reference(case), T.matmul_inputs(case)
        assert ref["gA"].shape == d["a"].shape and ref["gB"].shape == d["b"].shape and ref["y"].shape == d["gy"].shape


# ------------------------------------------------------------------------------------------------------ the offer table
@pytest.fixture
def mm():
    from adalog_amd import train_mm
    train_mm.reset_offers()
    old = train_mm.W_KMAJOR
    train_mm.W_KMAJOR = True
    yield train_mm
    train_mm.W_KMAJOR = old
    train_mm.reset_offers()


def _w(n=8, k=12, seed=0):
    return torch.randn(n, k, generator=R.gen(seed))


def _same_matrix(got, w):
    return got.shape == w.shape and torch.equal(got, w)


def test_offer_live_and_unmodified_is_taken_without_a_copy(mm):
    w = _w()
    img = w.t().contiguous()
    mm.offer_kmajor(w, img)
    got = mm._kmajor(w)
    assert got.data_ptr() == img.data_ptr() and got.stride() == (1, w.shape[0])
    assert _same_matrix(got, w)
    # views of the offering tensor share its address and take the image too
    mm.offer_kmajor(w, img)
    assert mm._kmajor(w.view(8, 12)).data_ptr() == img.data_ptr()


def test_offer_is_consumed_once(mm):
    w = _w()
    img = w.t().contiguous()
    mm.offer_kmajor(w, img)
    assert mm._kmajor(w).data_ptr() == img.data_ptr()
    assert w.data_ptr() not in mm._KMAJOR_OFFER
    again = mm._kmajor(w)
    assert again.data_ptr() != img.data_ptr() and _same_matrix(again, w) and again.stride() == (1, w.shape[0])


def test_offer_is_rebuilt_after_an_in_place_write(mm):
    w = _w()
    img = w.t().contiguous()
    mm.offer_kmajor(w, img)
    w.mul_(2.0)                                                           # bumps w._version: the image holds the old values
    got = mm._kmajor(w)
    assert got.data_ptr() != img.data_ptr()
    assert _same_matrix(got, w) and not torch.equal(got, img.t())


def test_offer_with_a_dead_referent_is_not_used(mm):
    w = _w()
    gone = _w(seed=1)
    stale, ref = gone.t().contiguous(), weakref.ref(gone)
    del gone
    gc.collect()
    assert ref() is None
    mm._KMAJOR_OFFER[w.data_ptr()] = (stale, w.shape[0], w.shape[1], ref, w._version)
    got = mm._kmajor(w)
    assert got.data_ptr() != stale.data_ptr() and _same_matrix(got, w)


def test_offer_of_another_shape_at_the_same_address_is_not_used(mm):
    w = _w(8, 12)
    img = w.t().contiguous()
    for other in (w.view(12, 8), w.view(4, 24)):
        mm.offer_kmajor(w, img)
        assert other.data_ptr() == w.data_ptr()
        got = mm._kmajor(other)
        assert got.data_ptr() != img.data_ptr() and _same_matrix(got, other)


def test_offer_for_a_non_contiguous_matrix_is_not_used(mm):
    base = torch.randn(8, 24, generator=R.gen(2))
    w = base[:, :12]                                                      # [8, 12] at base's address, rows 24 apart
    assert not w.is_contiguous()
    stale = torch.zeros(12, 8)
    mm.offer_kmajor(w, stale)
    got = mm._kmajor(w)
    assert got.data_ptr() != stale.data_ptr() and _same_matrix(got, w)


def test_offer_table_is_dropped_above_64_entries_and_stays_right(mm):
    ws = [_w(4, 8, seed=10 + i) for i in range(70)]
    sizes = []
    for w in ws:
        mm.offer_kmajor(w, w.t().contiguous())
        sizes.append(len(mm._KMAJOR_OFFER))
    assert max(sizes) <= 65 and sizes[-1] < 70 and 1 in sizes[1:]         # cleared wholesale once it held more than 64
    for w in ws:
        assert _same_matrix(mm._kmajor(w), w)
    assert not mm._KMAJOR_OFFER


def test_reset_offers_empties_the_table(mm):
    w = _w()
    img = w.t().contiguous()
    mm.offer_kmajor(w, img)
    assert len(mm._KMAJOR_OFFER) == 1
    mm.reset_offers()
    assert not mm._KMAJOR_OFFER
    got = mm._kmajor(w)
    assert got.data_ptr() != img.data_ptr() and _same_matrix(got, w)


def test_kmajor_leaves_rows_off_a_multiple_of_4_alone(mm):
    w = _w(6, 8)
    mm.offer_kmajor(w, torch.zeros(8, 6))
    assert mm._kmajor(w) is w
    mm.W_KMAJOR = False
    w2 = _w()
    assert mm._kmajor(w2) is w2


# ------------------------------------------------------------------------------------------------------------- dispatch
class _OnDevice:
    """The geometry of a CPU tensor, reported as a device tensor's (``offset``: bytes added to the address)."""
    is_cuda = True

    def __init__(self, t, offset=0):
        self._t, self._off = t, offset
        self.dtype, self.shape = t.dtype, t.shape

    def dim(self):
        return self._t.dim()

    def stride(self, i=None):
        return self._t.stride() if i is None else self._t.stride(i)

    def numel(self):
        return self._t.numel()

    def is_contiguous(self):
        return self._t.is_contiguous()

    def contiguous(self):
        return _OnDevice(self._t.contiguous(), self._off)

    def transpose(self, a, b):
        return _OnDevice(self._t.transpose(a, b), self._off)

    def data_ptr(self):
        return self._t.data_ptr() + self._off


@pytest.fixture
def cpu_backend():
    from adalog_amd import backend
    backend.set_backend(CB)
    yield
    backend.set_backend(None)


@pytest.mark.parametrize("case", T.LINEAR_CASES + T.QUANT_CASES, ids=lambda c: c.id)
def test_usable_decides_what_the_table_says(mm, cpu_backend, monkeypatch, case):
    monkeypatch.setattr(mm, "ENABLED", True)
    x2 = _OnDevice(torch.empty(case.M, case.K))
    w2 = _OnDevice(torch.empty(case.N, case.K))
    bias = torch.empty(case.N) if case.bias else None
    assert x2.data_ptr() % 16 == 0 and w2.data_ptr() % 16 == 0
    assert mm._usable(x2, w2, bias) is case.native, case.why
    # the rule, written out: 16-byte rows in both orientations, and a fused bias only on whole 16-column tiles
    assert case.native == (case.K % 4 == 0 and case.N % 4 == 0 and (not case.bias or case.N % 16 == 0))


def test_usable_refuses_other_devices_types_and_addresses(mm, cpu_backend, monkeypatch):
    monkeypatch.setattr(mm, "ENABLED", True)
    x, w = torch.empty(8, 16), torch.empty(32, 16)
    assert mm._usable(_OnDevice(x), _OnDevice(w), None)
    assert not mm._usable(x, w, None)                                     # CPU tensors
    assert not mm._usable(_OnDevice(x.double()), _OnDevice(w), None)
    assert not mm._usable(_OnDevice(x), _OnDevice(w.double()), None)
    assert not mm._usable(_OnDevice(x, 4), _OnDevice(w), None)
    assert not mm._usable(_OnDevice(x), _OnDevice(w, 8), None)
    assert not mm._usable(_OnDevice(x), _OnDevice(w), torch.empty(64)[::2])
    monkeypatch.setattr(mm, "ENABLED", False)
    assert not mm._usable(_OnDevice(x), _OnDevice(w), None)


def _operands(case):
    """The operands of tests/test_gpu_brecq_grads.py::_mm_operands for this case, as stand-ins."""
    d = T.matmul_inputs(case)
    a, b = d["a"], d["b"]
    if case.form.startswith("qk"):
        b = b.transpose(-1, -2)
    if case.form == "qk_strided":
        a = torch.stack([a, a], -1).flatten(-2)[..., ::2]
    if case.form == "pv_strided":
        b = torch.stack([b, b], -1).flatten(-2)[..., ::2]
    return _OnDevice(a, 4 if case.form == "qk_offset" else 0), _OnDevice(b)


@pytest.mark.parametrize("case", T.MATMUL_CASES, ids=lambda c: c.id)
def test_matmul_fits_decides_what_the_table_says(case):
    from adalog_amd import ops

    def fits(a_, b_):                                                      # the closure of train_mm.matmul, restated
        return ops.gemm_f32x3_ok(a_, b_.transpose(-1, -2)) and ops.gemm_f32x3_ok(a_.transpose(-1, -2), a_.transpose(-1, -2))
    a, b = _operands(case)
    same_lead = a.shape[:-2] == b.shape[:-2]
    first = same_lead and fits(a, b)
    assert (not first) is (case.copies or not same_lead)
    if same_lead and not first:
        a, b = a.contiguous(), b.contiguous()
    assert (same_lead and fits(a, b)) is case.native
