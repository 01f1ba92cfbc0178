"""CPU tier of the route choice of quant_forward's attention core (utils/models.py: _quant_attn_core): which backend functions are
called, in which order, for every row of the route table -- what the GPU tests assert by counting calls, pinned here without a device
or the library.  The backend is a recording fake: its functions note their names and return sentinels."""
from types import SimpleNamespace

import pytest

from adalog_amd.ops import BF16, I8
from adalog_amd.utils import models as M

LAUNCHES = ("gemm_out", "softmax_adalog_pack", "softmax_adalog_pack_long", "softmax_bias_adalog_pack", "attn_core", "attn_core_long")
THREE = {"plain": ["gemm_out", "softmax_adalog_pack", "gemm_out"], "long": ["gemm_out", "softmax_adalog_pack_long", "gemm_out"],
         "bias": ["gemm_out", "softmax_bias_adalog_pack", "gemm_out"]}


def _backend(calls, core_flag=True, core_ok=True, long_ok=True):
    """a backend whose launch functions append (name, args, kwargs) to ``calls`` and return a sentinel named after them"""
    be = SimpleNamespace(attn_core_ok=lambda N, D: core_ok and N <= 256, attn_core_long_ok=lambda N, D: long_ok and N <= 1024)
    if core_flag is not None:
        be.QF_ATTN_CORE = core_flag
    for name in LAUNCHES:
        setattr(be, name, lambda *a, _n=name, **kw: calls.append((_n, a, kw)) or ("out of", _n, len(calls)))
    return be


def _params():
    return M._CoreParams(("sA", "zA", 4), ("sB", "zB", 4), ("sV", "zV", 4), "a_scale", "qv", 4, "mant37", 0.5)


def _run(monkeypatch, switch, be, N, D, form):
    monkeypatch.setattr(M, "QF_ATTN_CORE", switch)
    H = 3
    if form == "bias":
        return M._quant_attn_core(be, "qp", "kp", "vp", 2 * H, N, D, H, H, _params(), bias=("table", "index", "mask"))
    return M._quant_attn_core(be, "qp", "kp", "vp", 2 * H, N, D, H, H, _params(), mul=0.125)


ROUTES = [(197, 64, "plain", "attn_core"), (577, 64, "long", "attn_core_long"), (49, 32, "bias", "attn_core")]


@pytest.mark.parametrize("N,D,form,one", ROUTES)
def test_switch_off_makes_the_three_launches(monkeypatch, N, D, form, one):
    calls = []
    out = _run(monkeypatch, False, _backend(calls), N, D, form)
    assert [c[0] for c in calls] == THREE[form]
    assert out == ("out of", "gemm_out", 3)                                  # the second product's result is what comes back
    scores, soft, pv = calls
    assert scores[1][:7] == (I8, "qp", "kp", N, N, 6, 3) and pv[1][:7] == (BF16, ("out of", soft[0], 2), "vp", N, D, 6, 3)
    assert pv[2] == dict(sa_mul=0.5, heads_last=3)
    assert soft[1][0] == ("out of", "gemm_out", 1)                           # the softmax pack reads the first product's scores
    if form == "bias":
        assert soft[1][1:] == (3, "table", "index", "mask", "a_scale", "qv", 4, "mant37")
    else:
        assert soft[1][1:] == (0.125, "a_scale", "qv", 4, "mant37")


@pytest.mark.parametrize("N,D,form,one", ROUTES)
def test_switch_on_makes_one_launch(monkeypatch, N, D, form, one):
    calls = []
    out = _run(monkeypatch, True, _backend(calls), N, D, form)
    assert [c[0] for c in calls] == [one] and out == ("out of", one, 1)
    name, args, kw = calls[0]
    mul = 1.0 if form == "bias" else 0.125
    assert args == ("qp", "kp", "vp", N, D, 3, 3, "sA", "sB", "sV", mul, "a_scale", "qv", 4, "mant37", 0.5)
    assert kw == (dict(table="table", index="index", mask="mask") if form == "bias" else {})


def test_long_rows_the_backend_refuses_fall_through_to_the_three_launches(monkeypatch):
    calls = []
    _run(monkeypatch, True, _backend(calls, long_ok=False), 577, 64, "long")
    assert [c[0] for c in calls] == THREE["long"]


def test_short_rows_the_backend_refuses_fall_through_to_the_three_launches(monkeypatch):
    calls = []
    _run(monkeypatch, True, _backend(calls, core_ok=False), 197, 64, "plain")
    assert [c[0] for c in calls] == THREE["plain"]


@pytest.mark.parametrize("switch", [False, True])
@pytest.mark.parametrize("N,D,form,one", ROUTES)
def test_backend_without_the_capability_flag_makes_the_three_launches(monkeypatch, switch, N, D, form, one):
    """no QF_ATTN_CORE attribute (the CPU specification backend), or a false one: the predicates are not even asked"""
    for flag in (None, False):
        calls = []
        be = _backend(calls, core_flag=flag)
        be.attn_core_ok = be.attn_core_long_ok = lambda N, D: pytest.fail("asked a backend without the capability")
        _run(monkeypatch, switch, be, N, D, form)
        assert [c[0] for c in calls] == THREE[form]


def test_functions_are_looked_up_when_they_are_called(monkeypatch):
    """a wrapper put on the backend after import is the one that runs (the GPU tests count calls this way)"""
    calls, seen = [], []
    be = _backend(calls)
    inner = be.attn_core
    be.attn_core = lambda *a, **kw: seen.append("wrapped") or inner(*a, **kw)
    _run(monkeypatch, True, be, 197, 64, "plain")
    assert seen == ["wrapped"] and [c[0] for c in calls] == ["attn_core"]
