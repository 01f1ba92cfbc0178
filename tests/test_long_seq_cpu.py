"""CPU tier of the long-row fused route (257 to 1024 tokens per attention group; csrc/operand.hip: adalog_softmax_adalog_pack_long_bf16,
csrc/attn_core.hip: adalog_attn_core_long, models.QF_LONG): the entry points validate their arguments before they touch the device,
the bounds of the existing entry points stand, and the model route's switch is off unless the environment turns it on."""
import ctypes
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from adalog_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _core(lib, bufs, N=577, D=64, Np=640, n_bits=4, G=3, H=3, gmod=3, null=()):
    """adalog_attn_core_long with host addresses for every pointer (never dereferenced: the call must be refused first)"""
    ptr = {k: (None if k in null else ctypes.addressof(bufs)) for k in
           ("qp", "kp", "vp", "sq", "sk", "sv", "a_scale", "qv", "mant", "out")}
    return lib.adalog_attn_core_long(ptr["qp"], ptr["kp"], ptr["vp"], G, N, D, H, gmod, Np, ptr["sq"], ptr["sk"], ptr["sv"], 1, 0.125,
                                     ptr["a_scale"], ptr["qv"], n_bits, ptr["mant"], 1.0, ptr["out"], None)


@pytest.mark.parametrize("kw,word", [
    (dict(null=("qp",)), b"null"), (dict(null=("vp",)), b"null"), (dict(null=("out",)), b"null"), (dict(null=("mant",)), b"null"),
    (dict(D=24), b"head dimension"), (dict(D=128), b"head dimension"), (dict(N=0, Np=0), b"N <= 1024"),
    (dict(N=1025, Np=1088), b"N <= 1024"), (dict(Np=576), b"Np"), (dict(Np=704), b"Np"), (dict(N=257, Np=257), b"Np"),
    (dict(n_bits=8), b"n_bits"), (dict(n_bits=1), b"n_bits"), (dict(G=4), b"multiple of H")])
def test_attn_core_long_rejects_bad_arguments_without_a_gpu(lib, kw, word):
    bufs = ctypes.create_string_buffer(256)
    rc = _core(lib, bufs, **kw)
    msg = lib.adalog_last_error()
    assert rc == -1 and b"attn_core_long" in msg and word in msg, (rc, msg)


def _soft(lib, bufs, rows=8, S=577, Kp=640, n_bits=4, null=()):
    ptr = {k: (None if k in null else ctypes.addressof(bufs)) for k in ("x", "scale", "qv", "mant", "out")}
    return lib.adalog_softmax_adalog_pack_long_bf16(ptr["x"], rows, S, 0.125, ptr["scale"], ptr["qv"], n_bits, ptr["mant"], ptr["out"],
                                                    Kp, None)


@pytest.mark.parametrize("kw,word", [
    (dict(null=("x",)), b"null"), (dict(null=("scale",)), b"null"), (dict(null=("qv",)), b"null"), (dict(null=("mant",)), b"null"),
    (dict(null=("out",)), b"null"), (dict(S=0, Kp=64), b"257 <= S"), (dict(S=256, Kp=256), b"257 <= S"),
    (dict(S=1025, Kp=1088), b"257 <= S"), (dict(S=1000, Kp=1088), b"Kp <= 1024"), (dict(Kp=576), b"257 <= S <= Kp"),
    (dict(Kp=600), b"multiple of 32"), (dict(n_bits=8), b"n_bits"), (dict(n_bits=1), b"n_bits"), (dict(rows=-1), b"rows")])
def test_softmax_pack_long_rejects_bad_arguments_without_a_gpu(lib, kw, word):
    bufs = ctypes.create_string_buffer(256)
    rc = _soft(lib, bufs, **kw)
    msg = lib.adalog_last_error()
    assert rc == -1 and b"softmax_adalog_pack_long" in msg and word in msg, (rc, msg)


def test_attn_core_long_supported_is_the_gate(lib):
    """adalog_attn_core_long_supported says what adalog_attn_core_long's argument checks say"""
    bufs = ctypes.create_string_buffer(256)
    for N in (0, 1, 197, 256, 257, 512, 513, 577, 1024, 1025, 4096):
        for D in (0, 8, 16, 24, 32, 48, 64, 80, 128):
            want = 1 if (1 <= N <= 1024 and D in (16, 32, 48, 64)) else 0
            assert lib.adalog_attn_core_long_supported(N, D) == want, (N, D)
            # G = 4 with H = 3 is refused after the shape checks: a supported shape gets as far as that, nothing is launched
            refused = _core(lib, bufs, N=N, D=D, Np=((N + 63) // 64) * 64, G=4)
            msg = lib.adalog_last_error()
            assert refused == -1 and (b"multiple of H" in msg) == bool(want), (N, D, msg)
            assert want or b"N <= 1024" in msg or b"head dimension" in msg, (N, D, msg)


def test_existing_bounds_stand(lib):
    """the <= 256 entry points keep their contracts: the long forms are new entry points, not wider old ones"""
    from adalog_amd import ops
    assert lib.adalog_attn_core_supported(257, 64) == 0 and lib.adalog_attn_core_supported(256, 64) == 1
    assert not ops.attn_core_ok(257, 64) and not ops.attn_core_ok(577, 64)
    assert not ops.softmax_adalog_pack_ok(257) and ops.softmax_adalog_pack_ok(256)
    assert ops.attn_core_long_ok(257, 64) and ops.attn_core_long_ok(577, 32) and ops.attn_core_long_ok(1024, 16)
    assert not ops.attn_core_long_ok(1025, 64) and not ops.attn_core_long_ok(577, 24)
    assert [S for S in (1, 256, 257, 577, 960, 1024, 1025) if ops.softmax_adalog_pack_long_ok(S)] == [257, 577, 960, 1024]
    assert ops.QF_LONG is True


def test_model_switch_is_off_by_default():
    """models.QF_LONG follows ADALOG_QF_LONG: unset or anything but "1" is off; the other two switches keep their defaults"""
    code = "from adalog_amd.utils import models as M; print(int(M.QF_LONG), int(M.QF_FUSED), int(M.QF_ATTN_CORE))"
    for val, want in ((None, "0 1 0"), ("0", "0 1 0"), ("yes", "0 1 0"), ("1", "1 1 0")):
        env = {k: v for k, v in os.environ.items() if k not in ("ADALOG_QF_LONG", "ADALOG_QF_FUSED", "ADALOG_QF_ATTN_CORE")}
        if val is not None:
            env["ADALOG_QF_LONG"] = val
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip() == want, (val, out.stdout)


def test_gate_refuses_long_rows_and_small_heads_unless_switched_on(monkeypatch):
    """Attention._fused_shape_ok: with QF_LONG off, 577 tokens and head dimension 32 are refused as they always were (the backend is
    not even asked); with it on, a backend without the capability flag refuses, one with it decides by softmax_adalog_pack_long_ok; and
    the whole gate refuses a 577-token input with the switch off."""
    from adalog_amd import backend
    from adalog_amd.utils import models as M
    a64, a32 = M.Attention(384, 6), M.Attention(192, 6)
    asked = []
    has = SimpleNamespace(QF_LONG=True, QF_EXTRAS=True,
                          softmax_adalog_pack_long_ok=lambda S: asked.append(S) or 256 < S <= 1024)
    old = backend._backend
    try:
        backend.set_backend(has)
        monkeypatch.setattr(M, "QF_LONG", False)
        assert a64._fused_shape_ok(197) and a64._fused_shape_ok(256)
        assert not a64._fused_shape_ok(257) and not a64._fused_shape_ok(577) and not a32._fused_shape_ok(197)
        assert asked == []
        assert not a64._fused_quant_forward_ok(torch.zeros(1, 577, 384))
        monkeypatch.setattr(M, "QF_LONG", True)
        assert a64._fused_shape_ok(197) and a64._fused_shape_ok(257) and a64._fused_shape_ok(577) and a64._fused_shape_ok(1024)
        assert not a64._fused_shape_ok(1025)
        assert a32._fused_shape_ok(197) and a32._fused_shape_ok(577) and not a32._fused_shape_ok(2000)
        assert not M.Attention(120, 5)._fused_shape_ok(197)                 # head dimension 24
        backend.set_backend(SimpleNamespace(QF_EXTRAS=True))                # (the CPU specification backend: no QF_LONG attribute)
        assert a64._fused_shape_ok(256) and not a64._fused_shape_ok(577) and not a32._fused_shape_ok(197)
    finally:
        backend._backend = old
