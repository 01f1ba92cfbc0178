"""CPU tier of the one-launch attention core (csrc/attn_core.hip): the entry point validates its arguments before it touches the
device, and the model route's switch is off unless the environment turns it on."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from adalog_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _call(lib, bufs, N=16, D=16, Np=64, n_bits=4, G=3, H=3, gmod=3, null=()):
    """adalog_attn_core with host addresses for every pointer (never dereferenced: the call must be refused first)"""
    ptr = {k: (None if k in null else ctypes.addressof(bufs)) for k in
           ("qp", "kp", "vp", "sq", "sk", "sv", "a_scale", "qv", "mant", "out")}
    return lib.adalog_attn_core(ptr["qp"], ptr["kp"], ptr["vp"], G, N, D, H, gmod, Np, ptr["sq"], ptr["sk"], ptr["sv"], 1, 0.125,
                                ptr["a_scale"], ptr["qv"], n_bits, ptr["mant"], 1.0, None, None, None, 0, ptr["out"], None)


@pytest.mark.parametrize("kw,word", [
    (dict(null=("qp",)), b"null"), (dict(null=("out",)), b"null"), (dict(null=("mant",)), b"null"),
    (dict(D=24), b"head dimension"), (dict(N=257, Np=320), b"N <= 256"), (dict(N=0), b"N <= 256"),
    (dict(n_bits=8), b"n_bits"), (dict(n_bits=1), b"n_bits"), (dict(Np=128), b"Np"), (dict(G=4), b"multiple of H")])
def test_attn_core_rejects_bad_arguments_without_a_gpu(lib, kw, word):
    bufs = ctypes.create_string_buffer(256)
    rc = _call(lib, bufs, **kw)
    msg = lib.adalog_last_error()
    assert rc == -1 and b"attn_core" in msg and word in msg, (rc, msg)


def test_attn_core_supported_is_the_gate(lib):
    for N, D, want in [(1, 16, 1), (197, 64, 1), (256, 48, 1), (49, 32, 1), (257, 64, 0), (0, 64, 0), (197, 24, 0), (197, 128, 0)]:
        assert lib.adalog_attn_core_supported(N, D) == want, (N, D)


def test_model_switch_is_off_by_default():
    """models.QF_ATTN_CORE follows ADALOG_QF_ATTN_CORE: unset or anything but "1" is off"""
    code = "from adalog_amd.utils import models as M; print(int(M.QF_ATTN_CORE))"
    for val, want in ((None, "0"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "ADALOG_QF_ATTN_CORE"}
        if val is not None:
            env["ADALOG_QF_ATTN_CORE"] = val
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip() == want, (val, out.stdout)
