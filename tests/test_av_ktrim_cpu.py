"""Host side of the trimmed-K softmax.v weight search (no GPU): row lengths from pad_k / mixed_k_align and the library's shape
predicate adalog_gemm_mixed_ktrim next to adalog_gemm_mixed_ok."""
import os

import pytest

from adalog_amd.ops import BF16, FP8, mixed_k_align, pad_k


def test_pad_k_at_sixteen_element_rows():
    # fp8 columns: k_align in bytes = elements; bf16 rows: 32 bytes = 16 elements
    for K, want in ((193, 208), (197, 208), (200, 208), (207, 208), (208, 208), (209, 224), (129, 144), (577, 592)):
        assert pad_k(K, FP8, 16) == want and pad_k(K, BF16, 32) == want
    assert pad_k(197, FP8, 256) == 256 and pad_k(197, BF16, 512) == 256      # the rows the trimmed form replaces
    assert pad_k(49, FP8, 64) == 64 and pad_k(49, BF16, 128) == 64


def test_mixed_k_align():
    assert mixed_k_align(49) == (64, 128) and mixed_k_align(49, 208) == (64, 128)     # windows: never trimmed
    assert mixed_k_align(197) == (256, 512) and mixed_k_align(197, 0) == (256, 512)
    for K in (193, 197, 207, 208):
        assert mixed_k_align(K, 208) == (16, 32)
        al_c, al_r = mixed_k_align(K, 208)
        assert pad_k(K, FP8, al_c) == pad_k(K, BF16, al_r) == 208
    assert mixed_k_align(209, 208) == (256, 512)          # a row length K does not pad to is not taken
    assert mixed_k_align(129, 208) == (256, 512)


@pytest.fixture(scope="module")
def lib():
    from adalog_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_ktrim_predicate(lib):
    P, H, D = 128, 6, 64
    ok = lambda M, K, G=12, gmod=H, p=P: lib.adalog_gemm_mixed_ok(M, D * p, G, gmod, p, K)
    kp = lambda M, K, G=12, gmod=H, p=P: lib.adalog_gemm_mixed_ktrim(M, D * p, G, gmod, p, K)
    for K in (193, 197, 200, 201, 207, 208):
        for M in (129, 197, 224):
            assert ok(M, K) == 1 and kp(M, K) == 208
    for p in (64, 256):
        assert kp(197, 197, p=p) == 208
    # K past 208: the 256-element rows stay; outside the mixed 197-token family there is nothing to trim
    for K in (209, 224, 256):
        assert ok(197, K) == 1 and kp(197, K) == 0
    assert kp(197, 192) == 0 and kp(197, 129) == 0 and ok(197, 129) == 0
    assert kp(33, 197) == 0 and kp(225, 197) == 0 and kp(128, 197) == 0
    assert kp(197, 197, G=6) == 0                          # fewer than 8 groups
    assert kp(197, 197, G=34, gmod=17) == 0                # more than 16 heads per image
    assert kp(197, 197, p=100) == 0                        # not a candidate count the group kernels take
    assert kp(49, 49, G=512, gmod=4) == 0                  # the window family keeps its 64-element rows
    assert kp(197, 1536, G=1, gmod=1) == 0                 # the wide streaming family


def test_switch_defaults_on():
    """ADALOG_AV_KTRIM is read when the module is imported, so the default is checked where nothing has imported it yet: one
    child interpreter, variable unset (on), then '0' (off), then '1' (on)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import os, importlib\n"
            "os.environ.pop('ADALOG_AV_KTRIM', None)\n"
            "from adalog_amd.quant_layers import matmul as MM\n"
            "out = [MM.AV_KTRIM]\n"
            "for v in ('0', '1'):\n"
            "    os.environ['ADALOG_AV_KTRIM'] = v\n"
            "    out.append(importlib.reload(MM).AV_KTRIM)\n"
            "print('KTRIM', out)\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "KTRIM [True, False, True]" in res.stdout, res.stdout[-500:]
