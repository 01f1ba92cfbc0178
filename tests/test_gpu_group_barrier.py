"""`-m gpu`: the barrier form of the q.k^T group kernel (k_gemm_grp).  The library takes it only with ADALOG_GEMM_GRPW=0 and reads
that switch once per process, so the cases of tests/group_cases.py run in one fresh child interpreter that has it set."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gemm_group_kernel_barrier_form():
    """int8 and fp8, P = 64, 128, 256, the shapes of test_gemm_group_kernel: every launch must carry a k_gemm_grp< label and
    every score must be within 3e-6 of tests/cpu_backend.py (the child asserts both and exits non-zero otherwise)."""
    env = dict(os.environ, ADALOG_GEMM_GRPW="0")
    # measured on an MI355X: 14 s for the child (imports, library load and the CPU specification dominate); 180 s leaves headroom
    r = subprocess.run([sys.executable, "-m", "tests.group_cases", "k_gemm_grp<"], capture_output=True, text=True,
                       timeout=180, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(" ok ") == 6, r.stdout[-2000:]
