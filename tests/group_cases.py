"""Cases of the q.k^T group kernels shared by the in-process `-m gpu` test (wave-private form, k_gemm_grpw) and the child
process of tests/test_gpu_group_barrier.py (barrier form, k_gemm_grp: reachable only with ADALOG_GEMM_GRPW=0, which the
library reads once per process).

    python -m tests.group_cases 'k_gemm_grp<'      # every dtype and P; exits non-zero unless every launch carries the label
"""
import sys

import torch

from tests import cpu_backend as CB

DEV = "cuda"
TOL = 3e-6
DTYPES = ("i8", "fp8")
PS = (64, 128, 256)
# (M, Ncols, G, K, gmod).  The last two leave the last row block one and three rows: the reference load is clamped to
# M - 4 and the owned elements are shifted by 12 and 4 bytes (the first three reach 0, 4 and 8 only).
SHAPES = ((197, 197, 12, 64, 6), (160, 37, 24, 48, 6), (224, 9, 18, 64, 6), (129, 5, 8, 16, 4), (131, 3, 8, 64, 4))


def rel_err(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


def run_group_case(ops, dtype, P):
    """Group kernel (attention q.k^T searches: int8 or fp8 storage, one 64-byte K-step, 129..224 rows, many image x head groups, scores
    summed over the columns): ragged and exact last row block, a column count that leaves the last stage and the last
    chunk partly empty, head-wise and tensor-wise scores -- against the CPU specification.  Returns the label of the kernel
    behind every launch."""
    from adalog_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(5200 + P)
    dt_c, dt_o = {"i8": (CB.I8, ops.I8), "fp8": (CB.FP8, ops.FP8)}[dtype]
    tdt = {"i8": torch.int8, "fp8": torch.float8_e4m3fn}[dtype]
    labels = []
    for M, Ncols, G, K, gmod in SHAPES:
        Kp = CB.pad_k(K, dt_c, 64)
        A = torch.zeros(1, G, M, Kp, dtype=tdt); B = torch.zeros(1, G, Ncols * P, Kp, dtype=tdt)
        A[..., :K] = torch.randint(-15, 16, (1, G, M, K), generator=gen).float().to(tdt)
        B[..., :K] = torch.randint(-15, 16, (1, G, Ncols * P, K), generator=gen).float().to(tdt)
        ref = torch.randn(G, Ncols, M, generator=gen) * 3                      # stored [G, N, M] (transposed)
        sa = torch.rand(gmod, generator=gen) * 0.02 + 0.01
        sb = torch.rand(P, gmod, generator=gen) * 0.5 + 0.5
        Ad, Bd = A.to(DEV), B.to(DEV)
        Ad.k_valid = K; Bd.k_valid = K
        for keep_h in (True, False):
            want = CB.gemm_score(dt_c, A, B, M, Ncols, P, G, gmod, ref, CB.Strided(sa, g=1), CB.Strided(sb, c=gmod, g=1), None,
                                 keep_h, False, 0.01, sa_mul=0.5, ref_div=P, ref_transposed=True)
            got = ops.gemm_score(dt_o, Ad, Bd, M, Ncols, P, G, gmod, ref.to(DEV), ops.Strided(sa.to(DEV), g=1),
                                 ops.Strided(sb.to(DEV), c=gmod, g=1), None, keep_h, False, 0.01, sa_mul=0.5, ref_div=P,
                                 order=2, ref_transposed=True)
            labels.append(lib.adalog_last_kernel().decode())
            assert got.shape == want.shape and rel_err(got.cpu(), want) <= TOL, (M, Ncols, G, K, keep_h, rel_err(got.cpu(), want))
    return labels


def main(prefix):
    from adalog_amd import backend
    backend.set_backend(None)
    ops = backend.get()
    for dtype in DTYPES:
        for P in PS:
            labels = run_group_case(ops, dtype, P)
            assert labels and all(k.startswith(prefix) for k in labels), (dtype, P, labels)
            print(dtype, P, "ok", sorted(set(labels)), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
