"""`-m gpu`: the launch sites of the scoring GEMM's host code (csrc/gemm_score.hip: gemm_score_impl, gemm_out_gen_impl) that no other
test pins by label at a small shape -- one table row per site, the smallest shape the layout sends there with the default switches, a
ragged last row tile and a ragged last column tile, the label of adalog_last_kernel asserted exactly and the scores compared with the
CPU specification at the tolerance test_gpu_kernels.py uses for that kernel (3e-6, test_gemm_stream_kernel_variants).

Where the other sites are pinned (small shapes, label and value asserted in the same test):
  k_gemm_score, k_gemm_cand (store form)        test_gpu_kernels.py::test_gemm_score_vs_spec, ::test_gemm_score_candidates_in_columns
  k_gemm_cand_glds                              test_gpu_kernels.py::test_gemm_score_candidates_in_columns
  k_gemm_cand_ex                                test_gpu_kernels.py::test_gemm_out_addend_and_heads_last
  k_gemm_cand_gen, k_gemm_cand_gen_ex           test_gpu_kernels.py::test_gemm_out_gen_equals_pack_then_gemm
  k_gemm_cand_gen_rows                          test_gpu_swin_quant_forward.py::test_gemm_out_gen_rows_equals_gather_and_scatter
  k_gemm_stream<i8|bf16|fp8>, narrow and wide   test_gpu_kernels.py::test_gemm_stream_kernel_variants
  k_gemm_stream<bf16xfp8>, k_gemm_stream<bf16>  test_gpu_kernels.py::test_gemm_mixed_streaming_weight_search (193 x 260 x 3 is its smallest)
  slab, group, window, avq, gen kernels         their own tests in test_gpu_kernels.py and test_gpu_group_barrier.py
That leaves k_gemm_stream<f32> (the narrow and the wide form share the label; the rows below take one each).

k_gemm_cand in its scoring form has no row: with the default switches every scoring launch with C = 1 that is not a streaming shape
has a row tile of at most 128 rows and goes to k_gemm_cand_glds; the scoring form is reached only with ADALOG_GEMM_GLDS=0, which the
library reads once per process.
"""
import pytest
import torch

from tests import cpu_backend as CB

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from adalog_amd import backend
    backend.set_backend(None)
    return backend.get()


def _last_kernel():
    from adalog_amd import _lib
    return _lib.load().adalog_last_kernel().decode()


def rel_err(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


# (label, dtype, M, reference columns, K, P, G): candidates in the GEMM columns (ref_div = P), transposed reference.
#   narrow: 160 bytes of K (< 512): two workgroups per CU, 128-row tiles -- M = 197 leaves 69 rows, 5 x 64 columns leave 64 of 256
#   wide:   520 bytes of K, M >= 192: one workgroup per CU, 256-row tile -- M = 200 leaves it ragged, K is no multiple of the K-step
STREAM_ROWS = [("k_gemm_stream<f32>", "f32", 197, 5, 40, 64, 3),
               ("k_gemm_stream<f32>", "f32", 200, 5, 130, 64, 3)]


@pytest.mark.parametrize("label,dtype,M,Ncols,K,P,G", STREAM_ROWS)
def test_stream_route(ops, label, dtype, M, Ncols, K, P, G):
    gen = torch.Generator().manual_seed(4100 + M + K)
    dt_c, dt_o, tdt = {"f32": (CB.F32, ops.F32, torch.float32)}[dtype]
    Kp = CB.pad_k(K, dt_c)
    A = torch.zeros(1, G, M, Kp, dtype=tdt); B = torch.zeros(1, G, Ncols * P, Kp, dtype=tdt)
    A[..., :K] = (torch.randint(-15, 16, (1, G, M, K), generator=gen).float() * 0.25).to(tdt)
    B[..., :K] = torch.randint(-15, 16, (1, G, Ncols * P, K), generator=gen).float().to(tdt)
    ref = torch.randn(G, Ncols, M, generator=gen) * 3                          # stored [G, N, M] (transposed)
    sa = torch.rand(1, generator=gen) * 0.002 + 0.001
    sb = torch.rand(P, Ncols, generator=gen) * 0.5 + 0.5
    rs = torch.rand(M, generator=gen) + 0.5; rb = torch.randn(M, generator=gen)
    b_cn = torch.randn(P, Ncols, generator=gen)
    Ad, Bd = A.to(DEV), B.to(DEV)
    Ad.k_valid = K; Bd.k_valid = K
    for keep_n in (True, False):                     # per-tile partials / per-workgroup fp64 accumulators
        for rows in (False, True):
            want = CB.gemm_score(dt_c, A, B, M, Ncols, P, G, 1, ref, CB.Strided(sa), CB.Strided(sb, c=Ncols, n=1),
                                 CB.Strided(b_cn, c=Ncols, n=1), False, keep_n, 0.01, sa_mul=0.5, ref_div=P, ref_transposed=True,
                                 row_scale=rs if rows else None, row_bias=rb if rows else None)
            got = ops.gemm_score(dt_o, Ad, Bd, M, Ncols, P, G, 1, ref.to(DEV), ops.Strided(sa.to(DEV)),
                                 ops.Strided(sb.to(DEV), c=Ncols, n=1), ops.Strided(b_cn.to(DEV), c=Ncols, n=1), False, keep_n, 0.01,
                                 sa_mul=0.5, ref_div=P, order=2, ref_transposed=True, row_scale=rs.to(DEV) if rows else None,
                                 row_bias=rb.to(DEV) if rows else None)
            assert _last_kernel() == label
            err = rel_err(got.cpu(), want)
            print(label, (M, Ncols, K), keep_n, rows, err)
            assert got.shape == want.shape and err <= 3e-6, (keep_n, rows, err)
