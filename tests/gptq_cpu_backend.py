"""CPU stand-in backend with the GPTQ entry points of adalog_amd/ops.py -- TEST INFRASTRUCTURE ONLY: tests.cpu_backend (through the
packed-code stand-in of tests/test_packed_cpu.py) plus gptq_sweep_ok / gptq_sweep / gptq_hessian_add from the numpy reference."""
import torch

from tests import gptq_reference as GR
from tests.test_packed_cpu import PackedCpuBackend


class GptqCpuBackend(PackedCpuBackend):
    def __init__(self):
        self.sweeps = []                                   # (R, K, n_bits) of every gptq_sweep call

    def gptq_sweep_ok(self, R, K):
        return R >= 1 and 32 <= K <= 4096 and K % 32 == 0

    def gptq_sweep(self, w2, scale, zero_point, n_bits, U, want_codes=False, want_objective=False):
        assert w2.dim() == 2 and U.dtype == torch.float64 and tuple(U.shape) == (w2.shape[1], w2.shape[1])
        assert self.gptq_sweep_ok(*w2.shape)
        self.sweeps.append((int(w2.shape[0]), int(w2.shape[1]), int(n_bits)))
        what, codes, obj = GR.sweep(w2.detach().numpy(), scale.detach().reshape(-1).numpy(), zero_point.detach().reshape(-1).numpy(),
                                    int(n_bits), U.numpy())
        out = (torch.from_numpy(what),) + ((torch.from_numpy(codes),) if want_codes else ()) \
            + ((torch.from_numpy(obj),) if want_objective else ())
        return out if len(out) > 1 else out[0]

    def gptq_hessian_add(self, H, xq, chunk=512):
        assert H.dtype == torch.float64 and xq.dim() == 2 and tuple(H.shape) == (xq.shape[1], xq.shape[1])
        x = xq.detach().double()
        H.add_(x.t() @ x)
        return H
