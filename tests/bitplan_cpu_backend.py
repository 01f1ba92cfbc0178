"""CPU stand-in backend with the bit-cost entry points of adalog_amd/ops.py -- TEST INFRASTRUCTURE ONLY: tests.gptq_cpu_backend plus
bit_cost_ok / bit_cost from the numpy reference (tests/bitplan_reference.py)."""
import torch

from tests import bitplan_reference as BR
from tests.gptq_cpu_backend import GptqCpuBackend


class BitplanCpuBackend(GptqCpuBackend):
    def __init__(self):
        super().__init__()
        self.costs = []                                    # (R, K, bits) of every bit_cost call

    def bit_cost_ok(self, R, K, n_widths):
        return R >= 1 and 32 <= K <= 4096 and K % 32 == 0 and 1 <= n_widths <= 8

    def bit_cost(self, w2, scales, zero_points, bits, H):
        bits = tuple(int(b) for b in bits)
        assert w2.dim() == 2 and H.dtype == torch.float64 and tuple(H.shape) == (w2.shape[1], w2.shape[1])
        assert self.bit_cost_ok(w2.shape[0], w2.shape[1], len(bits)) and all(b == 0 or 2 <= b <= 8 for b in bits)
        assert tuple(scales.shape) == tuple(zero_points.shape) and scales.shape[0] == len(bits) and scales.shape[1] in (1, w2.shape[0])
        self.costs.append((int(w2.shape[0]), int(w2.shape[1]), bits))
        cost, _ = BR.bit_cost(w2.detach().cpu().numpy(), scales.detach().cpu().numpy(), zero_points.detach().cpu().numpy(), bits,
                              H.detach().cpu().numpy())
        return torch.from_numpy(cost)
