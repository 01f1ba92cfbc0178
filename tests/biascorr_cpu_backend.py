"""CPU stand-in backend with the bias-correction entry point of adalog_amd/ops.py -- TEST INFRASTRUCTURE ONLY: the GPTQ stand-in
(tests/gptq_cpu_backend.py, itself over tests.cpu_backend) plus mean_err from the exactly rounded restatement."""
import torch

from tests import biascorr_reference as BR
from tests.gptq_cpu_backend import GptqCpuBackend


class BiasCorrCpuBackend(GptqCpuBackend):
    def __init__(self):
        super().__init__()
        self.mean_errs = []                                # (n, n_channels, inner) of every mean_err call

    def mean_err(self, a, b, n_channels=1, inner=None):
        assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.numel() == b.numel()
        n = a.numel()
        inner = max(1, n // n_channels) if inner is None else inner
        assert n % (n_channels * inner) == 0
        self.mean_errs.append((n, int(n_channels), int(inner)))
        return BR.mean_err(a.contiguous(), b.contiguous(), n_channels, inner)
