"""CPU stand-in backend with the act-order entry points of adalog_amd/ops.py -- TEST INFRASTRUCTURE ONLY: tests.gptq_cpu_backend plus
gptq_sweep(perm=...) and permute_sym.  The permuted sweep is the numpy restatement of tests/gptq_reference.py run on explicitly permuted
inputs, its outputs scattered back to natural column order -- the definition include/adalog_hip.h gives adalog_gptq_sweep_perm_f32."""
import numpy as np
import torch

from tests import gptq_reference as GR
from tests.gptq_cpu_backend import GptqCpuBackend


def check_perm(perm, K):
    p = np.asarray(perm)
    assert p.dtype == np.int32 and p.shape == (K,) and np.array_equal(np.sort(p), np.arange(K)), "perm is not a permutation of 0 .. K-1"
    return p.astype(np.int64)


def sweep_perm(W, scale, zero_point, n_bits, U, perm):
    """-> (What fp32 [R, K], codes uint8 [R, K], objective fp64 [R]) in NATURAL column order: GR.sweep on W[:, perm] with U the factor of
    the permuted Hessian; q and c of step j land at column perm[j]."""
    W = np.asarray(W, np.float32)
    p = check_perm(perm, W.shape[1])
    what_p, codes_p, obj = GR.sweep(np.ascontiguousarray(W[:, p]), scale, zero_point, n_bits, U)
    what, codes = np.empty_like(what_p), np.empty_like(codes_p)
    what[:, p], codes[:, p] = what_p, codes_p
    return what, codes, obj


class GptqPermCpuBackend(GptqCpuBackend):
    def __init__(self):
        super().__init__()
        self.perms = []                                    # the perm (numpy, or None) of every gptq_sweep call

    def gptq_sweep(self, w2, scale, zero_point, n_bits, U, want_codes=False, want_objective=False, perm=None):
        self.perms.append(None if perm is None else perm.numpy().copy())
        if perm is None:
            return super().gptq_sweep(w2, scale, zero_point, n_bits, U, want_codes, want_objective)
        assert w2.dim() == 2 and U.dtype == torch.float64 and tuple(U.shape) == (w2.shape[1], w2.shape[1]) and perm.dtype == torch.int32
        assert self.gptq_sweep_ok(*w2.shape)
        self.sweeps.append((int(w2.shape[0]), int(w2.shape[1]), int(n_bits)))
        what, codes, obj = sweep_perm(w2.detach().numpy(), scale.detach().reshape(-1).numpy(), zero_point.detach().reshape(-1).numpy(),
                                      int(n_bits), U.numpy(), perm.numpy())
        out = (torch.from_numpy(what),) + ((torch.from_numpy(codes),) if want_codes else ()) \
            + ((torch.from_numpy(obj),) if want_objective else ())
        return out if len(out) > 1 else out[0]

    def permute_sym(self, H, perm):
        assert H.dtype == torch.float64 and H.dim() == 2 and H.shape[0] == H.shape[1]
        p = torch.from_numpy(check_perm(perm.numpy(), int(H.shape[0])))
        return H[p][:, p].contiguous()
