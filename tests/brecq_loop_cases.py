"""The toy block of tests/golden/brecq_traj.npz in reconstruct_single_block calls that end or raise, and the state a block must be
left in either way: shared by tests/test_brecq_loop_cpu.py and tests/test_gpu_brecq_loop.py."""
import os

import numpy as np
import pytest
import torch

from adalog_amd.quantizers import _drop
from adalog_amd.utils import block_recon as BR
from tests import drop_reference as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "brecq_traj.npz")


class Boom(Exception):
    pass


def toy(device="cpu"):
    """-> (reconstructor with the reference's mini-batch sequence, block)"""
    blk, perms = DR.traj_block(np.load(GOLDEN, allow_pickle=False), torch.device(device))
    rec = object.__new__(BR.BlockReconstructor)
    rec.index_source = lambda it, n, b: perms[it][:b]
    return rec, blk


def snapshot(blk):
    return dict(grad=[(p_, p_.requires_grad) for p_ in blk.parameters()],
                drop=[(q_, q_.drop_prob) for q_ in _drop.activation_quantizers(blk)],
                tf32=torch.backends.cuda.matmul.allow_tf32)


def assert_left_as_finished(blk, snap):
    """the state of a block after reconstruct_single_block, however the call ended"""
    for name, m in blk.named_modules():
        if hasattr(m, "mode"):
            assert m.mode == "raw", name
        if hasattr(m, "w_quantizer"):
            assert not m.w_quantizer.soft_targets, name
        if hasattr(m, "training_mode"):
            assert not m.training_mode, name
    assert all(p_.requires_grad == was for p_, was in snap["grad"])
    assert any(was for _, was in snap["grad"])
    for q_, was in snap["drop"]:
        assert q_.drop_prob == was and q_.drop_state is None
    assert torch.backends.cuda.matmul.allow_tf32 == snap["tf32"]


def train_clean(device="cpu", iters=6, device_arg=None, **kw):
    """``device_arg``: what the call is given as its device (default: the torch.device)"""
    rec, blk = toy(device)
    rec.reconstruct_single_block("blk", blk, torch.device(device) if device_arg is None else device_arg, batch_size=4, iters=iters,
                                 quant_act=True, **kw)
    return DR.trained_tensors(blk)


def fail_in_iteration(device="cpu", at=3, iters=6, **kw):
    """an iter_hook that raises after iteration ``at`` -> the block and its state before the call"""
    rec, blk = toy(device)

    def hook(it, loss_func):
        if it == at:
            raise Boom()
    rec.iter_hook = hook
    snap = snapshot(blk)
    with pytest.raises(Boom):
        rec.reconstruct_single_block("blk", blk, torch.device(device), batch_size=4, iters=iters, **kw)
    return blk, snap
