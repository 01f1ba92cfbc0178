"""`-m gpu`: the BRECQ block loop's captured route on the toy block of tests/golden/brecq_traj.npz (16 features, batch 4) -- a device
given as a string, and an exception between two replays.  Twelve iterations pass the three eager ones, the capture and eight replays."""
import pytest
import torch

from tests.brecq_loop_cases import assert_left_as_finished, fail_in_iteration, train_clean

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_backend(monkeypatch):
    from adalog_amd import backend
    backend.set_backend(None)
    backend.get()
    for name in ("ADALOG_BRECQ_GRAPH", "ADALOG_BRECQ_ADAM", "ADALOG_BRECQ_ALPHA_STEP"):
        monkeypatch.delenv(name, raising=False)
    yield


def test_device_given_as_a_string(golden):
    """the replay route read ``device.type`` of its argument: 'cuda' raised AttributeError in the fifth iteration"""
    by_name = train_clean("cuda", iters=12, device_arg="cuda")
    by_object = train_clean("cuda", iters=12)
    assert by_name.keys() == by_object.keys() and len(by_name) == 8
    for k in by_name:
        assert by_name[k].is_cuda and torch.equal(by_name[k], by_object[k]), k


def test_exception_between_replays_leaves_a_finished_block_and_nothing_set(golden):
    iters, bs = [int(v) for v in golden("brecq_traj")["cfg"]]
    assert bs == 4 and iters > 8
    undisturbed = train_clean("cuda", iters=iters)                    # (the run of layer_cases.case_brecq_traj, graph on)
    blk, snap = fail_in_iteration("cuda", at=7, iters=12, quant_act=True, drop_prob=0.5)
    assert_left_as_finished(blk, snap)
    assert blk.raw_input is not None and blk.raw_out is not None
    from adalog_amd.quantizers import adaround
    assert adaround.COLLECT is None
    after = train_clean("cuda", iters=iters)
    assert undisturbed.keys() == after.keys() and len(after) == 8
    for k in after:
        assert torch.equal(undisturbed[k], after[k]), k
