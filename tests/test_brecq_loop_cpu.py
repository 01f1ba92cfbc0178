"""The parts of the BRECQ block loop (adalog_amd/utils/block_recon.py) on the CPU tier: the training scope on every way out, the
rows-ahead uploader, the schedule table against the objects it stands in for, and the two definitions of "what a block trains" /
"which modules carry an AdaRound quantiser".  Toy block and data: tests/golden/brecq_traj.npz (tests/drop_reference.py)."""
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

from adalog_amd import backend
from adalog_amd.utils import block_recon as BR
from tests import cpu_backend
from tests.brecq_loop_cases import ROOT, Boom, assert_left_as_finished, fail_in_iteration, snapshot, toy, train_clean


@pytest.fixture(autouse=True)
def _cpu_backend():
    backend.set_backend(cpu_backend)
    yield
    backend.set_backend(None)


@pytest.mark.parametrize("kw", [dict(quant_act=True, drop_prob=0.5), dict(quant_act=False)], ids=["qdrop", "weights_only"])
def test_exception_during_an_iteration_leaves_a_finished_block(kw):
    blk, snap = fail_in_iteration(**kw)
    assert_left_as_finished(blk, snap)
    assert blk.raw_input is not None and blk.raw_out is not None      # a failed block keeps its data


def test_exception_in_the_report_before_the_iterations_leaves_a_finished_block(monkeypatch):
    monkeypatch.delenv("ADALOG_BRECQ_REPORT", raising=False)
    rec, blk = toy()
    calls = []

    def first_forward_raises(*a, **k):
        calls.append(1)
        del blk.fc1.__dict__["forward"]                               # (this call only)
        raise Boom()
    blk.fc1.forward = first_forward_raises
    snap = snapshot(blk)
    with pytest.raises(Boom):
        rec.reconstruct_single_block("blk", blk, torch.device("cpu"), batch_size=4, iters=6, quant_act=True, drop_prob=0.5)
    assert calls == [1]
    assert_left_as_finished(blk, snap)
    assert blk.raw_input is not None


def test_clean_call_after_a_failed_one_trains_as_a_fresh_process_does(tmp_path):
    """nothing global stays set by a call that raised (adaround.COLLECT, train_mm's offers, the tf32 switch)"""
    out = str(tmp_path / "fresh.pt")
    code = ("import sys, torch; sys.path.insert(0, {!r}); from adalog_amd import backend; from tests import cpu_backend, brecq_loop_cases as T; "
            "backend.set_backend(cpu_backend); torch.save(T.train_clean(drop_prob=0.5), {!r})").format(ROOT, out)
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
    fresh = torch.load(out)
    fail_in_iteration(quant_act=True, drop_prob=0.5)
    after = train_clean(drop_prob=0.5)
    assert fresh.keys() == after.keys() and len(after) == 8
    for k in fresh:
        assert torch.equal(fresh[k], after[k]), k


def test_rows_ahead_serves_every_row_from_three_chunks():
    table = torch.arange(21 * 3, dtype=torch.float32).reshape(21, 3)
    calls = []

    def make_rows(it, cnt):
        calls.append((it, cnt))
        return table[it:it + cnt].clone()
    rows = BR._RowsAhead(make_rows, 21, "cpu", ahead=8)
    for it in range(21):
        assert torch.equal(rows.row(it), table[it])
    assert calls == [(0, 8), (8, 8), (16, 5)]
    assert BR._RowsAhead(make_rows, 21, "cpu").ahead == 256
    # the index instance: one draw per iteration, in order
    seen = []

    def index_source(it, n, bs):
        seen.append((it, n, bs))
        return torch.arange(bs) + it
    idx = BR._RowsAhead(functools.partial(BR._index_rows, index_source, None, 64, 4), 21, "cpu", ahead=8)
    for it in range(21):
        assert torch.equal(idx.row(it), torch.arange(4) + it)
    assert seen == [(it, 64, 4) for it in range(21)]
    # ... and without an index source the generator's own randperm sequence
    gen, ref = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    idx = BR._RowsAhead(functools.partial(BR._index_rows, None, gen, 64, 4), 21, "cpu", ahead=8)
    for it in range(21):
        assert torch.equal(idx.row(it), torch.randperm(64, generator=ref)[:4])


@pytest.mark.parametrize("qdrop", [False, True])
def test_schedule_table_rows_equal_the_stepped_objects(qdrop):
    iters, lr = 21, 4e-5
    kw = dict(round_loss="relaxation", weight=0.01, max_count=iters, rec_loss="mse", b_range=(20, 2), decay_start=0, warmup=0.2, p=2.0)
    table = BR._ScheduleTable(BR.LossFunction(None, **kw), iters, lr, torch.device("cpu"), seed=0xC0FFEE1234567890 if qdrop else None,
                              ahead=8)
    assert table.lr.item() == np.float32(lr)
    # the real objects, stepped in the loop's order: advance() before the iteration's optimiser step, the scheduler after it
    live = BR.LossFunction(None, **kw)
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=iters, eta_min=0.)
    gates = []
    for it in range(iters):
        row = table.row(it)
        active = live.advance()
        want = torch.tensor([float(live.b), 1.0 if active else 0.0, float(opt.param_groups[0]["lr"])], dtype=torch.float32)
        assert torch.equal(row[-3:], want), (it, row, want)
        assert torch.equal(torch.cat([table.b, table.gate, table.lr]), want), it      # the named views after the copy
        if qdrop:
            assert row.numel() == 4 and int(row[:1].view(torch.int32)) == it
            assert table.drop_state.tolist() == [0x34567890, 0xC0FFEE12 - 2 ** 32, it]
        else:
            assert row.numel() == 3 and table.drop_state is None
        gates.append(active)
        opt.step()
        sched.step()
    assert gates == [False] * 4 + [True] * 17                                       # (count < 0.2 * 21 = 4.2: off through count 4)
    assert table.row(20, copy=False).data_ptr() != table.words.data_ptr()


def test_adaround_modules_and_trained_list_what_the_hand_written_loops_listed():
    rec, blk = toy()
    assert BR.adaround_modules(blk) == []
    rec.wrap_quantizers_in_net(blk, "blk")
    assert [id(m) for m in BR.adaround_modules(blk)] == [id(blk.fc1), id(blk.fc2)]

    def same(got, want):
        return len(got) == len(want) and all(a is b for a, b in zip(got, want))
    w, a = BR._trained(blk, True)
    assert same(w, [blk.fc1.w_quantizer.alpha, blk.fc2.w_quantizer.alpha])
    assert same(a, [blk.fc1.a_quantizer.scale, blk.fc2.a_quantizer.scale, blk.matmul1.A_quantizer.scale, blk.matmul1.B_quantizer.scale,
                    blk.matmul2.A_quantizer.scale, blk.matmul2.B_quantizer.scale])
    assert same(rec._trained_tensors(blk, True),
                [blk.fc1.w_quantizer.alpha, blk.fc1.a_quantizer.scale, blk.fc2.w_quantizer.alpha, blk.fc2.a_quantizer.scale,
                 blk.matmul1.A_quantizer.scale, blk.matmul1.B_quantizer.scale, blk.matmul2.A_quantizer.scale, blk.matmul2.B_quantizer.scale])
    w, a = BR._trained(blk, False)
    assert same(w, [blk.fc1.w_quantizer.alpha, blk.fc2.w_quantizer.alpha]) and a == []
    assert same(rec._trained_tensors(blk, False), [blk.fc1.w_quantizer.alpha, blk.fc2.w_quantizer.alpha])
