"""`-m gpu`: k_gemm_avw_gen (the softmax.v weight search with generated candidates) where a workgroup runs SEVERAL items and an
item SEVERAL head-dim columns: the LDS image of the fixed operand handed over from one item to the next (another group each time),
the reference column staged in LDS once per workgroup and head-dim column (two buffers alternating over the columns, or one at
200 rows), ragged chunks, and 2 / 4 / 8 waves reading the shared reference buffer.  Shapes, helpers and the fp64 rule are those of
test_gpu_av_gen.py; the scores are compared for equality with pack + k_gemm_grpk8t<13> wherever that launch exists."""
import pytest
import torch

import tests.test_gpu_av_gen as T
from tests.test_gpu_av_gen import _case, _fp64_scores, _scores, ops  # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu

DEV, H, NEW, OLD = T.DEV, T.H, T.NEW, "k_gemm_grpk8t<13,bf16xfp8>"


def _items(wgs, G, Sp, P):
    """grp_chunks of csrc/gemm_score.hip: (items of the launch, 32-column blocks per chunk, chunks per group)"""
    cdiv = lambda a, b: -(-a // b)
    NB = Sp * P // 32
    CB = cdiv(cdiv(NB, max(1, cdiv(3 * wgs, G))), 8) * 8
    return G * cdiv(NB, CB), CB, cdiv(NB, CB)


def _both(ops, imgs, S, Sp, P, bits=4, headwise=True, seed=0):
    A, v, sc, zp = _case(imgs, S, Sp, P, bits, headwise, seed=seed)
    want, k_old = _scores(ops, False, A, v, sc, zp, P, bits, headwise)
    got, k_new = _scores(ops, True, A, v, sc, zp, P, bits, headwise)
    print(f"imgs={imgs} S=K={S} Sp={Sp} P={P}: old {k_old}, new {k_new}, differing {int((got != want).sum())}/{got.numel()}")
    return want, k_old, got, k_new


@pytest.mark.parametrize("S", [197, 193, 200])
def test_several_items_per_workgroup(ops, S):
    """G = 96 groups, 32 head-dim columns, 128 candidates: chunks of 8 column blocks = two head-dim columns per item, 16 chunks per
    group, 1 536 items -- three per workgroup at 512 workgroups, 512 items apart and so of another group each: every item loads a new
    image over the last one's, and its two columns use both reference buffers (197, 193 rows: the last row block holds 5 rows / 1
    row) or the single one (200 rows)."""
    imgs, Sp, P = 48, 32, 128
    wgs = ops.gemm_score_avw_ok(S, Sp, imgs * H, H, P, S, (S + 15) // 16 * 16, 4)
    items, CB, nch = _items(wgs, imgs * H, Sp, P)
    print(f"S={S}: {wgs} workgroups, {items} items, {CB} column blocks per chunk, {nch} chunks per group")
    assert wgs > 0 and items > wgs                   # more than one item per workgroup, on a part with more CUs too
    assert CB // (P // 32) >= 2                      # more than one head-dim column per item
    want, k_old, got, k_new = _both(ops, imgs, S, Sp, P)
    assert k_old == OLD and k_new == NEW
    assert torch.isfinite(want).all() and want.abs().max() > 0
    assert torch.equal(got, want)


def test_partial_row_blocks_many_items_ragged_chunk(ops):
    """the form for 192 rows or fewer: 33 rows (two row blocks, the second with one row), G = 512 groups, 128 column blocks in chunks
    of 48 / 48 / 32 (12 / 12 / 8 head-dim columns), 1 536 items.  No packed mixed group launch exists here: as in
    test_small_shapes_against_current_route the kernel's largest relative error against the fp64 objective may exceed that of the
    route the search ran by no more than that route's own spread over that test's cases (1.14e-7, recorded there).  Two launches
    on the same inputs give the same bits."""
    imgs, S, Sp, P, bits = 256, 33, 32, 128, 4
    wgs = ops.gemm_score_avw_ok(S, Sp, imgs * H, H, P, S, (S + 15) // 16 * 16, bits)
    items, CB, nch = _items(wgs, imgs * H, Sp, P)
    print(f"{wgs} workgroups, {items} items, {CB} column blocks per chunk, {nch} chunks per group")
    assert wgs > 0 and items > wgs and Sp * P // 32 % CB != 0          # a ragged last chunk
    A, v, sc, zp = _case(imgs, S, Sp, P, bits, True)
    want, k_old = _scores(ops, False, A, v, sc, zp, P, bits, True)
    got, k_new = _scores(ops, True, A, v, sc, zp, P, bits, True)
    again, _ = _scores(ops, True, A, v, sc, zp, P, bits, True)
    ref = _fp64_scores(A, v, A.to(DEV) @ v.to(DEV), sc, zp, bits, True)
    rel = lambda t: ((t.double() - ref).abs() / ref.abs()).max().item()
    e_old, e_new = rel(want), rel(got)
    print(f"old {k_old} rel err {e_old:.3e}, new {k_new} rel err {e_new:.3e}, differing {int((got != want).sum())}/{got.numel()}")
    assert "avw" not in k_old and k_new == NEW
    assert torch.isfinite(want).all() and want.abs().max() > 0
    assert torch.equal(got, again)
    assert e_new <= e_old + 1.14e-7


@pytest.mark.parametrize("P", [64, 256])
def test_two_and_eight_waves(ops, P):
    """64 and 256 candidates: 2 and 8 waves per workgroup stage and read the shared reference column (2 waves: two rows per lane)"""
    want, k_old, got, k_new = _both(ops, 24, 197, 32, P)
    assert k_old == OLD and k_new == NEW
    assert torch.isfinite(want).all() and want.abs().max() > 0
    assert torch.equal(got, want)


@pytest.mark.parametrize("row,col", [(195, 1), (70, 30)])
def test_planted_reference(ops, monkeypatch, row, col):
    """one attention row of one head-dim column of the reference (raw_out) carries values 1e3 times the rest: a reference column that
    is stale by one head-dim column, one buffer or one item moves the scores by far more than rounding.  (195, 1): the
    ragged last row block, the second column of an item; (70, 30): a whole row block, the first column of a later chunk."""
    layer = T._layer

    def planted(A, v, P, bits, headwise):
        lay = layer(A, v, P, bits, headwise)
        lay.raw_out[:, :, row, col] *= 1.0e3
        return lay

    base = _both(ops, 48, 197, 32, 128, seed=1)[0]
    monkeypatch.setattr(T, "_layer", planted)
    want, k_old, got, k_new = _both(ops, 48, 197, 32, 128, seed=1)
    assert k_old == OLD and k_new == NEW
    assert torch.isfinite(want).all()
    # the planted column moves every score by more than a thousand roundings of its fp32 value: a stale column cannot hide in them
    assert ((want - base).abs() > 1.0e3 * 2.0 ** -24 * base.abs()).all()
    assert torch.equal(got, want)
