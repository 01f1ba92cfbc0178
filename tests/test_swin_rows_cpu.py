"""The row map of the Swin block's fused quant_forward (utils/models.py: swin_token_rows, SwinTransformerBlock.token_rows): it equals
roll(-shift) + window_partition on token indices, window_reverse + roll(+shift) undoes it, and it leaves the state_dict alone (CPU tier)."""
import pytest
import torch

from adalog_amd.utils import models as M

CASES = [(56, 7, 0), (56, 7, 3), (28, 7, 0), (28, 7, 3), (14, 7, 0), (14, 7, 3), (7, 7, 0),
         (24, 12, 0), (24, 12, 6), (12, 12, 0), (16, 4, 0), (16, 4, 2)]


def _composed(res, ws, s):
    idx = torch.arange(res * res).view(1, res, res, 1)
    if s:
        idx = torch.roll(idx, shifts=(-s, -s), dims=(1, 2))
    return M.window_partition(idx, (ws, ws)).reshape(-1)


@pytest.mark.parametrize("res,ws,s", CASES)
def test_token_rows_equal_roll_then_partition(res, ws, s):
    rows = M.swin_token_rows((res, res), (ws, ws), (s, s))
    assert rows.dtype == torch.int32 and rows.shape == (res * res,) and rows.is_contiguous()
    assert torch.equal(rows.long(), _composed(res, ws, s))
    assert torch.equal(torch.sort(rows.long()).values, torch.arange(res * res))           # a permutation of the image's tokens


@pytest.mark.parametrize("res,ws,s", CASES)
def test_reverse_then_roll_back_inverts_the_map(res, ws, s):
    rows = M.swin_token_rows((res, res), (ws, ws), (s, s)).long()
    back = M.window_reverse(rows.view(-1, ws, ws, 1), (ws, ws), res, res)
    if s:
        back = torch.roll(back, shifts=(s, s), dims=(1, 2))
    assert torch.equal(back.reshape(-1), torch.arange(res * res))


@pytest.mark.parametrize("res,ws,s", CASES)
def test_gather_through_the_map_is_the_module_route_partition(res, ws, s):
    """x [B, H, W, C] gathered per image through the map, in periods of L = H * W rows (the GEMM loader's indexing), equals the
    module route's roll + window_partition; scattered back it is x again."""
    B, C, L = 3, 5, res * res
    x = torch.randn(B, res, res, C, generator=torch.Generator().manual_seed(res + ws + s))
    rows = M.swin_token_rows((res, res), (ws, ws), (s, s)).long()
    src = rows.repeat(B) + torch.arange(B).repeat_interleave(L) * L
    shifted = torch.roll(x, shifts=(-s, -s), dims=(1, 2)) if s else x
    assert torch.equal(x.reshape(-1, C)[src], M.window_partition(shifted, (ws, ws)).reshape(-1, C))
    out = torch.empty(B * L, C)
    out[src] = x.reshape(-1, C)[src]
    assert torch.equal(out, x.reshape(-1, C))


def test_block_carries_the_map_as_a_non_persistent_buffer():
    blk = M.SwinTransformerBlock(32, (14, 14), 2, window_size=7, shift_size=3)
    assert torch.equal(blk.token_rows, M.swin_token_rows((14, 14), (7, 7), (3, 3)))
    assert "token_rows" in dict(blk.named_buffers()) and "token_rows" not in blk.state_dict()
    whole = M.SwinTransformerBlock(32, (7, 7), 2, window_size=7, shift_size=3)      # window covers the map: no shift
    assert torch.equal(whole.token_rows, torch.arange(49, dtype=torch.int32))


@pytest.mark.parametrize("name", [k for k in M.MODEL_ZOO if k.startswith("swin")])
def test_state_dict_keys_of_zoo_swin_models_unchanged(monkeypatch, name):
    """The keys with the map equal those of the same model built without it (the reference's checkpoint layout)."""
    with_map = list(M.create_model(name, depth=1).state_dict().keys())
    init0 = M.SwinTransformerBlock.__init__

    def init_without_map(self, *a, **k):
        init0(self, *a, **k)
        del self._buffers["token_rows"]
    monkeypatch.setattr(M.SwinTransformerBlock, "__init__", init_without_map)
    without = M.create_model(name, depth=1)
    assert not any("token_rows" in n for n, _ in without.named_buffers())
    assert with_map == list(without.state_dict().keys())
