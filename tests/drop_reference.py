"""An independent Philox4x32-10 in numpy (uint64 arithmetic) and the QDrop keep mask built on it: what
adalog_amd/quantizers/_drop.py (torch integer ops) and the HIP kernels (csrc/common.h) are held against, bit for bit.

Known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 with 10 rounds):
    counter 0 0 0 0, key 0 0                        -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
    counter ffffffff x 4, key ffffffff x 2          -> 408f276d 41c83b0e a20bc7c6 6d5451fd
    counter 243f6a88 85a308d3 13198a2e 03707344, key a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
"""
import numpy as np

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (or ints) holding 32-bit words, key: two ints -> four uint64 arrays of 32-bit words"""
    c = [np.asarray(v, dtype=np.uint64) for v in ctr]
    k0, k1 = int(key[0]), int(key[1])
    lo32 = np.uint64(0xFFFFFFFF)
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        p0 = np.uint64(0xD2511F53) * c[0]                    # < 2^64: exact in uint64
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo32]
    return c


def keep_mask(seed, stream, iteration, n, p):
    """bool [n]: u_e < p with u_e = float32(word >> 8) * 2^-24, word e & 3 of the block at counter (e >> 2, iteration, stream)"""
    blk = np.arange((n + 3) // 4, dtype=np.uint64)
    full = np.zeros_like(blk)
    w = philox4x32_10((blk & np.uint64(0xFFFFFFFF), blk >> np.uint64(32), full + np.uint64(iteration & 0xFFFFFFFF),
                       full + np.uint64(stream & 0xFFFFFFFF)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    words = np.stack(w, axis=1).reshape(-1)[:n]
    u = (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u < np.float32(p)


def traj_block(g, device):
    """The toy block of tests/golden/brecq_traj.npz (the reference's own 20-iteration run: a uniform + AdaLog MLP and two attention
    products), calibrated state loaded, with its stored inputs / targets -> (block, per-iteration mini-batch indices)."""
    import torch
    from adalog_amd import quant_layers as Q
    I, Hd, H = 16, 32, 2

    def t(a):
        return torch.from_numpy(np.asarray(a)).to(device)

    class Blk(torch.nn.Module):
        def __init__(self):
            super().__init__()
            kw = dict(mode="raw", w_bit=4, a_bit=4, calib_batch_size=4, search_round=1, eq_n=128, fpcs=True, steps=2)
            self.fc1 = Q.AsymmetricallyBatchingQuantLinear(I, Hd, True, n_V=1, **kw)
            self.fc2 = Q.PostGeluLogBasedBatchingQuantLinear(Hd, I, True, n_V=1, quantizer="adalog", **kw)
            mk = dict(B_bit=4, mode="raw", calib_batch_size=4, search_round=1, eq_n=128, head_channel_wise=True, num_heads=H, fpcs=True,
                      steps=2)
            self.matmul1 = Q.AsymmetricallyBatchingQuantMatMul(A_bit=4, **mk)
            self.matmul2 = Q.PostSoftmaxAsymmetricallyBatchingQuantMatMul(A_bit=4, quantizer="adalog", **mk)

        def forward(self, x):
            B, N, C = x.shape
            h = x.reshape(B, N, H, C // H).permute(0, 2, 1, 3)
            a = self.matmul2(self.matmul1(h, h.transpose(-2, -1)).softmax(-1), h)
            x = x + a.permute(0, 2, 1, 3).reshape(B, N, C)
            return x + self.fc2(torch.nn.functional.gelu(self.fc1(x)))

    blk = Blk().eval().to(device)
    res = blk.load_state_dict({k[4:].replace("__", "."): t(v) for k, v in g.items() if k.startswith("cal_")}, strict=False)
    assert not res.unexpected_keys and not res.missing_keys, res
    for m in blk.modules():
        if hasattr(m, "mode"):
            m.calibrated = True
            for a in ("a_quantizer", "w_quantizer", "A_quantizer", "B_quantizer"):
                if hasattr(m, a):
                    getattr(m, a).inited = True
    blk.raw_input, blk.raw_out = t(g["x"]).clone(), t(g["tgt"]).clone()
    return blk, torch.from_numpy(g["perms"])


def trained_tensors(blk):
    out = {}
    for name, m in blk.named_modules():
        wq = getattr(m, "w_quantizer", None)
        if wq is not None and hasattr(wq, "alpha"):
            out[name + ".alpha"] = wq.alpha.detach().clone()
        for a in ("a_quantizer", "A_quantizer", "B_quantizer"):
            if hasattr(m, a):
                out[f"{name}.{a}.scale"] = getattr(m, a).scale.detach().clone()
    return out
