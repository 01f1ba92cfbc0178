"""Plain-torch reference of the report statistics (csrc/report.hip, adalog_amd/utils/report.py) -- TEST INFRASTRUCTURE ONLY.

The three statistics as torch expressions (fp64 sums; the uniform code in the fp32 op sequence x / s, round, + round(z) that the suite
already proves bit-exact against the fake-quant kernel) and ``recompute``: every number of quant_report from forward hooks, torch
reductions and torch.bincount, without going through adalog_amd/utils/report.py."""
import math

import torch


def _layout(n, n_channels, inner):
    n_channels = int(n_channels)
    inner = max(1, n // n_channels) if inner is None else int(inner)
    assert n % (n_channels * inner) == 0, (n, n_channels, inner)
    return n_channels, inner


def err_stats(a, b, n_channels=1, inner=None):
    """fp64 [n_channels, 4]: sum (a-b)^2, sum a^2, sum b^2, max |a-b| with channel(i) = (i // inner) % n_channels"""
    n_ch, inner = _layout(a.numel(), n_channels, inner)
    a64, b64 = a.detach().double().reshape(-1, n_ch, inner), b.detach().double().reshape(-1, n_ch, inner)
    d = a64 - b64
    out = torch.zeros(n_ch, 4, dtype=torch.float64, device=a.device)
    if a.numel():
        out[:, 0], out[:, 1], out[:, 2] = (d * d).sum((0, 2)), (a64 * a64).sum((0, 2)), (b64 * b64).sum((0, 2))
        out[:, 3] = d.abs().amax((0, 2))
    return out


def uniform_codes(x, scale, zp, n_channels=1, inner=None):
    """the code in front of the clamp, fp32: round(x / s) + round(z), as [rows, n_channels, inner]"""
    n_ch, inner = _layout(x.numel(), n_channels, inner)
    x3 = x.detach().float().reshape(-1, n_ch, inner)
    s, z = scale.detach().float().reshape(1, n_ch, 1), zp.detach().float().reshape(1, n_ch, 1)
    return torch.round(x3 / s) + torch.round(z)


def uniform_code_hist(x, scale, zp, n_bits, n_channels=1, inner=None):
    """int64 [n_channels, 2^b + 2]: codes 0 .. 2^b - 1, below, above"""
    levels = 2 ** int(n_bits)
    c = uniform_codes(x, scale, zp, n_channels, inner)
    n_ch = c.shape[1]
    idx = torch.where(c < 0, torch.full_like(c, levels), torch.where(c > levels - 1, torch.full_like(c, levels + 1), c)).long()
    idx = idx + torch.arange(n_ch, device=c.device).view(1, n_ch, 1) * (levels + 2)
    return torch.bincount(idx.reshape(-1), minlength=n_ch * (levels + 2)).view(n_ch, levels + 2)


def log_code_hist_from_bins(bins, n_bits):
    """int64 [2^b + 1] from the fake-quantiser's uint8 bins (255: the masked code -> the last entry)"""
    levels = 2 ** int(n_bits)
    b = bins.reshape(-1).long()
    return torch.bincount(torch.where(b == 255, torch.full_like(b, levels), b), minlength=levels + 1)


def sqnr_db(signal, noise):
    if noise == 0.0:
        return math.inf
    if signal == 0.0:
        return -math.inf
    return 10.0 * math.log10(signal / noise)


def entropy_bits(counts):
    total = sum(counts)
    return -sum((c / total) * math.log2(c / total) for c in counts if c)


# ------------------------------------------------------------------------------------------------ the whole report, from hooks
def _weight_view(m):
    w = m.weight.data
    if hasattr(m, "n_V"):
        return w.view(m.n_V, m.crb_rows, -1)
    return w.view(w.shape[0], -1) if w.dim() == 4 else w


def _quantiser_numbers(q, x):
    """(hist int64 list, err row fp64 [4]) of quantiser q over x, by torch.bincount and torch reductions; None where the report is null"""
    from adalog_amd.ops import broadcast_layout
    from adalog_amd.quantizers.logarithm import AdaLogQuantizer
    if q.n_bits == 32 or getattr(q, "training_mode", False) or not q.inited:
        return None
    x = x.detach().contiguous()
    if isinstance(q, AdaLogQuantizer):
        shift, sub = q._shift_args()
        hist = log_code_hist_from_bins(q.bins(x), q.n_bits)
        ref = x if (shift is None or sub) else x + shift.data
    else:
        if getattr(q, "sym", False):
            return None
        n_ch, inner = broadcast_layout(x.shape, q.scale.shape)
        if n_ch > 1 and inner < 64:
            return None
        hist = uniform_code_hist(x, q.scale.data, q.zero_point.data, q.n_bits, n_ch, inner).sum(0)
        ref = x
    return hist, err_stats(ref, q(x))[0]


def recompute(model, images):
    """{"modules": {name: {"cumulative": row, "local": row, "quantizers": {attr: (hist, row) | None}}}, "logits": {"batch": row,
    "per_image": rows}, "logits_quant": tensor}: the numbers of quant_report(model, images), all images at once, by forward hooks on
    the module route, torch reductions in fp64 and torch.bincount.  rows: fp64 (noise, signal, quant energy, max error)."""
    from torch import nn
    from adalog_amd.utils import models as M
    mods = [(n, m) for n, m in model.named_modules() if hasattr(m, "mode")]
    saved = (M.QF_FUSED, M.QF_ATTN_CORE, M.QF_LONG, [(m, m.mode) for _, m in mods])
    fp, rec = {}, {}
    try:
        M.QF_FUSED = M.QF_ATTN_CORE = M.QF_LONG = False
        with torch.no_grad():
            for _, m in mods:
                m.mode = "raw"
            hs = [m.register_forward_hook(lambda mod, a, out, n=n: fp.__setitem__(n, out.detach().clone())) for n, m in mods]
            y_fp = model(images)
            for h in hs:
                h.remove()
            for _, m in mods:
                m.mode = "quant_forward"
            hs = [m.register_forward_hook(lambda mod, a, out, n=n: rec.__setitem__(n, (tuple(t.detach().clone() for t in a[:2]),
                                                                                     out.detach().clone()))) for n, m in mods]
            y_q = model(images)
            for h in hs:
                h.remove()
            out = {"modules": {}, "logits_quant": y_q}
            for n, m in mods:
                args, y = rec[n]
                m.mode = "raw"
                raw = m(*args)
                m.mode = "quant_forward"
                e = {"cumulative": err_stats(fp[n], y)[0], "local": err_stats(raw, y)[0], "quantizers": {}}
                if hasattr(m, "w_quantizer"):
                    e["quantizers"]["w_quantizer"] = _quantiser_numbers(m.w_quantizer, _weight_view(m))
                if hasattr(m, "a_quantizer"):
                    skip = isinstance(m, nn.Conv2d) and m.a_quantizer.n_bits >= 8
                    e["quantizers"]["a_quantizer"] = None if skip else _quantiser_numbers(m.a_quantizer, args[0])
                if hasattr(m, "A_quantizer"):
                    e["quantizers"]["A_quantizer"] = _quantiser_numbers(m.A_quantizer, args[0])
                    e["quantizers"]["B_quantizer"] = _quantiser_numbers(m.B_quantizer, args[1])
                out["modules"][n] = e
            out["logits"] = {"batch": err_stats(y_fp, y_q)[0], "per_image": err_stats(y_fp, y_q, n_channels=y_fp.shape[0])}
    finally:
        M.QF_FUSED, M.QF_ATTN_CORE, M.QF_LONG = saved[:3]
        for m, mode in saved[3]:
            m.mode = mode
    return out
