"""QDrop (Wei et al., ICLR 2022) for the training form of the activation quantisers: the device-agnostic definition.

Inside a BRECQ iteration every element of an activation quantiser's output keeps its fake-quantised value with probability ``p``
and takes the quantiser's input otherwise; evaluation always quantises.  The mask comes from a counter-based generator, so no
mask is stored and the backward pass regenerates the mask of its forward:

    keep_e = u_e < p                           u_e = float(word >> 8) * 2^-24, compared in fp32 (p = 1 keeps all, p = 0 none)
    word   = output word e & 3 of Philox4x32-10 under key (seed_lo, seed_hi) at counter (e >> 2 low, e >> 2 high, iteration, stream)
    y_e    = keep_e ? fq(x_e) : x_e            (AdaLog with pre_gelu: GELU(x_e); shift variants: x_e itself)
    dy/dx  = keep_e ? straight-through factor : 1     (times GELU' when pre_gelu)
    dL/dscale, dL/dzero_point: sums over kept elements only

``e`` is the linear index in the quantiser's output in storage order, ``stream`` the quantiser's ordinal among its block's
activation quantisers, ``seed`` / ``iteration`` live in a small int32 device buffer {seed_lo, seed_hi, iteration} that the
reconstruction loop owns (utils/block_recon.py), so a captured HIP graph draws a new mask on every replay.

csrc/common.h holds the same generator for the HIP kernels (adalog_*_drop, include/adalog_hip.h).  The functions below are the
route of a backend without those kernels, composed from its undropped operations and ``torch.where``, and what the kernels are
tested against bit for bit.
"""
import torch

from .. import backend

_M0, _M1 = 0xD2511F53, 0xCD9E8D57              # Philox4x32 multipliers
_W0, _W1 = 0x9E3779B9, 0xBB67AE85              # Weyl increments of the key
_MASK32 = 0xFFFFFFFF


def _mulhilo(m: int, a):
    """(high, low) 32-bit words of m * a for a in [0, 2^32) held in int64: 16-bit limbs keep every intermediate below 2^49."""
    t = (a & 0xFFFF) * m
    u = (a >> 16) * m + (t >> 16)
    return u >> 16, ((u & 0xFFFF) << 16) | (t & 0xFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 (Salmon et al., SC'11) on int64 tensors (or ints) holding 32-bit words -> the four output words."""
    for _ in range(10):
        hi0, lo0 = _mulhilo(_M0, c0)
        hi1, lo1 = _mulhilo(_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _W0) & _MASK32, (k1 + _W1) & _MASK32
    return c0, c1, c2, c3


def _keep_mask(k0, k1, iteration, stream, n, p, device):
    blk = torch.arange((n + 3) // 4, dtype=torch.int64, device=device)
    zero = torch.zeros_like(blk)
    words = philox4x32_10(blk & _MASK32, blk >> 32, zero + iteration, zero + (int(stream) & _MASK32), k0, k1)
    u = (torch.stack(words, dim=1).reshape(-1)[:n] >> 8).to(torch.float32) * (2.0 ** -24)
    return u < torch.tensor(float(p), dtype=torch.float32, device=device)


def philox_keep_mask(seed: int, stream: int, iteration: int, n: int, p: float, device):
    """bool [n]: element e keeps its fake-quantised value.  ``seed``: 64-bit (key = its low and high word)."""
    return _keep_mask(int(seed) & _MASK32, (int(seed) >> 32) & _MASK32, int(iteration) & _MASK32, stream, n, p, device)


def keep_mask_from_state(buf, stream: int, n: int, p: float):
    """philox_keep_mask with seed and iteration read on the device from ``buf`` = int32 {seed_lo, seed_hi, iteration} (no host sync)."""
    s = buf.to(torch.int64) & _MASK32
    return _keep_mask(s[0], s[1], s[2], stream, n, p, buf.device)


def make_state(seed: int, iteration: int, device):
    """the device buffer {seed_lo, seed_hi, iteration} as int32"""
    words = [int(seed) & _MASK32, (int(seed) >> 32) & _MASK32, int(iteration) & _MASK32]
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32, device=device)


def storage_order(x, params):
    """-> (x contiguous in the order the quantiser runs over it, swapped): a transposed view of a contiguous tensor (k^T of an
    attention block) is quantised in its storage order when ``params`` do not vary along the last two dims (as _UniformSTE does)."""
    swap = (x.dim() >= 2 and not x.is_contiguous() and x.transpose(-1, -2).is_contiguous()
            and all(t is None or t.numel() == 1 or (t.dim() == x.dim() and t.shape[-1] == 1 and t.shape[-2] == 1) for t in params))
    if swap:
        x = x.transpose(-1, -2)
    return x.contiguous(), swap


# ------------------------------------------------------------------------------------------------ composed forms
def uniform_drop_forward(be, x, scale, zp, n_bits, sym, p, state):
    mask = keep_mask_from_state(state[0], state[1], x.numel(), p).view(x.shape)
    return torch.where(mask, be.uniform_fake_quant(x, scale, zp, n_bits, sym=sym), x)


def uniform_drop_backward(be, gy, x, scale, zp, n_bits, sym, want_gscale, want_gzp, p, state):
    """a dropped element enters the undropped backward with a zero gradient (it adds +-0 to the parameter sums) and takes gy itself"""
    mask = keep_mask_from_state(state[0], state[1], x.numel(), p).view(x.shape)
    gq, gs, gz = be.uniform_fake_quant_backward(torch.where(mask, gy, torch.zeros_like(gy)), x, scale, zp, n_bits, sym, want_gscale, want_gzp)
    return torch.where(mask, gq, gy), gs, gz


def _gelu_grad(x):
    """d GELU / dx (erf form): cdf + x * pdf"""
    cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440))
    return cdf + x * torch.exp(-0.5 * x * x) * 0.39894228040143267794


def log_drop_forward(be, x, scale, q, n_bits, shift, sub_shift, pre_gelu, p, state):
    mask = keep_mask_from_state(state[0], state[1], x.numel(), p).view(x.shape)
    kw = {"pre_gelu": True} if pre_gelu else {}
    fq = be.log_fake_quant(x, scale, q, None, None, n_bits, shift=shift, sub_shift=sub_shift, train_form=True, **kw)
    return torch.where(mask, fq, torch.nn.functional.gelu(x) if pre_gelu else x)


def log_drop_backward(be, gy, x, scale, q, n_bits, shift, sub_shift, pre_gelu, p, state):
    mask = keep_mask_from_state(state[0], state[1], x.numel(), p).view(x.shape)
    kw = {"pre_gelu": True} if pre_gelu else {}
    # (the backward's ``y`` argument, the saved output of the undropped node, is not read by any backend: x stands in for it)
    gq, gs = be.log_fake_quant_backward(torch.where(mask, gy, torch.zeros_like(gy)), x, x, scale, q, n_bits, shift, sub_shift, **kw)
    return torch.where(mask, gq, gy * _gelu_grad(x) if pre_gelu else gy), gs


# ------------------------------------------------------------------------------------------------ autograd nodes
def _native(be, name):
    """the HIP backend (adalog_amd.ops) always has the kernels; only a stand-in backend without them composes"""
    return hasattr(be, name)


def _uniform_native(be, x, scale):
    """... and the uniform drop kernels take per-tensor parameters and the [rows][inner] layout.  Parameters along the last dim
    (inner == 1: a channel-wise activation quantiser before its reparametrisation) compose too; their backward then ends where the
    undropped one does, in ops.uniform_fake_quant_backward, which has no training gradient for that layout."""
    if not _native(be, "uniform_fake_quant_drop"):
        return False
    n_ch, inner = be.broadcast_layout(x.shape, scale.shape)
    return not (inner == 1 and n_ch > 1)


class UniformDropSTE(torch.autograd.Function):
    """_UniformSTE with QDrop: the HIP kernels where the backend has them (adalog_uniform_fake_quant_drop_f32 /
    adalog_uniform_fq_backward_drop), the composed form above otherwise."""

    @staticmethod
    def forward(ctx, x, scale, zero_point, n_bits, sym, p, buf, stream):
        be = backend.get()
        zp = None if sym else zero_point
        x, ctx.swap = storage_order(x, (scale, zp))
        state = (buf, stream)
        ctx.native = _uniform_native(be, x, scale)
        if ctx.native:
            y = be.uniform_fake_quant_drop(x, scale, zp, n_bits, sym, p, state)
        else:
            y = uniform_drop_forward(be, x, scale, zp, n_bits, sym, p, state)
        ctx.save_for_backward(x, scale, zp)
        ctx.n_bits, ctx.sym, ctx.p, ctx.state = n_bits, sym, p, state
        return y.transpose(-1, -2) if ctx.swap else y

    @staticmethod
    def backward(ctx, gy):
        x, scale, zp = ctx.saved_tensors
        be = backend.get()
        if ctx.swap:
            gy = gy.transpose(-1, -2)
        gy = gy.contiguous()
        want = (ctx.needs_input_grad[1], ctx.needs_input_grad[2] and zp is not None)
        if ctx.native:
            gx, gs, gz = be.uniform_fake_quant_backward_drop(gy, x, scale, zp, ctx.n_bits, ctx.sym, want[0], want[1], ctx.p, ctx.state)
        else:
            gx, gs, gz = uniform_drop_backward(be, gy, x, scale, zp, ctx.n_bits, ctx.sym, want[0], want[1], ctx.p, ctx.state)
        return (gx.transpose(-1, -2) if ctx.swap else gx), gs, gz, None, None, None, None, None


class AdaLogDropSTE(torch.autograd.Function):
    """_AdaLogSTE with QDrop (adalog_log_fake_quant_drop_f32 / adalog_log_fq_backward_drop, or the composed form)."""

    @staticmethod
    def forward(ctx, x, scale, q, n_bits, shift, sub_shift, pre_gelu, p, buf, stream):
        be = backend.get()
        x = x.contiguous()
        state = (buf, stream)
        if _native(be, "log_fake_quant_drop"):
            y = be.log_fake_quant_drop(x, scale, q, n_bits, shift, sub_shift, pre_gelu, p, state)
        else:
            y = log_drop_forward(be, x, scale, q, n_bits, shift, sub_shift, pre_gelu, p, state)
        ctx.save_for_backward(x, scale, q, shift)
        ctx.n_bits, ctx.sub_shift, ctx.pre_gelu, ctx.p, ctx.state = n_bits, sub_shift, bool(pre_gelu), p, state
        return y

    @staticmethod
    def backward(ctx, gy):
        x, scale, q, shift = ctx.saved_tensors
        be = backend.get()
        gy = gy.contiguous()
        if _native(be, "log_fake_quant_backward_drop"):
            gx, gs = be.log_fake_quant_backward_drop(gy, x, scale, q, ctx.n_bits, shift, ctx.sub_shift, ctx.pre_gelu, ctx.p, ctx.state)
        else:
            gx, gs = log_drop_backward(be, gy, x, scale, q, ctx.n_bits, shift, ctx.sub_shift, ctx.pre_gelu, ctx.p, ctx.state)
        return gx, gs, None, None, None, None, None, None, None, None


def active(quantizer):
    """the quantiser takes the drop route in this forward"""
    return (quantizer.training_mode and torch.is_grad_enabled() and quantizer.drop_prob < 1.0
            and getattr(quantizer, "drop_state", None) is not None)


def activation_quantizers(block):
    """A block's activation quantisers in named_modules() order: their position is their Philox stream."""
    return [m for name, m in block.named_modules()
            if name.split('.')[-1] in ("a_quantizer", "A_quantizer", "B_quantizer") and hasattr(m, "drop_prob")]
