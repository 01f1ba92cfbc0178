"""fp64 restatement of quant_forward -- TEST INFRASTRUCTURE (tests/ only; no HIP op is called here).

Built from the oracle's quantiser definitions (oracle/adalog_oracle.py: uniform.py:25-36, logarithm.py:83-99, 127-135) and plain
torch.float64 arithmetic, on whatever device the inputs live on.  Three layers:

  * products -- ``gemm_out`` / ``gemm_out_gen`` semantics: out[g] = (A[g] . B[g]^T) * sa[g % gmod] * sa_mul * sb[g % gmod][n]
    + bias[n] (+ addend[g]), A or B broadcast from a single image, optionally stored heads-last [B, M, H, N];
  * the quant_forward of the six layer classes, from a layer's parameters;
  * a ViT block split into stages, each fed its recorded fp32 input (teacher forcing): qkv; attention core (split, q / k / v
    quantisers, q . k^T, * scale, softmax, post-softmax AdaLog, . v); proj + residual; fc1; GELU -> shifted AdaLog -> fc2 +
    residual;
  * a Swin block the same way: norm1 -> shifted-window row map -> qkv; window core (q * scale in fp32 BEFORE the q quantiser, scores +
    relative-position bias + shift mask by window mod nW, softmax, AdaLog, . v); proj -> row map back + residual; fc1; fc2 -- and
    PatchMerging's 2 x 2 regroup.  The row map and the shift mask are restated from coordinates, not from roll / reshape.

Uniform bins use the oracle's fp32 op sequence (rne(x / s) + rne(z), clamp, - rne(z)), which the kernels reproduce bit for bit;
every product and sum is fp64.  Softmax and GELU are fp64 here, so an AdaLog bin may legitimately differ from the kernel's where
the fp32 log-domain value lies within a few ulps (delta, ~1e-5 of a bin) of a rounding boundary: those elements are marked
ambiguous and each output element gets an allowance  tight bar + sum_ambiguous |dvalue| * |operand| * scales  (one extra product),
returned with the ambiguous fraction so a test can assert that the allowance is not vacuous.

Bars (per element, never max-over-tensor):
  int8 products:  |got - ref| <= 2^-22 (|acc sa sb| + |bias| + |addend|)           (the int32 sums are exact)
  bf16 products:  |got - ref| <= (K + 4) 2^-24 sum_k |a_k b_k| |sa sb| + 2^-23 (|bias| + |addend|)
(AdaLog values m * 2^-t and integer codes are both exact in bf16.)
"""
import math

import torch

from oracle import adalog_oracle as O

F64 = torch.float64
U22, U23, U24 = 2.0 ** -22, 2.0 ** -23, 2.0 ** -24
R37 = 37.0


def f32(v):
    """A Python / tensor scalar as the fp32 value a kernel receives."""
    return float(torch.tensor(float(v), dtype=torch.float32))


# ============================================================================================================ quantiser codes
def uniform_codes(x, scale, zero_point, n_bits):
    """Integer codes q - rne(z) of the asymmetric uniform quantiser (uniform.py:25-36), fp32 op sequence, returned as fp64.
    scale / zero_point broadcast against x."""
    x = x.float()
    s, z = scale.float(), zero_point.float()
    _, q = O.uniform_fake_quant(x, s, z, n_bits)
    return (q - torch.round(z)).to(F64)


def sym_codes(x, scale, n_bits):
    _, q = O.uniform_fake_quant(x.float(), scale.float(), None, n_bits, sym=True)
    return q.to(F64)


def adalog_numerators(q: int, n_bits: int, table_scale):
    """Integer numerators of the AdaLog mantissa table (linear.py:750-752 / matmul.py:299-302): round(2^(-j/37) / ts), j < 37."""
    table = torch.tensor([2 ** (-j / R37) for j in range(120)])
    ts = table_scale
    return torch.round(torch.round(table / ts) * ts / ts)[:37].to(F64)


def adalog_value(k, q: int, n_bits: int, mant):
    """Value / table_scale of AdaLog bin k (logarithm.py:94-99): mant[(k q) mod 37] * 2^-floor(k q / 37), 0 for masked bins
    (k >= 2^bits) and below 2^-100 -- exactly the bf16 operand the packers write."""
    k = k.long()
    kq = k.clamp(min=0) * int(q)
    t, j = kq // 37, kq % 37
    v = mant.to(k.device)[j] * torch.pow(torch.tensor(2.0, dtype=F64, device=k.device), -t.to(F64))
    return torch.where((k >= 2 ** n_bits) | (t > 100), torch.zeros_like(v), v)


def adalog_codes(u_log2, q: int, n_bits: int, mant, delta):
    """AdaLog of u = x / s given log2(clamp(u, 1e-15, 1)) in fp64 and a per-element uncertainty ``delta`` (in bins) of the kernel's
    fp32 log-domain value v = -log2(u) * 37 / q.  -> (value / ts [fp64], |dvalue| over the ambiguous bins [fp64], ambiguous mask)."""
    v = -u_log2 * (R37 / q)
    k = torch.round(v)
    k_lo, k_hi = torch.round(v - delta), torch.round(v + delta)
    val = adalog_value(k, q, n_bits, mant)
    amb = k_lo != k_hi
    d = torch.maximum((adalog_value(k_lo, q, n_bits, mant) - val).abs(), (adalog_value(k_hi, q, n_bits, mant) - val).abs())
    return val, torch.where(amb, d, torch.zeros_like(d)), amb


def log_domain_delta(u_log2, q: int, rel_err_u):
    """Uncertainty (in bins) of the kernel's fp32 v = -log2(u) * 37 / q: a relative error ``rel_err_u`` of the fp32 quotient u
    plus a few ulps of the log2 and of the scaling."""
    return (R37 / q) * (rel_err_u / math.log(2.0) + 4 * U24 * u_log2.abs() + 4 * U24)


def _log2_clamped(u):
    return u.clamp(min=1e-15, max=1.0).log2()


# ============================================================================================================ products
def per_group(t, G, gmod, device):
    """Per-group scalar parameters: [gmod] (or [1]) -> [G, 1, 1] fp64 by g % gmod."""
    t = t.reshape(-1).to(device=device, dtype=F64)
    if t.numel() == 1:
        return t.view(1, 1, 1).expand(G, 1, 1)
    return t[torch.arange(G, device=device) % gmod].view(G, 1, 1)


def product(A, B, sa, sb, bias=None, addend=None, sa_mul=1.0, gmod=1, heads_last=0, k_valid=None, kind="i8", amb_A=None,
            sb_cols=False):
    """Spec of gemm_out / gemm_out_gen.  A: [GA, M, K] codes or AdaLog values (GA = G, or 1 = broadcast), B: [GB, N, K].
    sa: per-group [gmod] / [1]; sb: per-group [gmod] / [1], or per-column [N] with ``sb_cols``; bias: [N] or None;
    addend: [G, M, N] or None.
    amb_A: |dvalue| of A's ambiguous elements ([GA, M, K]) -> adds the flip allowance.
    -> (ref fp64, bar fp64), in [G, M, N], or [G // H, M, H, N] when heads_last = H."""
    dev = A.device
    K = A.shape[-1] if k_valid is None else k_valid
    A, B = A[..., :K].to(F64), B[..., :K].to(F64)
    G = max(A.shape[0], B.shape[0])
    Ae, Be = A.expand(G, -1, -1), B.expand(G, -1, -1)
    acc = torch.bmm(Ae, Be.transpose(1, 2))
    sa_ = per_group(sa, G, gmod, dev) * f32(sa_mul)
    N = B.shape[1]
    sb_ = sb.reshape(1, 1, N).to(device=dev, dtype=F64) if sb_cols else per_group(sb, G, gmod, dev)
    alpha = sa_ * sb_
    ref = acc * alpha
    mag = torch.zeros_like(ref)
    if bias is not None:
        b = bias.detach().reshape(1, 1, -1).to(device=dev, dtype=F64)
        ref = ref + b
        mag = mag + b.abs()
    if addend is not None:
        a = addend.detach().reshape(G, -1, N).to(device=dev, dtype=F64)
        ref = ref + a
        mag = mag + a.abs()
    if kind == "i8":                                       # (any other kind: the bf16 form, which also bounds an fp32 product)
        bar = U22 * ((acc * alpha).abs() + mag)
    else:
        absacc = torch.bmm(Ae.abs(), Be.abs().transpose(1, 2))
        bar = (K + 4) * U24 * absacc * alpha.abs() + U23 * mag
    if amb_A is not None:
        bar = bar + torch.bmm(amb_A[..., :K].to(F64).expand(G, -1, -1), Be.abs().transpose(1, 2)) * alpha.abs()
    if heads_last:
        H = int(heads_last)
        ref = ref.view(G // H, H, *ref.shape[1:]).transpose(1, 2)
        bar = bar.view(G // H, H, *bar.shape[1:]).transpose(1, 2)
    return ref, bar


def check(got, ref, bar, what=""):
    """Per-element |got - ref| <= bar; -> the largest |got - ref| / bar (reported by the tests)."""
    got = got.detach().to(F64)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    ratio = err / bar.clamp_min(1e-300)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not bool((err <= bar).all()):
        i = int(torch.argmax(ratio))
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError(f"{what}: {int((err > bar).sum())} of {err.numel()} elements outside the bar; worst at {idx}: "
                             f"got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} bar {float(bar.flatten()[i])!r}")
    return worst


# ============================================================================================================ layer classes
def _wq(lay):
    """Weight codes [O, I] and per-output-row scales [O] of a per-channel asymmetric weight quantiser (n_V rows blocks)."""
    wq = lay.w_quantizer
    O_, I_ = lay.weight.shape[0], lay.weight.reshape(lay.weight.shape[0], -1).shape[1]
    s = wq.scale.data.reshape(-1)
    z = wq.zero_point.data.reshape(-1)
    cw = uniform_codes(lay.weight.data.reshape(O_, I_), s.view(O_, 1), z.view(O_, 1), wq.n_bits)
    return cw, s


def linear_qf(lay, x, addend=None, kind="i8"):
    """AsymmetricallyBatchingQuantLinear / ...ChannelWise... quant_forward (linear.py:46-51): per-tensor or per-channel
    activation quantiser, per-row weight quantiser.  -> (ref, bar) in x's leading shape.  kind="f32": the bar of an fp32
    composition (fake-quantise, then an fp32 product: the bf16 form of the bar) instead of the int8 product's."""
    aq = lay.a_quantizer
    lead = x.shape[:-1]
    x2 = x.reshape(1, -1, x.shape[-1])
    cw, sw = _wq(lay)
    add = None if addend is None else addend.reshape(1, -1, lay.out_features)
    if aq.scale.numel() == 1:
        cx = uniform_codes(x2, aq.scale.data.reshape(-1), aq.zero_point.data.reshape(-1), aq.n_bits)
        ref, bar = product(cx, cw.unsqueeze(0), aq.scale.data, sw, lay.bias, add, kind=kind, sb_cols=True)
    else:                                                  # per-channel activation: dequantise A, fp64 product, fp32-sized bar
        s, z = aq.scale.data.reshape(1, 1, -1), aq.zero_point.data.reshape(1, 1, -1)
        xa = uniform_codes(x2, s, z, aq.n_bits) * s.to(F64)
        ref, bar = product(xa, cw.unsqueeze(0), torch.ones(1), sw, lay.bias, add, kind="bf16", sb_cols=True)
    return ref.view(*lead, -1), bar.view(*lead, -1)


def gelu64(x):
    x = x.to(F64)
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def postgelu_qf(lay, x, pre_gelu=False, addend=None):
    """PostGeluLogBasedBatchingQuantLinear quant_forward (linear.py:46-51 with ShiftAdaLogQuantizer, logarithm.py:127-135): the input
    is x (``pre_gelu``: GELU(x), erf form, here in fp64), u = (input + shift) / scale; both bias states (bias_reparamed: the shift
    was folded into the bias, else the product subtracts it).  -> (ref, bar, ambiguous fraction)."""
    aq = lay.a_quantizer
    lead = x.shape[:-1]
    q = int(aq.q.reshape(-1)[0])
    n_bits = aq.n_bits
    ts = lay.table_scale
    mant = adalog_numerators(q, n_bits, ts).to(x.device)
    x2 = x.reshape(1, -1, x.shape[-1])
    shift = aq.shift.data.reshape(-1)[0].to(F64)
    scale = aq.scale.data.reshape(-1)[0].to(F64)
    g = gelu64(x2) if pre_gelu else x2.to(F64)
    xs = g + shift
    u = xs / scale
    l2 = _log2_clamped(u)
    # fp32 error of the kernel's (GELU(x) +) shift and of the division, relative to u
    eps_abs = 8 * U24 * (x2.to(F64).abs() + shift.abs()) if pre_gelu else 2 * U24 * (x2.to(F64).abs() + shift.abs())
    rel = eps_abs / xs.abs().clamp_min(1e-300) + 2 * U24
    val, dval, amb = adalog_codes(l2, q, n_bits, mant, log_domain_delta(l2, q, rel))
    cw, sw = _wq(lay)
    reparamed = bool(aq.bias_reparamed)
    bias = lay.bias.data.to(F64) if lay.bias is not None else torch.zeros(lay.out_features, dtype=F64, device=x.device)
    fold_mag = torch.zeros_like(bias)
    if not reparamed:                                      # y = q(x) - shift: the -shift . W_q term (reparam_bias, linear.py:999-1006)
        fold = shift * sw.to(F64) * cw.sum(1)
        fold_mag = fold.abs() + bias.abs()
        bias = bias - fold
    add = None if addend is None else addend.reshape(1, -1, lay.out_features)
    ref, bar = product(val, cw.unsqueeze(0), aq.scale.data, sw, bias, add, sa_mul=f32(ts), kind="bf16", amb_A=dval,
                       sb_cols=True)
    bar = bar + U22 * fold_mag.view(1, 1, -1)              # the fold is computed in fp32 (shift_fold)
    return ref.view(*lead, -1), bar.view(*lead, -1), float(amb.double().mean())


def matmul_qf(lay, A, B, kind="i8"):
    """AsymmetricallyBatchingQuantMatMul quant_forward (matmul.py:43-45): A [.., S, K], B [.., K, S'], per-head or per-tensor.
    kind as in linear_qf."""
    H = lay._heads()
    lead = A.shape[:-2]
    a3 = A.reshape(-1, A.shape[-2], A.shape[-1])
    bt3 = B.transpose(-2, -1).reshape(-1, B.shape[-1], B.shape[-2])
    G = a3.shape[0]
    sA, zA = lay.A_quantizer.scale.data.reshape(-1), lay.A_quantizer.zero_point.data.reshape(-1)
    sB, zB = lay.B_quantizer.scale.data.reshape(-1), lay.B_quantizer.zero_point.data.reshape(-1)
    ca = uniform_codes(a3, per_group(sA, G, H, A.device).float(), per_group(zA, G, H, A.device).float(), lay.A_quantizer.n_bits)
    cb = uniform_codes(bt3, per_group(sB, G, H, A.device).float(), per_group(zB, G, H, A.device).float(), lay.B_quantizer.n_bits)
    ref, bar = product(ca, cb, sA, sB, gmod=H, kind=kind)
    return ref.view(*lead, *ref.shape[1:]), bar.view(*lead, *bar.shape[1:])


def softmax_adalog(p, q, n_bits, ts, a_scale=1.0, rel_err=None):
    """Post-softmax AdaLog (logarithm.py:83-99) of probabilities p (fp64) -> (value / ts, |dvalue| on ambiguous, ambiguous mask).
    rel_err: relative uncertainty of the kernel's fp32 u (default: a few ulps)."""
    mant = adalog_numerators(q, n_bits, ts).to(p.device)
    u = p.to(F64) / float(a_scale)
    l2 = _log2_clamped(u)
    rel = 8 * U24 if rel_err is None else rel_err
    return adalog_codes(l2, q, n_bits, mant, log_domain_delta(l2, q, rel))


def postsoftmax_qf(lay, A, B):
    """PostSoftmaxAsymmetricallyBatchingQuantMatMul quant_forward: A (probabilities, fp32) through AdaLog, B uniform.
    -> (ref, bar, ambiguous fraction)."""
    H = lay._heads()
    lead = A.shape[:-2]
    a3 = A.reshape(-1, A.shape[-2], A.shape[-1])
    bt3 = B.transpose(-2, -1).reshape(-1, B.shape[-1], B.shape[-2])
    G = a3.shape[0]
    q = int(lay.A_quantizer.q.reshape(-1)[0])
    a_s = float(lay.A_quantizer.scale.data.reshape(-1)[0])
    val, dval, amb = softmax_adalog(a3, q, lay.A_quantizer.n_bits, lay.table_scale, a_s)
    sB, zB = lay.B_quantizer.scale.data.reshape(-1), lay.B_quantizer.zero_point.data.reshape(-1)
    cb = uniform_codes(bt3, per_group(sB, G, H, A.device).float(), per_group(zB, G, H, A.device).float(), lay.B_quantizer.n_bits)
    ref, bar = product(val, cb, lay.A_quantizer.scale.data, sB, sa_mul=f32(lay.table_scale), gmod=H, kind="bf16", amb_A=dval)
    return ref.view(*lead, *ref.shape[1:]), bar.view(*lead, *bar.shape[1:]), float(amb.double().mean())


def conv_qf(lay, x):
    """AsymmetricallyBatchingQuantConv2d quant_forward (conv.py:55-65): the input through the symmetric per-tensor quantiser below
    8 bits, left in fp32 from 8 bits on; per-output-channel asymmetric weight codes; fp64 convolution.  -> (ref, bar)."""
    aq = lay.a_quantizer
    if aq.n_bits >= 8:
        xa, sa = x.to(F64), torch.ones((), dtype=F64, device=x.device)
    else:
        xa, sa = sym_codes(x, aq.scale.data, aq.n_bits), aq.scale.data.reshape(-1)[0].to(F64)
    cw, sw = _wq(lay)
    w = cw.view(lay.weight.shape)
    acc = torch.nn.functional.conv2d(xa, w, None, lay.stride)
    absacc = torch.nn.functional.conv2d(xa.abs(), w.abs(), None, lay.stride)
    alpha = sa * sw.to(F64).view(1, -1, 1, 1)
    b = torch.zeros_like(alpha) if lay.bias is None else lay.bias.data.to(F64).view(1, -1, 1, 1)
    K = w[0].numel()
    return acc * alpha + b, (K + 4) * U24 * absacc * alpha.abs() + U23 * b.abs()


# ============================================================================================================ ViT block stages
def _qkv_codes(qkv, m1, m2, H, q_mul=None):
    """Split of a recorded qkv output [B, N, 3 C] and the codes of the q / k / v input quantisers, [B H, N, D] each; ``q_mul``: q is
    multiplied by it in fp32 (one multiply, as the module route does) BEFORE its quantiser.  -> (cq, ck, cv, sq, sk, sv, hm)."""
    B_, N, C3 = qkv.shape
    D = C3 // 3 // H
    hm = m1._heads()
    t = qkv.reshape(B_, N, 3, H, D).permute(2, 0, 3, 1, 4)          # [3, B, H, N, D]
    G = B_ * H

    def codes(x, quant):
        s, z = quant.scale.data.reshape(-1), quant.zero_point.data.reshape(-1)
        return uniform_codes(x.reshape(G, N, D), per_group(s, G, hm, qkv.device).float(), per_group(z, G, hm, qkv.device).float(),
                             quant.n_bits), s

    q = t[0].float() if q_mul is None else t[0].float() * q_mul
    cq, sq = codes(q, m1.A_quantizer)
    ck, sk = codes(t[1], m1.B_quantizer)
    cv, sv = codes(t[2], m2.B_quantizer)
    return cq, ck, cv, sq, sk, sv, hm


def _qk_scores(cq, ck, sq, sk, hm, mul=1.0):
    """fp64 q . k^T * scales * mul and the bound of an fp32 score's error: <= 2^-22 |s| from the int8 product, <= (D + 4) 2^-24
    sum |q k| |scales| from a composed (fp32) one."""
    G, _, D = cq.shape
    acc = torch.bmm(cq, ck.transpose(1, 2))
    alpha = per_group(sq, G, hm, cq.device) * per_group(sk, G, hm, cq.device)
    s = acc * alpha * f32(mul)
    s_err = torch.maximum(U22 * s.abs(), (D + 4) * U24 * torch.bmm(cq.abs(), ck.abs().transpose(1, 2)) * alpha * abs(f32(mul)))
    return s, s_err


def _softmax_adalog_v(p, rel, cv, sv, m2, hm, H):
    """Post-softmax AdaLog of the fp64 probabilities p [B H, N, N] (``rel``: relative uncertainty of the kernel's fp32 p), then . v,
    heads merged -> (ref [B, N, C], bar, ambiguous fraction)."""
    G, N, _ = p.shape
    q = int(m2.A_quantizer.q.reshape(-1)[0])
    a_s = float(m2.A_quantizer.scale.data.reshape(-1)[0])
    val, dval, amb = softmax_adalog(p, q, m2.A_quantizer.n_bits, m2.table_scale, a_s, rel_err=rel)
    ref, bar = product(val, cv.transpose(1, 2), m2.A_quantizer.scale.data, sv, sa_mul=f32(m2.table_scale), gmod=hm,
                       heads_last=H, kind="bf16", amb_A=dval)
    return ref.reshape(G // H, N, -1), bar.reshape(G // H, N, -1), float(amb.double().mean())


def attention_core(qkv, m1, m2, H, mul):
    """Attention core of a block from the qkv projection's recorded fp32 output [B, N, 3 C]: split, q / k / v input quantisers,
    q . k^T (fp64), * mul, softmax (fp64), post-softmax AdaLog, . v; merged heads -> (ref [B, N, C], bar, ambiguous fraction)."""
    cq, ck, cv, sq, sk, sv, hm = _qkv_codes(qkv, m1, m2, H)
    s, s_err = _qk_scores(cq, ck, sq, sk, hm, mul)
    p = torch.softmax(s, -1)
    # the softmax adds a few ulps to the scores' error: relative error of u per row
    rel = 2 * s_err.amax(-1, keepdim=True) + 16 * U24
    return _softmax_adalog_v(p, rel, cv, sv, m2, hm, H)


def block_stages(block, x):
    """All stages of a wrapped ViT block chained in fp64-reference form from the block input x (the CPU tests' composition): each
    stage takes the previous stage's fp64 reference rounded to fp32, as a recorded input would be.  -> dict of references."""
    out = {}
    h1 = block.norm1(x)
    attn = block.attn
    out["qkv"] = linear_qf(attn.qkv, h1)[0]
    core, _, out["amb_core"] = attention_core(out["qkv"].float(), attn.matmul1, attn.matmul2, attn.num_heads, attn.scale)
    out["core"] = core
    out["attn"] = linear_qf(attn.proj, core.float(), addend=x)[0]
    x1 = out["attn"].float()
    h2 = block.norm2(x1)
    out["fc1"] = linear_qf(block.mlp.fc1, h2)[0]
    out["mlp"], _, out["amb_fc2"] = postgelu_qf(block.mlp.fc2, out["fc1"].float(), pre_gelu=True, addend=x1)
    return out


# ============================================================================================================ Swin block stages
def swin_window_rows(res, ws, shift):
    """The token of an image [H, W] held by row r = (window, i, j) of its shifted windows, from coordinates alone (no roll, no
    reshape): window (wy, wx), position (i, j) reads token ((wy ws + i + shift) mod H, (wx ws + j + shift) mod W).  -> long [H W]"""
    (H, W), (wh, ww), (sh, sw) = res, ws, shift
    wy, wx, i, j = torch.meshgrid(torch.arange(H // wh), torch.arange(W // ww), torch.arange(wh), torch.arange(ww), indexing="ij")
    return (((wy * wh + i + sh) % H) * W + (wx * ww + j + sw) % W).reshape(-1)


def swin_shift_mask(res, ws, shift):
    """The shift mask [nW, N, N] from coordinates alone: in the rolled frame a position p of an axis of length L lies in region
    0 (p < L - ws), 1 (p < L - shift) or 2; tokens of different (row region, column region) do not see each other (-100)."""
    (H, W), (wh, ww), (sh, sw) = res, ws, shift
    if not (sh or sw):
        return None

    def region(p, L, w, s):
        return (p >= L - w).long() + (p >= L - s).long()
    wy, wx, i, j = torch.meshgrid(torch.arange(H // wh), torch.arange(W // ww), torch.arange(wh), torch.arange(ww), indexing="ij")
    lab = (3 * region(wy * wh + i, H, wh, sh) + region(wx * ww + j, W, ww, sw)).reshape(-1, wh * ww)
    return torch.where(lab[:, :, None] == lab[:, None, :], 0.0, -100.0)


def patch_merging_rows(x):
    """The 2 x 2 regroup in front of PatchMerging's norm: [B, H, W, C] -> [B, H / 2, W / 2, 4 C], channels in the order (row, column)
    parity (0, 0), (1, 0), (0, 1), (1, 1)."""
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)


def window_scores(qkv, m1, m2, H, q_mul):
    """q . k^T of the window attention as the int8 product gives it (before bias and mask) -> (ref [Bw H, N, N], bar)"""
    cq, ck, _, sq, sk, _, hm = _qkv_codes(qkv, m1, m2, H, q_mul=q_mul)
    return product(cq, ck, sq, sk, gmod=hm)


def window_core(qkv, m1, m2, H, table, index, mask, q_mul=None, s_mul=1.0):
    """Core of a window attention (wrap_net.py:35-52) from the recorded fp32 qkv output [Bw, N, 3 C] in window order: split,
    q * q_mul in fp32, q / k / v quantisers, fp64 scores  acc sa sb s_mul + table[index[i, j], h] + mask[window mod nW, i, j],
    softmax, post-softmax AdaLog, . v -> (ref [Bw, N, C], bar, ambiguous fraction).  (Swin: q_mul = scale, s_mul = 1.)

    The kernels form the score in fp32 and add bias and mask in fp32, one rounding each: on top of the product's error an absolute
    error <= 2^-24 (|s + bias| + |s + bias + mask|) <= 2^-23 (|s| + |bias| + |mask|) per score.  exp(s_j - max) takes one more rounding
    of the difference, 2^-24 |s_j - max| (up to 100 for a masked key), and a few ulps.  The relative error of a probability is its
    own score's error plus that of the row's normaliser, which is at most the largest error among the keys that carry the sum: keys
    with p <= 1e-12 are left out of that maximum, or the -100 entries would inflate every row's flip allowance."""
    Bw, N, _ = qkv.shape
    cq, ck, cv, sq, sk, sv, hm = _qkv_codes(qkv, m1, m2, H, q_mul=q_mul)
    s0, s_err = _qk_scores(cq, ck, sq, sk, hm, s_mul)
    bias = table.detach().to(F64)[index.reshape(-1).long()].view(N, N, H).permute(2, 0, 1)           # [H, N, N]
    add = bias.unsqueeze(0).expand(Bw, H, N, N)
    mag = s0.abs().view(Bw, H, N, N) + bias.abs().unsqueeze(0)
    if mask is not None:
        m = mask.detach().to(F64)[torch.arange(Bw, device=qkv.device) % mask.shape[0]].unsqueeze(1)  # [Bw, 1, N, N]
        add = add + m
        mag = mag + m.abs()
    s = s0 + add.reshape(Bw * H, N, N)
    s_err = s_err + U23 * mag.reshape(Bw * H, N, N)
    p = torch.softmax(s, -1)
    carried = torch.where(p > 1e-12, s_err, torch.zeros_like(s_err)).amax(-1, keepdim=True)
    rel = s_err + carried + 2 * U24 * (s - s.amax(-1, keepdim=True)).abs() + 16 * U24
    return _softmax_adalog_v(p, rel, cv, sv, m2, hm, H)


def window_attention_core(qkv, attn, mask):
    """window_core with a (wrapped) WindowAttention's parameters; ``mask``: the block's attn_mask, None for an unshifted block."""
    return window_core(qkv, attn.matmul1, attn.matmul2, attn.num_heads, attn.relative_position_bias_table.data,
                       attn.relative_position_index, mask, q_mul=attn.scale)


def swin_block_stages(block, x):
    """All stages of a wrapped Swin block chained in fp64-reference form from the block input x [B, H, W, C] (block_stages' analogue):
    norm1, the shifted-window row map, qkv, the window core, proj, the row map back + x, norm2, fc1, GELU -> AdaLog -> fc2 + residual.
    -> dict of references (qkv, core, proj in window order; attn, fc1, mlp in token order [B, H W, .])."""
    out = {}
    B, Hh, W, C = x.shape
    L = Hh * W
    attn = block.attn
    N = attn.window_area
    rows = swin_window_rows((Hh, W), block.window_size, block.shift_size).to(x.device)
    h1 = block.norm1(x).view(B, L, C)[:, rows].reshape(-1, N, C)
    out["qkv"] = linear_qf(attn.qkv, h1)[0]
    core, _, out["amb_core"] = window_attention_core(out["qkv"].float(), attn, block.attn_mask)
    out["core"] = core
    out["proj"] = linear_qf(attn.proj, core.float())[0]
    back = torch.empty(B, L, C, dtype=F64, device=x.device)
    back[:, rows] = out["proj"].view(B, L, C)
    out["attn"] = back + x.view(B, L, C).to(F64)
    x1 = out["attn"].float()
    out["fc1"] = linear_qf(block.mlp.fc1, block.norm2(x1))[0]
    out["mlp"], _, out["amb_fc2"] = postgelu_qf(block.mlp.fc2, out["fc1"].float(), pre_gelu=True, addend=x1)
    return out
