"""fp64 reference of the BRECQ autograd routes of adalog_amd/train_mm.py: the output and every gradient of the operation each
route stands for, by ordinary torch autograd on the textbook expression (plain torch on the CPU; adalog_amd is not imported).

Every function takes fp32 (or already fp64) tensors, promotes them to fp64 and returns a dict of fp64 tensors: ``y`` and one
``g<name>`` per leaf, in that leaf's own index order.  The quantised routes return each gradient twice -- by autograd with the
straight-through rounding ``(r.round() - r).detach() + r`` and in closed form from the lines the project's quantiser documents
(adalog_amd/quantizers/uniform.py:17-19):

    q = clamp(rne(x / s) + z, 0, 2^bits - 1),   inside = [0 <= rne(x / s) + z <= 2^bits - 1]   (taken BEFORE the clamp)
    dy/dx = inside,   dy/ds = (q - z) - (x / s) * inside

and, next to every scale gradient (a sum with cancellation), ``abs``: the sum of the absolute values of its terms, by which an
error of that sum is normalised.  Zero points are integers in every case of the table (the kernels round them; an integer needs
no rounding).

Inputs of a quantiser come from ``off_tie_input``: x = s * (k - z + f) with an integer k drawn from [-3, 2^bits + 2] (both clamp
sides and inside = 0 occur) and |f| <= 0.35, so x / s stays 0.15 away from every rounding tie -- three orders of magnitude more
than the fp32 rounding of x and of the quotient moves it -- and the fp32 kernels and this fp64 reference decide every bin alike.
That is a condition on the inputs (tests/test_brecq_grads_cpu.py asserts it for every case), not a tolerance: no element is left
out of any comparison.
"""
import torch

F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _leaf(t):
    return None if t is None else t.detach().to(F64).clone().requires_grad_(True)


def _ste(r):
    return (r.round() - r).detach() + r


def off_tie_input(shape, s, z, bits, g):
    """fp32 x = s * (k - z + f) of ``shape``; s, z broadcast against it.  -> (x, k): k the integer rne(x / s) + z before the clamp."""
    k = torch.randint(-3, 2 ** bits + 3, shape, generator=g).to(F64)
    f = (torch.rand(shape, generator=g, dtype=F64) * 2 - 1) * 0.35
    x = (s.to(F64) * (k - z.to(F64) + f)).float()
    return x, k


def bins(x, s, z, dtype):
    """rne(x / s) + z (before the clamp) with the division in ``dtype``: what decides q and inside."""
    return (torch.round(x.to(dtype) / s.to(dtype)) + z.to(dtype)).to(F64)


def quant_parts(x, s, z, bits):
    """(r, inside, xi) of the asymmetric uniform quantiser in fp64: r = x / s, xi = q - z."""
    qmax = 2 ** bits - 1
    r = x / s
    t = torch.round(r) + z
    inside = ((t >= 0) & (t <= qmax)).to(F64)
    return r, inside, t.clamp(0, qmax) - z


def _quant_autograd(x, s, z, bits):
    return ((_ste(x / s) + z).clamp(0, 2 ** bits - 1) - z) * s


# ---------------------------------------------------------------------------------------------------------------- linear
def linear(x, w, b, addend, gy):
    """y = x @ w^T + b (+ addend): x [..., K], w [N, K], b [N] | None, addend broadcastable to y | None."""
    x_, w_, b_, a_ = _leaf(x), _leaf(w), _leaf(b), _leaf(addend)
    y = x_ @ w_.t()
    if b_ is not None:
        y = y + b_
    if a_ is not None:
        y = a_ + y
    y.backward(gy.to(F64))
    return {"y": y.detach(), "gx": x_.grad, "gw": w_.grad, "gb": None if b_ is None else b_.grad,
            "gaddend": None if a_ is None else a_.grad}


# ---------------------------------------------------------------------------------------------------------- quant_linear
def quant_linear(x, s, z, bits, w, b, gy, addend=None):
    """y = (s * (q - z)) @ w^T + b (+ addend), per-tensor quantiser (s, z of one element).  Gradients of x, s, w, b by autograd;
    the same four in closed form under ``closed``; ``gs_abs`` = sum |term| of the scale gradient."""
    x_, s_, w_, b_ = _leaf(x), _leaf(s.reshape(())), _leaf(w), _leaf(b)
    z_ = z.detach().to(F64).reshape(())
    gy = gy.to(F64)
    y = _quant_autograd(x_, s_, z_, bits) @ w_.t()
    if b_ is not None:
        y = y + b_
    if addend is not None:
        y = addend.to(F64) + y
    y.backward(gy)
    with torch.no_grad():
        xd, sd, wd = x_.detach(), s_.detach(), w_.detach()
        r, inside, xi = quant_parts(xd, sd, z_, bits)
        gxs = gy @ wd                                            # dL/dx_sim
        terms = gxs * (xi - r * inside)
        gy2 = gy.reshape(-1, gy.shape[-1])
        closed = {"y": (sd * xi) @ wd.t() + (0 if b_ is None else b_.detach()) + (0 if addend is None else addend.to(F64)),
                  "gx": gxs * inside, "gs": terms.sum(), "gw": gy2.t() @ (sd * xi).reshape(-1, xi.shape[-1]),
                  "gb": None if b_ is None else gy2.sum(0)}
    return {"y": y.detach(), "gx": x_.grad, "gs": s_.grad, "gw": w_.grad, "gb": None if b_ is None else b_.grad,
            "gs_abs": terms.abs().sum(), "closed": closed}


# ---------------------------------------------------------------------------------------------------------------- matmul
def matmul(A, Bm, b_transposed, merge, gy):
    """A @ B batched.  ``b_transposed``: the leaf Bm is [..., N, K] and B = Bm.transpose(-1, -2) (k of q.k^T); its gradient comes
    back on Bm, in Bm's own index order.  ``merge`` (4-D): the result [B, H, R, D] passes through transpose(1, 2).reshape(B, R, H*D)
    and gy has that shape."""
    A_, B_ = _leaf(A), _leaf(Bm)
    y = A_ @ (B_.transpose(-1, -2) if b_transposed else B_)
    if merge:
        b, h, r, d = y.shape
        y = y.transpose(1, 2).reshape(b, r, h * d)
    y.backward(gy.to(F64))
    return {"y": y.detach(), "gA": A_.grad, "gB": B_.grad}


# ------------------------------------------------------------------------------------------------------- attention chain
def attention(x, H, scales, zps, bits, mul, gy):
    """x [B, N, 3*H*D] -> head split -> the three uniform quantisers (scales[p] / zps[p] of one element or of H) -> q.k^T ->
    softmax(. * mul) -> . v -> merged heads [B, N, H*D].  Gradients of x and of the three scales (shaped like scales[p]) by
    autograd; ``closed``: the same four from the closed form fed with autograd's gradient of each quantiser's OUTPUT;
    ``gs_abs``: per scale, sum |term| (per head where the scale is)."""
    B, N, C = x.shape
    D = C // (3 * H)
    x_ = _leaf(x)
    s_ = [_leaf(s) for s in scales]
    z_ = [z.detach().to(F64) for z in zps]
    parts = x_.reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    sims = []
    for p in range(3):
        sim = _quant_autograd(parts[p], s_[p].reshape(1, -1, 1, 1), z_[p].reshape(1, -1, 1, 1), bits[p])
        sim.retain_grad()
        sims.append(sim)
    q, k, v = sims
    attn = torch.softmax((q @ k.transpose(-1, -2)) * mul, dim=-1)
    y = (attn @ v).transpose(1, 2).reshape(B, N, H * D)
    y.backward(gy.to(F64))
    out = {"y": y.detach(), "gx": x_.grad, "gs": [s.grad for s in s_], "gs_abs": [], "closed": {"gs": []}}
    with torch.no_grad():
        gparts = []
        for p in range(3):
            r, inside, xi = quant_parts(parts[p].detach(), s_[p].detach().reshape(1, -1, 1, 1), z_[p].reshape(1, -1, 1, 1), bits[p])
            g_ = sims[p].grad
            terms = g_ * (xi - r * inside)
            per_head = scales[p].numel() > 1
            out["gs_abs"].append((terms.abs().sum(dim=(0, 2, 3)) if per_head else terms.abs().sum()).reshape(scales[p].shape))
            out["closed"]["gs"].append((terms.sum(dim=(0, 2, 3)) if per_head else terms.sum()).reshape(scales[p].shape))
            gparts.append(g_ * inside)
        out["closed"]["gx"] = torch.stack(gparts, 0).permute(1, 3, 0, 2, 4).reshape(B, N, C)
    return out
