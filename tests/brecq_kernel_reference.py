"""fp64 references of the elementwise and reduction kernels of csrc/brecq.hip (tests/test_brecq_kernels_cpu.py,
tests/test_gpu_brecq_kernels.py) -- CPU only, one pure function per kernel, the formulas of quantizers/{uniform,logarithm,adaround}.py
and utils/block_recon.py (lp_loss, the rounding loss), Adam as torch.optim.Adam's defaults.

Precision rule.  DECISIONS are taken exactly as the module takes them, in IEEE fp32 on the CPU: r = fl(x / s), t = rint(r) + rint(zp),
inside = qmin <= t <= qmax, floor(fl(w / s)), alpha >= 0, the sign of d, 0 <= v <= 1 of the rectified sigmoid, the AdaLog bin
(oracle.adalog_oracle.adalog_bins).  Everything SMOOTH -- sigmoid, powers, exp, sums, the Adam arithmetic -- is evaluated in fp64
from the fp32 inputs (scalars that reach a kernel as C floats -- b, lr, the betas, eps -- are fp32 inputs as well).

Every function returns a dict: the value(s); for a reduction ``<name>_abs`` = sum |term| (the normaliser of its error, the
convention of tests/brecq_grad_reference.py); for a decision that depends on a transcendental, ``near`` (bool, one per element:
the fp64 decision variable lies within the guard below of the threshold) and ``<name>_alts``: the values on the other side(s) of
the decision, each admissible where ``near`` is set.
"""
import math

import torch

from oracle import adalog_oracle as O

F64 = torch.float64
ULP1 = 2.0 ** -23                          # fp32 ulp at 1
SOFT_GUARD = 8 * ULP1                      # soft_h: v = 1.2 sigmoid(a) - 0.1 against 0 and 1 (v is O(1): a few fp32 ulp of the threshold)
BIN_GUARD = 8 * ULP1                       # AdaLog: t = -log2(u) 37 / q against k + 1/2, relative to max(1, t)
INSIDE_GUARD = 4 * ULP1                    # AdaRound: t = floor + h + z against 0 and qmax while h is not saturated (relative to qmax)


def d(t):
    return None if t is None else t.detach().to(F64)


def f32(v):
    """The fp32 value a C float argument takes, as a python float."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def ste_to(v, decided):
    """Straight-through rounding whose forward value is the given (fp32-decided) integer: differentiable like v."""
    return v + (decided - v).detach()


# ---------------------------------------------------------------------------------------------------------------- uniform
def uniform_decisions(x, s, z, bits, sym):
    """fp32: r = fl(x / s), rint(r), rint(zp), t, inside, q.  Returned as fp64 tensors (exact integers) / bool."""
    L = 2 ** (bits - 1)
    qmin, qmax = (-L, L - 1) if sym else (0, 2 * L - 1)
    r32 = x / s
    zr = torch.zeros((), dtype=torch.float32) if sym else torch.round(z)
    t = torch.round(r32) + zr
    inside = (t >= qmin) & (t <= qmax)
    return {"r32": r32, "rint": d(torch.round(r32)), "zr": d(zr), "t": d(t), "inside": inside, "q": d(t.clamp(qmin, qmax)),
            "qmin": qmin, "qmax": qmax}


def uniform_formula(x, s, z, dec):
    """uniform.py:29-35 (training form, round_ste) on tensors of any float type; ``dec`` supplies the roundings."""
    v = ste_to(x / s, dec["rint"])
    if z is None:
        return v.clamp(dec["qmin"], dec["qmax"]) * s
    zs = ste_to(z, dec["zr"])
    return ((v + zs).clamp(dec["qmin"], dec["qmax"]) - zs) * s


def uniform_backward(gy, x, s, z, bits, sym):
    """gx (exactly gy or 0, fp32), gs / gz shaped like s with gs_abs / gz_abs; ``gs_cond`` = sum |gy r| over the inside elements
    (the cancelling pieces (q - z) and r are each this large: what an fp32 evaluation of the term loses)."""
    dec = uniform_decisions(x, s, z, bits, sym)
    g, sd, r = d(gy), d(s), d(x) / d(s)
    ins = dec["inside"].to(F64)
    ts = g * ((dec["q"] - dec["zr"]) - ins * r)
    tz = -(1.0 - ins) * g * sd
    shp = s.shape if s.dim() == x.dim() else (1,) * (x.dim() - s.dim()) + tuple(s.shape)
    red = lambda t: t.sum_to_size(shp).reshape(s.shape)
    out = {"gx": torch.where(dec["inside"], gy, torch.zeros_like(gy)), "gs": red(ts), "gs_abs": red(ts.abs()),
           "gs_cond": red((g * r * ins).abs()), "dec": dec}
    if not sym:
        out["gz"], out["gz_abs"] = red(tz), red(tz.abs())
    return out


def uniform_int(x, s, z, bits):
    dec = uniform_decisions(x, s.reshape(()), z.reshape(()), bits, False)
    return {"y": (dec["q"] - dec["zr"]).float(), "dec": dec}


# ----------------------------------------------------------------------------------------------------------------- AdaLog
def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def log_decisions(x, s, q, bits, shift, pre_gelu):
    """fp32 as the module: (GELU,) + shift, ur = fl(xs / s), iu = 1e-15 <= ur <= 1, the bin and its mask from the oracle."""
    xv = torch.nn.functional.gelu(x) if pre_gelu else x
    xs = xv if shift is None else xv + shift
    ur = xs / s
    k, mask = O.adalog_bins(xs, s, q, bits)
    return {"iu": (ur >= 1e-15) & (ur <= 1.0), "k": d(k), "mask": mask}


def log_formula(x, s, q, bits, shift, sub_shift, pre_gelu, k_decided, iu_decided):
    """logarithm.py:88-92 (training form) behind an optional GELU; ``k_decided``: the bin (k, or 2L where masked); ``iu_decided``:
    where the clamp of u passes the gradient."""
    L = 2 ** (bits - 1)
    xv = gelu64(x) if pre_gelu else x
    xs = xv if shift is None else xv + shift
    ur = xs / s
    u = ur * iu_decided + (ur.clamp(min=1e-15, max=1.0) - ur * iu_decided).detach()
    k = ste_to(-u.log2() * 37.0 / q, k_decided)
    mask = (k < 2 * L).to(x.dtype).detach()
    out = 2 ** (-1 * k.clamp(0, 2 * L - 1) * q / 37.0) * s * mask
    return out - shift if (sub_shift and shift is not None) else out


def _log_values(g, xv, dg, sd, qd, sh, iu, k, mask):
    xs = xv + sh
    u = (xs / sd).clamp(min=1e-15, max=1.0)
    yv = torch.exp2(-k * qd / 37.0) * sd * mask
    dydx = yv / (u * sd) * iu.to(F64) * mask
    ts = g / sd * (yv - dydx * xs)
    return g * dydx * dg, ts, (g / sd * yv).abs() + (g / sd * dydx * xs).abs()


def log_backward(gy, x, s, q, bits, shift, sub_shift, pre_gelu=False):
    """gx elementwise and the scale gradient.  Inside the range the two pieces of a scale term cancel (d out / d s = 0 under the
    STE), so gs_abs sums the magnitudes of the PIECES (g yv / s and g dydx xs / s), which is what any evaluation adds up.
    near: t within BIN_GUARD of a tie; gx_alts: gx with the neighbouring bin."""
    dec = log_decisions(x, s, q, bits, shift, pre_gelu)
    L = 2 ** (bits - 1)
    g, xd, sd, qd = d(gy), d(x), d(s).reshape(()), float(q)
    sh = 0.0 if shift is None else d(shift).reshape(())
    xv = gelu64(xd) if pre_gelu else xd
    dg = (0.5 * (1.0 + torch.erf(xd * math.sqrt(0.5))) + xd * torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)) if pre_gelu \
        else torch.ones_like(xd)
    mask = dec["mask"].to(F64)
    gx, ts, pieces = _log_values(g, xv, dg, sd, qd, sh, dec["iu"], dec["k"], mask)
    t = -((xv + sh) / sd).clamp(min=1e-15, max=1.0).log2() * 37.0 / qd
    near = ((t - t.floor()) - 0.5).abs() <= BIN_GUARD * t.clamp(min=1.0)
    lo, hi = t.floor(), t.floor() + 1.0
    kraw = torch.where(dec["mask"], dec["k"], torch.full_like(t, 2.0 * L))          # the bin before the clamp (2L stands for "masked")
    k_alt = torch.where(kraw.clamp(max=2.0 * L) == lo.clamp(max=2.0 * L), hi, lo)
    m_alt = (k_alt < 2 * L).to(F64)
    gx_alt, ts_alt, _ = _log_values(g, xv, dg, sd, qd, sh, dec["iu"], k_alt.clamp(0, 2 * L - 1), m_alt)
    return {"gx": gx, "gx_alts": [gx_alt], "near": near, "gs": ts.sum().reshape(s.shape), "gs_abs": pieces.sum().reshape(s.shape),
            "gs_slack": (ts_alt - ts).abs()[near].sum(), "dec": dec, "k_decided": kraw}


# --------------------------------------------------------------------------------------------------------------- AdaRound
def soft_h(alpha):
    """h, dh / d alpha in fp64 with the fp32 decision ``lin`` (0 <= v <= 1 as adaround.py:141 evaluates it on the CPU), near, and
    the fp32 h itself (the kernel's decisions downstream of h -- the sign of d, inside -- are taken on it)."""
    a32 = alpha
    v32 = torch.sigmoid(a32) * 1.2000000000000002 + (-0.1)
    lin = (v32 >= 0) & (v32 <= 1)
    sg = torch.sigmoid(d(alpha))
    v = sg * f32(1.2) - f32(0.1)
    dh_lin = f32(1.2) * sg * (1.0 - sg)
    near = (v.abs() <= SOFT_GUARD) | ((v - 1.0).abs() <= SOFT_GUARD)
    return {"h": v.clamp(0, 1), "dh": dh_lin * lin.to(F64), "dh_alt": dh_lin * (~lin).to(F64), "lin": lin, "near": near,
            "h32": v32.clamp(0, 1), "v": v}


def adaround_formula(w, alpha, s, z, qmax, soft, fl_decided):
    """adaround.py:43-60 on [rows, inner] with per-row s, z (no rounding of z here)."""
    s, z = s.view(-1, 1), z.view(-1, 1)
    h = torch.clamp(torch.sigmoid(alpha) * f32(1.2) - f32(0.1), 0, 1) if soft else (alpha >= 0).to(w.dtype)
    return (torch.clamp(ste_to(w / s, fl_decided).detach() + h + z, 0, qmax) - z) * s


def adaround(w, alpha, s, z, bits, soft, gy=None):
    """Forward y; with gy also ga = d/d alpha and its admissible alternatives (the other side of ``lin`` and / or ``inside``)."""
    qmax = float(2 ** bits - 1)
    s2, z2 = s.view(-1, 1), z.view(-1, 1)
    fl32 = torch.floor(w / s2)
    sh = soft_h(alpha)
    h32 = sh["h32"] if soft else (alpha >= 0).float()
    t32 = fl32 + h32 + z2
    inside = (t32 >= 0) & (t32 <= qmax)
    h = sh["h"] if soft else (alpha >= 0).to(F64)
    t = d(fl32) + h + d(z2)
    out = {"y": (t.clamp(0, qmax) - d(z2)) * d(s2), "fl": d(fl32), "inside": inside, "near": torch.zeros_like(inside)}
    if gy is None or not soft:
        if gy is not None:
            out["ga"], out["ga_alts"] = torch.zeros_like(t), []
        return out
    unsat = (sh["v"] > 0) & (sh["v"] < 1)
    near_in = unsat & ((t.abs() <= INSIDE_GUARD * qmax) | ((t - qmax).abs() <= INSIDE_GUARD * qmax))
    base = d(gy) * d(s2)
    ins = inside.to(F64)
    out["ga"] = base * sh["dh"] * ins
    out["ga_alts"] = [base * sh["dh_alt"] * ins, base * sh["dh"] * (1 - ins), base * sh["dh_alt"] * (1 - ins)]
    out["near"] = sh["near"] | near_in
    out["near_lin"], out["near_inside"] = sh["near"], near_in
    return out


# ------------------------------------------------------------------------------------------------------------- round loss
def round_loss(alpha, b):
    """sum_i (1 - |2 h - 1|^b) and d/d alpha elementwise (block_recon.py:205-210, adaround.py:143-146).  ``active``: elements whose
    |d| lies strictly between 0 and 1 (the others contribute exactly 1 or 0)."""
    b = f32(b)
    sh = soft_h(alpha)
    d32 = 2.0 * (sh["h32"] - 0.5)
    sgn = torch.sign(d32).to(F64)
    ad = (2.0 * (sh["h"] - 0.5)).abs()
    nz = sgn != 0
    safe = torch.where(nz, ad, torch.ones_like(ad)).clamp(min=1e-300)
    term = 1.0 - torch.where(nz, safe ** b, torch.zeros_like(ad))
    pm1 = torch.where(nz, safe ** (b - 1.0), torch.zeros_like(ad))
    grad = -b * pm1 * sgn * 2.0 * sh["dh"]
    alt = -b * pm1 * sgn * 2.0 * sh["dh_alt"]
    return {"loss": term.sum(), "loss_abs": term.abs().sum(), "grad": grad, "grad_alts": [alt], "near": sh["near"],
            "active": int(((ad > 0) & (ad < 1)).sum())}


def round_loss_formula(alpha, b):
    h = torch.clamp(torch.sigmoid(alpha) * f32(1.2) - f32(0.1), 0, 1)
    return (1 - ((h - .5).abs() * 2).pow(f32(b))).sum()


def round_loss_multi(alphas, b, weight, gate=None):
    """weight * sum_t loss_t (times gate) and the UNGATED gradients weight * grad_t (ops.round_loss_multi's contract)."""
    w = f32(weight)
    parts = [round_loss(a, b) for a in alphas]
    gt = 1.0 if gate is None else float(d(gate).reshape(()))
    return {"loss": w * sum(p["loss"] for p in parts) * gt, "loss_abs": abs(w) * sum(p["loss_abs"] for p in parts),
            "grads": [w * p["grad"] for p in parts], "grads_alts": [[w * p["grad_alts"][0]] for p in parts],
            "near": [p["near"] for p in parts], "active": sum(p["active"] for p in parts)}


# --------------------------------------------------------------------------------------------------------------- rec loss
def rec_loss(pred, tgt, scale):
    diff = d(pred) - d(tgt)
    sc = f32(scale)
    return {"loss": sc * (diff * diff).sum(), "loss_abs": abs(sc) * (diff * diff).sum()}


def rec_loss_backward(pred, tgt, scale, gmul):
    return {"gpred": (d(pred) - d(tgt)) * (2.0 * f32(scale) * float(d(gmul).reshape(())))}


# ---------------------------------------------------------------------------------------------------------------- softmax
def scaled_softmax(x, scale):
    t = d(x) * f32(scale)
    return {"y": torch.softmax(t, dim=-1), "tmax": torch.where(torch.isfinite(t), t.abs(), torch.zeros_like(t)).amax(-1)}


def scaled_softmax_backward(gy, y, scale):
    """gx = scale y (gy - sum_j gy_j y_j) from the fp32 y the kernel is handed; ``row_abs`` = |scale| sum_j |gy_j y_j| per row."""
    g, yd, sc = d(gy), d(y), f32(scale)
    dot = (g * yd).sum(-1, keepdim=True)
    return {"gx": (g - dot) * yd * sc, "row_abs": abs(sc) * (g * yd).abs().sum(-1)}


# ------------------------------------------------------------------------------------------------------------------- Adam
def adam(params, grads, m, v, step, lr, beta1, beta2, eps):
    """One step of torch.optim.Adam (defaults) after ``step`` earlier ones.  -> new params / m / v (fp64 lists), the updates
    ``dp`` = new - old, the bias corrections and the new step count."""
    b1, b2, e_, lr_ = f32(beta1), f32(beta2), f32(eps), f32(lr)
    t = float(step) + 1.0
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    out = {"p": [], "m": [], "v": [], "dp": [], "bc1": bc1, "bc2": bc2, "step": t}
    for p_, g_, m_, v_ in zip(params, grads, m, v):
        g64 = d(g_)
        mn = d(m_) + (1.0 - b1) * (g64 - d(m_))
        vn = b2 * d(v_) + (1.0 - b2) * g64 * g64
        dp = -(lr_ / bc1) * (mn / (vn.sqrt() / math.sqrt(bc2) + e_))
        out["p"].append(d(p_) + dp); out["m"].append(mn); out["v"].append(vn); out["dp"].append(dp)
    return out


def alpha_grad(w, alpha, gw, s, z, bits, b, weight, gmul, gate):
    """dL/d alpha of one AdaRound layer inside a captured iteration: ga (through w_sim, zero where gw is None) +
    weight * grl * gmul * gate (zero where gmul is None); alternatives as in adaround() / round_loss()."""
    rl = round_loss(alpha, b)
    ar = adaround(w, alpha, s, z, bits, True, gy=torch.zeros_like(w) if gw is None else gw)
    f = 0.0 if gmul is None else f32(weight) * float(d(gmul).reshape(())) * (1.0 if gate is None else float(d(gate).reshape(())))
    g = ar["ga"] + f * rl["grad"]
    alts = [ar["ga_alts"][0] + f * rl["grad_alts"][0], ar["ga_alts"][1] + f * rl["grad"], ar["ga_alts"][2] + f * rl["grad_alts"][0]]
    return {"g": g, "g_alts": alts, "near": ar["near"] | rl["near"]}
