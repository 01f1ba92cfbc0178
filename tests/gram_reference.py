"""References of the Gram-form search tests (tests/test_gram_cases_cpu.py, tests/test_gpu_gram_edges.py).

Weight search (csrc/gram.hip).  ``WeightRef`` extends the exact-integer specification tests/cpu_backend.GramState -- whose results it
does not change -- by the three terms of every score,
    score = -norm (S0 - 2 sigma (w . c) 2^-e + sigma^2 w^T G w),
so that a test can bound the kernel's error PER ELEMENT of [P, O] by what fp64 can do to that cancelling sum (``weight_bar``), and by
the plain fp64 token-form evaluation sum_t (r - sigma x_int . w_int)^2 on the specification's own integer operands
(cpu_backend.score_w_gen's formula), which checks the specification itself (``weight_selfcheck_bound``).

Activation search (csrc/gram_act.hip).  ``ActRef`` evaluates cpu_backend.GramActState's formula in fp64 for ALL candidates and returns
the terms S0, 2 s <X_p, C>, s^2 <H, X_p^T X_p> together with the sums of absolute values that the kernels' roundings act on
(``act_bound``).

Everything here is device-agnostic torch fp64 / int64: the large cases of the GPU tier evaluate it on the device.
"""
import torch

from tests import cpu_backend as CB

F64 = torch.float64
E24 = 2.0 ** -24
E53 = 2.0 ** -53
TINY32 = 2.0 ** -150          # half the spacing of fp32 denormals: the output rounding of a score that underflows


# ---------------------------------------------------------------------------------------------------------------- predicates
NJ_OK = (1, 2, 3, 4, 6, 8, 12, 16, 24)


def g_limbs(T, a_bits):
    """g_limbs of csrc/gram.hip: balanced int8 limbs that hold T qmax^2."""
    gmax = T * (2 ** a_bits - 1) ** 2
    cover = 127
    for L in range(1, 8):
        if gmax <= cover:
            return L
        cover = cover * 256 + 127
    return 8


def limb_switches(a_bits, t_max):
    """[(T, T + 1)]: T the largest token count of each limb count, up to t_max."""
    out, cover, q2 = [], 127, (2 ** a_bits - 1) ** 2
    for _ in range(1, 8):
        T = cover // q2
        if 1 <= T <= t_max:
            out.append((T, T + 1))
        cover = cover * 256 + 127
    return out


def gram_supported(T, O, K, a_bits, w_bits, P):
    """adalog_gram_supported, restated."""
    if not (T >= 1 and O >= 1 and K >= 32 and K % 32 == 0 and 2 <= a_bits <= 7 and 4 * O < 2 ** 30):
        return False
    if K // 32 not in NJ_OK or not 2 <= w_bits <= 7 or P < 32 or P % 32:
        return False
    qw = 2 ** w_bits - 1
    if 128 * qw * K >= 2 ** 23:                            # an accumulator is a 24-bit multiplicand
        return False
    if (4 if w_bits > 4 else 16) * 128 * qw * qw * K >= 2 ** 31:      # GRP products added in an int
        return False
    return O * P // 32 < 2 ** 30


def gram_act_supported(T, O, K, a_bits, w_bits, P):
    """adalog_gram_act_supported, restated."""
    if not (T >= 1 and O >= 1 and K >= 32 and K % 32 == 0 and T * K < 2 ** 31 and 4 * T < 2 ** 30 and P >= 1):
        return False
    return K // 32 in NJ_OK and 2 <= a_bits <= 7 and 2 <= w_bits <= 7 and P <= 65535 and O < 2 ** 15


# ---------------------------------------------------------------------------------------------------------------- weight search
class WeightRef:
    """The integer operands of cpu_backend.GramState (same formulas, kept: X [T, K], v [O, T], e [O]) and G, c, S0 from them."""

    def __init__(self, x2, sa, za, a_bits, ref_t, bias):
        self.T, self.K = x2.shape
        self.O = ref_t.shape[-2]
        self.sa = sa.reshape(-1)[:1].clone()
        z = torch.round(za.reshape(-1)[0])
        self.X = ((torch.round(x2 / self.sa) + z).clamp(0, 2 ** a_bits - 1) - z).to(torch.int64)
        self.rb = ref_t.reshape(self.O, self.T) - (bias.view(-1, 1) if bias is not None else 0.0)       # fp32 subtract
        am = self.rb.abs().amax(1)
        self.am = am
        self.e = torch.where(am > 0, 29 - torch.floor(torch.log2(am.double())), torch.zeros_like(am, dtype=F64))
        self.v = torch.round(self.rb.double() * torch.exp2(self.e).view(-1, 1)).to(torch.int64)
        Xd = self.X.double()                               # (fp64 BLAS on integers below 2^53: exact)
        self.G = Xd.t() @ Xd
        self.c = self.v.double() @ Xd                      # |c| < 2^30 * 127 * T: exact up to T = 2^16
        self.S0 = (self.v.double() ** 2).sum(1) * torch.exp2(-2 * self.e)
        # delta[o]: the largest |r - r_fix| of the column: half a step of the 2^-e grid (nothing is rounded in an all-zero column)
        self.delta = torch.where(am > 0, torch.exp2(-self.e - 1), torch.zeros_like(self.e))

    def _wq(self, w2, sc, zp, w_bits):
        P, O = sc.shape[0], w2.shape[0]
        s, z = sc.reshape(P, O, 1), torch.round(zp.reshape(P, O, 1))
        return ((torch.round(w2.unsqueeze(0) / s) + z).clamp(0, 2 ** w_bits - 1) - z).double()

    def terms(self, w2, sc, zp, w_bits, norm, chunk=32):
        """dict of [P, O] fp64: score, S0, lin2 = 2 sigma |w . c| 2^-e, quad = sigma^2 w^T G w, quad_int_abs = |w|^T |G| |w| (the
        largest partial sum the integer recombination of w^T G w can meet)."""
        P, (O, K) = sc.shape[0], w2.shape
        out = {k: [] for k in ("score", "S0", "lin2", "quad", "quad_int_abs")}
        Ga = self.G.abs()
        for p0 in range(0, P, chunk):
            s = sc[p0:p0 + chunk]
            n = s.shape[0]
            wd = self._wq(w2, s, zp[p0:p0 + chunk], w_bits)
            quad = ((wd.view(n * O, K) @ self.G).view(n, O, K) * wd).sum(-1)
            qa = ((wd.abs().view(n * O, K) @ Ga).view(n, O, K) * wd.abs()).sum(-1)
            lin = (wd * self.c.view(1, O, K)).sum(-1) * torch.exp2(-self.e).view(1, O)
            sig = (self.sa.float() * s.reshape(n, O).float()).double()
            S0 = self.S0.view(1, O).expand(n, O)
            out["score"].append(-norm * (S0 - 2.0 * sig * lin + sig * sig * quad))
            out["S0"].append(S0)
            out["lin2"].append(2.0 * sig * lin.abs())
            out["quad"].append(sig * sig * quad)
            out["quad_int_abs"].append(qa)
        return {k: torch.cat(v, 0) for k, v in out.items()}

    def token_form(self, w2, sc, zp, w_bits, norm, chunk=32):
        """cpu_backend.score_w_gen's formula in fp64 on the specification's integer operands and the UNROUNDED reference r:
        -norm sum_t (r[t, o] - sigma x_int[t] . w_int_p[o])^2, and sum_t (|r| + |sigma x . w|)^2 (what its own roundings act on)."""
        P, O = sc.shape[0], w2.shape[0]
        Xd, r = self.X.double(), self.rb.double()
        sc_out, ab_out = [], []
        for p0 in range(0, P, chunk):
            s = sc[p0:p0 + chunk]
            n = s.shape[0]
            wd = self._wq(w2, s, zp[p0:p0 + chunk], w_bits)
            sig = (self.sa.float() * s.reshape(n, O).float()).double()
            y = torch.einsum("tk,pok->pot", Xd, wd) * sig.unsqueeze(-1)           # integer dot products: exact, then one rounding
            sc_out.append(-norm * ((r.unsqueeze(0) - y) ** 2).sum(-1))
            ab_out.append(((r.abs().unsqueeze(0) + y.abs()) ** 2).sum(-1))
        return torch.cat(sc_out, 0), torch.cat(ab_out, 0)


WEIGHT_C = 16


def weight_bar(t, norm, c=WEIGHT_C):
    """Per element of [P, O]:  2^-24 |spec| + 2^-150 + c 2^-53 norm (S0 + 2 sigma |lin| + sigma^2 quad).

    2^-24 |spec| is the one rounding of the score to fp32 (2^-150: that rounding where the score underflows to a denormal).  c counts
    the fp64 operations of gram_pass that can round, each by 2^-53 of a quantity no larger than the sum of the three terms:
      w . c      3 additions of the four limb rows a lane holds, 1 across the wave's halves, 3 across the waves of a cooperative pass
                 (the products with 2^(8 j) and 2^-e are exact)                                                              7
      w^T G w    an integer below 2^53 at every case of the table (quad_int_abs is asserted): its additions are exact          0
      the score  sigma * lin, sigma * sigma, * quad, the two additions, * norm  (2.0 * is exact)                              6
    13, taken as 16."""
    return E24 * t["score"].abs() + TINY32 + c * E53 * norm * (t["S0"] + t["lin2"] + t["quad"])


def weight_selfcheck_bound(ref, t, tok, tok_abs, norm):
    """|specification - token form| per element.  The specification scores r_fix = v 2^-e in place of r, |r_fix - r| <= delta =
    2^-e / 2 <= 2^-30 max|r| of the column.  With y = sigma x . w:
        sum (r_fix - y)^2 - sum (r - y)^2 = sum (r_fix - r)(r_fix - r + 2 (r - y)),
    so the two differ by at most delta (2 sum_t |r - y| + T delta) <= delta (2 sqrt(T S) + T delta), S = sum (r - y)^2 the token-form
    sum (Cauchy-Schwarz).  On top, fp64: the token form rounds y, r - y, the square and T additions -- (T + 4) 2^-53 of
    sum (|r| + |y|)^2 -- and the specification's recombination 16 x 2^-53 of the sum of its three terms."""
    S = (tok / -norm).clamp(min=0)
    d = ref.delta.view(1, -1)
    rounding = d * (2.0 * torch.sqrt(ref.T * S) + ref.T * d)
    fp = E53 * ((ref.T + 4) * tok_abs + 16 * (t["S0"] + t["lin2"] + t["quad"]))
    return norm * (rounding + fp)


# ---------------------------------------------------------------------------------------------------------------- activation search
class ActRef:
    """cpu_backend.GramActState's operands in fp64: Wq = s_w w_int [O, K], r = fl32(raw_out - bias) [T, O]."""

    def __init__(self, x2, raw_out2, bias, w2, sw, zw, w_bits, a_bits):
        self.x, self.a_bits = x2, a_bits
        self.T, self.K = x2.shape
        self.O = w2.shape[0]
        z = torch.round(zw.reshape(-1, 1))
        s = sw.reshape(-1, 1)
        self.sw = s.double().reshape(-1)
        self.Wq = ((torch.round(w2 / s) + z).clamp(0, 2 ** w_bits - 1) - z).double() * s.double()
        rb = raw_out2 - (bias.view(1, -1) if bias is not None else 0.0)
        self.r = rb.double()
        self.S0 = float((self.r ** 2).sum())
        self.C = self.r @ self.Wq                            # [T, K]
        self.H = self.Wq.t() @ self.Wq
        self.amax = (rb * sw.reshape(1, -1)).abs().amax(1).double()               # [T]: max_o |fl32(r s_w)|, the row's fixed-point scale

    def terms(self, scale, zp, norm, chunk=8):
        """dict of [P] fp64.  score: the direct sum -norm sum_{t,o} (r - s y)^2, y = Wq x_p;  S0, lin2 = 2 s |<X_p, C>|,
        quad = s^2 <H, X_p^T X_p>;  and what the kernels' roundings act on: lin_abs = 2 s sum |x_p| |C|, quad_abs = s^2 sum |H| |G_p|,
        cross_abs = 2 s sum |r| |y|, fix_abs = 2 s sum_t amax_t sum_o |y_int|, csum = s sum |C|."""
        scale, zp = scale.reshape(-1), torch.round(zp.reshape(-1))
        keys = ("score", "lin2", "quad", "lin_abs", "quad_abs", "cross_abs", "fix_abs", "csum", "gram")
        out = {k: [] for k in keys}
        Ha, Ca = self.H.abs(), self.C.abs()
        qmax = 2 ** self.a_bits - 1
        for p0 in range(0, scale.numel(), chunk):
            s32 = scale[p0:p0 + chunk].float().view(-1, 1, 1)
            z = zp[p0:p0 + chunk].view(-1, 1, 1)
            xq = ((torch.round(self.x.unsqueeze(0) / s32) + z).clamp(0, qmax) - z).double()          # [n, T, K]
            s = s32.double().view(-1)
            y = xq @ self.Wq.t()                                                                    # [n, T, O]
            out["score"].append(-norm * ((self.r.unsqueeze(0) - y * s.view(-1, 1, 1)) ** 2).sum((1, 2)))
            lin = (xq * self.C).sum((1, 2))
            G = xq.transpose(1, 2) @ xq                                                             # exact integers
            quad = (G * self.H).sum((1, 2))
            out["lin2"].append(2 * s * lin.abs())
            out["quad"].append(s * s * quad)
            out["gram"].append(-norm * (self.S0 - 2 * s * lin + s * s * quad))
            out["lin_abs"].append(2 * s * (xq.abs() * Ca).sum((1, 2)))
            out["quad_abs"].append(s * s * (G.abs() * Ha).sum((1, 2)))
            out["cross_abs"].append(2 * s * (self.r.abs().unsqueeze(0) * y.abs()).sum((1, 2)))
            out["fix_abs"].append(2 * s * ((y.abs() / self.sw.view(1, 1, -1)).sum(2) * self.amax.view(1, -1)).sum(1))
            out["csum"].append(s * float(Ca.sum()))
        t = {k: torch.cat(v, 0) for k, v in out.items()}
        t["S0"] = torch.full_like(t["score"], self.S0)
        return t


def act_bound(ref, t, norm):
    """Per candidate, what the kernels of csrc/gram_act.hip may differ by from the fp64 direct sum.  With A = S0 + lin_abs + quad_abs:
      2^-24 |score| + 2^-150   the score rounded to fp32
      2^-24 cross_abs          k_ga_rfix forms r s_w[o] in fp32 before it is cut to fixed point: a relative 2^-24 on every term
                               r[t,o] s_w[o] (w_int[o] . x_p[t]) of the linear term, i.e. 2 s sum |r| |y| at worst
      2^-30 fix_abs            the one rounding of a token row to 30-bit fixed point, |.| <= 2^-30 max_o |r s_w| of the row, against
                               sum_o |w_int[o] . x_p[t]|
      2^-53 x                  fp64: H is a sum over O channels and <H, G_p> one over K^2 entries in some order: (O + K^2 + 16)
                               quad_abs;  C enters exactly, the 2^b + 2 runs of the linear term each take two prefix sums that carry
                               <= 40 roundings (4 + 6 + 2 within a block of 1024, the scan of the block sums) of sum |C| and a level
                               |q - z| <= qmax: 4 qmax (2^b + 2) 40 s sum |C|, and their sum (2^b + 2) lin_abs;  S0 is a sum over O,
                               then T: (T + O) S0;  the combination: 8 A."""
    b = ref.a_bits
    qmax, runs = 2 ** b - 1, 2 ** b + 2
    A = t["S0"] + t["lin_abs"] + t["quad_abs"]
    fp = E53 * ((ref.O + ref.K * ref.K + 16) * t["quad_abs"] + runs * t["lin_abs"] + 4 * qmax * runs * 40 * t["csum"]
                + (ref.T + ref.O) * t["S0"] + 8 * A)
    return E24 * t["score"].abs() + TINY32 + norm * (E24 * t["cross_abs"] + 2.0 ** -30 * t["fix_abs"] + fp)


def act_gram_vs_direct_bound(ref, t, norm):
    """The reference's own check: its Gram-form recombination (t["gram"]) against its direct sum, both fp64: every term is a sum of
    at most T max(O, K^2) products, each rounding by 2^-53 of the absolute sums."""
    n = ref.T * max(ref.O, ref.K * ref.K) + 16
    return norm * E53 * n * (t["S0"] + t["lin_abs"] + t["quad_abs"] + t["cross_abs"])
