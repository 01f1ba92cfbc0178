"""An independent replay of the FPCS search driver (adalog_amd.search.fpcs) -- TEST INFRASTRUCTURE ONLY.

Plain torch on the CPU; imports nothing from adalog_amd.ops and nothing from tests/cpu_backend.py, so that it shares no code with
either of the two backends the driver runs on.  It follows reference quant_layers/linear.py:483-523 and oracle/adalog_oracle.py:fpcs:

    step 0          score the caller's grid [P, cols]                       -> the `width` best of every column survive
    step 1 .. n-2   score width x new_cnt neighbours of the survivors       -> the `width` best survive, spacing /= new_cnt - 0.5
    step n-1        score the last grid                                     -> the best candidate of every column is committed

``Spy`` records what a search's scorer was handed and what it answered; ``replay`` recomputes every hand-over from those records
and compares bit for bit.  A trajectory that ``replay`` accepts IS the reference's loop run on the recorded scores.
"""
from collections import namedtuple

import torch

Step = namedtuple("Step", "scale zp third scores delta_in")      # host copies of one scoring call (delta_in: None where not visible)


class Mismatch(AssertionError):
    """what ``replay`` raises: where the recorded trajectory leaves the reference's loop"""


def bits_equal(a, b) -> bool:
    """same shape and the same fp32 bit patterns (NaN == NaN, +0 != -0)"""
    if a is None or b is None:
        return a is None and b is None
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape != b.shape:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def rank(scores, k: int):
    """the k best candidates of every column of scores [P, cols] -> indices [k, cols] (int64): score descending, candidate index
    ascending, NaN first -- the order csrc/fpcs_tail.h documents.  Three keys, least significant first, through stable sorts."""
    s = scores.detach().cpu().to(torch.float32)
    nan = torch.isnan(s)
    by_score = torch.sort(torch.where(nan, torch.zeros_like(s), s), dim=0, descending=True, stable=True)[1]   # ties: index ascending
    nan_sorted = torch.gather(nan, 0, by_score)
    nan_first = torch.sort((~nan_sorted).to(torch.int8), dim=0, stable=True)[1]
    return torch.gather(by_score, 0, nan_first)[:k].contiguous()


def next_grid(scale, zp, third, idx, delta, new_cnt: int, clamp_min=None):
    """the grid around the survivors idx [k, cols] of (scale, zp, third) [P, cols] -> ((scale', zp', third') [k * new_cnt, cols],
    delta / (new_cnt - 0.5)).  Survivor-major rows; scale[w] + (lin[i] - 0.5) * delta as separate fp32 operations (torch's CPU
    elementwise kernels do not contract); max(., clamp_min) when a clamp is given; zp / third copied from the survivor."""
    k, cols = idx.shape
    scale, delta = scale.detach().cpu().float(), delta.detach().cpu().float().reshape(cols)
    lin = torch.linspace(0, 1, steps=new_cnt)                                # (the reference evaluates it on the host: linear.py:492)
    top_s = torch.gather(scale, 0, idx)                                      # [k, cols]
    off = (lin - 0.5).view(1, new_cnt, 1) * delta.view(1, 1, cols)           # product rounded to fp32 ...
    grid = (top_s.view(k, 1, cols) + off).reshape(k * new_cnt, cols)         # ... then the sum rounded to fp32
    if clamp_min is not None:
        grid = torch.maximum(grid, torch.tensor(clamp_min, dtype=torch.float32))
    copy = lambda t: None if t is None else torch.gather(t.detach().cpu().float(), 0, idx).repeat_interleave(new_cnt, dim=0).contiguous()
    return (grid.contiguous(), copy(zp), copy(third)), delta / torch.tensor(new_cnt - 0.5, dtype=torch.float32)


def winner(scale, zp, third, scores):
    """the planes [cols] of the best candidate of every column"""
    idx = rank(scores, 1)
    pick = lambda t: None if t is None else torch.gather(t.detach().cpu().float(), 0, idx).reshape(-1)
    return pick(scale), pick(zp), pick(third)


def replay(steps_record, delta0, width: int, eq_n: int, clamp_min=None, committed=None, first=None):
    """Check the recorded scoring calls of ONE search against the reference's loop, bit for bit; raises Mismatch.

    steps_record   [Step] in call order (Spy.steps)
    delta0         the spacing [cols] the search was started with
    committed      what the search returned: (scale, zp | None, third | None) [cols]; None when the caller only has the record
    first          the (scale, zp, third) grid the search was started with (checked against call 0 when given)
    Checked: grid i+1 == next_grid(rank(scores i, width)) of grid i; the spacing used at step i is delta0 divided i times (through
    the grid values, and directly where the spy saw the tail's delta_in); committed == row rank(scores last, 1) of the last grid."""
    new_cnt = int(eq_n / width)
    n = len(steps_record)
    if n < 2:
        raise Mismatch("a committing search has at least two scoring calls, got %d" % n)
    d = delta0.detach().cpu().float().reshape(-1).clone()
    if first is not None:
        for name, a, b in zip(("scale", "zp", "third"), first, steps_record[0][:3]):
            if not bits_equal(a, b):
                raise Mismatch("call 0: the %s plane is not the caller's grid" % name)
    for i in range(n - 1):
        cur, nxt = steps_record[i], steps_record[i + 1]
        if cur.scores.shape != cur.scale.shape:
            raise Mismatch("call %d: scores %s for a grid %s" % (i, tuple(cur.scores.shape), tuple(cur.scale.shape)))
        if cur.delta_in is not None and not bits_equal(cur.delta_in.reshape(-1), d):
            raise Mismatch("call %d: the spacing handed to the tail is not the initial spacing divided %d times" % (i, i))
        want, d = next_grid(cur.scale, cur.zp, cur.third, rank(cur.scores, width), d, new_cnt, clamp_min)
        for name, a, b in zip(("scale", "zp", "third"), want, nxt[:3]):
            if not bits_equal(a, b):
                where = ""
                if a is not None and b is not None and a.shape == b.shape:
                    bad = (a.view(torch.int32) != b.detach().cpu().contiguous().view(torch.int32)).nonzero()
                    where = ": %d elements differ, first at [row %d, col %d]" % (len(bad), bad[0][0], bad[0][1])
                raise Mismatch("call %d -> %d: the %s plane is not the grid around the %d best%s" % (i, i + 1, name, width, where))
    last = steps_record[-1]
    if last.scores.shape != last.scale.shape:
        raise Mismatch("call %d: scores %s for a grid %s" % (n - 1, tuple(last.scores.shape), tuple(last.scale.shape)))
    want = winner(last.scale, last.zp, last.third, last.scores)
    if committed is not None:
        for name, a, b in zip(("scale", "zp", "third"), want, committed):
            if not bits_equal(a, None if b is None else b.reshape(-1)):
                raise Mismatch("commit: the %s plane is not the best candidate of the last grid" % name)
    return want


class Spy:
    """Wraps a search's ``score_fn``: every call's candidate planes and scores are copied to the host before the call returns (fused
    scorers reuse buffers, and a fused tail overwrites its targets in the same launch).  Keeps the attributes the driver routes on.
    When the scorer hands back partial sums (an object with ``finish()``), the scores are those of a second, identical call: the
    scoring kernels are bit-reproducible, and the driver's own object stays untouched for its finish kernel."""

    def __init__(self, fn):
        self.fn = fn
        self.steps = []
        self.returned = []                      # what every call gave back to the driver (its type decides the driver's route)
        for attr in ("fused_tail", "global_scores"):
            if hasattr(fn, attr):
                setattr(self, attr, getattr(fn, attr))

    def __call__(self, scale, zp, third, **kw):
        host = lambda t: None if t is None else t.detach().cpu().clone()
        planes = host(scale), host(zp), host(third)
        tail = kw.get("tail")
        delta_in = host(tail.keep[1]) if tail is not None and getattr(tail, "keep", None) is not None else None
        res = self.fn(scale, zp, third, **kw)
        if torch.is_tensor(res):
            scores = host(res)
        else:
            scores = host(self.fn(scale, zp, third).finish())
        self.steps.append(Step(*planes, scores, delta_in))
        self.returned.append(res)
        return res
