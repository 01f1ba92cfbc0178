"""Mixed-precision weight bit plans: which Linear layer gets how many weight bits at a given average (no counterpart in the reference).

``plan_bits(model, images, widths=(3, 4, 6), avg_bits=4.0)`` runs on a wrapped model, calibrated or not -- only the weights and the FP
activations are used:

  1. Hessian.  The model runs in ``raw`` mode and a forward hook per eligible layer adds x^T x of its FP input into an fp64 [K, K]
     accumulator (ops.gptq_hessian_add, the capture loop of utils/gptq.py -- there on quant_input(x), here on x itself).
  2. Cost.  One ops.bit_cost launch per layer (csrc/bitcost.hip, fp64 matrix cores) returns, for every row r,
     sum_jk d_j H_jk d_k with d = w - q_b(w) for every width b, and w H w^T (the layer's output energy) beside them.
     q_b is the per-row min/max asymmetric quantiser -- s = (max - min) / (2^b - 1), z = -min / s, the quantiser's own initialisation.
  3. Allocation.  ``allocate``: an exact multiple-choice knapsack by dynamic programming, minimising sum_l cost_l(b_l) subject to
     sum_l n_l b_l <= avg_bits sum_l n_l (n_l = R K).  With normalise="output" (default) a layer's cost is its relative output error
     cost_l(b) / signal_l, which is commensurable across layers; "none" takes the raw costs.

THE PLAN IS A PROXY.  The costs come from min/max scales, not from the scales the calibration's search will commit, from one layer at a
time (no error propagates), and from the second-order model d H d^T of the layer's own output; whether a plan beats uniform widths at
the same budget is a question for the calibrated model (profiles/bitplan_outcome.json).

Eligible: nn.Linear layers with a w_quantizer whose [R, K] ops.bit_cost_ok takes and whose name contains none of the ``keep``
substrings.  Everything else is listed under "skipped" with the reason and keeps cfg.w_bit; the patch-embedding convolution is out of
scope, as for GPTQ.  The plan goes to wrap_modules_in_net as cfg.w_bit_plan (quant_mixed.py --bit-plan).

    python -m adalog_amd.utils.bitplan --model deit_small --config configs/4bit.py --avg-bits 4 [--widths 3,4,6] [--images 32] \\
        [--dataset ROOT] [--keep head] --out plan.json
"""
import argparse
import json
import logging
import math
import time
from collections import OrderedDict

import torch
from torch import nn

from .. import backend

FORMAT = "adalog-bitplan-v1"
MAX_CELLS = 1 << 22                    # cells of the allocator's table before layer sizes are coarsened
CONV_REASON = "convolution: out of scope for the bit plan"


def minmax_scales(w2, widths):
    """The per-row min/max asymmetric quantiser of fp32 w2 [R, K] at every width at once: (scales, zero points) fp32 [n_widths, R];
    s = (max - min) / (2^b - 1), z = -min / s; s = 1, z = 0 for a constant row and for width 0 (bit_cost's signal row)."""
    mn, mx = w2.amin(dim=1), w2.amax(dim=1)
    levels = torch.tensor([float(2 ** b - 1) if b else 1.0 for b in widths], dtype=torch.float32, device=w2.device).view(-1, 1)
    live = ((mx != mn).view(1, -1)) & torch.tensor([b != 0 for b in widths], device=w2.device).view(-1, 1)
    one, zero = torch.ones((), dtype=torch.float32, device=w2.device), torch.zeros((), dtype=torch.float32, device=w2.device)
    s = torch.where(live, (mx - mn).view(1, -1) / levels, one)
    z = torch.where(live, -mn.view(1, -1) / s, zero)
    return s.contiguous(), z.contiguous()


def allocate(sizes, costs, widths, avg_bits, max_cells=MAX_CELLS):
    """The widths b_l (one of ``widths`` per layer) minimising sum_l costs[l][k_l] subject to sum_l sizes[l] b_l <= avg_bits sum_l sizes[l]:
    an exact multiple-choice knapsack.  costs[l][k]: the cost of layer l at widths[k].  Sizes are counted in units of their gcd; when the
    table (layers x budget) would exceed ``max_cells`` cells, sizes are rounded UP to a coarser unit (logged): the plan then is the
    optimum of a slightly tighter problem and never exceeds the budget.  Ties: fewer total bits, then the lexicographically smallest
    width tuple in layer order.  ValueError when even the smallest width everywhere exceeds the budget.  -> list of widths."""
    sizes = [int(n) for n in sizes]
    widths = [int(b) for b in widths]
    L = len(sizes)
    if L == 0:
        return []
    if len(costs) != L or any(len(c) != len(widths) for c in costs) or min(sizes) < 1 or len(set(widths)) != len(widths):
        raise ValueError("allocate: one positive size per layer, one cost per layer and width, distinct widths")
    unit = 0
    for n in sizes:
        unit = math.gcd(unit, n)
    total = sum(sizes)
    budget_bits = avg_bits * total                                     # in elements x bits
    units = [n // unit for n in sizes]
    cap = int(math.floor(budget_bits / unit + 1e-9))
    if L * (cap + 1) > max_cells:
        factor = -(-(L * (cap + 1)) // max_cells)
        # (rounding a size up may add up to one coarse unit per layer: raise the factor until the table fits)
        while True:
            coarse = [-(-u // factor) for u in units]
            ccap = int(math.floor(budget_bits / (unit * factor) + 1e-9))
            if L * (ccap + 1) <= max_cells:
                break
            factor += 1
        logging.info(f"bitplan: allocator table of {L} x {cap + 1} cells exceeds {max_cells}: layer sizes rounded up to units of "
                     f"{unit * factor} weights (the budget is not exceeded; the plan may spend slightly less than it could)")
        units, cap = coarse, ccap
    order = sorted(range(len(widths)), key=lambda k: widths[k])        # ascending widths: the lexicographic tie-break
    if sum(u * widths[order[0]] for u in units) > cap:
        raise ValueError(f"allocate: even {widths[order[0]]} bits everywhere exceeds the budget of {avg_bits} bits per weight")
    # best[l][c]: (cost, real bits) of layers l.. with c units x bits left, compared as tuples; choice[l][c]: the width index taken.
    # Filled from the last layer backwards so that, walking forwards, the first layer takes the smallest width among equal keys.
    INF = (math.inf, math.inf)
    best = [(0.0, 0)] * (cap + 1)
    choice = []
    for l in range(L - 1, -1, -1):
        cur, ch = [INF] * (cap + 1), [-1] * (cap + 1)
        for c in range(cap + 1):
            for k in order:
                need = units[l] * widths[k]
                if need > c or best[c - need] is INF:
                    continue
                tail = best[c - need]
                key = (costs[l][k] + tail[0], sizes[l] * widths[k] + tail[1])
                if key < cur[c]:
                    cur[c], ch[c] = key, k
        best = cur
        choice.append(ch)
    choice.reverse()
    out, c = [], cap
    for l in range(L):
        k = choice[l][c]
        out.append(widths[k])
        c -= units[l] * widths[k]
    return out


def _why_not(be, name, module, n_widths, keep):
    """None when the layer is planned, else the reason it keeps cfg.w_bit"""
    if not isinstance(module, nn.Linear):
        return CONV_REASON if isinstance(module, nn.Conv2d) else f"{type(module).__name__} is not a Linear layer"
    for k in keep:
        if k and k in name:
            return f"kept: the name contains '{k}'"
    rows, cols = int(module.weight.shape[0]), int(module.weight.shape[1])
    if not be.bit_cost_ok(rows, cols, n_widths):
        return f"shape [{rows}, {cols}] not taken by the bit-cost kernel (K a multiple of 32 in [32, 4096])"
    return None


def plan_bits(model, images, widths=(3, 4, 6), avg_bits=4.0, batch_size=32, normalise="output", keep=(), hessians=None):
    """The bit plan of a wrapped ``model`` from ``images`` (on the model's device); see the module text.  ``hessians``: {layer name: H}
    to use in place of the capture pass (tests feed two backends the same matrices).
    -> {"widths", "avg_bits_target", "avg_bits" (of the planned layers), "normalise", "layers": {name: {"R", "K", "bits", "cost": {b: ..},
    "signal"}}, "plan": {name: bits}, "uniform": {b: total cost at uniform b}, "skipped": {name: reason}, "seconds"}."""
    from .gptq import capture_hessians
    from .packed import _quantised_layers
    if normalise not in ("output", "none"):
        raise ValueError("plan_bits: normalise must be 'output' or 'none'")
    widths = tuple(int(b) for b in widths)
    if not widths or len(set(widths)) != len(widths) or any(not 2 <= b <= 7 for b in widths) or len(widths) > 7:
        raise ValueError("plan_bits: widths must be up to seven distinct integers in [2, 7] (what wrap_modules_in_net takes)")
    be = backend.get()
    t0 = time.perf_counter()
    bits = (0,) + widths
    skipped, todo = OrderedDict(), []
    for name, m in _quantised_layers(model):
        why = _why_not(be, name, m, len(bits), tuple(keep))
        if why is None:
            todo.append((name, m))
        else:
            skipped[name] = why
    if hessians is None:
        hess = capture_hessians(model, [m for _, m in todo], images, batch_size, lambda m, args: args[0].reshape(-1, m.in_features))
        hessians = {name: hess[id(m)] for name, m in todo}
    layers = OrderedDict()
    sizes, costs = [], []
    for name, m in todo:
        with torch.no_grad():
            w2 = m.weight.data.reshape(m.weight.shape[0], -1)
            s, z = minmax_scales(w2, bits)
            cost = be.bit_cost(w2, s, z, bits, hessians[name]).sum(dim=1).tolist()
        signal = float(cost[0])
        raw = [float(c) for c in cost[1:]]
        if normalise == "output":
            used = [c / signal if signal != 0.0 else 0.0 for c in raw]
        else:
            used = raw
        R, K = int(w2.shape[0]), int(w2.shape[1])
        layers[name] = {"R": R, "K": K, "bits": None, "cost": {b: c for b, c in zip(widths, used)}, "signal": signal}
        sizes.append(R * K)
        costs.append(used)
    chosen = allocate(sizes, costs, widths, avg_bits)
    plan = OrderedDict()
    for (name, _), b in zip(todo, chosen):
        layers[name]["bits"] = plan[name] = int(b)
    total = sum(sizes)
    res = {"widths": list(widths), "avg_bits_target": float(avg_bits),
           "avg_bits": (sum(n * b for n, b in zip(sizes, chosen)) / total) if total else 0.0, "normalise": normalise, "layers": layers,
           "plan": plan, "uniform": {b: sum(c[k] for c in costs) for k, b in enumerate(widths)}, "skipped": skipped,
           "seconds": time.perf_counter() - t0}
    logging.info(f"bitplan: {len(plan)} layers planned at {res['avg_bits']:.3f} bits per weight (target {avg_bits}), {len(skipped)} keep "
                 f"the config's width; cost {sum(layers[n]['cost'][b] for n, b in plan.items()):.6g} against uniform "
                 + ", ".join(f"{b}b {c:.6g}" for b, c in res["uniform"].items()))
    return res


def main(argv=None):
    from .packed import build_wrapped
    from .report import _dataset_images
    ap = argparse.ArgumentParser(description="Per-layer weight bit plan of a model at an average width (adalog-bitplan-v1)")
    ap.add_argument("--model", required=True)
    ap.add_argument("--config", required=True, help="the config file the model will be calibrated with")
    ap.add_argument("--avg-bits", type=float, required=True, help="average weight bits over the planned layers")
    ap.add_argument("--widths", default="3,4,6", help="the widths to choose from, comma separated")
    ap.add_argument("--out", required=True)
    ap.add_argument("--checkpoint", default=None, help="FP weights (a state dict of the unwrapped model); default: the seeded random init")
    ap.add_argument("--img-size", type=int, default=None)
    ap.add_argument("--depth", type=int, default=None, help="truncate the block count")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dataset", default=None, help="ImageNet root: the first --images validation images instead of a seeded randn batch")
    ap.add_argument("--keep", action="append", default=[], help="layers whose name contains this keep the config's width (repeatable)")
    ap.add_argument("--normalise", default="output", choices=("output", "none"))
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    model = build_wrapped(args.model, args.config, device, img_size=args.img_size, depth=args.depth)
    if args.checkpoint:
        logging.info(str(model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"), strict=False)))
    if args.dataset:
        images = _dataset_images(args.dataset, args.model, args.images, device)
    else:
        size = args.img_size or getattr(getattr(model, "patch_embed", None), "img_size", (224, 224))[0]
        images = torch.randn(args.images, 3, size, size, generator=torch.Generator().manual_seed(args.seed)).to(device)
    res = plan_bits(model, images, widths=tuple(int(b) for b in args.widths.split(",")), avg_bits=args.avg_bits,
                    batch_size=args.batch_size, normalise=args.normalise, keep=tuple(args.keep))
    out = {"format": FORMAT, "model": args.model, "images": int(images.shape[0])}
    out.update({k: v for k, v in res.items()})
    out["layers"] = {n: dict(e, cost={str(b): c for b, c in e["cost"].items()}) for n, e in res["layers"].items()}
    out["uniform"] = {str(b): c for b, c in res["uniform"].items()}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    hist = {b: sum(1 for v in res["plan"].values() if v == b) for b in res["widths"]}
    print(f"{args.out}: {len(res['plan'])} layers at {res['avg_bits']:.3f} bits per weight (target {args.avg_bits}), "
          + ", ".join(f"{n} at {b}b" for b, n in hist.items()) + f"; {len(res['skipped'])} keep the config's width; {res['seconds']:.2f} s")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
