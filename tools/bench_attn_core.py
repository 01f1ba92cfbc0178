"""Times quant_forward of calibrated models at 32 images with the one-launch attention core (utils/models.py: QF_ATTN_CORE, csrc/attn_core.hip)
off and on: captured-graph replay (utils/graph_forward.py) and eager, both switch positions in ONE process and interleaved round by
round, so that clock and box drift hit both columns alike.

Random-init weights, a 1-round / 2-step calibration on a few synthetic images (timing only).  Device events around each forward after
warm-up.  Prints, per model and switch position: the median over all repetitions, the spread of the per-round medians (run-to-run
spread inside the process), kernels per forward (torch.profiler), and whether the two positions give the same logits.

    python tools/bench_attn_core.py [--models deit_small swin_tiny swin_base] [--batch 32] [--rounds 5] [--reps 10] [--bits 4]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_swin_qf import calibrated, kernels, time_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--models", nargs="+", default=["deit_small", "swin_tiny", "swin_base"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bits", type=int, default=4)
    args = ap.parse_args()
    from adalog_amd.utils import models as M
    from adalog_amd.utils.graph_forward import GraphedForward
    old = M.QF_ATTN_CORE
    for name in args.models:
        model = calibrated(name, args.bits)
        n_blocks = sum(1 for m in model.modules() if isinstance(m, (M.SwinTransformerBlock, M.Block)))
        x = torch.randn(args.batch, 3, 224, 224, generator=torch.Generator().manual_seed(2)).cuda()
        eager = torch.no_grad()(model)
        rec = {"model": name, "batch": args.batch, "bits": args.bits, "blocks": n_blocks}
        graphs, ys, times = {}, {}, {}
        try:
            for pos in (False, True):                        # capture one graph per switch position (the route is fixed at capture)
                M.QF_ATTN_CORE = pos
                ys[pos] = eager(x).clone()
                graphs[pos] = GraphedForward(model)
                ys[pos, "graph"] = graphs[pos](x).clone()
                rec["kernels_on" if pos else "kernels_off"] = kernels(eager, x)
                times[pos, "graph"], times[pos, "eager"] = [], []
            for _ in range(args.rounds):
                for pos in (False, True):
                    M.QF_ATTN_CORE = pos
                    times[pos, "graph"].append(time_ms(graphs[pos], x, args.reps))
                    times[pos, "eager"].append(time_ms(eager, x, args.reps))
        finally:
            M.QF_ATTN_CORE = old
        rec["logits_equal_on_vs_off"] = bool(torch.equal(ys[True], ys[False]))
        rec["graph_equals_eager"] = bool(torch.equal(ys[True, "graph"], ys[True]) and torch.equal(ys[False, "graph"], ys[False]))
        for pos in (False, True):
            for mode in ("graph", "eager"):
                rounds = [statistics.median(r) for r in times[pos, mode]]
                allv = [v for r in times[pos, mode] for v in r]
                rec[f"{mode}_{'on' if pos else 'off'}"] = {"ms_median": statistics.median(allv), "round_medians_min": min(rounds),
                                                          "round_medians_max": max(rounds), "ms_min": min(allv)}
        for mode in ("graph", "eager"):
            off, on = rec[f"{mode}_off"], rec[f"{mode}_on"]
            print(f"{name:10s} {mode:5s}  off {off['ms_median']:8.3f} ms [{off['round_medians_min']:.3f}, {off['round_medians_max']:.3f}]   "
                  f"on {on['ms_median']:8.3f} ms [{on['round_medians_min']:.3f}, {on['round_medians_max']:.3f}]   "
                  f"on / off = {on['ms_median'] / off['ms_median']:.3f}")
        print(f"{name:10s} kernels / forward: off {rec['kernels_off']}, on {rec['kernels_on']} ({n_blocks} blocks); "
              f"logits equal: {rec['logits_equal_on_vs_off']}, graph == eager: {rec['graph_equals_eager']}")
        print(json.dumps(rec), flush=True)
        del model, graphs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
