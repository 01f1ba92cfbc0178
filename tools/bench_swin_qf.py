"""Times quant_forward of a calibrated Swin at 32 images on the module route and on the fused block route (utils/models.py:
SwinTransformerBlock._fused_attn_residual), each eager and as a captured-graph replay (utils/graph_forward.py).

Random-init weights, a 1-round / 2-step calibration on a few synthetic images (timing only).  Device events around each forward after
warm-up, several repetitions: prints median and spread in ms per 32 images, kernels per forward and per block (torch.profiler), and
max |logit difference| between the routes.

    python tools/bench_swin_qf.py [--models swin_tiny swin_base] [--batch 32] [--reps 20] [--bits 4]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _cfg(bits):
    spec = importlib.util.spec_from_file_location(f"cfg{bits}", os.path.join(ROOT, "configs", f"{bits}bit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = mod.Config()
    cfg.search_round, cfg.steps = 1, 2
    return cfg


def calibrated(name, bits, n_calib=8):
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.models import create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    torch.manual_seed(0)
    model = wrap_modules_in_net(create_model(name).eval().cuda(), _cfg(bits), reparam=True)
    xc = torch.randn(n_calib, 3, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    QuantCalibrator(model, [(xc[i:i + 4], None) for i in range(0, n_calib, 4)]).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model).cuda().eval()
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
        if hasattr(m, "mode"):
            m.mode = "quant_forward"
    return model


def time_ms(fn, x, reps, warmup=3):
    for _ in range(warmup):
        fn(x)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(x)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def kernels(fn, x):
    from torch.profiler import ProfilerActivity, profile
    fn(x)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(x)
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if "DeviceType.CUDA" in str(getattr(e, "device_type", "")))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--models", nargs="+", default=["swin_tiny", "swin_base"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bits", type=int, default=4)
    args = ap.parse_args()
    from adalog_amd.utils import models as M
    from adalog_amd.utils.graph_forward import GraphedForward
    for name in args.models:
        model = calibrated(name, args.bits)
        n_blocks = sum(1 for m in model.modules() if isinstance(m, M.SwinTransformerBlock))
        x = torch.randn(args.batch, 3, 224, 224, generator=torch.Generator().manual_seed(2)).cuda()
        rec = {"model": name, "batch": args.batch, "bits": args.bits, "blocks": n_blocks}
        ys = {}
        try:
            for route, fused in (("module", False), ("fused", True)):
                M.QF_FUSED = fused
                eager = torch.no_grad()(model)
                ys[route] = eager(x).clone()
                t_e = time_ms(eager, x, args.reps)
                gf = GraphedForward(model)
                t_g = time_ms(gf, x, args.reps)
                ys[route + "_graph"] = gf(x)
                n_k = kernels(eager, x)
                rec[route] = {"eager_ms_median": statistics.median(t_e), "eager_ms_min": min(t_e), "eager_ms_max": max(t_e),
                              "graph_ms_median": statistics.median(t_g), "graph_ms_min": min(t_g), "graph_ms_max": max(t_g),
                              "kernels_per_forward": n_k}
                del gf
        finally:
            M.QF_FUSED = True
        rec["max_abs_logit_diff_fused_vs_module"] = (ys["fused"] - ys["module"]).abs().max().item()
        rec["graph_equals_eager_fused"] = bool(torch.equal(ys["fused_graph"], ys["fused"]))
        for route in ("module", "fused"):
            r = rec[route]
            print(f"{name:10s} {route:6s}  eager {r['eager_ms_median']:8.3f} ms [{r['eager_ms_min']:.3f}, {r['eager_ms_max']:.3f}]   "
                  f"graph {r['graph_ms_median']:8.3f} ms [{r['graph_ms_min']:.3f}, {r['graph_ms_max']:.3f}]   "
                  f"{r['kernels_per_forward']} kernels / forward")
        print(f"{name:10s} max |logit fused - module| = {rec['max_abs_logit_diff_fused_vs_module']:.3e}, "
              f"graph replay == eager: {rec['graph_equals_eager_fused']}")
        print(json.dumps(rec))
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
