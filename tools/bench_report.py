"""Timing of the quantisation report (adalog_amd/utils/report.py) and its three kernels (csrc/report.hip) on deit_small with 32
images, against the same numbers computed the composed way in the same process: the ``bins`` outputs of the fake-quant kernels plus
torch.bincount, and torch reductions in fp64.  Writes profiles/report_timing.md.

    python tools/bench_report.py [--model deit_small] [--images 32] [--out profiles/report_timing.md]
"""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup=3, iters=10):
    """median milliseconds of fn() between two events on the current stream"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="deit_small")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--depth", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_timing.md"))
    ap.add_argument("--save-checkpoint", default=None, help="also write the calibrated model's plain state_dict here (for the command line)")
    args = ap.parse_args(argv)
    from adalog_amd import ops
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.models import create_model
    from adalog_amd.utils.report import quant_report
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    from tests import report_reference as RR
    dev = "cuda"
    spec = importlib.util.spec_from_file_location("cfg4bench", os.path.join(ROOT, "configs", "4bit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = mod.Config()
    cfg.search_round, cfg.steps = 1, 2
    torch.manual_seed(0)
    model = wrap_modules_in_net(create_model(args.model, depth=args.depth).eval().to(dev), cfg, reparam=True).to(dev)
    x = torch.randn(args.images, 3, 224, 224, generator=torch.Generator().manual_seed(0)).to(dev)
    QuantCalibrator(model, [(x, None)]).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model).to(dev).eval()
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    if args.save_checkpoint:
        torch.save(model.state_dict(), args.save_checkpoint)

    lines = [f"# Report timing: {args.model}, {args.images} images, W4A4", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Median of 10 timed calls after 3 warm-up calls, events on the launch stream.", ""]
    t_report = timed(lambda: quant_report(model, x), warmup=1, iters=3)
    t_recomp = timed(lambda: RR.recompute(model, x), warmup=1, iters=3)
    lines += ["## Whole report", "", "| form | ms |", "|---|---|",
              f"| quant_report (kernels of csrc/report.hip, one read-back) | {t_report:.1f} |",
              f"| composed (hooks + bins kernels + torch.bincount + torch fp64 reductions, tests/report_reference.py) | {t_recomp:.1f} |", ""]

    # the three kernels on the widest activation of the model: fc2's input [images, tokens, 4 * dim]
    blk = model.blocks[0]
    seen = {}
    h = blk.mlp.fc2.register_forward_pre_hook(lambda m, a: seen.__setitem__("x", a[0].detach().clone()))
    with torch.no_grad():
        model(x)
    h.remove()
    t = seen["x"].contiguous()
    n, gb = t.numel(), t.numel() * 4 / 1e9
    aq = blk.mlp.fc2.a_quantizer
    shift = aq.shift.data
    uq = blk.mlp.fc1.a_quantizer
    s, z = uq.scale.data.reshape(1), uq.zero_point.data.reshape(1)
    y = ops.uniform_fake_quant(t, s, z, 4)
    rows = []
    ms = timed(lambda: ops.err_stats(t, y))
    ms_c = timed(lambda: RR.err_stats(t, y))
    rows.append(("err_stats (k_err_stats)", ms, 2 * gb / ms * 1e3, "torch fp64 reductions", ms_c))
    ms = timed(lambda: ops.uniform_code_hist(t, s, z, 4))
    ms_c = timed(lambda: torch.bincount(ops.uniform_fake_quant(t, s, z, 4, want_bins=True, want_y=False)[1].reshape(-1).long(), minlength=16))
    rows.append(("uniform_code_hist (k_code_hist_uniform)", ms, gb / ms * 1e3, "bins kernel + torch.bincount (clip counts not included)", ms_c))
    ms = timed(lambda: ops.log_code_hist(t, aq.scale.data, aq.q, 4, shift=shift))
    ms_c = timed(lambda: RR.log_code_hist_from_bins(aq.bins(t), 4))
    rows.append(("log_code_hist (k_code_hist_log)", ms, gb / ms * 1e3, "bins kernel + torch.bincount", ms_c))
    ms_fq = timed(lambda: ops.uniform_fake_quant(t, s, z, 4))
    lines += [f"## Kernels on fc2's input, {list(t.shape)} fp32 ({gb * 1e3:.1f} MB: it fits the 256 MiB last-level cache, so the rates "
              "below are cache rates, not HBM rates)", "",
              "| kernel | ms | GB/s read | composed form | composed ms |", "|---|---|---|---|---|"]
    for name, ms, rate, cname, ms_c in rows:
        lines.append(f"| {name} | {ms:.3f} | {rate:.0f} | {cname} | {ms_c:.3f} |")
    lines += [f"| k_uniform_rows (uniform_fake_quant, reads and writes the tensor) | {ms_fq:.3f} | {gb / ms_fq * 1e3:.0f} read, "
              f"{2 * gb / ms_fq * 1e3:.0f} read + write | | |", ""]
    slower = [r[0] for r in rows if r[1] > r[4]] + (["quant_report"] if t_report > t_recomp else [])
    lines += ["## Verdict", "",
              ("Every form of the report is at least as fast as the composed form." if not slower else
               "Slower than the composed form: " + ", ".join(slower) + ".  See the notes below."), ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
