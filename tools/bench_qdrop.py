#!/usr/bin/env python3
"""QDrop cost: BRECQ iterations per second of a deit_small block at drop_prob 1.0 and 0.5, and the achieved bytes per second of
every drop kernel next to its undropped sibling at the deit_small fc2-input size.

    python tools/bench_qdrop.py [--iters 2000] [--repeats 3] [--out profiles/qdrop_bench.json] [--outcome profiles/qdrop_outcome.json]

The block is set up like bench.py --full's BRECQ leg (brecq_rate): blocks.0 of a calibrated random-weight model, 64 optimisation
images, batch 32, a 100-iteration warm-up call, then the steady state of one reconstruct_single_block call (iterations
iters/4+1 .. iters).  The drop_prob = 1.0 figure is measured ``repeats`` times in this process: its spread is the run-to-run
spread a comparison with another build has to respect.  ADALOG_LIB selects another build of the library for such a comparison
(the recorded one against the parent commit, collected from several such runs, is profiles/qdrop_parent_ab.json: not written here).
--outcome: logit SQNR of a depth-2 random-weight deit_small against its FP twin after calibration, after BRECQ at drop_prob 1.0 and
after BRECQ at 0.5 (an observation: no pretrained weights, no ImageNet)."""
import argparse
import copy
import importlib.util
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_cfg(bits):
    spec = importlib.util.spec_from_file_location("cfg", os.path.join(ROOT, "configs", f"{bits}bit.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod.Config()


def calibrated(model_name, bits, dev, depth=None):
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.models import create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    torch.manual_seed(5)
    base = (create_model(model_name) if depth is None else create_model(model_name, depth=depth)).eval()
    full = copy.deepcopy(base).to(dev).eval()
    model = wrap_modules_in_net(base, load_cfg(bits), reparam=True).to(dev)
    imgs = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(5)).to(dev)
    QuantCalibrator(model, [(imgs, None)], capture="block").batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model)
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    return model, full


def block_rate(model, full, dev, iters, drop_prob):
    """steady-state iterations per second of one reconstruct_single_block call on a copy of the calibrated model"""
    from adalog_amd.utils.block_recon import BlockReconstructor
    model = copy.deepcopy(model)
    opt = torch.randn(64, 3, 224, 224, generator=torch.Generator().manual_seed(6)).to(dev)
    rec = BlockReconstructor(model, full, [(opt[:32], None), (opt[32:], None)])
    name = "blocks.0"
    block, fblock = rec.blocks[name], rec.full_blocks[name]
    kw = {"drop_prob": drop_prob} if drop_prob < 1.0 else {}
    rec.init_block_raw_data(block, fblock, name, dev)
    rec.reconstruct_single_block(name, block, dev, quant_act=True, iters=100, **kw)
    rec.init_block_raw_data(block, fblock, name, dev)
    marks = {}

    def hook(it, loss_func):
        if it in (iters // 4, iters):
            torch.cuda.synchronize()
            marks[it] = time.perf_counter()
    rec.iter_hook = hook
    rec.reconstruct_single_block(name, block, dev, quant_act=True, iters=iters, **kw)
    torch.cuda.synchronize()
    return (iters - iters // 4) / (marks[iters] - marks[iters // 4])


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(3):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best * 1e-3


def kernel_rates(dev):
    """bytes / s of every drop kernel and its sibling on the fc2 input of a deit_small BRECQ iteration: [32, 197, 1536] fp32"""
    from adalog_amd import ops
    from adalog_amd.quantizers import _drop
    from adalog_amd.quant_layers.linear import GELU_SHIFT
    x = torch.randn(32, 197, 1536, device=dev)
    gy = torch.randn_like(x)
    n = x.numel()
    s, z = torch.tensor([0.21], device=dev), torch.tensor([7.0], device=dev)
    s2, qd, sh = torch.tensor([2.3], device=dev), torch.tensor([37], device=dev), torch.tensor([GELU_SHIFT], device=dev)
    st = (_drop.make_state(1234, 0, dev), 0)
    y = ops.log_fake_quant(x, s2, qd, None, None, 4, shift=sh, sub_shift=True, train_form=True)
    B, N, H, D = 32, 197, 6, 64
    xq = torch.randn(B, N, 3 * H * D, device=dev)
    sc = [torch.full((1, H, 1, 1), 0.3, device=dev) for _ in range(3)]
    zp = [torch.full((1, H, 1, 1), 7.0, device=dev) for _ in range(3)]
    gq = [torch.randn(B, H, N, D, device=dev) for _ in range(3)]
    qst = (st[0], (0, 1, 2))
    pairs = {
        "uniform_fwd": (8 * n, lambda: ops.uniform_fake_quant(x, s, z, 4), lambda: ops.uniform_fake_quant_drop(x, s, z, 4, False, 0.5, st)),
        "uniform_bwd": (12 * n, lambda: ops.uniform_fake_quant_backward(gy, x, s, z, 4, False, True, False),
                        lambda: ops.uniform_fake_quant_backward_drop(gy, x, s, z, 4, False, True, False, 0.5, st)),
        "adalog_fwd": (8 * n, lambda: ops.log_fake_quant(x, s2, qd, None, None, 4, shift=sh, sub_shift=True, train_form=True),
                       lambda: ops.log_fake_quant_drop(x, s2, qd, 4, sh, True, False, 0.5, st)),
        "adalog_bwd": (12 * n, lambda: ops.log_fake_quant_backward(gy, x, y, s2, qd, 4, sh, True),
                       lambda: ops.log_fake_quant_backward_drop(gy, x, s2, qd, 4, sh, True, False, 0.5, st)),
        "adalog_pre_gelu_fwd": (8 * n, lambda: ops.log_fake_quant(x, s2, qd, None, None, 4, shift=sh, sub_shift=True, train_form=True, pre_gelu=True),
                                lambda: ops.log_fake_quant_drop(x, s2, qd, 4, sh, True, True, 0.5, st)),
        "adalog_pre_gelu_bwd": (12 * n, lambda: ops.log_fake_quant_backward(gy, x, y, s2, qd, 4, sh, True, pre_gelu=True),
                                lambda: ops.log_fake_quant_backward_drop(gy, x, s2, qd, 4, sh, True, True, 0.5, st)),
        "qkv_split_quant": (8 * xq.numel(), lambda: ops.qkv_split_quant(xq, H, sc, zp, (4, 4, 4)),
                            lambda: ops.qkv_split_quant_drop(xq, H, sc, zp, (4, 4, 4), (0.5, 0.5, 0.5), qst)),
        "qkv_merge_quant_bwd": (12 * xq.numel(), lambda: ops.qkv_merge_quant_backward(gq, xq, H, sc, zp, (4, 4, 4)),
                                lambda: ops.qkv_merge_quant_backward_drop(gq, xq, H, sc, zp, (4, 4, 4), (0.5, 0.5, 0.5), qst)),
    }
    out = {}
    for name, (nbytes, plain, drop) in pairs.items():
        tp, td = timed(plain), timed(drop)
        out[name] = {"bytes": nbytes, "plain_us": round(tp * 1e6, 2), "drop_us": round(td * 1e6, 2),
                     "plain_TBps": round(nbytes / tp * 1e-12, 3), "drop_TBps": round(nbytes / td * 1e-12, 3)}
    return out


def logit_sqnr(model, full, imgs):
    with torch.no_grad():
        ref, got = full(imgs), model(imgs)
    return float(10 * torch.log10(ref.pow(2).sum() / (ref - got).pow(2).sum().clamp_min(1e-30)))


def outcome(dev, bits, iters):
    from adalog_amd.utils.block_recon import BlockReconstructor
    model, full = calibrated("deit_small", bits, dev, depth=2)
    held = torch.randn(64, 3, 224, 224, generator=torch.Generator().manual_seed(99)).to(dev)
    opt = torch.randn(64, 3, 224, 224, generator=torch.Generator().manual_seed(6)).to(dev)
    loader = [(opt[:32], None), (opt[32:], None)]
    res = {"model": "deit_small depth 2, random weights", "bits": bits, "iters_per_block": iters, "optimisation_images": 64,
           "held_out_images": 64, "calibrated_sqnr_db": round(logit_sqnr(model, full, held), 3)}
    for p in (1.0, 0.5):
        m = copy.deepcopy(model)
        BlockReconstructor(m, full, loader).reconstruct_model(quant_act=True, iters=iters, **({"drop_prob": p} if p < 1 else {}))
        res[f"brecq_drop_{p}_sqnr_db"] = round(logit_sqnr(m, full, held), 3)
    res["note"] = "an observation on random weights and random images, not evidence of accuracy on a trained model"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qdrop_bench.json"))
    ap.add_argument("--outcome", default=None)
    ap.add_argument("--outcome-iters", type=int, default=500)
    args = ap.parse_args()
    dev = torch.device("cuda")
    from adalog_amd import _lib
    model, full = calibrated("deit_small", args.bits, dev)
    ones = [round(block_rate(model, full, dev, args.iters, 1.0), 1) for _ in range(args.repeats)]
    half = round(block_rate(model, full, dev, args.iters, 0.5), 1)
    res = {"library": os.path.relpath(_lib.LIB_PATH, ROOT) if _lib.LIB_PATH.startswith(ROOT) else "ADALOG_LIB", "block": "deit_small blocks.0",
           "batch": 32, "iters": args.iters, "steady_iters_per_s_drop_1.0": ones, "spread_drop_1.0": round(max(ones) - min(ones), 1),
           "steady_iters_per_s_drop_0.5": half, "kernels_fc2_input_32x197x1536": kernel_rates(dev)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if args.outcome:
        o = outcome(dev, args.bits, args.outcome_iters)
        with open(args.outcome, "w") as f:
            json.dump(o, f, indent=1)
        print(json.dumps(o))


if __name__ == "__main__":
    main()
