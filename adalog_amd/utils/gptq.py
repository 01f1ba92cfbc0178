"""GPTQ weight rounding for a calibrated model (Frantar et al., "GPTQ", ICLR 2023): a closed-form, second-order alternative to BRECQ.

``gptq_model(model, images)`` runs where ``--optimize`` would -- on a calibrated model, channel-wise layers un-wrapped, ``reparam_bias``
done -- and needs one pass over the images and no training loop:

  1. Hessian.  The model runs in ``raw`` mode (the FP model, as the calibrator captures it) and a forward hook on every eligible layer
     adds quant_input(x)^T . quant_input(x) into an fp64 [K, K] accumulator (ops.gptq_hessian_add: gemm_f32x3 products of exact
     fixed-point slices per chunk of tokens, summed in fp64).  Nothing the size of an activation is kept.
  2. Factor.  A column with H_jj = 0 gets H_jj = 1, H += damp * mean(diag H) * I, U = cholesky(cholesky_inverse(cholesky(H)),
     upper) in fp64 with torch.linalg ON THE HOST (set-up work of K^3 / 3 flops per layer; the seconds are logged).
  3. Sweep.  ops.gptq_sweep (csrc/gptq.hip, one launch per layer) quantises the weight one input column at a time with the layer's
     committed quantiser and pushes each column's rounding error onto the columns behind it through U.
  4. Commit.  ``weight.data`` <- the swept weight, then invalidate_packed_weight() / forget_codes_fit() exactly as load_packed does.

The scale and zero point do not change and the new weight lies on the quantiser's grid (w_quantizer(weight) == weight bit for bit),
so the result is an ordinary calibrated model: quant_forward, the report, validation and the packed export work on it unchanged.

Eligible: quantised Linear layers whose weight utils.packed would store as codes (committed asymmetric uniform quantiser, 2..8 bits, one
scale or one per row) and whose shape ops.gptq_sweep_ok takes.  Everything else keeps its weight and is listed with the reason.

``sweep_conv=True`` adds the patch-embedding convolution (kernel == stride, no padding: a GEMM over flattened patches,
quant_layers/conv.py) under the same conditions, K = C * kh * kw; the rows of its Hessian are the patches, flattened in the weight's
(c, kh, kw) order.  ``act_order=True`` visits the columns in the order of decreasing diag H (stable: ties to the lower index; a dead
column counts with the diagonal 1 that damped_factor gives it): the Hessian is permuted on the device (ops.permute_sym), factored
as before, and ops.gptq_sweep(perm=...) gathers and scatters inside the kernel, so the committed weight is in natural column order
and the permutation is not kept.  Both are off by default: the default call commits what it always did.

    python -m adalog_amd.utils.gptq --model deit_small --config configs/4bit.py --checkpoint plain.pth --out gptq.pth [--packed] [--bias-correct]
                                    [--act-order] [--sweep-conv]
"""
import argparse
import logging
import time
from collections import OrderedDict

import torch
from torch import nn

from .. import backend
from .packed import _ineligible, _quantised_layers, _rows_cols

CONV_REASON = "convolution: out of scope for the GPTQ sweep"


def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize(t.device)


def _patch_conv_why_not(module):
    """None for a non-overlapping patch convolution (kernel == stride, no padding: a GEMM over flattened patches), else the reason"""
    pad = module.padding if isinstance(module.padding, tuple) else (module.padding, module.padding)
    if not hasattr(module, "_patches") or tuple(module.kernel_size) != tuple(module.stride) or tuple(pad) != (0, 0) \
            or tuple(module.dilation) != (1, 1) or module.groups != 1:
        return "convolution: not a non-overlapping patch convolution (kernel == stride, no padding, groups = 1)"
    return None


def _why_not(be, module, sweep_conv=False):
    """None when the layer is swept, else the reason it is left as it is."""
    if isinstance(module, nn.Conv2d):
        why = _patch_conv_why_not(module) if sweep_conv else CONV_REASON
        if why is not None:
            return why
    elif not isinstance(module, nn.Linear):
        return f"{type(module).__name__} is not a Linear layer"
    why = _ineligible(module)
    if why is not None:
        return why
    rows, cols = _rows_cols(module)
    if not be.gptq_sweep_ok(rows, cols):
        return f"shape [{rows}, {cols}] not taken by the sweep kernel (K a multiple of 32 in [32, 4096])"
    return None


def damped_factor(H, damp):
    """(U, Hd) on the host in fp64: Hd = H with dead columns' diagonal set to 1 and damp * mean(diag) added to the diagonal,
    U upper triangular with Hd^-1 = U^T U."""
    Hd = H.detach().to("cpu", torch.float64).clone()
    d = torch.diagonal(Hd)
    d[d == 0] = 1.0
    d += float(damp) * float(d.mean())
    L = torch.linalg.cholesky(Hd)
    U = torch.linalg.cholesky(torch.cholesky_inverse(L), upper=True)
    return U.contiguous(), Hd


def act_order_perm(H):
    """The act-order of a captured (undamped) Hessian: int32 [K] on H's device, the columns by decreasing fp64 diagonal, ties to the
    lower index (a stable sort).  A dead column counts with the diagonal damped_factor gives it, 1, not with its 0."""
    d = torch.diagonal(H).detach().to("cpu", torch.float64).clone()
    d[d == 0] = 1.0
    return torch.argsort(d, descending=True, stable=True).to(torch.int32).to(H.device)


def _gemm_rows(m, x):
    """fp32 [tokens, K]: the rows of the GEMM the layer runs on its (quantised) input x -- flattened patches for a convolution"""
    xq = m.quant_input(x)
    if isinstance(m, nn.Conv2d):
        return m._patches(xq)[0]
    return xq.reshape(-1, m.in_features)


def _quadratic(D, Hd):
    """sum_r D[r] Hd D[r]^T in fp64 (the layer's objective for the weight difference D)"""
    D = D.double()
    return float(((D @ Hd) * D).sum())


def capture_hessians(model, modules, images, batch_size, rows_of):
    """One pass of ``images`` through ``model`` in ``raw`` mode (the FP model, fused switches off): a forward hook on every module of
    ``modules`` adds X^T X of X = rows_of(module, args) -- fp32 [tokens, in_features] -- into an fp64 accumulator
    (ops.gptq_hessian_add).  Hooks, modes and switches are restored.  -> {id(module): H fp64 [K, K] on the module's device}."""
    from . import models
    be = backend.get()
    moded = [m for m in model.modules() if hasattr(m, "mode")]
    saved_modes = [(m, m.mode) for m in moded]
    saved_switches = (models.QF_FUSED, models.QF_ATTN_CORE, models.QF_LONG)
    hess = {}
    handles = []

    def capture(m, args, out):
        be.gptq_hessian_add(hess[id(m)], rows_of(m, args))

    B = int(images.shape[0])
    try:
        models.QF_FUSED = models.QF_ATTN_CORE = models.QF_LONG = False
        for m in moded:
            m.mode = "raw"
        for m in modules:
            K = _rows_cols(m)[1]
            hess[id(m)] = torch.zeros((K, K), dtype=torch.float64, device=m.weight.device)
            handles.append(m.register_forward_hook(capture))
        with torch.no_grad():
            for s in range(0, B, max(1, int(batch_size))):
                model(images[s:s + max(1, int(batch_size))])
    finally:
        for h in handles:
            h.remove()
        for m, mode in saved_modes:
            m.mode = mode
        models.QF_FUSED, models.QF_ATTN_CORE, models.QF_LONG = saved_switches
    return hess


def gptq_model(model, images, damp=0.01, batch_size=32, bias_correct=False, act_order=False, sweep_conv=False):
    """GPTQ rounding of every eligible layer of a wrapped, calibrated ``model`` from ``images`` (on the model's device); see the module
    text.  Every module's ``mode`` is restored afterwards (quant_forward for a calibrated model).  ``bias_correct``: afterwards, the
    empirical bias correction of utils/bias_correct.py on the same images (its result under "bias_correct"), against FP biases fixed
    before the sweep -- which also takes out of fc2's bias the shift fold the sweep made stale.  ``act_order``: columns in the order of
    decreasing diag H (act_order_perm).  ``sweep_conv``: the patch-embedding convolution is swept too.
    -> {"images", "damp", "layers": {name: {"R", "K", "n_bits", "objective_before" (round-to-nearest under the same damped H),
    "objective_after", "seconds" (factor + sweep), "act_order"}}, "skipped": {name: reason}, "seconds": {"capture", "factor", "sweep"}}."""
    be = backend.get()
    skipped, todo = OrderedDict(), []
    for name, m in _quantised_layers(model):
        why = _why_not(be, m, sweep_conv)
        if why is None:
            todo.append((name, m))
        else:
            skipped[name] = why
    if bias_correct:
        from .bias_correct import bias_correct_model, remember_fp_biases
        remember_fp_biases(model)                          # the fold in fc2's bias is that of q(W) as it is now
    B = int(images.shape[0])
    t0 = time.perf_counter()
    hess = capture_hessians(model, [m for _, m in todo], images, batch_size, lambda m, args: _gemm_rows(m, args[0]))
    _sync(images)
    seconds = {"capture": time.perf_counter() - t0, "factor": 0.0, "sweep": 0.0}

    layers = OrderedDict()
    for name, m in todo:
        wq = m.w_quantizer
        rows, cols = _rows_cols(m)
        dev = m.weight.device
        t1 = time.perf_counter()
        H = hess.pop(id(m))
        perm = act_order_perm(H) if act_order else None
        U, Hd = damped_factor(H if perm is None else be.permute_sym(H, perm), damp)      # (Hd: in the sweep's column order)
        U, Hd = U.to(dev), Hd.to(dev)
        _sync(m.weight)
        t2 = time.perf_counter()
        with torch.no_grad():
            w2 = m.weight.data.reshape(rows, cols)
            scale, zp = wq.scale.data.reshape(-1), wq.zero_point.data.reshape(-1)
            if perm is None:
                what, obj = be.gptq_sweep(w2, scale, zp, int(wq.n_bits), U, want_objective=True)
            else:
                what, obj = be.gptq_sweep(w2, scale, zp, int(wq.n_bits), U, want_objective=True, perm=perm)
            _sync(what)
            t3 = time.perf_counter()
            d_rtn = w2 - m.quant_weight_bias()[0].reshape(rows, cols)
            before = _quadratic(d_rtn if perm is None else d_rtn[:, perm.long()], Hd)
            after = float(obj.sum())
            m.weight.data.copy_(what.reshape(m.weight.shape))
        if hasattr(m, "invalidate_packed_weight"):
            m.invalidate_packed_weight()
        for q in (wq, getattr(m, "a_quantizer", None)):
            if hasattr(q, "forget_codes_fit"):
                q.forget_codes_fit()
        seconds["factor"] += t2 - t1
        seconds["sweep"] += t3 - t2
        layers[name] = {"R": rows, "K": cols, "n_bits": int(wq.n_bits), "objective_before": before, "objective_after": after,
                        "seconds": t3 - t1, "act_order": bool(act_order)}
        logging.info(f"gptq {name}: [{rows}, {cols}] {wq.n_bits}b  objective {before:.6g} -> {after:.6g}  "
                     f"factor (host) {t2 - t1:.3f} s, sweep {t3 - t2:.4f} s")
    logging.info(f"gptq: {len(layers)} layers swept, {len(skipped)} left; capture {seconds['capture']:.2f} s, factor (host) "
                 f"{seconds['factor']:.2f} s, sweep {seconds['sweep']:.3f} s")
    res = {"images": B, "damp": float(damp), "layers": layers, "skipped": skipped, "seconds": seconds}
    if bias_correct:
        res["bias_correct"] = bias_correct_model(model, images, batch_size=batch_size)
    return res


def main(argv=None):
    from .packed import BIT_PLAN_HELP, build_wrapped, load_plain, plan_kwargs, save_packed
    from .report import _dataset_images
    ap = argparse.ArgumentParser(description="GPTQ weight rounding of a plain calibrated checkpoint")
    ap.add_argument("--model", required=True)
    ap.add_argument("--config", required=True, help="the config file the checkpoint was calibrated with")
    ap.add_argument("--checkpoint", required=True, help="plain checkpoint written by test_quant.py")
    ap.add_argument("--out", required=True)
    ap.add_argument("--packed", action="store_true", help="write the result in the adalog-packed-v1 format")
    ap.add_argument("--img-size", type=int, default=None)
    ap.add_argument("--depth", type=int, default=None, help="truncate the block count (as the checkpoint's model was)")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--damp", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dataset", default=None, help="ImageNet root: the first --images validation images instead of a seeded randn batch")
    ap.add_argument("--bias-correct", action="store_true", help="after the sweep, correct the biases on the same images (utils/bias_correct.py)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--bit-plan", default=None, help=BIT_PLAN_HELP)
    ap.add_argument("--act-order", action="store_true", help="visit the columns in the order of decreasing diag H")
    ap.add_argument("--sweep-conv", action="store_true", help="sweep the patch-embedding convolution too")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    device = torch.device(args.device)
    model = build_wrapped(args.model, args.config, device, img_size=args.img_size, depth=args.depth, **plan_kwargs(args.bit_plan))
    model = load_plain(model, args.checkpoint, device)
    if args.dataset:
        images = _dataset_images(args.dataset, args.model, args.images, device)
    else:
        size = args.img_size or getattr(getattr(model, "patch_embed", None), "img_size", (224, 224))[0]
        images = torch.randn(args.images, 3, size, size, generator=torch.Generator().manual_seed(args.seed)).to(device)
    res = gptq_model(model, images, damp=args.damp, batch_size=args.batch_size, bias_correct=args.bias_correct, act_order=args.act_order,
                     sweep_conv=args.sweep_conv)
    if args.packed:
        save_packed(model, args.out)
    else:
        torch.save(model.state_dict(), args.out)
    before = sum(e["objective_before"] for e in res["layers"].values())
    after = sum(e["objective_after"] for e in res["layers"].values())
    s = res["seconds"]
    bc = f"; {len(res['bias_correct']['layers'])} biases corrected" if args.bias_correct else ""
    print(f"{args.out}: {len(res['layers'])} layers swept, {len(res['skipped'])} left as they were; objective {before:.6g} -> {after:.6g}; "
          f"capture {s['capture']:.2f} s, factor (host) {s['factor']:.2f} s, sweep {s['sweep']:.3f} s{bc}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
