"""Empirical bias correction of a calibrated model (Nagel et al., "Data-Free Quantization Through Weight Equalization and Bias
Correction", ICCV 2019, section 4.2, in its empirical form): closed-form, no training loop, the weights are left alone.

For a layer with a bias, d = y_fp - y_q is the difference between the layer's output in the FP model and in the quantised model on
the same images, and m_c its mean over the tokens of output channel c.  ``bias_correct_model(model, images)`` runs where ``--optimize``
and GPTQ run -- on a calibrated model, channel-wise layers un-wrapped, ``reparam_bias`` done -- and is defined by this recurrence over
the eligible layers in the order the forward pass reaches them:

    for layer l = 1 .. L:   m = mean over tokens of (y_fp[l] - y_q[l]),  y_q[l] with layers 1 .. l-1 already corrected
                            bias[l] += float32(m)

Measurement.  Per layer and chunk of images, two forward passes that stop behind the layer (a forward hook raises a private
exception): the FP side, then the quantised side on the module route (models.QF_FUSED / QF_ATTN_CORE / QF_LONG off, restored
afterwards: the fused routes bypass ``module.__call__`` and its hooks).  ops.mean_err (csrc/report.hip: one streaming pass, fp64,
a fixed summation order) turns the two outputs into sum d, sum d^2 and max |y_fp| per channel; the chunks' sums are added in fp64 in
chunk order.  Only the two outputs of the chunk in flight are alive: nothing the size of an activation is kept across chunks or layers.

The FP side.  ``raw`` mode shares the bias Parameter with ``quant_forward``, so a committed correction would move the reference with
it (d does not depend on the shared bias at all).  The FP side therefore runs ``raw`` mode with the layers' FP biases put in place for
the pass: the bias as it was before the first correction, kept on the module (``_bc_fp_bias``, not part of the state_dict), and for a
post-GELU layer whose bias ``reparam_bias`` has folded shift . rowsum(q(W)) into, that bias less the fold of the current q(W) -- the
folded bias belongs to the quantised operand q(x + shift), not to the FP layer.  remember_fp_biases() fixes them ahead of a step that
changes q(W) (gptq_model(bias_correct=True) calls it before the sweep, so the correction also takes out the fold the sweep made stale).
The kept biases live as long as the module objects: a checkpoint holds the corrected biases only, so correct ONCE, from the calibrated
(or swept) checkpoint -- correcting a reloaded corrected checkpoint would add the same means a second time.

Eligible: quantised nn.Linear layers and the patch-embedding nn.Conv2d, with a bias, calibrated, in ``quant_forward`` mode and reached
once per forward.  Everything else -- the MatMul modules, bias-free layers, uncalibrated layers -- is listed with the reason.

Nothing in the forward routes is derived from a bias: the packed weight image (_wp_cache) is keyed on weight, scale and zero point,
the shift fold of an un-reparamed fc2 is recomputed from ``bias.data`` in every forward, and the GEMM epilogues (bias, residual) read
``bias.data`` through its pointer.  The commit is an in-place add on ``bias.data``, so the pointer -- and a captured HIP graph that
holds it -- stays valid, and no cache needs dropping; weight, scale and zero point are not written.

    python -m adalog_amd.utils.bias_correct --model deit_small --config configs/4bit.py --checkpoint plain.pth --out bc.pth [--packed]
"""
import argparse
import logging
import time
from collections import OrderedDict

import torch
from torch import nn

from .. import backend


class _Stop(Exception):
    """raised by the measuring hook: the forward pass has produced the layer's output and need not go on"""


def _why_not(m):
    """None when the module can be corrected, else the reason it is left as it is."""
    if not isinstance(getattr(m, "weight", None), torch.Tensor) or not hasattr(m, "w_quantizer"):
        return f"{type(m).__name__} has no weight and no bias (a product of two activations)"
    if not isinstance(m, (nn.Linear, nn.Conv2d)):
        return f"{type(m).__name__} is neither a Linear layer nor a convolution"
    if m.bias is None:
        return "no bias"
    if not getattr(m, "calibrated", False):
        return "not calibrated"
    if m.mode != "quant_forward":
        return f"mode {m.mode!r}, not quant_forward"
    return None


def _fold_of(be, m):
    """the shift fold reparam_bias added to the bias of a post-GELU layer, from the current q(W) (fp32 [O]); None: no fold in the bias"""
    aq = getattr(m, "a_quantizer", None)
    if not hasattr(m, "reparam_bias") or not hasattr(aq, "_shift_args"):
        return None
    shift, sub = aq._shift_args()
    if shift is None or sub:
        return None
    from ..ops import BF16
    _, rowsum = m._pack_w_fixed(BF16, want_rowsum=True)
    return be.shift_fold(rowsum.view(1, -1), m.w_quantizer.scale.data.view(1, -1), shift.data, None).view(-1)


def _fp_bias(be, m):
    """the bias of the FP layer: the remembered one, else the current bias (less the shift fold where reparam_bias added it)"""
    kept = m.__dict__.get("_bc_fp_bias")
    if kept is not None:
        return kept
    fold = _fold_of(be, m)
    b = m.bias.data
    return b.clone() if fold is None else b - fold.to(b.dtype)


def remember_fp_biases(model):
    """Fix the FP bias of every layer with a bias and a weight quantiser as of now (kept ones are not touched); see the module text."""
    be = backend.get()
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, "w_quantizer") and isinstance(getattr(m, "bias", None), torch.Tensor) and "_bc_fp_bias" not in m.__dict__:
                m.__dict__["_bc_fp_bias"] = _fp_bias(be, m)


class _Measurement:
    """The state of one measuring run: switches off, hooks and modes restored on every exit (a context manager)."""

    def __init__(self, model, images, batch_size):
        from . import models
        self.models, self.be = models, backend.get()
        self.model, self.images = model, images
        self.step = max(1, int(batch_size))
        self.moded = [(name, m) for name, m in model.named_modules() if hasattr(m, "mode")]
        self.saved_modes = [(m, m.mode) for _, m in self.moded]
        self.saved_switches = (models.QF_FUSED, models.QF_ATTN_CORE, models.QF_LONG)
        self.handles, self.swapped, self.fp = [], [], {}

    def __enter__(self):
        self.models.QF_FUSED = self.models.QF_ATTN_CORE = self.models.QF_LONG = False
        return self

    def __exit__(self, *exc):
        self._restore_pass()
        for m, mode in self.saved_modes:
            m.mode = mode
        self.models.QF_FUSED, self.models.QF_ATTN_CORE, self.models.QF_LONG = self.saved_switches
        return False

    def _restore_pass(self):
        for h in self.handles:
            h.remove()
        self.handles = []
        for m, data in self.swapped:
            m.bias.data = data
        self.swapped = []

    def plan(self):
        """-> (todo [(name, module)] in forward order, skipped {name: reason}): one FP pass over the first image records the order"""
        skipped, cand = OrderedDict(), {}
        for name, m in self.moded:
            why = _why_not(m)
            if why is None:
                cand[id(m)] = (name, m)
            else:
                skipped[name] = why
        calls = []
        self._pass("raw", [(m, lambda mod, args, out: calls.append(id(mod))) for _, m in cand.values()], self.images[:1])
        todo = []
        for name, m in cand.values():
            n = calls.count(id(m))
            if n != 1:
                skipped[name] = "not reached by the model's forward" if n == 0 else f"reached {n} times per forward"
        for i in calls:
            if calls.count(i) == 1:
                todo.append(cand[i])
        return todo, skipped

    def _pass(self, side, hooks, x):
        """one forward of ``x`` with ``hooks`` [(module, fn)] on: side "raw" = the FP model (FP biases in place), "quant" = as saved"""
        try:
            if side == "raw":
                for _, m in self.moded:
                    m.mode = "raw"
                for m in self.model.modules():
                    if hasattr(m, "w_quantizer") and isinstance(getattr(m, "bias", None), torch.Tensor):
                        if id(m) not in self.fp:           # (once per run: a commit does not move a layer's FP bias)
                            self.fp[id(m)] = _fp_bias(self.be, m)
                        self.swapped.append((m, m.bias.data))
                        m.bias.data = self.fp[id(m)]
            else:
                for m, mode in self.saved_modes:
                    m.mode = mode
            self.handles = [m.register_forward_hook(fn) for m, fn in hooks]
            try:
                self.model(x)
            except _Stop:
                pass
        finally:
            self._restore_pass()

    def _output(self, side, m, x):
        got = []

        def grab(mod, args, out):
            got.append(out.detach())
            raise _Stop

        self._pass(side, [(m, grab)], x)
        if len(got) != 1:
            raise RuntimeError(f"bias correction: the forward pass did not reach {type(m).__name__} on the {side} side")
        return got[0]

    def layer(self, m, quant_max=False):
        """-> (stats fp64 [C, 3 | 4] on the device: sum d, sum d^2, max |y_fp| [, max |y_q|]; T tokens per channel) over all images"""
        acc, T = None, 0
        for s in range(0, int(self.images.shape[0]), self.step):
            x = self.images[s:s + self.step]
            y_fp = self._output("raw", m, x)
            y_q = self._output("quant", m, x)
            if y_fp.shape != y_q.shape:
                raise RuntimeError(f"bias correction: FP output {tuple(y_fp.shape)} against quantised output {tuple(y_q.shape)}")
            y_fp, y_q, C, inner = _channel_form(m, y_fp, y_q)
            st = self.be.mean_err(y_fp, y_q, C, inner)
            if quant_max:
                st = torch.cat([st, self.be.mean_err(y_q, y_fp, C, inner)[:, 2:3]], 1)
            if acc is None:
                acc = st.clone()
            else:
                acc[:, :2] += st[:, :2]
                acc[:, 2:] = torch.maximum(acc[:, 2:], st[:, 2:])
            T += y_fp.numel() // C
            del y_fp, y_q
        return acc, T


def _channel_form(m, y_fp, y_q):
    """(y_fp, y_q, C, inner) as ops.mean_err takes them, without a copy where the memory already has one of its two layouts: a Linear
    output is [tokens, C] (inner = 1); a convolution's [B, C, H, W] is either contiguous (inner = H W) or -- the patch GEMM's
    permuted view -- contiguous as [B, H, W, C] (inner = 1)."""
    if isinstance(m, nn.Conv2d):
        C = int(y_fp.shape[1])
        a, b = y_fp.permute(0, 2, 3, 1), y_q.permute(0, 2, 3, 1)
        if a.is_contiguous() and b.is_contiguous():
            return a, b, C, 1
        return y_fp.contiguous(), y_q.contiguous(), C, int(y_fp.shape[2] * y_fp.shape[3])
    C = int(y_fp.shape[-1])
    return y_fp.reshape(-1, C), y_q.reshape(-1, C), C, 1


def measure_bias_error(model, images, batch_size=32, quant_max=False):
    """Read-only: the per-channel error moments of every eligible layer of a wrapped, calibrated ``model`` on ``images`` (on the model's
    device), each layer measured in the model as it stands.  -> {"images", "layers": {name: {"C", "T" (tokens per channel), "mean"
    (m_c = sum d / T), "sq_err" (sum d^2 per channel), "max_abs_fp" (max |y_fp| per channel) [, "max_abs_q" with ``quant_max``]; fp64
    host tensors [C]}}, "skipped": {name: reason}}."""
    layers = OrderedDict()
    with torch.no_grad(), _Measurement(model, images, batch_size) as run:
        todo, skipped = run.plan()
        for name, m in todo:
            acc, T = run.layer(m, quant_max=quant_max)
            acc = acc.cpu()
            layers[name] = {"C": int(acc.shape[0]), "T": T, "mean": acc[:, 0] / T, "sq_err": acc[:, 1].clone(), "max_abs_fp": acc[:, 2].clone()}
            if quant_max:
                layers[name]["max_abs_q"] = acc[:, 3].clone()
    return {"images": int(images.shape[0]), "layers": layers, "skipped": skipped}


def bias_correct_model(model, images, batch_size=32):
    """Bias correction of every eligible layer of a wrapped, calibrated ``model`` from ``images`` (on the model's device) by the
    recurrence of the module text; modes, switches and hooks are restored on every exit.  -> {"images", "layers": {name: {"C", "T",
    "mean_abs_before" (mean_c |m_c|), "sq_err_before" (sum d^2), "sq_err_after_predicted" (sum d^2 - T sum_c m_c^2: an identity for a
    fixed upstream), "max_delta" (max_c |float32(m_c)|)}}, "skipped": {name: reason}, "seconds"}."""
    t0 = time.perf_counter()
    layers = OrderedDict()
    with torch.no_grad(), _Measurement(model, images, batch_size) as run:
        todo, skipped = run.plan()
        remember_fp_biases(model)
        for name, m in todo:
            acc, T = run.layer(m)
            mean = acc[:, 0] / T
            delta = mean.to(m.bias.dtype)
            m.bias.data.add_(delta)                        # in place: the pointer the epilogues (and a captured graph) read stays
            host = torch.stack([mean, acc[:, 1], delta.double()], 1).cpu()
            before = float(host[:, 1].sum())
            layers[name] = {"C": int(host.shape[0]), "T": T, "mean_abs_before": float(host[:, 0].abs().mean()), "sq_err_before": before,
                            "sq_err_after_predicted": before - T * float((host[:, 0] ** 2).sum()),
                            "max_delta": float(host[:, 2].abs().max())}
            logging.info(f"bias correction {name}: C {host.shape[0]}, T {T}, mean |m| {layers[name]['mean_abs_before']:.4g}, "
                         f"sum d^2 {before:.6g} -> {layers[name]['sq_err_after_predicted']:.6g}")
    seconds = time.perf_counter() - t0
    logging.info(f"bias correction: {len(layers)} layers corrected, {len(skipped)} left; {seconds:.2f} s")
    return {"images": int(images.shape[0]), "layers": layers, "skipped": skipped, "seconds": seconds}


def main(argv=None):
    from .packed import BIT_PLAN_HELP, build_wrapped, load_plain, plan_kwargs, save_packed
    from .report import _dataset_images
    ap = argparse.ArgumentParser(description="Empirical bias correction of a plain calibrated checkpoint")
    ap.add_argument("--model", required=True)
    ap.add_argument("--config", required=True, help="the config file the checkpoint was calibrated with")
    ap.add_argument("--checkpoint", required=True, help="plain checkpoint written by test_quant.py (or by utils/gptq.py)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--packed", action="store_true", help="write the result in the adalog-packed-v1 format")
    ap.add_argument("--img-size", type=int, default=None)
    ap.add_argument("--depth", type=int, default=None, help="truncate the block count (as the checkpoint's model was)")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dataset", default=None, help="ImageNet root: the first --images validation images instead of a seeded randn batch")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--bit-plan", default=None, help=BIT_PLAN_HELP)
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
    res = bias_correct_model(model, images, batch_size=args.batch_size)
    if args.packed:
        save_packed(model, args.out)
    else:
        torch.save(model.state_dict(), args.out)
    before = sum(e["sq_err_before"] for e in res["layers"].values())
    after = sum(e["sq_err_after_predicted"] for e in res["layers"].values())
    print(f"{args.out}: {len(res['layers'])} layers corrected, {len(res['skipped'])} left as they were; "
          f"sum d^2 {before:.6g} -> {after:.6g} (predicted); {res['seconds']:.2f} s")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
