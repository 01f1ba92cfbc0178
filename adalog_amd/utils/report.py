"""Per-layer quantisation report of a calibrated model: which layers lose the signal, which quantisers waste or clip their codes.

``quant_report(model, images)`` runs the model twice over the images -- once in ``raw`` mode, keeping the output of every quantised
module, once in ``quant_forward`` mode -- and measures, with the streaming kernels of csrc/report.hip (ops.err_stats,
ops.uniform_code_hist, ops.log_code_hist: one pass over each tensor, nothing of its size written):

  per module (every module with a ``mode``, in named_modules() order)
    cumulative  the quant-path output against the FP-path output: what has piled up until here
    local       the module in ``raw`` mode on its quant-path inputs against its quant_forward output on them: its own share
  per quantiser (w_quantizer, a_quantizer, A_quantizer, B_quantizer)
    the code histogram of what it quantises on the quant path (weights once, activations from the module's quant-path inputs),
    clip fractions, used codes, the entropy of the stored codes, and its own SQNR err_stats(x, q(x))
  logits        per image and over the batch

The pass runs module by module (models.QF_FUSED / QF_ATTN_CORE / QF_LONG off, restored afterwards): the fused routes bypass
``module.__call__``, so hooks do not see them; their logits are pinned bit-identical to the module route by the test suite, so the
report describes them too.  Everything stays on the device until one read-back at the end.

    python -m adalog_amd.utils.report --model deit_small --config configs/4bit.py --checkpoint plain.pth [--packed] --out report.json
"""
import argparse
import json
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

from .. import backend
from .._lib import AdalogHipError
from ..ops import broadcast_layout
from ..quantizers.adaround import AdaRoundQuantizer
from ..quantizers.logarithm import AdaLogQuantizer
from ..quantizers.uniform import UniformQuantizer

QUANTIZER_ATTRS = ("w_quantizer", "a_quantizer", "A_quantizer", "B_quantizer")
MIN_INNER = 64                      # uniform_code_hist: several channels need rows of at least this many elements


# ------------------------------------------------------------------------------------------------ what can be measured
def _ineligible(q):
    """None when the quantiser's codes can be counted, else the reason its entry is null (a short string)."""
    if isinstance(q, AdaRoundQuantizer):
        if q.round_mode != "nearest" or getattr(q, "alpha", None) is not None:
            return "AdaRound rounding not committed"
    elif not isinstance(q, (UniformQuantizer, AdaLogQuantizer)):
        return f"quantiser {type(q).__name__} is neither uniform nor AdaLog"
    if int(q.n_bits) == 32:
        return "32-bit: not quantised"
    if getattr(q, "training_mode", False):
        return "quantiser in training mode"
    if not getattr(q, "inited", False):
        return "not calibrated"
    if not isinstance(q, AdaLogQuantizer) and getattr(q, "sym", False):
        return "symmetric quantiser"
    if not 2 <= int(q.n_bits) <= 8:
        return f"n_bits {q.n_bits} outside [2, 8]"
    if isinstance(q, AdaLogQuantizer) and q.scale.numel() != 1:
        return f"AdaLog quantiser with {q.scale.numel()} scales"
    return None


def _weight_view(m):
    """the view of the weight its quantiser sees (quant_weight_bias of the layer classes)"""
    w = m.weight.data
    if hasattr(m, "n_V") and hasattr(m, "crb_rows"):
        return w.view(m.n_V, m.crb_rows, -1)
    if w.dim() == 4 and m.w_quantizer.scale.dim() == 2:
        return w.view(w.shape[0], -1)
    return w


def _activation_inputs(m, args, kwargs):
    """{attr: tensor | reason} -- what each activation quantiser of the module quantises on this call"""
    out = {}
    if hasattr(m, "A_quantizer") or hasattr(m, "B_quantizer"):
        for attr, i, flag in (("A_quantizer", 0, "a_pre"), ("B_quantizer", 1, "b_pre")):
            if hasattr(m, attr):
                pre = kwargs.get(flag, args[i + 2] if len(args) > i + 2 else False)
                out[attr] = "operand quantised before the module" if pre else args[i]
        return out
    if hasattr(m, "a_quantizer"):
        x = args[0]
        if isinstance(m, nn.Conv2d) and int(m.a_quantizer.n_bits) >= 8:
            out["a_quantizer"] = "8-bit convolution input is left in fp32"
        else:
            out["a_quantizer"] = F.gelu(x) if kwargs.get("pre_gelu", False) else x
    return out


# ------------------------------------------------------------------------------------------------ device-side accumulation
class _Acc:
    """fp64 sums / maxima and int64 histograms on the device, added chunk by chunk; one read-back (``fetch``)."""

    def __init__(self):
        self.stats, self.hists, self.rows = OrderedDict(), OrderedDict(), OrderedDict()

    def stat(self, key, t):
        cur = self.stats.get(key)
        if cur is None:
            self.stats[key] = t.clone()
        else:
            cur[:, :3] += t[:, :3]
            cur[:, 3] = torch.maximum(cur[:, 3], t[:, 3])

    def stat_rows(self, key, t):
        self.rows.setdefault(key, []).append(t)

    def hist(self, key, t):
        cur = self.hists.get(key)
        if cur is None:
            self.hists[key] = t.clone()
        else:
            cur += t

    def fetch(self):
        """-> ({key: fp64 [C, 4]}, {key: int64 [bins]}) on the host, through ONE device-to-host copy"""
        stats = OrderedDict(self.stats)
        for k, parts in self.rows.items():
            stats[k] = torch.cat(parts, 0)
        flat = [t.reshape(-1) for t in stats.values()] + [h.reshape(-1).view(torch.float64) for h in self.hists.values()]
        if not flat:
            return {}, {}
        host = torch.cat(flat).cpu()
        out_s, out_h, o = OrderedDict(), OrderedDict(), 0
        for k, t in stats.items():
            out_s[k] = host[o:o + t.numel()].view(t.shape)
            o += t.numel()
        for k, h in self.hists.items():
            out_h[k] = host[o:o + h.numel()].view(torch.int64).view(h.shape)
            o += h.numel()
        return out_s, out_h


def _measure_quantiser(be, acc, key, q, x, count_hist=True):
    """histogram of the quantiser's codes over x and its own error err_stats(x, q(x)); -> None or the reason it was refused"""
    x = x.detach()
    x = x if x.is_contiguous() else x.contiguous()
    if isinstance(q, AdaLogQuantizer):
        shift, sub = q._shift_args()
        if count_hist:
            acc.hist(key, be.log_code_hist(x, q.scale.data, q.q, int(q.n_bits), shift=None if shift is None else shift.data))
        # (after reparam_bias the quantiser no longer subtracts its shift: it then answers for x + shift)
        ref = x if (shift is None or sub) else x + shift.data
    else:
        n_ch, inner = broadcast_layout(x.shape, q.scale.shape)
        if n_ch > 1 and inner < MIN_INNER:
            return f"per-channel layout ({n_ch} channels, inner {inner} < {MIN_INNER}) is not counted"
        if q.zero_point.numel() != q.scale.numel():
            return f"{q.scale.numel()} scales / {q.zero_point.numel()} zero points"
        if count_hist:
            try:
                h = be.uniform_code_hist(x, q.scale.data, q.zero_point.data, int(q.n_bits), n_ch, inner)
            except AdalogHipError as e:
                return f"refused by the kernel: {e}"
            acc.hist(key, h.sum(0) if h.shape[0] > 1 else h[0])
        ref = x
    acc.stat(key, be.err_stats(ref, q(x)))
    return None


# ------------------------------------------------------------------------------------------------ derived numbers (host)
def _err_entry(row):
    noise, signal, quant, mx = (float(v) for v in row)
    if noise == 0.0:
        sqnr = math.inf
    elif signal == 0.0:
        sqnr = -math.inf
    else:
        sqnr = 10.0 * math.log10(signal / noise)
    return {"signal": signal, "noise": noise, "quant_energy": quant, "sqnr_db": sqnr, "max_err": mx}


def _hist_entry(kind, n_bits, hist):
    """the numbers of one histogram.  uniform: [codes..., below, above]; adalog: [bins..., masked]."""
    h = [int(v) for v in hist]
    levels = 2 ** n_bits
    total = sum(h)
    if kind == "uniform":
        below, above = h[levels], h[levels + 1]
        stored = list(h[:levels])                         # what a deployment stores: clipped elements sit on the end codes
        stored[0] += below
        stored[-1] += above
        clip_low, clip_high = (below / total, above / total) if total else (0.0, 0.0)
    else:
        stored = list(h)                                  # the masked code is a stored symbol of its own
        clip_low, clip_high = (h[levels] / total if total else 0.0), None   # below the last bin; u > 1 shares bin 0 and is not told apart
    ent = 0.0
    for c in stored:
        if c:
            p = c / total
            ent -= p * math.log2(p)
    return {"kind": kind, "n_bits": n_bits, "elements": total, "hist": h, "clip_low": clip_low, "clip_high": clip_high,
            "used_codes": sum(1 for c in stored[:levels] if c), "entropy_bits": ent}


# ------------------------------------------------------------------------------------------------ the report
def quant_report(model, images, *, chunk=None, tensors=None):
    """The report of a wrapped, calibrated ``model`` on ``images`` (on the model's device) as a dict of plain Python numbers:
    {"images", "modules": {name: {"type", "cumulative", "local", "quantizers": {attr: {...} | None}, "skipped": {attr: reason}}},
    "logits": {"batch", "per_image"}}.  ``chunk``: images per forward (default: all at once); sums and histograms are added over the
    chunks, maxima maxed, so the result depends on it only through the fp64 summation order.  ``tensors``: a dict that receives the
    FP and quant-path logits of the run as device tensors (``logits_fp``, ``logits_quant``)."""
    from . import models
    be = backend.get()
    mods = [(name, m) for name, m in model.named_modules() if hasattr(m, "mode")]
    names = {id(m): name for name, m in mods}
    B = int(images.shape[0])
    step = B if not chunk else max(1, int(chunk))
    acc = _Acc()
    skipped = {name: {} for name, _ in mods}
    saved_modes = [(m, m.mode) for _, m in mods]
    saved_switches = (models.QF_FUSED, models.QF_ATTN_CORE, models.QF_LONG)
    handles = []
    fp_out, calls = {}, {}
    logits_fp, logits_q = [], []

    def set_mode(mode):
        for _, m in mods:
            m.mode = mode

    def keep_output(m, args, out):
        fp_out.setdefault(id(m), []).append(out.detach())

    def measure(m, args, kwargs, out):
        name = names[id(m)]
        i = calls.get(id(m), 0)
        calls[id(m)] = i + 1
        acc.stat((name, "cumulative"), be.err_stats(fp_out[id(m)][i], out))
        m.mode = "raw"
        try:
            raw = m.forward(*args, **kwargs)              # (forward, not __call__: no hook runs)
        finally:
            m.mode = "quant_forward"
        acc.stat((name, "local"), be.err_stats(raw, out))
        for attr, x in _activation_inputs(m, args, kwargs).items():
            q = getattr(m, attr)
            why = x if isinstance(x, str) else (_ineligible(q) or _measure_quantiser(be, acc, (name, attr), q, x))
            if why is not None:
                skipped[name][attr] = why

    try:
        models.QF_FUSED = models.QF_ATTN_CORE = models.QF_LONG = False
        with torch.no_grad():
            # weights: counted once
            for name, m in mods:
                if hasattr(m, "w_quantizer") and isinstance(getattr(m, "weight", None), torch.Tensor):
                    why = _ineligible(m.w_quantizer) or _measure_quantiser(be, acc, (name, "w_quantizer"), m.w_quantizer, _weight_view(m))
                    if why is not None:
                        skipped[name]["w_quantizer"] = why
            for s in range(0, B, step):
                x = images[s:s + step]
                fp_out.clear()
                calls.clear()
                set_mode("raw")
                handles = [m.register_forward_hook(keep_output) for _, m in mods]
                y_fp = model(x)
                for h in handles:
                    h.remove()
                set_mode("quant_forward")
                handles = [m.register_forward_hook(measure, with_kwargs=True) for _, m in mods]
                y_q = model(x)
                for h in handles:
                    h.remove()
                handles = []
                acc.stat(("logits", "batch"), be.err_stats(y_fp, y_q))
                acc.stat_rows(("logits", "per_image"), be.err_stats(y_fp, y_q, n_channels=int(y_fp.shape[0])))
                logits_fp.append(y_fp)
                logits_q.append(y_q)
    finally:
        for h in handles:
            h.remove()
        for m, mode in saved_modes:
            m.mode = mode
        models.QF_FUSED, models.QF_ATTN_CORE, models.QF_LONG = saved_switches
        fp_out.clear()

    if tensors is not None:
        tensors["logits_fp"], tensors["logits_quant"] = torch.cat(logits_fp, 0), torch.cat(logits_q, 0)
    stats, hists = acc.fetch()                            # the one read-back
    report = OrderedDict(images=B, chunk=step, modules=OrderedDict())
    for name, m in mods:
        entry = OrderedDict(type=type(m).__name__)
        for which in ("cumulative", "local"):
            entry[which] = _err_entry(stats[(name, which)][0]) if (name, which) in stats else None
        entry["quantizers"], entry["skipped"] = OrderedDict(), skipped[name]
        for attr in QUANTIZER_ATTRS:
            if not hasattr(m, attr):
                continue
            key = (name, attr)
            if key in skipped[name] or key not in hists or key not in stats:
                entry["quantizers"][attr] = None
                skipped[name].setdefault(attr, "the module's forward did not reach this quantiser")
                continue
            q = getattr(m, attr)
            e = _hist_entry("adalog" if isinstance(q, AdaLogQuantizer) else "uniform", int(q.n_bits), hists[key].tolist())
            e["channels"] = int(q.scale.numel())
            e.update(_err_entry(stats[key][0]))
            entry["quantizers"][attr] = e
        report["modules"][name] = entry
    report["logits"] = OrderedDict(batch=_err_entry(stats[("logits", "batch")][0]),
                                   per_image=[_err_entry(r) for r in stats[("logits", "per_image")]])
    return report


# ------------------------------------------------------------------------------------------------ command line
def _fmt_db(v):
    return "    inf" if v == math.inf else "   -inf" if v == -math.inf else f"{v:7.2f}"


def format_table(report):
    """one line per module (both SQNRs), one per quantiser (clip fractions, used codes) -- what the command line prints"""
    lines = [f"{'module':<44} {'cumulative dB':>13} {'local dB':>9} {'max err':>10}"]
    for name, e in report["modules"].items():
        cu, lo = e["cumulative"], e["local"]
        lines.append(f"{name:<44} {_fmt_db(cu['sqnr_db']):>13} {_fmt_db(lo['sqnr_db']):>9} {cu['max_err']:10.3e}")
        for attr, qe in e["quantizers"].items():
            if qe is None:
                lines.append(f"    {attr:<14} null: {e['skipped'].get(attr, '')}")
                continue
            hi = "     -" if qe["clip_high"] is None else f"{qe['clip_high']:6.4f}"
            lines.append(f"    {attr:<14} {qe['kind']:<7} {qe['n_bits']}b  clip_low {qe['clip_low']:6.4f}  clip_high {hi}  "
                         f"used {qe['used_codes']:>3}/{2 ** qe['n_bits']:<3}  entropy {qe['entropy_bits']:5.2f}b  sqnr {_fmt_db(qe['sqnr_db'])} dB")
    lg = report["logits"]["batch"]
    lines.append(f"{'logits (' + str(report['images']) + ' images)':<44} {_fmt_db(lg['sqnr_db']):>13} {'':>9} {lg['max_err']:10.3e}")
    return "\n".join(lines)


def _dataset_images(root, model_name, n, device):
    from .datasets import ViTImageNetLoaderGenerator
    loader = ViTImageNetLoaderGenerator(root, n, 0, kwargs={"model": model_name}).val_loader()
    return next(iter(loader))[0][:n].to(device)


def main(argv=None):
    from .packed import BIT_PLAN_HELP, build_wrapped, load_packed, load_plain, plan_kwargs
    ap = argparse.ArgumentParser(description="Per-layer quantisation report of a calibrated checkpoint")
    ap.add_argument("--model", required=True)
    ap.add_argument("--config", required=True, help="the config file the checkpoint was calibrated with")
    ap.add_argument("--checkpoint", required=True, help="plain checkpoint of test_quant.py, or a packed one with --packed")
    ap.add_argument("--packed", action="store_true", help="the checkpoint is in the adalog-packed-v1 format")
    ap.add_argument("--img-size", type=int, default=None)
    ap.add_argument("--depth", type=int, default=None, help="truncate the block count (as the checkpoint's model was)")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=None, help="images per forward (default: all at once)")
    ap.add_argument("--dataset", default=None, help="ImageNet root: the first --images validation images instead of a seeded randn batch")
    ap.add_argument("--out", default=None, help="write the full report as JSON")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--bit-plan", default=None, help=BIT_PLAN_HELP)
    args = ap.parse_args(argv)
    device = torch.device(args.device)
    model = build_wrapped(args.model, args.config, device, img_size=args.img_size, depth=args.depth, **plan_kwargs(args.bit_plan))
    model = (load_packed if args.packed else load_plain)(model, args.checkpoint, device)
    if args.dataset:
        images = _dataset_images(args.dataset, args.model, args.images, device)
    else:
        size = args.img_size or getattr(getattr(model, "patch_embed", None), "img_size", (224, 224))[0]
        images = torch.randn(args.images, 3, size, size, generator=torch.Generator().manual_seed(args.seed)).to(device)
    report = quant_report(model, images, chunk=args.chunk)
    print(format_table(report))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
        print(f"{args.out}: {len(report['modules'])} modules")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
