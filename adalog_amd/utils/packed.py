"""Packed low-bit checkpoints (format ``adalog-packed-v1``): the calibrated weights as the integers a deployment stores.

``save_model`` of test_quant.py writes the plain state_dict -- fp32 weights plus quantiser parameters, as large as the FP model.
Here the weight of every layer with a calibrated asymmetric uniform weight quantiser is stored as its ``b``-bit codes
q = clamp(rne(w / s) + rne(z), 0, 2^b - 1), 32 codes per group of ``b`` 32-bit words (csrc/packed.hip), about 32 / b times smaller;
everything else of the state_dict is stored unchanged.  ``load_packed`` rebuilds the weight as (q - rne(z)) * s.  That value
quantises to the same code again (|q - rne(z)| <= 255, so fl(fl(n s) / s) is within a few 2^-24 |n| of n), hence the fake-quantised
weight and every packed operand image of it are bit for bit those of the calibrated model: ``quant_forward`` computes the same
logits on every route.

    python -m adalog_amd.utils.packed --model deit_small --config configs/4bit.py --checkpoint plain.pth --out packed.pth

``ADALOG_PACKED_DIRECT=1``: ``load_packed`` also installs the operand image quant_forward would pack on its first call, unpacked
from the codes, in each Linear's packed-weight cache.
"""
import argparse
import importlib.util
import logging
import os
from collections import OrderedDict

import torch
from torch import nn

from .. import backend, parallel
from ..ops import BF16, I8, pad_k
from ..quantizers.adaround import AdaRoundQuantizer
from ..quantizers.uniform import UniformQuantizer

FORMAT = "adalog-packed-v1"


def _rows_cols(module):
    w = module.weight
    return int(w.shape[0]), int(w.numel() // w.shape[0])


def _ineligible(module):
    """None when the module's weight is stored as codes, else the reason it stays fp32 (a short string)."""
    wq = module.w_quantizer
    if isinstance(wq, AdaRoundQuantizer):
        if wq.round_mode != "nearest" or getattr(wq, "alpha", None) is not None:
            return "AdaRound rounding not committed"
    elif not isinstance(wq, UniformQuantizer):
        return f"weight quantiser {type(wq).__name__} is not uniform"
    if getattr(wq, "sym", False):
        return "symmetric quantiser"
    if getattr(wq, "training_mode", False):
        return "quantiser in training mode"
    if not getattr(wq, "inited", False) or not getattr(module, "calibrated", False):
        return "not calibrated"
    if not 2 <= int(wq.n_bits) <= 8:
        return f"n_bits {wq.n_bits} outside [2, 8]"
    rows, _ = _rows_cols(module)
    n_s, n_z = wq.scale.numel(), wq.zero_point.numel()
    if n_s != n_z or n_s not in (1, rows):
        return f"{n_s} scales / {n_z} zero points for {rows} rows"
    return None


def _quantised_layers(model):
    return [(name, m) for name, m in model.named_modules()
            if hasattr(m, "w_quantizer") and isinstance(getattr(m, "weight", None), torch.Tensor)]


def packed_state_dict(model):
    """{"format", "meta", "state"}: the model's state_dict with ``<name>.weight`` of every eligible layer replaced by
    ``<name>.weight_packed`` (int32 [rows, b * ceil(cols / 32)], on the CPU).  meta["packed"][name] = {n_bits, rows, cols, per_row,
    shape}; meta["kept_fp32"][name] = why a layer with a weight quantiser keeps its fp32 weight."""
    be = backend.get()
    state = model.state_dict()
    packed, kept, fp32_bytes, new_bytes = {}, {}, 0, 0
    swap = {}
    for name, m in _quantised_layers(model):
        key = (name + "." if name else "") + "weight"
        fp32_bytes += m.weight.numel() * m.weight.element_size()
        why = _ineligible(m)
        if why is not None:
            kept[name] = why
            new_bytes += m.weight.numel() * m.weight.element_size()
            continue
        wq = m.w_quantizer
        rows, cols = _rows_cols(m)
        with torch.no_grad():
            codes = be.pack_codes(m.weight.data.reshape(rows, cols), wq.scale.data.reshape(-1), wq.zero_point.data.reshape(-1),
                                  int(wq.n_bits)).cpu()
        swap[key] = codes
        new_bytes += codes.numel() * codes.element_size()
        packed[name] = {"n_bits": int(wq.n_bits), "rows": rows, "cols": cols, "per_row": bool(wq.scale.numel() == rows and rows > 1),
                        "shape": [int(d) for d in m.weight.shape]}
    out = OrderedDict()
    for k, v in state.items():
        if k in swap:
            out[k + "_packed"] = swap[k]
        else:
            out[k] = v
    meta = {"packed": packed, "kept_fp32": kept, "weight_bytes": {"fp32": int(fp32_bytes), "packed": int(new_bytes)}}
    return {"format": FORMAT, "meta": meta, "state": out}


def save_packed(model, path):
    """Write packed_state_dict(model) to ``path`` (rank 0 only, like save_model); returns what was built."""
    obj = packed_state_dict(model)
    if parallel.rank() == 0:
        logging.info(f"Saving packed checkpoint to {path}")
        torch.save(obj, path)
    return obj


def prepare_for_load(model):
    """A freshly wrapped model made ready to receive a calibrated state_dict, as load_model of test_quant.py prepares it: every
    quantised module calibrated and in quant_forward mode, quantisers initialised, the bias a LayerNorm fold gave to Swin's
    bias-free ``reduction`` layers created."""
    for name, module in model.named_modules():
        if hasattr(module, 'mode'):
            module.calibrated = True
            module.mode = 'quant_forward'
        if isinstance(module, nn.Linear) and 'reduction' in name:
            module.bias = nn.Parameter(torch.zeros(module.out_features))
        for attr in ['a_quantizer', 'w_quantizer', 'A_quantizer', 'B_quantizer']:
            if hasattr(module, attr):
                getattr(module, attr).inited = True
    return model


def _install_direct(module, codes, cols):
    """ADALOG_PACKED_DIRECT: the operand image quant_forward's _pack_w_cached() would build on its first call, from the codes."""
    from ..quant_layers.linear import AsymmetricallyBatchingQuantLinear, PostGeluLogBasedBatchingQuantLinear
    if not isinstance(module, AsymmetricallyBatchingQuantLinear):
        return False
    wq = module.w_quantizer
    if isinstance(module, PostGeluLogBasedBatchingQuantLinear):
        # fc2 reads a bf16 image; with the shift not yet folded into the bias it also wants the row sums: left to the first forward
        if module.a_quantizer._shift_args()[1] or not wq.codes_fit(-256, 256):
            return False
        dt = BF16
    else:
        if wq.n_bits > 7 or not wq.codes_fit(-128, 127):
            return False
        dt = I8
    Kp = pad_k(cols, dt)
    img = backend.get().unpack_codes(codes, cols, wq.scale.data.reshape(-1), wq.zero_point.data.reshape(-1), int(wq.n_bits), dt, Kp=Kp)
    img = img.view(1, 1, img.shape[0], Kp)
    img.k_valid = cols
    module.__dict__["_wp_cache"] = (module._wp_cache_key(dt, False), img)
    return True


def load_packed(model, path, device):
    """Load a packed checkpoint into a freshly wrapped model: the state non-strictly, every packed weight unpacked to fp32 into
    ``module.weight`` with the module's own (loaded) scale and zero point.  Returns the model in quant_forward mode."""
    obj = torch.load(path, map_location="cpu")
    fmt = obj.get("format") if isinstance(obj, dict) else None
    if fmt != FORMAT:
        raise ValueError(f"{path}: not an {FORMAT} checkpoint (format: {fmt!r})")
    meta = obj["meta"]["packed"]
    state = OrderedDict((k, v) for k, v in obj["state"].items() if not k.endswith("weight_packed"))
    prepare_for_load(model)
    result = model.load_state_dict(state, strict=False)
    expected = {(n + "." if n else "") + "weight" for n in meta}
    result = result._replace(missing_keys=[k for k in result.missing_keys if k not in expected])
    logging.info(str(result))
    model.to(device)
    model.eval()
    be = backend.get()
    modules = dict(model.named_modules())
    direct = os.environ.get("ADALOG_PACKED_DIRECT", "0") == "1"
    for name, info in meta.items():
        m = modules.get(name)
        if m is None or not hasattr(m, "w_quantizer"):
            raise ValueError(f"{path}: packed weight for '{name}', which is not a quantised layer of this model")
        wq = m.w_quantizer
        rows, cols, n_bits = int(info["rows"]), int(info["cols"]), int(info["n_bits"])
        if list(m.weight.shape) != list(info["shape"]) or int(wq.n_bits) != n_bits:
            raise ValueError(f"{path}: '{name}' was packed as {info['shape']} at {n_bits} bits, the model has "
                             f"{list(m.weight.shape)} at {wq.n_bits} bits")
        codes = obj["state"][(name + "." if name else "") + "weight_packed"].to(device)
        with torch.no_grad():
            w = be.unpack_codes(codes, cols, wq.scale.data.reshape(-1), wq.zero_point.data.reshape(-1), n_bits)
            m.weight.data.copy_(w.reshape(m.weight.shape))
        if hasattr(m, "invalidate_packed_weight"):
            m.invalidate_packed_weight()
        for q in (wq, getattr(m, "a_quantizer", None)):
            if hasattr(q, "forget_codes_fit"):
                q.forget_codes_fit()
        if direct:
            _install_direct(m, codes, cols)
    return model


def load_plain(model, path, device):
    """load_model of test_quant.py: a plain calibrated state_dict into a freshly wrapped model."""
    prepare_for_load(model)
    logging.info(str(model.load_state_dict(torch.load(path, map_location="cpu"), strict=False)))
    model.to(device)
    model.eval()
    return model


BIT_PLAN_HELP = "adalog-bitplan-v1 file of utils/bitplan.py: the per-layer weight widths the checkpoint was calibrated with"


def load_bit_plan(path):
    """{module name: bits} of an adalog-bitplan-v1 file (utils/bitplan.py), or of a bare JSON object of names and widths"""
    import json
    with open(path) as f:
        obj = json.load(f)
    if isinstance(obj, dict) and "format" in obj:
        if obj["format"] != "adalog-bitplan-v1" or not isinstance(obj.get("plan"), dict):
            raise ValueError(f"{path}: not an adalog-bitplan-v1 file")
        obj = obj["plan"]
    if not isinstance(obj, dict):
        raise ValueError(f"{path}: a bit plan is a JSON object of module names and widths")
    return {str(k): int(v) for k, v in obj.items()}


def plan_kwargs(path):
    """build_wrapped's keyword for a --bit-plan flag: none when the flag was not given"""
    return {"bit_plan": load_bit_plan(path)} if path else {}


def build_wrapped(model_name, config_path, device, img_size=None, depth=None, bit_plan=None):
    """The model of the zoo wrapped for loading a calibrated checkpoint (test_quant.py with --load-calibrate-checkpoint).
    ``bit_plan``: {module name: bits}, the cfg.w_bit_plan of a mixed-width checkpoint (wrap_modules_in_net)."""
    from .models import create_model
    from .wrap_net import wrap_modules_in_net
    spec = importlib.util.spec_from_file_location("adalog_packed_cfg", config_path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = mod.Config()
    if bit_plan is not None:
        cfg.w_bit_plan = dict(bit_plan)
    model = create_model(model_name, depth=depth, img_size=img_size)
    model = wrap_modules_in_net(model.to(device).eval(), cfg, reparam=False)
    return model.to(device).eval()


def main(argv=None):
    ap = argparse.ArgumentParser(description="Convert a plain calibrated checkpoint into a packed one (adalog-packed-v1)")
    ap.add_argument("--model", required=True)
    ap.add_argument("--config", required=True, help="the config file the checkpoint was calibrated with")
    ap.add_argument("--checkpoint", required=True, help="plain checkpoint written by test_quant.py")
    ap.add_argument("--out", required=True)
    ap.add_argument("--img-size", type=int, default=None)
    ap.add_argument("--depth", type=int, default=None, help="truncate the block count (as the checkpoint's model was)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--bit-plan", default=None, help=BIT_PLAN_HELP)
    args = ap.parse_args(argv)
    device = torch.device(args.device)
    model = build_wrapped(args.model, args.config, device, img_size=args.img_size, depth=args.depth, **plan_kwargs(args.bit_plan))
    model = load_plain(model, args.checkpoint, device)
    obj = save_packed(model, args.out)
    wb = obj["meta"]["weight_bytes"]
    print(f"{args.out}: weight entries {wb['fp32']} bytes -> {wb['packed']} bytes "
          f"({len(obj['meta']['packed'])} packed, {len(obj['meta']['kept_fp32'])} kept fp32)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
