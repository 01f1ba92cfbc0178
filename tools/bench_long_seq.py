"""Times quant_forward of a ViT / DeiT at an image size whose sequence is longer than 256 tokens (384 px: 577) on four routes: module by
module (ADALOG_QF_FUSED=0), the default (long rows off: the attention declines the fused route), long rows on (ADALOG_QF_LONG=1:
utils/models.py QF_LONG, csrc/operand.hip adalog_softmax_adalog_pack_long_bf16) and long rows on with the one-launch attention core
(ADALOG_QF_ATTN_CORE=1 as well: csrc/attn_core.hip adalog_attn_core_long).  Captured-graph replay (utils/graph_forward.py), all four
routes in ONE process and interleaved round by round, so that clock and box drift hit every column alike.

Random-init weights; the quantisers of the blocks get min/max parameters from a raw forward of a few synthetic images instead of a
calibration (timing only; the patch embedding and the head stay in raw mode on every route).  Device events around each forward after
warm-up.  Prints, per route: kernels per forward (torch.profiler), the median ms per forward over all repetitions, the spread of the
per-round medians (run-to-run spread inside the process), and whether the logits equal the module route's.

    python tools/bench_long_seq.py [--model deit_small] [--img-size 384] [--batch 32] [--rounds 5] [--reps 10] [--bits 4]
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

from bench_swin_qf import _cfg, kernels, time_ms  # noqa: E402

GELU_SHIFT = 0.16997124254703522
ROUTES = (("module", dict(QF_FUSED=False, QF_LONG=False, QF_ATTN_CORE=False)),
          ("long_off", dict(QF_FUSED=True, QF_LONG=False, QF_ATTN_CORE=False)),
          ("long_on", dict(QF_FUSED=True, QF_LONG=True, QF_ATTN_CORE=False)),
          ("long_on_core", dict(QF_FUSED=True, QF_LONG=True, QF_ATTN_CORE=True)))


def _minmax(t, bits, per=None):
    if per is None:
        mn, mx = t.min(), t.max()
    else:
        red = [d for d in range(t.dim()) if d not in per]
        mn, mx = t.amin(dim=red, keepdim=True), t.amax(dim=red, keepdim=True)
    s = (mx - mn).clamp_min(1e-6) / (2 ** bits - 1)
    return s, torch.round(-mn / s).clamp(0, 2 ** bits - 1)


def _arm(q, s, z):
    q.scale.data.copy_(s.reshape(q.scale.shape))
    q.zero_point.data.copy_(z.reshape(q.zero_point.shape))
    q.inited = True
    q._zp_on_grid = True
    if hasattr(q, "forget_codes_fit"):
        q.forget_codes_fit()


def armed(name, img_size, bits, n_images=2):
    """the wrapped model with every block's quantisers set from the ranges of a raw forward, blocks in quant_forward mode"""
    from adalog_amd.utils.models import Block, create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net
    torch.manual_seed(0)
    model = wrap_modules_in_net(create_model(name, img_size=img_size).eval(), _cfg(bits)).cuda()
    x = torch.randn(n_images, 3, img_size, img_size, generator=torch.Generator().manual_seed(1)).cuda()
    blocks = [m for m in model.modules() if isinstance(m, Block)]
    seen, hooks = {}, []
    for i, b in enumerate(blocks):
        for nm, mod in (("qkv", b.attn.qkv), ("proj", b.attn.proj), ("fc1", b.mlp.fc1), ("fc2", b.mlp.fc2)):
            hooks.append(mod.register_forward_pre_hook(lambda m, a, k=(i, nm): seen.__setitem__(k, a[0])))
        for nm, mod in (("mm1", b.attn.matmul1), ("mm2", b.attn.matmul2)):
            hooks.append(mod.register_forward_pre_hook(lambda m, a, k=(i, nm): seen.__setitem__(k, a)))
    with torch.no_grad():
        model(x)
    for h in hooks:
        h.remove()
    for i, b in enumerate(blocks):
        attn, mlp = b.attn, b.mlp
        for lay in (attn.qkv, attn.proj, mlp.fc1, mlp.fc2):
            _arm(lay.w_quantizer, *_minmax(lay.weight.data.view(lay.n_V, lay.crb_rows, -1), bits, per=(0, 1)))
        for nm, lay in (("qkv", attn.qkv), ("proj", attn.proj), ("fc1", mlp.fc1)):
            _arm(lay.a_quantizer, *_minmax(seen[(i, nm)], bits))
        m1, m2 = attn.matmul1, attn.matmul2
        hp = (1,) if m1._heads() > 1 else None
        _arm(m1.A_quantizer, *_minmax(seen[(i, "mm1")][0], bits, per=hp))
        _arm(m1.B_quantizer, *_minmax(seen[(i, "mm1")][1], bits, per=hp))
        _arm(m2.B_quantizer, *_minmax(seen[(i, "mm2")][1], bits, per=hp))
        m2.A_quantizer.q.fill_(29)
        m2.A_quantizer.update_table(29)
        m2._q_host = None
        aq = mlp.fc2.a_quantizer
        aq.shift.data.fill_(GELU_SHIFT)
        aq.scale.data.fill_((float(seen[(i, "fc2")].max()) + GELU_SHIFT) * 0.9)
        aq.q.fill_(41)
        aq.update_table(41)
        aq.inited = True
        mlp.fc2._q_host = None
        for m in b.modules():
            if hasattr(m, "calibrated"):
                m.calibrated = True
                m.mode = "quant_forward"
    return model, len(blocks)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="deit_small")
    ap.add_argument("--img-size", type=int, default=384)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bits", type=int, default=4)
    args = ap.parse_args()
    from adalog_amd.utils import models as M
    from adalog_amd.utils.graph_forward import GraphedForward
    model, n_blocks = armed(args.model, args.img_size, args.bits)
    tokens = model.patch_embed.num_patches + 1
    x = torch.randn(args.batch, 3, args.img_size, args.img_size, generator=torch.Generator().manual_seed(2)).cuda()
    eager = torch.no_grad()(model)
    rec = {"model": args.model, "img_size": args.img_size, "tokens": tokens, "batch": args.batch, "bits": args.bits, "blocks": n_blocks}
    old = {k: getattr(M, k) for k in ROUTES[0][1]}
    graphs, ys, times = {}, {}, {}

    def switch(pos):
        for k, v in pos.items():
            setattr(M, k, v)
    try:
        for route, pos in ROUTES:                              # capture one graph per route (the route is fixed at capture)
            switch(pos)
            ys[route] = eager(x).clone()
            graphs[route] = GraphedForward(model)
            ys[route, "graph"] = graphs[route](x).clone()
            rec[f"kernels_{route}"] = kernels(eager, x)
            times[route] = []
        for _ in range(args.rounds):
            for route, pos in ROUTES:
                switch(pos)
                times[route].append(time_ms(graphs[route], x, args.reps))
    finally:
        switch(old)
    print(f"{args.model} at {args.img_size} px: {tokens} tokens, {args.batch} images, {n_blocks} blocks, graph replay, "
          f"{args.rounds} rounds x {args.reps} forwards")
    for route, _ in ROUTES:
        rounds = [statistics.median(r) for r in times[route]]
        allv = [v for r in times[route] for v in r]
        rec[route] = {"ms_median": statistics.median(allv), "round_medians_min": min(rounds), "round_medians_max": max(rounds),
                      "ms_min": min(allv), "logits_equal_module": bool(torch.equal(ys[route], ys["module"])),
                      "graph_equals_eager": bool(torch.equal(ys[route, "graph"], ys[route]))}
    for route, _ in ROUTES:
        r = rec[route]
        print(f"  {route:13s} {rec[f'kernels_{route}']:5d} kernels  {r['ms_median']:9.3f} ms [{r['round_medians_min']:.3f}, "
              f"{r['round_medians_max']:.3f}]  {r['ms_median'] / rec['long_off']['ms_median']:.3f} x long_off  "
              f"logits == module: {r['logits_equal_module']}, graph == eager: {r['graph_equals_eager']}")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
