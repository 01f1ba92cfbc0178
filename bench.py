#!/usr/bin/env python3
"""Benchmark of the AdaLog calibration hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One *step* = one complete calibration (QuantCalibrator.batching_quant_calib: capture + every module's FPCS search) of
BASELINE.json configs[1]: deit_small, W4A4 (configs/4bit.py), 32 synthetic 224x224 calibration images PER GPU
(weak scaling: the global calibration set is 32*N images sharded by rank, scores all-reduced over RCCL).
Inputs (images, random-init weights) are resident in HBM before the timed region.  Rank 0 prints ONE JSON line:
  value      = calibration images per second, whole job  (= 32*N*K / wall, wall = max over ranks); ms_per_step = wall / K
  roofline   = the dominant scoring kernel (largest summed launch time; the library reports which kernel each launch used):
               algorithmic flops of its launches / their summed duration, measured live with events on the launch stream
               during the timed steps; config.scoring_kernels lists every kernel the same way
A plain run does only that: set-up, W warm-up steps, the K timed steps, the dump, the line.  --full adds
  config.other_schedule = the same K steps timed again on the other schedule (not with --no-rerun-all)
  hbm_kernels = the HBM-class kernels of the path (fake-quant, self-MSE scoring, quantile, packing) against 8 TB/s
  brecq      = BRECQ iterations per second on one block (bounded sample)
  quant_forward = the calibrated model's quant_forward pass (graph replay, eager, raw FP32)
  cpu_baseline = the CPU oracle (a port of the reference's algorithm, oracle/) timed on the host cores on a bounded
               sample of the same workload and scaled to images/s with the work model of BASELINE.md section 2
(the last four on one GPU only, and not with --no-cpu-baseline).
--dump-outputs DIR writes what the last timed step computed (dump_outputs) so that two builds can be compared.
"""
import argparse
import copy
import importlib.util
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_TOPS = {0: 5000.0, 1: 2500.0, 2: 157.3, 3: 5000.0, 4: 2500.0}      # dense MFMA peaks, TFLOP/s (MI355X_MICROARCH.md): i8 = fp8 = 2x bf16; 4 = bf16 MFMA fed from fp8 storage
DT_NAME = {0: "i8", 1: "bf16", 2: "f32", 3: "fp8", 4: "bf16xfp8"}


def load_cfg(bits):
    spec = importlib.util.spec_from_file_location(f"cfg{bits}", os.path.join(ROOT, "configs", f"{bits}bit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Config()


class GemmProfiler:
    """Collects the event pairs adalog_amd.ops records around every scoring launch (on the launch stream) together with
    the true (un-padded) K of the operands and the name of the kernel the library picked (adalog_last_kernel), so that
    ALGORITHMIC flops = 2*M*N*K*C*G are divided by kernel time, per kernel."""

    def __init__(self, ops):
        self.ops = ops

    def start(self):
        self.ops.GEMM_EVENTS = []

    def stop(self):
        ev, self.ops.GEMM_EVENTS = self.ops.GEMM_EVENTS, None
        torch.cuda.synchronize()
        by, shapes, kern = {}, {}, {}
        for dt, M, N, K, C, G, s, e, name in ev:
            ms = s.elapsed_time(e)
            for d, key in ((by, dt), (shapes, (dt, M, N, K, C, G, name)), (kern, (name, dt))):
                b = d.setdefault(key, [0.0, 0.0, 0])
                b[0] += 2.0 * M * N * K * C * G
                b[1] += ms
                b[2] += 1
        self.shapes, self.kernels = shapes, kern
        return by

    def top_shapes(self, steps, n=14):
        """Per-shape totals (rows x columns x K, candidates, groups), largest time first."""
        rows = sorted(self.shapes.items(), key=lambda kv: -kv[1][1])[:n]
        return [{"kernel": k[6], "dtype": DT_NAME[k[0]], "M": k[1], "N": k[2], "K": k[3], "cands": k[4], "groups": k[5],
                 "launches_per_step": v[2] / steps, "ms_per_step": round(v[1] / steps, 2),
                 "tflops": round(v[0] / (v[1] * 1e-3) / 1e12, 1)} for k, v in rows]

    @staticmethod
    def template_of(label):
        """`k_gemm_slab128_gen<fp8>` / `k_gemm_slab_wgen<fp8>` -> `k_gemm_slab<fp8>`: the generated-operand and 128-column forms are instantiations of
        one kernel template; `k_act_fused_asm<12,4,bf16>` -> `k_act_fused_asm<bf16>`."""
        import re
        head, _, tail = label.partition("<")
        head = head.replace("128", "").replace("_wgen", "").replace("_gen", "")
        args = tail.rstrip(">").split(",")
        return f"{head}<{args[-1]}>" if tail else head

    def by_template(self, steps):
        """Kernel TEMPLATES, largest summed launch time first, each with its instantiations as sub-rows."""
        groups = {}
        for (name, dt), v in self.kernels.items():
            g = groups.setdefault((self.template_of(name), dt), {"flops": 0.0, "ms": 0.0, "n": 0, "rows": []})
            g["flops"] += v[0]; g["ms"] += v[1]; g["n"] += v[2]
            g["rows"].append({"kernel": name, "launches_per_step": v[2] / steps, "ms_per_step": round(v[1] / steps, 2),
                              "frac_of_peak": round(v[0] / (v[1] * 1e-3) / 1e12 / PEAK_TOPS[dt], 3)})
        return sorted(groups.items(), key=lambda kv: -kv[1]["ms"])

    def by_kernel(self, steps):
        rows = sorted(self.kernels.items(), key=lambda kv: -kv[1][1])
        return [{"kernel": k[0], "dtype": DT_NAME[k[1]], "launches_per_step": v[2] / steps, "ms_per_step": round(v[1] / steps, 2),
                 "tflops": round(v[0] / (v[1] * 1e-3) / 1e12, 1), "frac_of_peak": round(v[0] / (v[1] * 1e-3) / 1e12 / PEAK_TOPS[k[1]], 3)}
                for k, v in rows]


def pmc_traffic(kernel, workload_is_default):
    """HBM bytes per launch of `kernel`, REPLAYED from the committed PMC passes of this same command
    (tools/pmc_bench.sh -> profiles/r0N_pmc_bench_traffic.json, the latest round: FETCH_SIZE x2 per the gfx950 correction + WRITE_SIZE, averaged
    over every dispatch of one calibration step).  None for any other workload or when the summary is absent."""
    if not workload_is_default:
        return None
    import glob
    found = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_pmc_bench_traffic.json")))
    path = found[-1] if found else os.path.join(ROOT, "profiles", "r03_pmc_bench_traffic.json")     # the latest round's passes
    try:
        with open(path) as f:
            rows = json.load(f)
    except OSError:
        return None
    def matches(pmc_name):
        """the library's kernel label (adalog_note_kernel) against the demangled instantiation name rocprofv3 reports"""
        base, _, targs = pmc_name.partition("<")
        targs = [a.strip() for a in targs.rstrip(">").split(",")] if targs else []
        label, _, ldt = kernel.partition("<")
        ldt = ldt.rstrip(">")
        if label.startswith("k_gemm_slab"):                        # k_gemm_slab<NREF, ROWS, DT, NB, GEN>
            if base != "k_gemm_slab" or len(targs) < 5:
                return False
            wgen, gen, nb128 = label.endswith("_wgen"), label.endswith("_gen"), "128" in label
            # GEN = true: ROWS = true is the activation form (`_gen`), ROWS = false the weight form (`_wgen`)
            return ((targs[4] == "true") == (gen or wgen) and (not (gen or wgen) or (targs[1] == "true") == gen)
                    and (targs[3] == "4") == nb128 and targs[2] == {"fp8": "3", "i8": "0"}.get(ldt, targs[2]))
        return pmc_name.startswith(label)
    tot, n = 0.0, 0
    for name, v in rows.items():
        if matches(name) and v.get("hbm_read_bytes_per_launch") is not None:
            tot += (v["hbm_read_bytes_per_launch"] + (v.get("hbm_write_bytes_per_launch") or 0.0)) * v["launches"]
            n += v["launches"]
    return tot / n if n else None


def hbm_kernels(ops, dev):
    """Class-E (HBM-bound) kernels of the path at the deit_small / 32-image layer shapes: algorithmic bytes over the
    event time per launch, against 8 TB/s.  Every launch of a timed batch reads a DIFFERENT copy of its input: the copies
    together (>= 620 MB) exceed the 256 MiB Infinity Cache, so a launch streams from HBM (round 2 looped over one 77 MB working
    set -- cache-resident; MI355X_MICROARCH.md: scale past L3)."""
    NCOPY = 16

    def timeit(fn, reps=3):
        """median over `reps` of the time of NCOPY back-to-back launches (one per input copy) / NCOPY"""
        for j in range(NCOPY):
            fn(j)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for j in range(NCOPY):
                fn(j)
            b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / NCOPY)
        return sorted(ts)[len(ts) // 2]
    g = torch.Generator().manual_seed(3)
    M = 32 * 197
    out = []
    x0 = torch.randn(M, 1536, generator=g).to(dev)                         # fc2 input sized tensor (38.7 MB)
    xs = [x0 + 0.001 * j for j in range(NCOPY)]                            # 16 x 38.7 MB = 620 MB
    xgs = [torch.nn.functional.gelu(v) for v in xs]
    sc1, zp1 = torch.tensor([0.21], device=dev), torch.tensor([7.0], device=dev)
    P = 128
    cs = (torch.rand(P, 1, generator=g) * 0.2 + 0.1).to(dev)
    cz = torch.randint(4, 12, (P, 1), generator=g).float().to(dev)
    Ws = [(torch.randn(1536, 384, generator=g) * 0.05).to(dev) for _ in range(NCOPY)]
    csw = (torch.rand(P, 1536, generator=g) * 0.01 + 0.005).to(dev)
    czw = torch.randint(4, 12, (P, 1536), generator=g).float().to(dev)
    q = torch.tensor([37], dtype=torch.int64, device=dev)
    from adalog_amd.quantizers.logarithm import AdaLogQuantizer
    t1, t2 = AdaLogQuantizer.make_tables(37, 8)                             # 4 bit: n_levels = 8, 16-entry tables
    t1, t2 = t1.to(dev), t2.to(dev)
    shift = torch.tensor([0.17], device=dev)
    nb = x0.numel() * 4
    sps = [ops.sorted_prefix(v.view(1, -1)) for v in xs[:4]]
    rows = [
        ("k_uniform_rows (K1 uniform fake-quant, fp32 in/out)", 2 * nb, lambda j: ops.uniform_fake_quant(xs[j], sc1, zp1, 4)),
        ("k_adalog (K2/K3 shifted AdaLog fake-quant)", 2 * nb,
         lambda j: ops.log_fake_quant(xgs[j], sc1, q, t1, t2, 4, shift=shift, sub_shift=True)),
        ("sorted_prefix build (K10 once per tensor: hand-written LSD radix sort, 4 passes x (count, scatter) + fp64 prefix sums; read 4 B, "
         "write 20 B per element)", 6 * nb,
         lambda j: ops.sorted_prefix(xs[j].view(1, -1))),
        ("k_sel_hist_pick (K5 quantile, 4 radix passes, the pick folded into the counting kernel)", 4 * nb, lambda j: ops.quantile_rows(xs[j].view(1, -1), [0.9, 1.0, 0.1, 0.0], 1)),
        ("k_log2_shift (input of the fused search, once per layer)", 2 * nb, lambda j: ops.log2_shift(xgs[j], 0.17)),
        ("k_pack_uniform_tab (fc2 weight candidates: 128 x 384 x 1536 -> bf16 operand, write side)",
         Ws[0].numel() * 4 + Ws[0].numel() * P * 2,
         lambda j: ops.pack_uniform(Ws[j].t().contiguous().unsqueeze(0), csw[:, :384].contiguous(), czw[:, :384].contiguous(), P, 384, 1, 0, 1,
                                    4, ops.BF16, c_inner=True)),
    ]
    for name, nbytes, fn in rows:
        try:
            ms = timeit(fn)
            out.append({"kernel": name, "algorithmic_bytes": int(nbytes), "ms": round(ms, 4), "achieved_GBps": round(nbytes / ms / 1e6, 1),
                        "frac_of_8TBps": round(nbytes / ms / 1e6 / 8000.0, 3)})
        except Exception as ex:                                   # a micro-benchmark must never take the headline down
            out.append({"kernel": name, "error": repr(ex)[:200]})
    # latency-class: a step of the self-MSE search is 2^bits x 128 bisections over the sorted tensor, not a pass over it
    try:
        ms = timeit(lambda j: ops.score_self_sorted(sps[j % 4], cs, cz, 4, 1.0))
        out.append({"kernel": "k_score_sorted (K10 per FPCS step: 128 candidates x 16 bisections over 9.7 M sorted values)", "ms": round(ms, 4),
                    "bound": "latency", "elements_per_s_equivalent": round(x0.numel() * P / ms / 1e6, 1),
                    "note": "the pass it replaces (k_score_a_self, 128 candidates per element) took 0.89 ms at this size"})
    except Exception as ex:
        out.append({"kernel": "k_score_sorted", "error": repr(ex)[:200]})
    return out


def brecq_rate(model_name, bits, dev, iters=2000, depth=None):
    """BRECQ (utils/block_recon.py:84-137) iterations per second on blocks.0 of the benchmarked model: a bounded sample
    (the reference runs 20 000 iterations per block) with the reference's schedule in proportion (first 20 % without the
    rounding regulariser); wall time for one block and the whole model follow by scaling."""
    from adalog_amd.utils.block_recon import BlockReconstructor
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.models import create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    cfg = load_cfg(bits)
    torch.manual_seed(5)
    from adalog_amd import train_mm
    nblk_full = None
    if depth is not None:                                     # a shallow copy of the architecture: the block itself is the same
        nblk_full = len(BlockReconstructor(create_model(model_name).eval(), create_model(model_name).eval(), []).blocks)
    base = (create_model(model_name) if depth is None else create_model(model_name, depth=depth)).eval()
    full = copy.deepcopy(base).to(dev).eval()
    model = wrap_modules_in_net(base, cfg, reparam=True).to(dev)
    imgs = torch.randn(32, 3, 224, 224, generator=torch.Generator().manual_seed(5)).to(dev)
    QuantCalibrator(model, [(imgs, None)], capture="block").batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model)
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    opt = torch.randn(64, 3, 224, 224, generator=torch.Generator().manual_seed(6)).to(dev)
    rec = BlockReconstructor(model, full, [(opt[:32], None), (opt[32:], None)])
    name = "blocks.0"
    block, fblock = rec.blocks[name], rec.full_blocks[name]
    rec.init_block_raw_data(block, fblock, name, dev)
    rec.reconstruct_single_block(name, block, dev, quant_act=True, iters=100)         # warm-up (releases the block data)
    rec.init_block_raw_data(block, fblock, name, dev)
    # steady state: the clock is read (after a device synchronisation) when iteration iters / 4 and the last one have finished;
    # what comes before is the per-block set-up of a reconstruction call (optimisers, three eager iterations, the graph capture),
    # paid once per 20 000 iterations in the reference's schedule
    marks = {}

    def hook(it, loss_func):
        if it in (iters // 4, iters):
            torch.cuda.synchronize()
            marks[it] = time.perf_counter()
    rec.iter_hook = hook
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec.reconstruct_single_block(name, block, dev, quant_act=True, iters=iters)
    torch.cuda.synchronize()
    t_call = time.perf_counter() - t0
    rec.iter_hook = None
    n_steady = iters - iters // 4
    dt_it = (marks[iters] - marks[iters // 4]) / n_steady                        # seconds per iteration, steady state
    setup = max(0.0, t_call - iters * dt_it)
    dt = setup + iters * dt_it                                                   # (= t_call)
    nblk = nblk_full if nblk_full is not None else len(rec.blocks)
    # iters_per_s is the WHOLE-CALL figure (set-up, eager iterations and graph capture included), as rounds 1-3 reported it;
    # steady_iters_per_s is the steady state (round 4 had put that one under the name iters_per_s)
    return {"model": model_name, "iters_per_s": round(iters / t_call, 1), "steady_iters_per_s": round(1.0 / dt_it, 1),
            "ms_per_iter": round(dt_it * 1e3, 3),
            "how": f"iters_per_s: one whole reconstruct_single_block call of {iters} iterations; steady_iters_per_s: its iterations "
                   f"{iters // 4 + 1}..{iters} (HIP-graph replay)",
            "setup_s_per_block": round(setup, 3), "block": name, "batch": 32,
            "sample_iters": iters, "blocks_in_model": nblk,
            "contractions": (("csrc/brecq_gemm.hip (adalog_gemm_f32x3 on the bf16 MFMA, fp32 accumulation; bf16 terms per general operand: "
                              f"forward {3 if not train_mm.FWD_TERMS else 2}, gradients {3 if not train_mm.GRAD_TERMS else 2} "
                              "(2 terms = 2^-16 relative: 3 products per pair of general operands, 2 against the integer activation; "
                              "3 terms = 6 / 3 products, <= rocBLAS fp32 error); trained values within 1e-3 of the reference's own loop "
                              "either way: tests/test_gpu_layers.py)") if train_mm.ENABLED else "rocBLAS fp32"),
            "multi_gpu": "block-parallel (blocks dealt to ranks, no collective inside an iteration); ADALOG_BRECQ_DP=batch = batch split",
            "extrapolated_s_per_block_20000_iters": round(setup + 20000 * dt_it, 1),
            "extrapolated_s_whole_model": round((setup + 20000 * dt_it) * nblk, 1)}


def quant_forward_rate(calibrated, images, dev, reps=5):
    """K15 (reference linear.py:46-51, matmul.py:43-45, conv.py:60-65): a validate()-style forward of the calibrated model with
    every layer in quant_forward mode (test_quant.py's flow: un-wrap the channel-wise layers, fold the post-GELU shift into the
    biases), against the same model in raw mode.  Bounded sample: `reps` forwards of the calibration batch each."""
    from adalog_amd import _lib
    from adalog_amd.utils.wrap_net import wrap_reparamed_modules_in_net
    model = wrap_reparamed_modules_in_net(copy.deepcopy(calibrated)).to(dev).eval()
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    lib = _lib.load()
    labels = {}

    def run(mode):
        for m in model.modules():
            if hasattr(m, "mode"):
                m.mode = mode
        with torch.no_grad():
            model(images)                                         # warm-up (packs the weights once: they are cached)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                out = model(images)
            e1.record()
            torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, out

    hooks = []
    if True:                                                       # which GEMM kernel served each layer class (adalog_last_kernel)
        def mk(cls):
            def hook(mod, inp, out):
                if getattr(mod, "mode", "") == "quant_forward":
                    labels.setdefault(cls, set()).add(lib.adalog_last_kernel().decode())
            return hook
        for m in model.modules():
            if hasattr(m, "mode"):
                m.mode = "quant_forward"
                hooks.append(m.register_forward_hook(mk(type(m).__name__)))
        with torch.no_grad():                                      # (listeners on the modules' forward select the module-by-module route)
            out_mod = model(images)
    for h in hooks:
        h.remove()
    ms_q, out_q = run("quant_forward")                             # no listeners: the fused block route (utils/models.py)
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with torch.no_grad(), profile(activities=[ProfilerActivity.CUDA]) as prof:
            model(images)
            torch.cuda.synchronize()
        launches = int(sum(e.count for e in prof.key_averages() if "DeviceType.CUDA" in str(getattr(e, "device_type", ""))))
    except Exception:                                              # the count is a report item only
        launches = None
    ms_r, out_r = run("raw")
    # the same quant_forward as a captured HIP graph (what validate() replays per batch shape: utils/graph_forward.py)
    from adalog_amd.utils.graph_forward import GraphedForward
    for m in model.modules():
        if hasattr(m, "mode"):
            m.mode = "quant_forward"
    gf = GraphedForward(model)
    out_g = gf(images)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out_g = gf(images)
    e1.record()
    torch.cuda.synchronize()
    ms_g = e0.elapsed_time(e1) / reps
    graph_equal = bool(torch.equal(out_g, out_q))
    n = images.shape[0]
    rel = float((out_q - out_r).norm() / out_r.norm())
    return {"images": n, "ms_per_forward": round(ms_g, 3), "images_per_s": round(n / ms_g * 1e3, 1),
            "how": "HIP-graph replay of the quant_forward pass (validate()'s route); eager launches of the same kernels below",
            "eager_ms_per_forward": round(ms_q, 3), "eager_images_per_s": round(n / ms_q * 1e3, 1),
            "graph_output_equals_eager": graph_equal,
            "raw_ms_per_forward": round(ms_r, 3), "raw_images_per_s": round(n / ms_r * 1e3, 1),
            "launches_per_forward": launches,
            "fused_vs_module_route_rel_diff": float((out_q - out_mod).norm() / out_mod.norm()),
            "kernels_by_layer_class": {k: sorted(v) for k, v in labels.items()},
            "output_rel_diff_vs_fp": round(rel, 4),
            "note": "timed: the fused block route (utils/models.py, round 6) -- per transformer block qkv / proj / fc1 in ONE launch each "
                    "(activation quantised in the GEMM's loader, residual added in proj's and fc2's epilogue), q / k / v split + "
                    "quantised + packed in one launch, scale + softmax + AdaLog quantiser + pack in one launch, softmax.v written as "
                    "[B,N,H,D], GELU inside fc2's operand packer; kernels_by_layer_class: the module-by-module route (a forward with "
                    "listeners on every module), kept for callers that hook modules; packed weights cached; raw = the FP32 model (rocBLAS)"}


DUMP_SAMPLE = 1 << 16         # elements written of a larger tensor by dump_outputs


def dump_outputs(model, out_dir):
    """What a caller of the timed path receives: the calibrated model's state_dict (every quantiser's scale, zero point, log
    base and tables, and the weights / LayerNorm parameters that re-parameterisation rewrote), one <out_dir>/<key>.npy per
    entry in its own shape, float32 (float64 for float64 and integer entries).  An entry of more than DUMP_SAMPLE elements
    is written as DUMP_SAMPLE of its flattened elements, at sorted indices from a generator with a fixed seed (the same in
    every run and build): ~14 MB in all for deit_small."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for key, t in model.state_dict().items():
        t = t.detach().cpu()
        if t.numel() > DUMP_SAMPLE:
            idx = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))[:DUMP_SAMPLE].sort().values
            t = t.reshape(-1)[idx]
        dt = torch.float32 if t.dtype in (torch.float32, torch.float16, torch.bfloat16, torch.bool) else torch.float64
        np.save(os.path.join(out_dir, key + ".npy"), t.to(dt).numpy())


def _cpu_sample(threads, n_cand, min_seconds=0.0):
    """Seconds the oracle needs for one weight-scoring + one activation-scoring call of ``n_cand`` candidates each at
    deit_small attn.proj size (32 images x 197 tokens, 384 -> 384, W4A4) on ``threads`` host threads (thread-count probe, and
    the tensors of the HIP cross-check)."""
    from oracle import adalog_oracle as O
    torch.set_num_threads(threads)
    O.PCHUNK = 16
    g = torch.Generator().manual_seed(5)
    N, T, I, Oc, bits = 32, 197, 384, 384, 4
    x = torch.randn(N, T, I, generator=g)
    W = torch.randn(Oc, I, generator=g) * 0.05
    b = torch.zeros(Oc)
    ro = torch.nn.functional.linear(x, W, b)
    w3 = W.view(1, Oc, I)
    scw, zpw = O.weight_candidates(w3, bits)
    sca, zpa = O.activation_candidates(x, bits, False)
    xq = O.uniform_fake_quant(x, sca[:, 60], zpa[:, 60].float(), bits)[0]
    wq = O.uniform_fake_quant(w3, scw[60], zpw[60].float(), bits)[0].view(Oc, I)
    t0 = time.perf_counter()
    reps = 0
    while True:
        ref_w = O.score_w(xq, w3, b, ro, scw[:n_cand], zpw[:n_cand], bits, 32)
        ref_a = O.score_a(x, wq, b, ro, sca[:, :n_cand], zpa[:, :n_cand], bits, 32)
        reps += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            break
    return dt, reps, (x, W, b, ro, scw, zpw, sca, zpa, ref_w, ref_a)


def _cpu_class_samples(threads, seconds_per_class=2.5, n_cand=16):
    """one layer of EACH of the six layer classes at config 1's shapes (deit_tiny W6A6, 32 images,
    T = 197, D = 192, 3 heads), the class's output-search scoring calls on ``n_cand`` candidates (candidates are scored
    independently, linear.py:363-380), looped for ~seconds_per_class.  -> {class: (GFLOP/s of candidate-GEMM work, seconds)}."""
    from oracle import adalog_oracle as O
    torch.set_num_threads(threads)
    O.PCHUNK = n_cand
    g = torch.Generator().manual_seed(5)
    N, T, D, H, MLP, bits = 32, 197, 192, 3, 768, 6
    hd = D // H
    sub = slice(0, n_cand)
    out = {}

    def run(name, flops_per_cand, parts):
        """parts: [(candidates of this kind in one layer's search, fn scoring n_cand of them)].  Each kind is timed on its own for
        its share of seconds_per_class; the class rate is the layer's candidate-GEMM flops over the layer's projected time."""
        total_c = sum(c for c, _ in parts)
        t_layer, spent = 0.0, 0.0
        for cnt, fn in parts:
            fn()                                                     # warm the allocator / thread pool
            t0 = time.perf_counter()
            reps = 0
            while True:
                fn()
                reps += 1
                dt = time.perf_counter() - t0
                if dt >= seconds_per_class * cnt / total_c:
                    break
            t_layer += cnt * dt / (reps * n_cand)
            spent += dt
        gemm_c = sum(c for c, fn in parts if not getattr(fn, "no_gemm", False))
        out[name] = (gemm_c * flops_per_cand / t_layer / 1e9, spent)

    def linear_ops(I, Oc, n_V):
        x = torch.randn(N, T, I, generator=g)
        W = torch.randn(Oc, I, generator=g) * 0.05
        b = torch.randn(Oc, generator=g) * 0.1
        ro = torch.nn.functional.linear(x, W, b)
        w3 = W.view(n_V, Oc // n_V, I)
        scw, zpw = O.weight_candidates(w3, bits)
        sca, zpa = O.activation_candidates(x, bits, False)
        xq = O.uniform_fake_quant(x, sca[:, 60], zpa[:, 60].float(), bits)[0]
        wq = O.uniform_fake_quant(w3, scw[60], zpw[60].float(), bits)[0].view(Oc, I)
        return x, W, b, ro, w3, scw, zpw, sca, zpa, xq, wq

    # 1. AsymmetricallyBatchingQuantLinear: attn.proj 192 -> 192 (linear.py:355-430)
    x, W, b, ro, w3, scw, zpw, sca, zpa, xq, wq = linear_ops(D, D, 1)
    # (per layer: 3 rounds x 6 steps x 128 candidates of each operand, linear.py:536-539)
    run("linear(proj)", 2.0 * N * T * D * D,
        [(2304, lambda: O.score_w(xq, w3, b, ro, scw[sub], zpw[sub], bits, 32)),
         (2304, lambda: O.score_a(x, wq, b, ro, sca[:, sub], zpa[:, sub], bits, 32))])
    # 2. AsymmetricallyChannelWiseBatchingQuantLinear: attn.qkv 192 -> 576: per-channel self-MSE search, then the plain search
    x, W, b, ro, w3, scw, zpw, sca, zpa, xq, wq = linear_ops(D, 3 * D, 3)
    sca_c, zpa_c = O.activation_candidates(x, bits, True)
    cw_self = lambda: O.score_a_self(x, sca_c[:, sub], zpa_c[:, sub], bits, True, 32)      # 768 per-channel self-MSE candidates, no GEMM
    cw_self.no_gemm = True
    run("linear_channelwise(qkv)", 2.0 * N * T * D * 3 * D,
        [(768, cw_self), (2304, lambda: O.score_w(xq, w3, b, ro, scw[sub], zpw[sub], bits, 32)),
         (2304, lambda: O.score_a(x, wq, b, ro, sca[:, sub], zpa[:, sub], bits, 32))])
    # 3. PostGeluLogBasedBatchingQuantLinear: mlp.fc2 768 -> 192 (linear.py:816-931)
    xg = torch.nn.functional.gelu(2.0 * torch.randn(N, T, MLP, generator=g))
    Wg = torch.randn(D, MLP, generator=g) * 0.03
    bg = torch.randn(D, generator=g) * 0.1
    rog = torch.nn.functional.linear(xg, Wg, bg)
    w3g = Wg.view(1, D, MLP)
    scwg, zpwg = O.weight_candidates(w3g, bits)
    wqg = O.uniform_fake_quant(w3g, scwg[60], zpwg[60].float(), bits)[0].view(D, MLP)
    shift = torch.tensor(O.GELU_SHIFT)
    table = O.search_table(bits)
    ud, sc_all = O.postgelu_candidates(xg, shift.item())
    scs = (ud[:, 0:1] + (ud[:, 1:] - ud[:, 0:1]) * torch.tensor([i / 15 for i in range(16)]).view(1, -1))[:, :n_cand]
    qs = torch.tensor([17, 23, 31, 37, 45, 60, 90, 137] * 2).view(1, -1)[:, :n_cand]
    xqg = O.shift_adalog_fake_quant(xg, sc_all[:, -2].clone(), 41, bits, shift, False)[0]
    # (3 rounds x (128 bases + 6 x 128 joint candidates) activation, 3 x 6 x 128 weight: linear.py:941-997)
    run("linear_postgelu(fc2)", 2.0 * N * T * MLP * D,
        [(2688, lambda: O.score_postgelu(xg, wqg, bg, rog, scs, qs, shift, bits, table, 32)),
         (2304, lambda: O.score_w(xqg, w3g, bg, rog, scwg[sub], zpwg[sub], bits, 32))])
    # 4. AsymmetricallyBatchingQuantMatMul: q.k^T [32,3,197,64].[32,3,64,197] (matmul.py:135-209)
    A = torch.randn(N, H, T, hd, generator=g)
    B = torch.randn(N, H, T, hd, generator=g).transpose(-2, -1)
    rom = A @ B
    sA, zA = O.matmul_candidates(A, bits)
    sB, zB = O.matmul_candidates(B, bits)
    Bq = O.uniform_fake_quant(B, sB[60], zB[60].float(), bits)[0]
    Aq = O.uniform_fake_quant(A, sA[60], zA[60].float(), bits)[0]
    run("matmul(qk)", 2.0 * N * H * T * T * hd,
        [(2304, lambda: O.score_matmul(A, B, rom, sA[sub], zA[sub], bits, "A", Bq, True, 32)),
         (2304, lambda: O.score_matmul(A, B, rom, sB[sub], zB[sub], bits, "B", Aq, True, 32))])
    # 5. PostSoftmaxAsymmetricallyBatchingQuantMatMul: softmax.v (matmul.py:321-358)
    As = torch.softmax(4.0 * torch.randn(N, H, T, T, generator=g), dim=-1)
    Bv = torch.randn(N, H, T, hd, generator=g)
    ros = As @ Bv
    sBv, zBv = O.matmul_candidates(Bv, bits)
    Bvq = O.uniform_fake_quant(Bv, sBv[60], zBv[60].float(), bits)[0]
    Asq = O.adalog_fake_quant(As, torch.ones(1, 1, 1, 1), 29, bits)[0]
    qsub = torch.tensor([10 + 8 * i for i in range(n_cand)]).view(-1, 1, 1, 1, 1)
    # (3 rounds x (128 log bases + 6 x 128 B candidates): matmul.py:360-378)
    run("matmul_postsoftmax(av)", 2.0 * N * H * T * T * hd,
        [(384, lambda: O.score_log_base_A(As, Bvq, ros, qsub, bits, table, 32)),
         (2304, lambda: O.score_matmul(As, Bv, ros, sBv[sub], zBv[sub], bits, "B", Asq, True, 32))])
    # 6. AsymmetricallyBatchingQuantConv2d: patch embedding 3 -> 192, 16 x 16 / 16 (conv.py:226-263)
    xi = torch.randn(N, 3, 224, 224, generator=g)
    Wc = torch.randn(D, 3, 16, 16, generator=g) * 0.05
    bc = torch.randn(D, generator=g) * 0.1
    roc = torch.nn.functional.conv2d(xi, Wc, bc, (16, 16))
    w2 = Wc.view(D, -1)
    scc, zpc = O.weight_candidates(w2, bits, conv=True)
    run("conv(patch_embed)", 2.0 * N * 196 * 768 * D,
        [(768, lambda: O.score_conv_w(xi, w2, bc, roc, scc[sub], zpc[sub], bits, (16, 16), (16, 16), 32))])
    return out


def cpu_baseline(nproc, with_hip=True):
    """The CPU oracle (a port of the reference's algorithm, validated against the reference's golden traces) on a BOUNDED sample,
    as BASELINE.md section 3.2 plans it: one layer of each of the six layer classes at config 1's shapes (deit_tiny W6A6, 32
    images), each class's rate weighted by its share of the benchmarked model's candidate-GEMM work.
    Thread count: the best of 8 / 32 / nproc on a quick probe (the reference's elementwise chains over [N,T,I,P] temporaries are
    memory-bound: more threads than memory channels only adds contention); `cores` is the host's core count, `threads` what ran.
    BASELINE.md section 3.1 measured the reference's own code at 24-46 GFLOP/s on 8 vCPUs."""
    N, T, I, Oc, bits = 32, 197, 384, 384, 4
    tried = {}
    for th in sorted({min(8, nproc), min(32, nproc), nproc}):
        dt, reps, _ = _cpu_sample(th, 16)                       # probe: 16 candidates per call
        tried[th] = reps * 2 * 2.0 * N * T * I * Oc * 16 / dt / 1e9
    best = max(tried, key=tried.get)
    classes = _cpu_class_samples(best)
    # candidate-GEMM work of the benchmarked model (deit_small, 32 images) by layer class, TFLOP:
    # 4608 scored candidates per plain / channel-wise Linear and q.k^T, 4992 per post-GELU Linear, 2688 per softmax.v, 768 per conv
    D, Hh, Tt, MLP, NI = 384, 6, 197, 1536, 32
    MT = NI * Tt
    work = {"linear(proj)": 12 * 4608 * 2.0 * MT * D * D + 4608 * 2.0 * NI * D * 1000,
            "linear_channelwise(qkv)": 12 * 4608 * 2.0 * MT * D * (3 * D + MLP),
            "linear_postgelu(fc2)": 12 * 4992 * 2.0 * MT * MLP * D,
            "matmul(qk)": 12 * 4608 * 2.0 * NI * Hh * Tt * Tt * (D // Hh),
            "matmul_postsoftmax(av)": 12 * 2688 * 2.0 * NI * Hh * Tt * Tt * (D // Hh),
            "conv(patch_embed)": 768 * 2.0 * NI * 196 * 768 * D}
    total = sum(work.values())                                  # = 1354 TFLOP
    seconds = sum(work[k] / (classes[k][0] * 1e9) for k in work)
    sample_s = sum(v[1] for v in classes.values())
    dt, reps, (x, W, b, ro, scw, zpw, sca, zpa, ref_w, ref_a) = _cpu_sample(best, 128, 0.0)     # tensors of the HIP cross-check
    out = {"value": 32.0 / seconds, "unit": "images/s", "cores": nproc, "threads": best, "kind": "port",
           "sample": f"oracle scoring calls (16 candidates each, ~2.5 s per class) of one layer of each of the six layer classes at "
                     f"config 1's shapes (deit_tiny W6A6, 32 images) on {best} threads (best of {sorted(tried)} in a probe; host has "
                     f"{nproc} cores): {sample_s:.1f} s of CPU work; per-class candidate-GEMM rates weighted by deit_small's "
                     f"{total / 1e12:.0f} TFLOP of candidate GEMMs per 32-image calibration -> {seconds:.0f} s per calibration",
           "sample_seconds": sample_s,
           "gflops_by_class": {k: round(v[0], 1) for k, v in classes.items()},
           "work_tflop_by_class": {k: round(v / 1e12, 1) for k, v in work.items()},
           "gflops_by_threads_probe": {str(k): round(v, 1) for k, v in tried.items()},
           "reference_code_gflops_8vcpu": {"linear(proj)": 45.9, "matmul(qk)": 24.1, "matmul_postsoftmax(av)": 26.3,
                                           "linear_postgelu(fc2)": 37.3}}
    if not with_hip:
        return out
    # the oracle as the CHECKER at full layer size: the same two scoring calls through the product path (HIP kernels)
    from adalog_amd import quant_layers as Q
    dev = torch.device("cuda")
    lay = Q.AsymmetricallyBatchingQuantLinear(I, Oc, True, "raw", bits, bits, calib_batch_size=32, search_round=1, eq_n=128,
                                              n_V=1, fpcs=True, steps=6).to(dev)
    lay.weight.data.copy_(W); lay.bias.data.copy_(b)
    lay.raw_input, lay.raw_out = x.to(dev), ro.to(dev)
    lay.a_quantizer.scale.data.copy_(sca[:, 60].view(-1)); lay.a_quantizer.zero_point.data.copy_(zpa[:, 60].float().view(-1))
    lay.w_quantizer.scale.data.copy_(scw[60]); lay.w_quantizer.zero_point.data.copy_(zpw[60].float())
    got_w = lay._score_w(lay._pack_x_fixed(), scw.reshape(128, -1).to(dev), zpw.reshape(128, -1).float().to(dev)).cpu()
    got_a = lay._score_a(lay._pack_w_fixed(), sca.t().contiguous().to(dev), zpa.t().contiguous().float().to(dev)).cpu()
    rw, ra = ref_w.reshape(128, -1), ref_a.reshape(-1, 128).t()
    err_w = float(((got_w - rw).abs() / rw.abs()).max())
    err_a = float(((got_a - ra).abs() / ra.abs()).max())
    same_top = bool(torch.equal(torch.topk(got_a[:, 0], 16).indices.sort().values, torch.topk(ra[:, 0], 16).indices.sort().values))
    out["parity_vs_hip"] = {"max_rel_err_weight_scores": err_w, "max_rel_err_activation_scores": err_a,
                            "same_top16_activation_candidates": same_top,
                            "note": "same inputs and candidates through adalog_amd (HIP) at full layer size; bar 1e-3"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="deit_small")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--images-per-gpu", type=int, default=32)
    ap.add_argument("--images-total", type=int, default=None,
                    help="fixed calibration-set size sharded over the GPUs (strong scaling; BASELINE config 4 = 1024 over 8); "
                         "default: --images-per-gpu x N (weak scaling)")
    ap.add_argument("--depth", type=int, default=None, help="truncate the block count (debug only; invalidates the metric)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also time the other schedule, the HBM-class kernels, BRECQ, quant_forward and "
                         "the CPU-oracle baseline (with its HIP cross-check)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the calibrated model of the last timed step to DIR/<state_dict key>.npy (see dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip hbm_kernels, brecq, quant_forward and cpu_baseline")
    ap.add_argument("--schedule", choices=("reference", "product"), default="reference",
                    help="what the main timed region (`value`) runs.  reference: every search of every round, as reference "
                         "quant_layers/linear.py:536-541 / matmul.py:275-277 do -- no candidate work is skipped.  product: the "
                         "package's default, which does not re-run a search whose inputs are bit-identical to the previous round's "
                         "nor the dead weight self-search (same calibrated model).  With --full the other schedule is timed in a "
                         "second region of the same run and reported under config.other_schedule")
    ap.add_argument("--no-rerun-all", action="store_true", help="with --full: skip the second timed region")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # launched as `python bench.py --gpus N`: start one rank per GPU under torch.distributed.run as a CHILD process
        # (nothing in this process has touched the GPU yet) and leave with its exit code
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        from adalog_amd import parallel
        if os.environ.get("ADALOG_DIST_BACKEND", "nccl") != "nccl":
            local_rank = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local_rank)
        # RCCL ("nccl") is the product path.  ADALOG_DIST_BACKEND=gloo lets several ranks share ONE GPU: a functional check of
        # the sharded code path on a single-GPU box (collectives then stage through the host: not a performance mode)
        be_name = os.environ.get("ADALOG_DIST_BACKEND", "nccl")
        if be_name == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank), timeout=parallel.dist_timeout())
        else:
            dist.init_process_group(backend=be_name, timeout=parallel.dist_timeout())
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    from adalog_amd import backend, parallel
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.models import create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net
    ops = backend.get()

    cfg = load_cfg(args.bits)
    if args.images_total is not None:
        assert args.images_total % world == 0, "--images-total must divide over the GPUs"
        args.images_per_gpu = args.images_total // world
    cfg.calib_size = args.images_per_gpu * world
    torch.manual_seed(5)                                           # reference default seed (test_quant.py:77)
    base = create_model(args.model, depth=args.depth).eval()
    base = wrap_modules_in_net(base, cfg, reparam=True).to(dev)
    images = torch.randn(cfg.calib_size, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    lo, hi = rank * args.images_per_gpu, (rank + 1) * args.images_per_gpu
    local = images[lo:hi].to(dev)
    loader = [(local[i:i + cfg.calib_batch_size], None) for i in range(0, local.shape[0], cfg.calib_batch_size)]

    prof = GemmProfiler(ops)

    from adalog_amd import search as _search
    from adalog_amd.quant_layers import linear as _linear
    product_defaults = (_search.SKIP_CONVERGED, _linear.RUN_DEAD_W_SELF)

    def set_schedule(name):
        if name == "reference":
            _search.SKIP_CONVERGED, _linear.RUN_DEAD_W_SELF = False, True
        else:
            _search.SKIP_CONVERGED, _linear.RUN_DEAD_W_SELF = product_defaults

    set_schedule(args.schedule)
    cals = []

    def one_step(model):
        cal = QuantCalibrator(model, loader, capture="block")
        cal.batching_quant_calib()
        cals.append(cal)

    models = [copy.deepcopy(base) for _ in range(args.warmup + args.steps)]
    for i in range(args.warmup):
        one_step(models[i])
    torch.cuda.synchronize()
    parallel.barrier()
    torch.cuda.synchronize()
    prof.start()
    parallel.reset_stats()
    _search.reset_round_stats()
    t0 = time.perf_counter()
    for i in range(args.steps):
        one_step(models[args.warmup + i])
    torch.cuda.synchronize()
    parallel.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    by = prof.stop()
    coll = parallel.collective_stats()
    round_stats = _search.round_stats() if args.schedule == "product" else None
    if args.dump_outputs and rank == 0:
        dump_outputs(models[args.warmup + args.steps - 1], args.dump_outputs)
    # second timed region: the same K steps on the OTHER schedule (both produce the same calibrated model, tests/calibrator_cases.py)
    wall_all = None
    other = "product" if args.schedule == "reference" else "reference"
    if args.full and not args.no_rerun_all:
        set_schedule(other)
        _search.reset_round_stats()
        more = [copy.deepcopy(base) for _ in range(args.steps)]
        torch.cuda.synchronize()
        parallel.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for m in more:
            one_step(m)
        torch.cuda.synchronize()
        parallel.barrier()
        torch.cuda.synchronize()
        wall_all = time.perf_counter() - t1
        if other == "product":
            round_stats = _search.round_stats()              # (the product schedule is the one that compares quantiser states)
        set_schedule(args.schedule)
        del more
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([wall, wall_all if wall_all is not None else 0.0], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t[0].item())
        wall_all = float(t[1].item()) if wall_all is not None else None

    if rank == 0:
        ms_per_step = wall * 1e3 / args.steps
        value = cfg.calib_size * args.steps / wall
        # the dominant KERNEL (largest summed launch time over the timed steps) carries the roofline object
        # the dominant kernel TEMPLATE (largest summed launch time over the timed steps; the generated-operand and packed forms
        # of the slab kernel are one template) carries the roofline object, its instantiations are listed as sub-rows
        templ = prof.by_template(args.steps)
        if templ:
            (dom_name, dom), gdom = templ[0]
            fl, ms, n, dom_rows = gdom["flops"], gdom["ms"], gdom["n"], gdom["rows"]
        else:
            (dom_name, dom), (fl, ms, n), dom_rows = ("", 0), (0.0, 1.0, 1), []
        achieved = fl / (ms * 1e-3) / 1e12
        # the instantiation with the largest time stands for the template in the PMC replay
        dom_label = max(dom_rows, key=lambda r: r["ms_per_step"])["kernel"] if dom_rows else dom_name
        gemm_ms_total = sum(v[1] for v in by.values())
        timed = cals[args.warmup:args.warmup + args.steps]
        fpcs = [sum(c.fpcs_seconds().values()) for c in timed]
        capt = [c.capture_device_seconds() for c in timed]
        default_workload = (args.model == "deit_small" and args.bits == 4 and args.images_per_gpu == 32 and world == 1
                            and args.depth is None)
        result = {
            "metric": "calib_images_per_sec", "value": value, "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
            "scaling": "strong" if args.images_total is not None else "weak",
            "vs_baseline": None, "dtype": DT_NAME[dom], "data": "synthetic",
            "dtype_note": "operand STORAGE type of the dominant scoring kernel: fp8 (e4m3) / int8 hold the exact integers q - z of the "
                          "<= 4-bit / <= 6-bit operands, bf16 holds the AdaLog values m * 2^-t exactly; products accumulate in fp32 "
                          "(sums < 2^24: exact) or int32 -- not a narrower precision than the reference's fp32 GEMM",
            "config": {"workload": f"{args.model} W{cfg.w_bit}A{cfg.a_bit} --calibrate, {args.images_per_gpu} calib images "
                                   f"per GPU ({cfg.calib_size} total), eq_n=128, 3 rounds, FPCS 6 steps",
                       "calib_wall_s_per_step": wall / args.steps,
                       "scoring_gemm_ms_per_step": gemm_ms_total / args.steps,
                       "scoring_gemm_by_dtype": {DT_NAME[d]: {"launches_per_step": v[2] / args.steps,
                                                              "ms_per_step": v[1] / args.steps,
                                                              "tflops": v[0] / (v[1] * 1e-3) / 1e12} for d, v in by.items()},
                       "scoring_kernels": prof.by_kernel(args.steps),
                       "scoring_gemm_top_shapes": prof.top_shapes(args.steps),
                       "fpcs_seconds_per_step": sum(fpcs) / max(len(fpcs), 1),
                       "capture_seconds_per_step": sum(capt) / max(len(capt), 1),
                       "fpcs_note": "device events on the search stream around every module's hyperparameter_searching (+ reparam), "
                                    "summed over the modules (rank 0); capture = the FP forward passes that record the activations",
                       "collectives": {"per_step": coll["collectives"] / args.steps, "bytes_per_step": coll["bytes"] / args.steps,
                                       # every all-reduce SITE this rank passed, also in a one-rank run (payloads do not depend on the
                                       # world size): what each rank of an N-GPU job puts on the fabric per calibration
                                       "planned_per_step": coll.get("planned_collectives", 0) / args.steps,
                                       "planned_bytes_per_step": coll.get("planned_bytes", 0) / args.steps,
                                       "stream_ms_per_step": None if coll["device_ms"] is None else coll["device_ms"] / args.steps,
                                       "schedule": "two lanes (two modules' searches side by side, each on its own stream and "
                                                   "communicator, one global issue order)" if world > 1 and os.environ.get("ADALOG_INTERLEAVE", "0") == "1"
                                                   else "sequential (one communicator, one stream; ADALOG_INTERLEAVE=1 = two lanes)",
                                       "note": "score / min-max / histogram all-reduces of rank 0 during the timed steps; stream_ms = "
                                               "summed event time around them on their lane's stream (includes waiting for the peers)"},
                       "schedule": {
                           "timed": args.schedule,
                           "reference": "every search of every round is run, as reference quant_layers/linear.py:536-541 and "
                                        "matmul.py:275-277 do: no candidate work is skipped",
                           "product": "the package default: an output-MSE search of round 2..3 whose inputs (the other operand's "
                                      "quantiser) are bit-identical to the previous round's is not re-run (a pure function of unchanged "
                                      "inputs: it would commit what is committed), nor is the weights' self-MSE search whose result "
                                      "the first round overwrites unread; same calibrated model tensor for tensor "
                                      "(tests/calibrator_cases.py); ADALOG_SKIP_CONVERGED=0 ADALOG_DEAD_W_SELF=1 = reference schedule",
                           "round_checks_per_step": None if round_stats is None else round_stats["checked"] / args.steps,
                           "round_inputs_unchanged_per_step": None if round_stats is None else round_stats["unchanged"] / args.steps,
                           "round_stats_from": "the product-schedule region (the reference schedule takes no snapshots)"},
                       "other_schedule": None if wall_all is None else {
                           "schedule": other, "ms_per_step": wall_all * 1e3 / args.steps,
                           "images_per_s": cfg.calib_size * args.steps / wall_all, "steps": args.steps,
                           "how": "second timed region of this run (same barriers and synchronisation, no warm-up of its own)"},
                       "depth_override": args.depth},
            "roofline": {"bound": "mfma", "kernel": dom_name, "achieved": achieved,
                         "peak": PEAK_TOPS[dom], "unit": "TFLOP/s", "frac": achieved / PEAK_TOPS[dom],
                         "instantiations": dom_rows,
                         "traffic": pmc_traffic(dom_label, default_workload), "traffic_kernel": dom_label,
                         "traffic_source": "REPLAYED, not measured by this run: profiles/r0N_pmc_bench_traffic.json (latest round) holds the rocprofv3 --pmc "
                                           "passes of this same command (tools/pmc_bench.sh; FETCH_SIZE x2 per the gfx950 note + "
                                           "WRITE_SIZE, per launch); null for any other workload",
                         "launches": n, "avg_launch_ms": ms / max(n, 1)},
        }
        if args.full and not args.no_cpu_baseline and world == 1:
            result["hbm_kernels"] = hbm_kernels(ops, dev)
            try:
                result["brecq"] = brecq_rate(args.model, args.bits, dev)
                if args.model != "vit_base":                  # BASELINE configs 3 and 5 reconstruct base-width blocks
                    result["brecq"]["vit_base_block"] = brecq_rate("vit_base", args.bits, dev, iters=1000, depth=1)
            except Exception as ex:
                result["brecq"] = {"error": repr(ex)[:300]}
            try:
                result["quant_forward"] = quant_forward_rate(models[-1], local[:32], dev)
            except Exception as ex:
                result["quant_forward"] = {"error": repr(ex)[:300]}
            result["cpu_baseline"] = cpu_baseline(os.cpu_count() or 1)
        print(json.dumps(result))
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
