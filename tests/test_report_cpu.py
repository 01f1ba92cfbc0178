"""The per-layer quantisation report without a device: self-checks of the plain-torch reference (tests/report_reference.py), and the
host logic of adalog_amd/utils/report.py -- quant_report and its command line -- on a tiny ViT and a tiny Swin calibrated with the
stand-in backend (tests.cpu_backend behind a proxy that adds the three report ops from the reference)."""
import copy
import importlib.util
import json
import math
import os

import pytest
import torch

from adalog_amd import backend
from adalog_amd._lib import AdalogHipError
from tests import report_reference as RR
from tests.test_packed_cpu import PackedCpuBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG4 = os.path.join(ROOT, "configs", "4bit.py")


# ------------------------------------------------------------------------------------------------ the reference checks itself
def test_reference_histogram_and_clip_counts_sum_to_n():
    g = torch.Generator().manual_seed(0)
    for bits in (2, 3, 4, 6, 8):
        for shape, p_shape in (((1000,), (1,)), ((3, 65), (3, 1)), ((2, 3, 5, 16), (1, 3, 1, 1))):
            x = torch.randn(shape, generator=g) * 3
            n_ch = max(p_shape)
            s, z = torch.rand(n_ch, generator=g) * 0.2 + 0.05, torch.rand(n_ch, generator=g) * (2 ** bits)
            inner = x.numel() // shape[0] // n_ch if len(shape) == 4 else (shape[-1] if n_ch > 1 else x.numel())
            h = RR.uniform_code_hist(x, s, z, bits, n_ch, inner)
            assert tuple(h.shape) == (n_ch, 2 ** bits + 2) and h.dtype == torch.int64
            assert int(h.sum()) == x.numel() and bool((h.sum(1) == x.numel() // n_ch).all())


def test_reference_hand_computed_case():
    # x / s = -3, -0.52, 0, 0.5, 1.5, 2.5, 7.2, 200 -> rne: -3, -1, 0, 0 (tie to even), 2 (tie to even), 2 (tie to even), 7, 200
    # + rne(1.5) = 2 -> -1, 1, 2, 2, 4, 4, 9, 202; two bits: codes 0..3
    x = torch.tensor([-1.5, -0.26, 0.0, 0.25, 0.75, 1.25, 3.6, 100.0])
    h = RR.uniform_code_hist(x, torch.tensor([0.5]), torch.tensor([1.5]), 2)
    assert h.tolist() == [[0, 1, 2, 0, 1, 4]]
    e = RR.err_stats(torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.tensor([1.0, 2.0, 3.0, 2.0]))
    assert e.tolist() == [[4.0, 30.0, 18.0, 2.0]]
    e2 = RR.err_stats(torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), torch.zeros(6), n_channels=3, inner=1)
    assert e2[:, 1].tolist() == [1.0 + 16.0, 4.0 + 25.0, 9.0 + 36.0] and e2[:, 3].tolist() == [4.0, 5.0, 6.0]
    assert RR.log_code_hist_from_bins(torch.tensor([0, 3, 3, 255, 1], dtype=torch.uint8), 2).tolist() == [1, 1, 0, 2, 1]


def test_reference_sqnr_of_a_known_pair():
    a = torch.tensor([3.0, 4.0])
    b = torch.tensor([3.0, 3.5])
    noise, signal, _, _ = RR.err_stats(a, b)[0].tolist()
    assert RR.sqnr_db(signal, noise) == pytest.approx(20.0)           # 25 / 0.25 = 100
    assert RR.sqnr_db(1.0, 0.0) == math.inf and RR.sqnr_db(0.0, 1.0) == -math.inf
    assert RR.entropy_bits([4, 4, 0, 8]) == pytest.approx(1.5)


# ------------------------------------------------------------------------------------------------ stand-in backend
class ReportCpuBackend:
    """a proxy over tests.cpu_backend (through the packed-checkpoint proxy, for the command line's load_packed): forwards every
    attribute and adds the three report ops of adalog_amd/ops.py from the reference"""

    def __init__(self):
        self._base = PackedCpuBackend()

    def __getattr__(self, name):
        return getattr(self._base, name)

    def err_stats(self, a, b, n_channels=1, inner=None):
        return RR.err_stats(a, b, n_channels, inner)

    def uniform_code_hist(self, x, scale, zp, n_bits, n_channels=1, inner=None):
        n_ch, inner = RR._layout(x.numel(), n_channels, inner)
        if n_ch > 1 and inner < 64:
            raise AdalogHipError("uniform_code_hist: several channels need inner >= 64")
        return RR.uniform_code_hist(x, scale, zp, n_bits, n_ch, inner)

    def log_code_hist(self, x, scale, q, n_bits, shift=None, pre_gelu=False):
        assert not pre_gelu
        bins = self._base.log_fake_quant(x, scale, q, None, None, n_bits, shift=shift, train_form=True, want_bins=True, want_y=False)[1]
        return RR.log_code_hist_from_bins(bins, n_bits)


@pytest.fixture(scope="module")
def be():
    impl = ReportCpuBackend()
    backend.set_backend(impl)
    yield impl
    backend.set_backend(None)


def _cfg():
    spec = importlib.util.spec_from_file_location("cfg4report", CFG4)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = mod.Config()
    cfg.search_round, cfg.steps = 1, 2
    return cfg


def tiny_vit():
    from adalog_amd.utils.models import VisionTransformer
    return VisionTransformer(img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=4, num_classes=10).eval()


def tiny_swin():
    from adalog_amd.utils.models import SwinTransformer
    return SwinTransformer(img_size=56, patch_size=4, embed_dim=32, depths=(1, 1), num_heads=(2, 4), window_size=7, num_classes=10).eval()


def calibrate(model, x, device="cpu"):
    """W4A4, one search round of two steps, as tests/test_packed_cpu.py calibrates its toy"""
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    for p in model.parameters():
        p.data.mul_(8.0)
    model = wrap_modules_in_net(model.to(device), _cfg(), reparam=True).to(device)
    half = x.shape[0] // 2
    QuantCalibrator(model, [(x[:half], None), (x[half:], None)]).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model).to(device).eval()
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    return model


MAKERS = {"vit": (tiny_vit, 32), "swin": (tiny_swin, 56)}


@pytest.fixture(scope="module")
def toys(be):
    out = {}
    for kind, (make, size) in MAKERS.items():
        torch.manual_seed(5)
        x = torch.randn(4, 3, size, size, generator=torch.Generator().manual_seed(1))
        out[kind] = (calibrate(make(), x), x)
    return out


def _moded(model):
    return [(n, m) for n, m in model.named_modules() if hasattr(m, "mode")]


def _close(a, b, rel):
    return a == b or abs(a - b) <= rel * max(abs(a), abs(b))


@pytest.mark.parametrize("kind", ["vit", "swin"])
def test_report_visits_every_module_in_order_and_agrees_with_the_recomputation(toys, kind):
    from adalog_amd.utils.report import QUANTIZER_ATTRS, quant_report
    model, x = toys[kind]
    keep = {}
    rep = quant_report(model, x, tensors=keep)
    mods = _moded(model)
    assert list(rep["modules"]) == [n for n, _ in mods] and len(mods) >= 8
    assert rep["images"] == 4 and len(rep["logits"]["per_image"]) == 4
    want = RR.recompute(model, x)
    assert torch.equal(keep["logits_quant"], want["logits_quant"])
    counted = 0
    for name, m in mods:
        e, w = rep["modules"][name], want["modules"][name]
        assert e["type"] == type(m).__name__
        for which in ("cumulative", "local"):
            noise, signal, quant, mx = w[which].tolist()
            got = e[which]
            assert _close(got["noise"], noise, 1e-12) and _close(got["signal"], signal, 1e-12) and got["max_err"] == mx
            assert got["sqnr_db"] == pytest.approx(RR.sqnr_db(signal, noise), abs=1e-9)
        assert set(e["quantizers"]) == {a for a in QUANTIZER_ATTRS if hasattr(m, a)}
        for attr, qe in e["quantizers"].items():
            ref = w["quantizers"][attr]
            if ref is None:
                assert qe is None and e["skipped"][attr], (name, attr)
                continue
            counted += 1
            hist, row = ref
            q = getattr(m, attr)
            levels = 2 ** q.n_bits
            assert qe["hist"] == hist.tolist() and qe["elements"] == int(hist.sum()) and qe["n_bits"] == q.n_bits, (name, attr)
            h = hist.tolist()
            if qe["kind"] == "uniform":
                assert len(h) == levels + 2
                assert qe["clip_low"] == h[levels] / sum(h) and qe["clip_high"] == h[levels + 1] / sum(h)
                stored = [h[0] + h[levels]] + h[1:levels - 1] + [h[levels - 1] + h[levels + 1]]
            else:
                assert len(h) == levels + 1 and qe["clip_low"] == h[levels] / sum(h) and qe["clip_high"] is None
                stored = h
            assert qe["used_codes"] == sum(1 for c in stored[:levels] if c)
            assert qe["entropy_bits"] == pytest.approx(RR.entropy_bits(stored), abs=1e-12)
            assert _close(qe["noise"], float(row[0]), 1e-12) and _close(qe["signal"], float(row[1]), 1e-12) and qe["max_err"] == float(row[3])
    assert counted >= 12
    # the patch embedding's 8-bit input is not quantised: null, with the reason
    first = rep["modules"]["patch_embed.proj"]
    assert first["quantizers"]["a_quantizer"] is None and "8-bit" in first["skipped"]["a_quantizer"]
    if kind == "vit":
        assert first["quantizers"]["w_quantizer"] is not None
    else:                                                                    # 32 rows of 3 * 4 * 4 = 48 weights: a layout the kernel refuses
        assert first["quantizers"]["w_quantizer"] is None and "inner 48" in first["skipped"]["w_quantizer"]
    lb = want["logits"]["batch"].tolist()
    assert _close(rep["logits"]["batch"]["noise"], lb[0], 1e-12) and rep["logits"]["batch"]["max_err"] == lb[3]
    for got, row in zip(rep["logits"]["per_image"], want["logits"]["per_image"].tolist()):
        assert _close(got["noise"], row[0], 1e-12) and _close(got["signal"], row[1], 1e-12) and got["max_err"] == row[3]
    json.dumps(rep)                                                          # plain Python numbers only


def _same_err(a, b, rel=1e-12):
    assert _close(a["noise"], b["noise"], rel) and _close(a["signal"], b["signal"], rel), (a, b)
    assert _close(a["quant_energy"], b["quant_energy"], rel), (a, b)
    if rel == 1e-12:
        assert a["max_err"] == b["max_err"]


def _batch_dependent_modules(model, x):
    """Names of the moded modules whose OUTPUT torch computes differently for one image than for the same image inside the batch
    (this build's CPU Linear takes a matrix-vector route for a single row: the classifier head), in raw or quant_forward mode, plus
    every moded module downstream of one.  That is the model's forward, not the report: for these the all-at-once and the per-image
    forwards do not see the same fp32 tensors."""
    from adalog_amd.utils import models as M
    mods = _moded(model)
    bad, saved = set(), (M.QF_FUSED, [(m, m.mode) for _, m in mods])
    try:
        M.QF_FUSED = False
        for mode in ("raw", "quant_forward"):
            for _, m in mods:
                m.mode = mode
            runs = []
            for xs in [x] + [x[i:i + 1] for i in range(x.shape[0])]:
                rec = {}
                hs = [m.register_forward_hook(lambda mod, a, out, n=n: rec.__setitem__(n, out.detach().clone())) for n, m in mods]
                with torch.no_grad():
                    model(xs)
                for h in hs:
                    h.remove()
                runs.append(rec)
            seen_bad = False
            for n, _ in mods:
                seen_bad = seen_bad or not torch.equal(runs[0][n], torch.cat([r[n] for r in runs[1:]], 0))
                if seen_bad:
                    bad.add(n)
    finally:
        M.QF_FUSED = saved[0]
        for m, mode in saved[1]:
            m.mode = mode
    return bad


@pytest.mark.parametrize("kind", ["vit", "swin"])
def test_report_does_not_depend_on_the_chunk(toys, kind):
    """chunk=1 against all images at once: histograms equal, fp64 sums to 1e-12 relative, maxima equal -- wherever the model's forward
    gives the same fp32 tensors for an image alone and inside the batch.  Where torch itself does not (_batch_dependent_modules: only
    modules at the end of the network may be, and their entries are then held to 1e-6, the fp32 rounding of that forward), and in full
    against the four single-image reports merged by hand, which see the same forwards as chunk=1: sums add, histograms add, maxima max."""
    from adalog_amd.utils.report import quant_report
    model, x = toys[kind]
    whole, single = quant_report(model, x), quant_report(model, x, chunk=1)
    assert whole["chunk"] == 4 and single["chunk"] == 1
    assert list(whole["modules"]) == list(single["modules"])
    loose = _batch_dependent_modules(model, x)
    names = list(whole["modules"])
    assert len(loose) <= 2 and all(n in names[-2:] for n in loose), loose
    for name, a in whole["modules"].items():
        b = single["modules"][name]
        rel = 1e-6 if name in loose else 1e-12
        _same_err(a["cumulative"], b["cumulative"], rel)
        _same_err(a["local"], b["local"], rel)
        assert a["skipped"] == b["skipped"]
        for attr, qa in a["quantizers"].items():
            qb = b["quantizers"][attr]
            if qa is None:
                assert qb is None
                continue
            assert qa["hist"] == qb["hist"] and qa["used_codes"] == qb["used_codes"] and qa["entropy_bits"] == qb["entropy_bits"]
            assert qa["clip_low"] == qb["clip_low"] and qa["clip_high"] == qb["clip_high"]
            _same_err(qa, qb)
    rel = 1e-6 if loose else 1e-12
    _same_err(whole["logits"]["batch"], single["logits"]["batch"], rel)
    for a, b in zip(whole["logits"]["per_image"], single["logits"]["per_image"]):
        _same_err(a, b, rel)
    # the four single-image reports, merged by hand
    parts = [quant_report(model, x[i:i + 1]) for i in range(4)]

    def merged(get):
        es = [get(p) for p in parts]
        return {"noise": math.fsum(e["noise"] for e in es), "signal": math.fsum(e["signal"] for e in es),
                "quant_energy": math.fsum(e["quant_energy"] for e in es), "max_err": max(e["max_err"] for e in es)}

    for name, b in single["modules"].items():
        for which in ("cumulative", "local"):
            _same_err(merged(lambda p: p["modules"][name][which]), b[which])
        for attr, qb in b["quantizers"].items():
            if qb is None or attr == "w_quantizer":                          # (weights are counted once, whatever the chunk)
                continue
            assert qb["hist"] == [sum(c) for c in zip(*(p["modules"][name]["quantizers"][attr]["hist"] for p in parts))]
            _same_err(merged(lambda p: p["modules"][name]["quantizers"][attr]), qb)
    _same_err(merged(lambda p: p["logits"]["batch"]), single["logits"]["batch"])
    for i, b in enumerate(single["logits"]["per_image"]):
        _same_err(parts[i]["logits"]["per_image"][0], b)
    for name, e in parts[0]["modules"].items():
        if e["quantizers"].get("w_quantizer") is not None:
            assert e["quantizers"]["w_quantizer"] == single["modules"][name]["quantizers"]["w_quantizer"]


def test_switches_and_modes_are_restored_also_when_a_hook_raises(toys, be, monkeypatch):
    from adalog_amd.utils import models as M
    from adalog_amd.utils.report import quant_report
    model, x = toys["vit"]
    mods = _moded(model)
    modes = ["quant_forward" if i % 2 else "raw" for i in range(len(mods))]
    for (_, m), mode in zip(mods, modes):
        m.mode = mode
    monkeypatch.setattr(M, "QF_FUSED", True)
    monkeypatch.setattr(M, "QF_ATTN_CORE", True)
    monkeypatch.setattr(M, "QF_LONG", True)
    try:
        quant_report(model, x)
        assert (M.QF_FUSED, M.QF_ATTN_CORE, M.QF_LONG) == (True, True, True)
        assert [m.mode for _, m in mods] == modes
        real, calls = be.err_stats, []

        def failing(a, b, n_channels=1, inner=None):
            calls.append(1)
            if len(calls) == 20:                                             # inside the quant pass of the first chunk
                raise RuntimeError("boom")
            return real(a, b, n_channels, inner)
        monkeypatch.setattr(be, "err_stats", failing, raising=False)
        with pytest.raises(RuntimeError, match="boom"):
            quant_report(model, x, chunk=2)
        assert (M.QF_FUSED, M.QF_ATTN_CORE, M.QF_LONG) == (True, True, True)
        assert [m.mode for _, m in mods] == modes
        assert not any(m._forward_hooks or m._forward_pre_hooks for _, m in mods)
    finally:
        for _, m in mods:
            m.mode = "quant_forward"


def test_null_with_a_reason(toys):
    from adalog_amd.utils.report import quant_report
    model = copy.deepcopy(toys["vit"][0])
    x = toys["vit"][1]
    model.head.a_quantizer.n_bits = 32                                       # a 32-bit quantiser: the identity
    model.blocks[0].attn.proj.w_quantizer.n_bits = 32
    model.blocks[0].mlp.fc1.a_quantizer.init_training()
    model.blocks[1].attn.matmul1.A_quantizer.sym = True
    rep = quant_report(model, x)
    e = rep["modules"]["head"]
    assert e["quantizers"]["a_quantizer"] is None and "32-bit" in e["skipped"]["a_quantizer"]
    assert e["quantizers"]["w_quantizer"] is not None and "w_quantizer" not in e["skipped"]
    e = rep["modules"]["blocks.0.attn.proj"]
    assert e["quantizers"]["w_quantizer"] is None and "32-bit" in e["skipped"]["w_quantizer"]
    e = rep["modules"]["blocks.0.mlp.fc1"]
    assert e["quantizers"]["a_quantizer"] is None and "training" in e["skipped"]["a_quantizer"]
    e = rep["modules"]["blocks.1.attn.matmul1"]
    assert e["quantizers"]["A_quantizer"] is None and "symmetric" in e["skipped"]["A_quantizer"]
    assert e["quantizers"]["B_quantizer"] is not None
    # a per-channel activation quantiser (inner = 1): the layout the kernel refuses
    fc1 = model.blocks[1].mlp.fc1
    aq = fc1.a_quantizer
    aq.scale = torch.nn.Parameter(aq.scale.data.reshape(1).repeat(fc1.in_features))
    aq.zero_point = torch.nn.Parameter(aq.zero_point.data.reshape(1).repeat(fc1.in_features))
    rep = quant_report(model, x)
    e = rep["modules"]["blocks.1.mlp.fc1"]
    assert e["quantizers"]["a_quantizer"] is None and "inner 1" in e["skipped"]["a_quantizer"]


def test_command_line_round_trips_through_plain_and_packed_checkpoints(be, tmp_path, capsys):
    from adalog_amd.utils import packed as P
    from adalog_amd.utils import report as R
    from adalog_amd.utils.models import create_model
    torch.manual_seed(3)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(2))
    model = calibrate(create_model("deit_tiny", depth=1, img_size=32).eval(), x)
    plain, packed, grid = (str(tmp_path / n) for n in ("plain.pth", "packed.pth", "grid.pth"))
    torch.save(model.state_dict(), plain)
    P.save_packed(model, packed)
    # the packed checkpoint holds the weights on their quantisers' grids; its plain twin is the state_dict of the model it loads into
    twin = P.load_packed(P.build_wrapped("deit_tiny", CFG4, "cpu", img_size=32, depth=1), packed, "cpu")
    torch.save(twin.state_dict(), grid)
    common = ["--model", "deit_tiny", "--depth", "1", "--img-size", "32", "--config", CFG4, "--images", "3", "--seed", "7", "--device", "cpu"]
    outs = {}
    for tag, ckpt, extra in (("plain", plain, []), ("grid", grid, []), ("packed", packed, ["--packed"])):
        out = str(tmp_path / f"{tag}.json")
        assert R.main(common + ["--checkpoint", ckpt, "--out", out] + extra) == 0
        text = capsys.readouterr().out
        outs[tag] = json.load(open(out))
        names = list(outs[tag]["modules"])
        lines = text.splitlines()
        assert all(any(ln.startswith(n + " ") for ln in lines) for n in names), text     # one line per module
        assert sum("w_quantizer" in ln for ln in lines) == sum(hasattr(m, "w_quantizer") for m in model.modules())
        assert any(ln.startswith("logits (3 images)") for ln in lines)
    # the same weights in both formats: the same JSON
    assert outs["grid"] == outs["packed"]
    # against the fp32 weights the packed model's quant path is the same (every code histogram), its FP path is not (rebuilt weights)
    for name, e in outs["plain"]["modules"].items():
        for attr, qe in e["quantizers"].items():
            qp = outs["packed"]["modules"][name]["quantizers"][attr]
            assert (qe is None) == (qp is None)
            if qe is not None:
                # (a rebuilt weight sits on the grid: what the fp32 weight had beyond a clamp is on the end code there)
                fold = lambda q: q["hist"] if q["kind"] != "uniform" else \
                    [q["hist"][0] + q["hist"][-2]] + q["hist"][1:-3] + [q["hist"][-3] + q["hist"][-1]]
                assert fold(qe) == fold(qp) and qe["used_codes"] == qp["used_codes"], (name, attr)
