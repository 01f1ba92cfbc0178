"""Bit plans without a device: the allocator of adalog_amd/utils/bitplan.py against brute force (tests/bitplan_reference.py), its
coarsened-unit path, plan_bits and the refactored capture loop of utils/gptq.py on a stand-in backend (tests/bitplan_cpu_backend.py),
and cfg.w_bit_plan through wrap_modules_in_net."""
import copy
import random

import numpy as np
import pytest
import torch

from adalog_amd import backend
from tests import bitplan_reference as BR
from tests import gptq_reference as GR
from tests.bitplan_cpu_backend import BitplanCpuBackend
from tests.test_packed_cpu import _cfg, _fresh

WIDTHS = (3, 4, 6)


# ------------------------------------------------------------------------------------------------ the allocator
def _instance(seed):
    """<= 6 layers x 3 widths: sizes that share a gcd, costs that fall with the width at layer-specific rates"""
    rng = random.Random(seed)
    L = rng.randint(2, 6)
    sizes = [32 * rng.randint(1, 9) for _ in range(L)]
    costs = []
    for _ in range(L):
        a = rng.uniform(0.1, 10.0)
        costs.append([a * 4.0 ** -b * rng.uniform(0.7, 1.3) for b in WIDTHS])
    return sizes, costs


def _total(costs, plan):
    return sum(c[WIDTHS.index(b)] for c, b in zip(costs, plan))


@pytest.mark.parametrize("seed", range(12))
def test_allocator_equals_brute_force(seed):
    from adalog_amd.utils.bitplan import allocate
    sizes, costs = _instance(seed)
    kinds = set()
    for avg in (3.0, 3.2, 3.5, 4.0, 4.6, 5.2, 6.0, 7.0):
        want = BR.brute_force(sizes, costs, WIDTHS, avg)
        got = allocate(sizes, costs, WIDTHS, avg)
        assert tuple(got) == want[0], (avg, got, want)
        assert sum(n * b for n, b in zip(sizes, got)) <= avg * sum(sizes)
        for b in WIDTHS:                                                        # never worse than a uniform width that fits
            if b <= avg:
                assert _total(costs, got) <= _total(costs, [b] * len(sizes))
        kinds.add("low" if set(got) == {3} else "high" if set(got) == {6} else "between")
    assert kinds == {"low", "high", "between"}


def test_allocator_tie_breaks_and_infeasible_budget():
    from adalog_amd.utils.bitplan import allocate
    # integer costs, equal sizes.  Budget 8 bits over two layers: (3, 4) and (4, 4) both cost 2, (3, 3) and (4, 3) cost 3 -> fewer bits
    sizes, costs = [64, 64], [[1.0, 1.0, 0.0], [2.0, 1.0, 0.0]]
    assert allocate(sizes, costs, WIDTHS, 4.0) == [3, 4] == list(BR.brute_force(sizes, costs, WIDTHS, 4.0)[0])
    # budget 7 bits: (3, 4) and (4, 3) both cost 3 at 7 bits, (3, 3) costs 4 -> the lexicographically smaller tuple
    costs = [[2.0, 1.0, 0.0], [2.0, 1.0, 0.0]]
    assert allocate(sizes, costs, WIDTHS, 3.5) == [3, 4] == list(BR.brute_force(sizes, costs, WIDTHS, 3.5)[0])
    # ... and it is the tuple that decides, not the layer order of the costs: with layer 1 cheaper at 4 bits, (4, 3) loses on cost
    assert allocate(sizes, [[2.0, 1.0, 0.0], [2.0, 0.5, 0.0]], WIDTHS, 3.5) == [3, 4]
    assert allocate(sizes, [[2.0, 0.5, 0.0], [2.0, 1.0, 0.0]], WIDTHS, 3.5) == [4, 3]
    costs = [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]                # all equal: the fewest bits
    assert allocate([32, 64, 96], costs, WIDTHS, 6.0) == [3, 3, 3]
    # the widths may come in any order: the tie-break is on the widths, not on their positions
    assert allocate(sizes, [[0.0, 1.0, 2.0], [0.0, 1.0, 2.0]], (6, 4, 3), 3.5) == [3, 4]
    with pytest.raises(ValueError):
        allocate(sizes, costs[:2], WIDTHS, 2.9)
    assert allocate([], [], WIDTHS, 4.0) == []


@pytest.mark.parametrize("seed", range(6))
def test_coarsened_units_never_exceed_the_budget(seed, caplog):
    import logging
    from adalog_amd.utils.bitplan import allocate
    rng = random.Random(100 + seed)
    L = 6
    sizes = [rng.randint(1000, 9000) for _ in range(L)]                         # gcd 1 almost surely: a table of ~10^5 cells
    costs = [[rng.uniform(0.1, 10.0) * 4.0 ** -b for b in WIDTHS] for _ in range(L)]
    for avg in (3.3, 4.0, 5.0):
        with caplog.at_level(logging.INFO):
            caplog.clear()
            got = allocate(sizes, costs, WIDTHS, avg, max_cells=2000)
        assert any("rounded up" in r.getMessage() for r in caplog.records)
        assert sum(n * b for n, b in zip(sizes, got)) <= avg * sum(sizes)
        exact = allocate(sizes, costs, WIDTHS, avg)
        assert _total(costs, exact) <= _total(costs, got) + 1e-12               # the coarse problem is a tighter one
        assert sum(n * b for n, b in zip(sizes, exact)) <= avg * sum(sizes)


# ------------------------------------------------------------------------------------------------ plan_bits, host logic
@pytest.fixture(scope="module")
def be():
    impl = BitplanCpuBackend()
    backend.set_backend(impl)
    yield impl
    backend.set_backend(None)


def _tiny_cfg():
    cfg = _cfg(4)
    return cfg


@pytest.fixture(scope="module")
def tiny(be):
    """a wrapped, uncalibrated depth-2 deit_tiny and two images"""
    from adalog_amd.utils.models import create_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net
    torch.manual_seed(3)
    model = wrap_modules_in_net(create_model("deit_tiny", depth=2).eval(), _tiny_cfg(), reparam=False).eval()
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(3))
    return model, x


def test_minmax_scales_are_the_reference_quantiser():
    from adalog_amd.utils.bitplan import minmax_scales
    W = np.random.default_rng(0).standard_normal((7, 32)).astype(np.float32)
    W[3] = 0.25                                                                 # a constant row: s = 1, z = 0
    s, z = minmax_scales(torch.from_numpy(W), (0, 3, 4, 6))
    S, Z = BR.minmax_params(W, (0, 3, 4, 6))
    assert np.array_equal(s.numpy(), S) and np.array_equal(z.numpy(), Z)
    assert (S[:, 3] == 1).all() and (Z[:, 3] == 0).all() and (S[0] == 1).all()


def test_plan_bits_host_logic(tiny, be):
    from adalog_amd.utils.bitplan import CONV_REASON, plan_bits
    model, x = tiny
    mods = dict(model.named_modules())
    linear = [n for n, m in mods.items() if isinstance(m, torch.nn.Linear) and hasattr(m, "w_quantizer")]
    hooks = {n: len(m._forward_hooks) for n, m in mods.items()}
    modes = {n: m.mode for n, m in mods.items() if hasattr(m, "mode")}
    weights = {n: mods[n].weight.data.clone() for n in linear}
    be.costs.clear()
    res = plan_bits(model, x, widths=WIDTHS, avg_bits=4.0, batch_size=1, keep=("head",))
    planned = [n for n in linear if "head" not in n]
    assert len(planned) == 8 and list(res["plan"]) == planned == list(res["layers"])
    assert set(res["skipped"]) == {"patch_embed.proj", "head"} and res["skipped"]["patch_embed.proj"] == CONV_REASON
    assert "head" in res["skipped"]["head"]
    assert res["avg_bits"] <= res["avg_bits_target"] == 4.0 and set(res["plan"].values()) <= set(WIDTHS)
    assert be.costs == [(mods[n].out_features, mods[n].in_features, (0,) + WIDTHS) for n in planned]    # one launch per layer
    sizes = [mods[n].out_features * mods[n].in_features for n in planned]
    assert res["avg_bits"] == sum(n * res["plan"][k] for n, k in zip(sizes, planned)) / sum(sizes)
    for n in planned:
        e = res["layers"][n]
        assert (e["R"], e["K"], e["bits"]) == (mods[n].out_features, mods[n].in_features, res["plan"][n])
        assert e["signal"] > 0 and e["cost"][3] > e["cost"][4] > e["cost"][6] > 0
    total = sum(res["layers"][n]["cost"][b] for n, b in res["plan"].items())
    assert total <= res["uniform"][4] and total <= res["uniform"][3] and set(res["uniform"]) == set(WIDTHS)
    costs = [[res["layers"][n]["cost"][b] for b in WIDTHS] for n in planned]
    assert tuple(res["plan"].values()) == BR.brute_force(sizes, costs, WIDTHS, 4.0)[0]
    # nothing of the model changed
    assert {n: len(m._forward_hooks) for n, m in mods.items()} == hooks
    assert {n: m.mode for n, m in mods.items() if hasattr(m, "mode")} == modes
    assert all(torch.equal(mods[n].weight.data, weights[n]) for n in linear)
    # the cost is the reference's under the Hessian of the FP input, normalised by the signal
    got = []
    h = mods["blocks.1.mlp.fc2"].register_forward_hook(lambda m, a, o: got.append(a[0].reshape(-1, m.in_features).double()))
    with torch.no_grad():
        model(x)
    h.remove()
    H = (got[0].t() @ got[0]).numpy()
    W = weights["blocks.1.mlp.fc2"].numpy()
    S, Z = BR.minmax_params(W, (0,) + WIDTHS)
    c, _ = BR.bit_cost(W, S, Z, (0,) + WIDTHS, H)
    e = res["layers"]["blocks.1.mlp.fc2"]
    np.testing.assert_allclose(e["signal"], c[0].sum(), rtol=1e-9)
    np.testing.assert_allclose([e["cost"][b] for b in WIDTHS], c[1:].sum(axis=1) / c[0].sum(), rtol=1e-9)
    raw = plan_bits(model, x, widths=WIDTHS, avg_bits=4.0, batch_size=2, normalise="none", keep=("head",))
    np.testing.assert_allclose([raw["layers"]["blocks.1.mlp.fc2"]["cost"][b] for b in WIDTHS], c[1:].sum(axis=1), rtol=1e-9)
    with pytest.raises(ValueError):
        plan_bits(model, x, widths=(3, 8), avg_bits=4.0)
    with pytest.raises(ValueError):
        plan_bits(model, x, widths=WIDTHS, avg_bits=2.5)


def test_gptq_model_sweeps_what_the_reference_sweeps_after_the_capture_refactor(be):
    """gptq_model on the shared capture helper: the committed weights are, bit for bit, the reference sweep under the Hessian of
    quant_input(x) that the loop this helper replaced accumulated (restated here with a plain hook)."""
    from adalog_amd.utils.calibrator import QuantCalibrator
    from adalog_amd.utils.gptq import damped_factor, gptq_model
    from adalog_amd.utils.wrap_net import wrap_modules_in_net, wrap_reparamed_modules_in_net
    model = wrap_modules_in_net(_fresh(), _cfg(), reparam=True)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    QuantCalibrator(model, [(x[:2], None), (x[2:], None)]).batching_quant_calib()
    model = wrap_reparamed_modules_in_net(model)
    for m in model.modules():
        if hasattr(m, "reparam_bias"):
            m.reparam_bias()
    src = copy.deepcopy(model)
    names = ["blocks.0.attn.qkv", "blocks.0.attn.proj", "blocks.0.mlp.fc1", "blocks.0.mlp.fc2", "head"]
    res = gptq_model(model, x, damp=0.01, batch_size=3)
    assert list(res["layers"]) == names and set(res["skipped"]) == {"patch_embed.proj"}
    assert set(res) == {"images", "damp", "layers", "skipped", "seconds"} and set(res["seconds"]) == {"capture", "factor", "sweep"}
    # the loop as it was: raw mode, a hook per layer, batches of 3 + 1 images
    smods = dict(src.named_modules())
    for mm in src.modules():
        if hasattr(mm, "mode"):
            mm.mode = "raw"
    hess = {n: torch.zeros(smods[n].in_features, smods[n].in_features, dtype=torch.float64) for n in names}
    def hook(n):
        def capture(m, a, o):
            be.gptq_hessian_add(hess[n], m.quant_input(a[0]).reshape(-1, m.in_features))
        return capture
    handles = [smods[n].register_forward_hook(hook(n)) for n in names]
    with torch.no_grad():
        src(x[:3]); src(x[3:])
    for h in handles:
        h.remove()
    mods = dict(model.named_modules())
    for n in names:
        U, _ = damped_factor(hess[n], 0.01)
        wq = smods[n].w_quantizer
        want, _, obj = GR.sweep(smods[n].weight.data.numpy(), wq.scale.data.reshape(-1).numpy(), wq.zero_point.data.reshape(-1).numpy(),
                                int(wq.n_bits), U.numpy())
        assert np.array_equal(want.view(np.int32), mods[n].weight.data.numpy().view(np.int32)), n
        assert res["layers"][n]["objective_after"] == float(torch.from_numpy(obj).sum())     # (summed as gptq_model sums it)
    assert all(m.mode == "quant_forward" for m in model.modules() if hasattr(m, "mode"))


# ------------------------------------------------------------------------------------------------ cfg.w_bit_plan
def _widths(model):
    return {n: (type(m).__name__, int(m.w_quantizer.n_bits)) for n, m in model.named_modules() if hasattr(m, "w_quantizer")}


@pytest.mark.parametrize("reparam", [True, False])
def test_wrap_modules_in_net_takes_a_bit_plan(reparam):
    from adalog_amd.utils.wrap_net import wrap_modules_in_net
    plain = _widths(wrap_modules_in_net(_fresh(), _cfg(), reparam=reparam))
    assert {b for _, b in plain.values()} == {6}
    cfg = _cfg()
    assert not hasattr(cfg, "w_bit_plan")
    plan = {"blocks.0.attn.qkv": 3, "blocks.0.attn.proj": 4, "blocks.0.mlp.fc1": 2, "blocks.0.mlp.fc2": 7, "head": 5}
    cfg.w_bit_plan = dict(plan)
    model = wrap_modules_in_net(_fresh(), cfg, reparam=reparam)
    got = _widths(model)
    assert {n: c for n, (c, _) in got.items()} == {n: c for n, (c, _) in plain.items()}        # the same classes
    assert {n: b for n, (_, b) in got.items()} == dict(plan, **{"patch_embed.proj": 6})
    assert cfg.w_bit_plan == plan
    cfg.w_bit_plan = {"head": 4}                                                # a partial plan: the rest keeps cfg.w_bit
    part = _widths(wrap_modules_in_net(_fresh(), cfg, reparam=reparam))
    assert {n: b for n, (_, b) in part.items()} == {n: (4 if n == "head" else 6) for n in plain}
    for bad in ({"blocks.0.attn.nope": 4}, {"patch_embed.proj": 4}, {"blocks.0": 4}, {"head": 1}, {"head": 8}, {"head": 4.5}, {"head": True}):
        cfg.w_bit_plan = bad
        with pytest.raises(ValueError):
            wrap_modules_in_net(_fresh(), cfg, reparam=reparam)
    for empty in (None, {}):                                                    # no plan: exactly as before
        cfg.w_bit_plan = empty
        assert _widths(wrap_modules_in_net(_fresh(), cfg, reparam=reparam)) == plain


def test_bit_plan_files_load(tmp_path):
    import json
    from adalog_amd.utils.packed import load_bit_plan, plan_kwargs
    p = tmp_path / "plan.json"
    p.write_text(json.dumps({"format": "adalog-bitplan-v1", "plan": {"head": 6, "blocks.0.attn.qkv": 3}, "avg_bits": 3.5}))
    assert load_bit_plan(str(p)) == {"head": 6, "blocks.0.attn.qkv": 3} and plan_kwargs(str(p)) == {"bit_plan": load_bit_plan(str(p))}
    assert plan_kwargs(None) == {}
    p.write_text(json.dumps({"head": 4}))
    assert load_bit_plan(str(p)) == {"head": 4}
    p.write_text(json.dumps({"format": "something-else", "plan": {}}))
    with pytest.raises(ValueError):
        load_bit_plan(str(p))
