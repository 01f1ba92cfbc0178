"""The case table of the scoring GEMM's edge suite (tests/gemm_cases.py) and its fp64 reference (tests/gemm_reference.py), checked where
no GPU is needed:
  * the reference against the specification tests/cpu_backend.gemm_score on every case: fp32 of the fp64 score, equal to 1 ulp;
  * every case's declared route against the limits of csrc/gemm_score.hip's *_ok functions, layout_of and pick_wide, restated here: a
    threshold that moves breaks the table here, not on the GPU;
  * sensitivity: two mutants computed from the reference's own e^2 must each move at least one score of the case by more than twice
    its bar --
      (a) one valid element dropped: row M - 1, last column, last group;
      (b) one masked element added: row M of a group's last row tile, last column -- the reference clamped to row M - 1 as the kernels
          clamp it, against the product of the row the tile holds there: the next group's first row where G >= 2 (added to group
          G - 2; in the ext cases the next group is the one with the 10^3 x larger values), else a row of zeros.
    In a ``hit`` case (b) must show at the planted candidate.  (a) cannot show there, whatever the shape: the planted candidate's
    e^2 is at most (2^-24 ref)^2 per element, below the k^2 u^2 a^2 >= (2^-24 ref)^2 share of the same element in its bar; (a) is
    asked of the case's other candidates.  Only ``nan`` cases opt out.
"""
import pytest
import torch

from tests import cpu_backend as CB
from tests import gemm_cases as T
from tests import gemm_reference as R


@pytest.fixture(scope="module")
def built():
    return {}


def _inputs(built, case):
    if case.id not in built:
        built.clear()                                       # one case's tensors at a time
        built[case.id] = T.inputs(case)
    return built[case.id]


def test_table_covers_every_route_in_three_kinds():
    for route in T.ROUTES:
        kinds = {c.kind for c in T.CASES if c.route == route}
        assert {"spread", "hit", "ext"} <= kinds, (route, kinds)
    fams = {c.route.split("<")[0] for c in T.CASES}
    assert fams == {c.route.split("<")[0] for c in T.CASES if c.kind == "nan"}
    assert all(c.opt_out == (c.kind == "nan") for c in T.CASES)
    assert len({c.id for c in T.CASES}) == len(T.CASES)


# ---------------------------------------------------------------------------------------------------------------- route limits
BK3 = 64                                                    # bytes of a K-step


def pick_wide(M, kvb):
    """gemm_score.hip pick_wide"""
    if kvb < 512 or M < 192:
        return 0
    up = lambda n: -(-M // n) * n
    pad4, pad3, pad2 = up(256), up(192), up(128)
    ri = 4 if pad4 <= pad3 + pad3 // 32 else 3
    padw = pad4 if ri == 4 else pad3
    return ri if padw <= pad2 + pad2 // 8 else 0


def expected_route(c):
    """route_of / layout_of with the default switches, for the launches of the table"""
    name = T.DT_NAME[c.dtype]
    N = c.ncols * (c.P if c.form != "grid" else 1)
    es = T.ESZ[c.dtype]
    kvb, kb = c.k_valid * es, c.K * es
    if c.form == "grid":
        assert c.C > 1
        return "k_gemm_score"
    cand_cols = c.form == "cols" and c.P in (64, 128, 256)
    reduce_cols = not c.keep_n
    grp_shape = (128 < c.M <= 224 and c.G >= 8 and c.gmod <= 16 and c.bias == "none" and not c.rows and c.attn and N % c.P == 0)
    win_shape = (4 <= c.M <= 64 and c.G >= 256 and c.gmod <= 32 and c.bias == "none" and not c.rows and c.attn and c.ncols <= 64)
    if c.dtype == T.BF16_FP8:
        wide = pick_wide(c.M, kvb)
        if c.k_valid > 256:
            return "k_gemm_stream<bf16xfp8>" if (cand_cols and wide and c.K % 64 == 0) else None
        if not (cand_cols and reduce_cols):
            return None
        if c.k_valid <= 64:
            return "k_gemm_winb<bf16xfp8>" if (win_shape and c.K == 64) else None
        if not (192 < c.k_valid <= 256 and grp_shape):
            return None
        if c.K == 208 and c.k_valid <= 208:
            return "k_gemm_grpk8t<%d,bf16xfp8>" % (13 if c.k_valid <= 200 else 14)
        return "k_gemm_grpk8<bf16xfp8>" if c.K == 256 else None
    wide = pick_wide(c.M, kvb) if cand_cols else 0
    stream = cand_cols
    if stream and c.dtype in (T.I8, T.FP8) and c.G == 1 and kvb > BK3 and c.M % 32 == 0 and c.M >= 768 and c.M * kb <= 16 << 20:
        if kb <= 6 * BK3:
            return "k_gemm_slab<%s>" % name
        if kb <= 12 * BK3 and c.P in (64, 128):
            return "k_gemm_slab128<%s>" % name
    acc = stream and reduce_cols
    byte_ops = c.dtype in (T.I8, T.FP8)
    if acc and byte_ops and kvb <= BK3 and win_shape:
        return "k_gemm_win<%s>" % name
    if acc and byte_ops and kvb <= BK3 and grp_shape:
        return "k_gemm_grpw<%s>" % name                      # (wave-private form: every wave owns one head, 4 waves x >= 16 workgroups)
    if acc and c.dtype == T.BF16 and 6 * BK3 < kvb <= 7 * BK3 and grp_shape:
        return "k_gemm_grpk<bf16>"
    if stream:
        return "k_gemm_stream<%s>" % name
    return "k_gemm_cand_glds" if c.dtype != T.FP8 else None


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_declared_route_limits(case):
    c = case
    assert expected_route(c) == c.route
    es = T.ESZ[c.dtype]
    assert 1 <= c.k_valid <= c.K and c.G % c.gmod == 0
    if c.dtype != T.BF16_FP8:
        assert (c.K * es) % 64 == 0 or (c.K * es == 32 and c.route.startswith("k_gemm_win<"))
        if not (c.form == "cols" and c.P in (64, 128, 256)):
            assert (c.K * es) % 128 == 0                    # 64-byte row padding: streaming shapes only
    if "stream" in c.route:
        wide = pick_wide(c.M, c.k_valid * es)
        assert (c.M >= 192) == bool(wide)                  # the table's narrow rows have M < 192, its wide rows K >= 512 bytes
    if c.route.startswith("k_gemm_slab"):
        units = -(-c.ncols * c.P // (256 if "128" not in c.route else 128)) * (c.M // 32)
        assert units <= 8 * 64                              # gemm_reference.chain: R = 8 units per workgroup on >= 64 CUs


# ---------------------------------------------------------------------------------------------------------------- reference vs specification
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_reference_equals_specification(built, case):
    i = _inputs(built, case)
    args, kw = T.call_args(case, i, CB)
    want = CB.gemm_score(*args, **kw)
    got = i["terms"]["score"].float()
    assert got.shape == want.shape == (case.cands, (case.gmod if case.keep_h else 1) * (case.ncols if case.keep_n else 1))
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert bool(((got[ok] - want[ok]).abs().double() <= R.ulp32(want[ok])).all())
    if case.kind == "nan":
        assert bool(torch.isnan(want).any()) and not bool(torch.isnan(want).all() and want.shape[1] > 1)
    else:
        assert bool(torch.isfinite(want).all())


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def mutants(case, t):
    """|score(mutant) - score| [cands, cols] for (a) and (b)"""
    c = case
    N = c.ncols
    e2 = t["e2"]
    za = torch.zeros_like(e2)
    za[:, c.G - 1, c.M - 1, N - 1] = e2[:, c.G - 1, c.M - 1, N - 1]
    zb = torch.zeros_like(e2)
    g = max(c.G - 2, 0)
    held = t["out"][:, g + 1, 0, N - 1] if c.G >= 2 else (t["out"] - t["lin"]).expand_as(e2)[:, 0, c.M - 1, N - 1]
    zb[:, g, c.M - 1, N - 1] = (t["r"][0, g, c.M - 1, N - 1] - held) ** 2
    return T.NORM * t["reduce"](za), T.NORM * t["reduce"](zb)


@pytest.mark.parametrize("case", [c for c in T.CASES if not c.opt_out], ids=lambda c: c.id)
def test_one_element_shows(built, case):
    i = _inputs(built, case)
    t = i["terms"]
    bar = T.case_bar(case, t)
    da, db = mutants(case, t)
    ra, rb = (da / bar), (db / bar)
    print(f"{case.id}: dropped element {float(ra.max()):.1f} x bar, masked element {float(rb.max()):.1f} x bar")
    assert float(ra.max()) > 2.0, (case.id, "a", float(ra.max()))
    assert float(rb.max()) > 2.0, (case.id, "b", float(rb.max()))
    if case.kind == "hit":
        cols = torch.arange(bar.shape[1])
        at = rb[i["planted"], cols]
        hit_cols = db[i["planted"], cols] > 0               # the score columns the mutated element belongs to
        assert bool(hit_cols.any()) and bool((at[hit_cols] > 2.0).all()), (case.id, at)
