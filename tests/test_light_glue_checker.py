"""CPU: tests/light_glue_checker.py (the contracts of the light-side glue operators in torch, own code) against the fixtures the
UNMODIFIED reference produced in fp32 and fp64 (oracle/make_golden_light_glue.py -> tests/golden/g18_lightglue_*.npz):

  * in fp64 it matches every fp64 fixture to 1e-12 (rel-L2; relative for the scalars of the albedo scale);
  * in fp32 it takes the branches the reference's fp32 run took;
  * the fixtures reach the paths they are named for, the encoder lattice holds every interpolation phase and both clamped borders;
  * the margin condition: on every regression and albedo-scale input the GPU tests use, each branch quantity (det / n against 1e-2, a11
    and the second denominator against 1e-5, cSpec against 1e-3) is at least a factor 2 from its threshold in BOTH precisions."""
import os

import numpy as np
import pytest
import torch

import light_glue_checker as LG
from conftest import GOLDEN_DIR, rel_l2

PIN = 1e-12
F32, F64 = torch.float32, torch.float64


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g18_lightglue_{name}.npz"))


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


SHADING_TAGS = ["k13", "k24w", "k24", "k24one", "k1", "k1one"]
SCALE_TAGS = ["nospec", "clip_lo", "clip_hi", "noclip", "clip_hi_dark", "big"]
DS_TAGS = [f"ds_{k}_12x16" for k in LG.DIFFSPEC_BRANCH_CASES + ("cd_0001",)] + ["ds_regular_1x1"]
LS_TAGS = ["ls_regular", "ls_clamp_lo", "ls_clamp_hi", "ls_floor"]


def test_fixture_lists_are_complete():
    assert load("shading")["tags"].tolist() == SHADING_TAGS and load("scale")["tags"].tolist() == SCALE_TAGS
    z = load("regress")
    assert z["ds_tags"].tolist() == DS_TAGS and z["ls_tags"].tolist() == LS_TAGS


# ---- shading ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", SHADING_TAGS)
def test_shading_checker_is_pinned_to_the_reference(tag):
    z = load("shading")
    K, R, C, eh, ew = [int(v) for v in z[tag + "_cfg"]]
    got = LG.shading(z[tag + "_pred"], eh, ew, K, 1, F64)
    assert tuple(got.shape) == (1, 3, R, C)
    assert err(got[0], z[tag + "_ref64"]) <= PIN
    assert rel_l2(LG.shading(z[tag + "_pred"], eh, ew, K, 1, F32)[0], z[tag + "_ref32"]) <= 1e-5
    # premap = 0 takes the mapped lamb / weight
    p = torch.from_numpy(z[tag + "_pred"]).double()
    p[:, 3 * K:] = torch.tan(np.pi / 2.0 * (p[:, 3 * K:] * 0.999))
    assert err(LG.shading(p, eh, ew, K, 0, F64), got) <= PIN


def test_shading_fixtures_reach_the_second_lobe_instantiation():
    z = load("shading")
    cfgs = {tuple(int(v) for v in z[t + "_cfg"]) for t in SHADING_TAGS}
    assert {(13, 5, 13, 8, 16), (24, 5, 13, 16, 32), (24, 5, 13, 8, 16), (24, 1, 1, 8, 16)} <= cfgs
    assert any(c[0] == 1 for c in cfgs) and any(c[1:3] == (1, 1) for c in cfgs)


# ---- albedo scale -------------------------------------------------------------------------------------------------------------------------
def _ref_branch(ref, albedo):
    cLight, cAlbedo, cDiff, cSpec = [float(v) for v in ref]
    if cSpec < 1e-3:
        return "nospec"
    if cAlbedo == 1e-3:
        return "clip_lo"
    return "clip_hi" if cAlbedo == 1 / float(albedo.max()) else "noclip"


@pytest.mark.parametrize("tag", SCALE_TAGS)
def test_albedo_scale_checker_is_pinned_to_the_reference(tag):
    z = load("scale")
    args = [z[f"{tag}_{k}"] for k in ("diffuseNew", "diffuse", "specNew", "spec", "albedo")]
    got64, br64 = LG.albedo_scale(*args, dtype=F64)
    for g, r in zip(got64, z[tag + "_ref64"]):
        assert abs(g - r) <= PIN * abs(r), (tag, got64, z[tag + "_ref64"])
    got32, br32 = LG.albedo_scale(*args, dtype=F32)
    assert br32 == br64 == _ref_branch(z[tag + "_ref32"], args[4]) == _ref_branch(z[tag + "_ref64"], args[4])
    for g, r in zip(got32, z[tag + "_ref32"]):
        assert abs(g - r) <= 1e-6 * abs(r)
    assert LG.albedo_scale_margins_ok(*args)[0]


def test_albedo_scale_fixtures_cover_every_branch_and_two_sizes():
    z = load("scale")
    seen = {_ref_branch(z[t + "_ref64"], z[t + "_albedo"]) for t in SCALE_TAGS}
    assert seen == {"nospec", "clip_lo", "clip_hi", "noclip"}
    assert {z[t + "_diffuse"].size for t in SCALE_TAGS} == {576, 3 * 74 * 74}
    assert 3 * 74 * 74 > 64 * 256                       # more than one step of the 64 x 256 grid-stride loop


# ---- regressions --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", DS_TAGS)
def test_diffspec_checker_is_pinned_to_the_reference(tag):
    z = load("regress")
    d, s, i = z[tag + "_diff"], z[tag + "_spec"], z[tag + "_im"]
    for name, dt, tol in (("64", F64, PIN), ("32", F32, 1e-5)):
        coef, _ = LG.diffspec_coef(d, s, i, dt)
        v = coef.double().reshape(-1, 2, 1, 1, 1)
        assert err(v[:, 0] * torch.from_numpy(d).double(), z[f"{tag}_diffScaled{name}"]) <= tol, (tag, name)      # 1e-5 in fp32: the same branch
        assert err(v[:, 1] * torch.from_numpy(s).double(), z[f"{tag}_specScaled{name}"]) <= tol, (tag, name)
    ok, rep = LG.diffspec_margins_ok(d, s, i)
    assert ok, rep


def test_diffspec_fixtures_reach_the_paths_they_are_named_for():
    z = load("regress")
    info = {t: LG.diffspec_coef(z[t + "_diff"], z[t + "_spec"], z[t + "_im"], F64)[1] for t in DS_TAGS}
    one = lambda t, k: float(info[t][k][0])
    assert one("ds_regular_12x16", "det_over_n") > 2e-2 and one("ds_regular_1x1", "det_over_n") > 2e-2
    for t in ("ds_spec_small_12x16", "ds_spec_parallel_12x16", "ds_cd_1000_12x16", "ds_cd_0001_12x16", "ds_all_masked_12x16"):
        assert one(t, "det_over_n") < 5e-3 and np.abs(z[t + "_specScaled64"]).max() == 0.0
    assert one("ds_cs_zero_12x16", "det_over_n") > 2e-2 and one("ds_cs_zero_12x16", "cs_raw") < -0.1 and one("ds_cs_zero_12x16", "cs") == 0.0
    assert one("ds_cd_1000_12x16", "cd") == 1000.0 and one("ds_cd_0001_12x16", "cd") == 0.001
    assert one("ds_all_masked_12x16", "a11") == 0.0 and z["ds_all_masked_12x16_im"].min() >= 0.9
    assert one("ds_all_masked_12x16", "cim") == 1000.0
    assert z["ds_regular_1x1_diff"].shape == (1, 3, 1, 1)


@pytest.mark.parametrize("tag", LS_TAGS)
def test_lsregress_checker_is_pinned_to_the_reference(tag):
    z = load("regress")
    p, g = z[tag + "_pred"], z[tag + "_gt"]
    c64, info = LG.lsregress_coef(p, g, F64)
    assert abs(float(c64[0]) - z[tag + "_coef64"][0]) <= PIN * z[tag + "_coef64"][0]
    assert err(c64.reshape(1, 1, 1, 1) * torch.from_numpy(p).double(), z[tag + "_scaled64"]) <= PIN
    c32, _ = LG.lsregress_coef(p, g, F32)
    assert abs(float(c32[0]) - z[tag + "_coef32"][0]) <= 1e-5 * z[tag + "_coef32"][0]
    assert LG.lsregress_margins_ok(p, g)[0]
    want = dict(ls_clamp_lo=0.001, ls_clamp_hi=1000.0).get(tag)
    if want is not None:
        assert float(c64[0]) == want and z[tag + "_coef32"][0] == np.float64(np.float32(want))
    if tag == "ls_floor":
        assert float(info["den"][0]) < 5e-6


# ---- encoder input ------------------------------------------------------------------------------------------------------------------------
def test_encoder_input_checker_is_pinned_to_the_reference():
    z = load("encoder")
    args = [z[k] for k in ("im", "albedo_raw", "normalPred", "roughPred", "depth_raw")]
    out, alb_n, dep_n = LG.encoder_input(*args, size=(480, 640), dtype=F64)
    rows, cols = torch.from_numpy(z["rows"]), torch.from_numpy(z["cols"])
    lat = out[:, :, rows][:, :, :, cols]
    for g, (a, b) in LG.GROUPS.items():
        for img in range(out.shape[0]):
            assert err(lat[img, a:b], z["ref64_light_in"][img, a:b]) <= PIN, (g, img)
    assert err(out.sum(dim=(2, 3)), z["ref64_sum"][0]) <= PIN and err((out ** 2).sum(dim=(2, 3)), z["ref64_sum"][1]) <= PIN
    out32, _, _ = LG.encoder_input(*args, size=(480, 640), dtype=F32)
    assert rel_l2(out32[:, :, rows][:, :, :, cols], z["ref32_light_in"]) <= 1e-6
    assert bool(torch.isfinite(out).all()) and float(alb_n[1].abs().max()) == 0.0 and float(dep_n.min()) >= 0.0


def test_encoder_fixture_holds_the_floor_the_borders_and_every_phase():
    z = load("encoder")
    assert z["im"].shape == (2, 3, 32, 48) and np.abs(z["albedo_raw"][1]).max() == 0.0 and z["albedo_raw"][0].mean() > 0.01
    assert np.abs(z["ref64_light_in"][1, 3:6]).max() == 0.0
    rows, cols = z["rows"].tolist(), z["cols"].tolist()
    assert {0, 1, 478, 479} <= set(rows) and {0, 1, 638, 639} <= set(cols)
    assert {r % 15 for r in rows} == set(range(15))                      # 480 / 32: the source position repeats every 15 rows
    assert {c % 40 for c in cols} == set(range(40))                      # 640 / 48 = 40 / 3: every 40 columns
    assert z["ref64_light_in"].shape == (2, 11, len(rows), len(cols)) and z["ref64_light_in"].dtype == np.float64
    for k in ("im", "albedo_raw", "normalPred", "roughPred", "depth_raw"):
        assert z[k].dtype == np.float32


# ---- the margin condition on every checker-driven input of the GPU tests ------------------------------------------------------------------
@pytest.mark.parametrize("kinds,R,C,seed", LG.DIFFSPEC_BATCHES)
def test_margin_condition_diffspec(kinds, R, C, seed):
    d, s, i = LG.diffspec_batch(kinds, R, C, seed)
    ok, rep = LG.diffspec_margins_ok(d, s, i)
    assert ok, rep
    i32, i64 = LG.diffspec_coef(d, s, i, F32)[1], LG.diffspec_coef(d, s, i, F64)[1]
    assert torch.equal(i32["two"], i64["two"]) and LG.diffspec_raw_clear(i32) and LG.diffspec_raw_clear(i64)
    for b, k in enumerate(kinds):      # each image is the case it is named for
        assert LG.diffspec_case_is(k, i64, b) and LG.diffspec_case_is(k, i32, b), (k, float(i64["det_over_n"][b]))


@pytest.mark.parametrize("kinds,n,seed", LG.LSREGRESS_BATCHES)
def test_margin_condition_lsregress(kinds, n, seed):
    p, g = LG.lsregress_batch(kinds, n, seed)
    ok, rep = LG.lsregress_margins_ok(p, g)
    assert ok, rep
    for dt in (F32, F64):
        c, info = LG.lsregress_coef(p, g, dt)
        for b, k in enumerate(kinds):
            raw = float(info["raw"][b])
            assert not (0.9e-3 < raw < 1.1e-3) and not (900 < raw < 1100)
            assert (float(c[b]) == (0.001 if dt == F64 else float(np.float32(0.001)))) == (k == "clamp_lo") and (float(c[b]) == 1000.0) == (k == "clamp_hi")
            assert (float(info["den"][b]) < 1e-5) == (k == "floor")


@pytest.mark.parametrize("n,where,branch", LG.SCALE_CASES)
def test_margin_condition_albedo_scale(n, where, branch):
    args = LG.scale_case(n, where, branch, 7000 + n)
    ok, rep = LG.albedo_scale_margins_ok(*args)
    assert ok, rep
    (_, cAlbedo, _, cSpec), br = LG.albedo_scale(*args, dtype=F64)
    assert (cSpec < 1e-3) == (branch == "nospec")
    if where == "negative":
        assert cAlbedo < 0 and float(args[4].max()) < 0          # np.clip with hi < lo returns hi: 1 / max, negative
    else:
        assert br == branch and float(args[4].max()) == 0.8125
