"""GPU: the light-side glue kernels -- ``sgr.light_encoder_input`` (sgr_glue.hip: mean_stage, light_input_kernel), ``sgr.light_albedo_scale``
(scale_stage1 / 2), ``sgr.predToShading`` (shading_fast_kernel) and the coefficient operators ``torch.ops.sgrender.lsregress_coef`` /
``lsregress_diffspec_coef`` (sgr_loss.hip: dot2_partial, diffspec_partial_a, loss_stage_b, diffspec_finish) -- against
tests/light_glue_checker.py in fp64, which tests/test_light_glue_checker.py pins at 1e-12 to fixtures the unmodified reference produced
(tests/golden/g18_lightglue_*.npz), and against those fixtures themselves.

Bounds.  ``e_ref`` is the reference's own fp32-vs-fp64 distance: the fixture's where there is one, else the checker in fp32 against the
checker in fp64 on the same inputs.
  encoder input, normalised albedo / depth   rel-L2 per image and channel group <= max(2 e_ref, 1e-6); a group that is zero in fp64 is zero
  shading                                    rel-L2 per image <= max(2 e_ref, 1e-5) (the bound of tests/test_gpu_glue.py)
  scalars and coefficients                   conftest.scalar_close(got, ref64, |ref32 - ref64|, rtol=1e-5)
  a coefficient the fp64 checker puts on a clamp (0, 0.001, 1000; for the two-factor products: both factors on one) equals it exactly
Two runs, an image alone against its slice of the batch, and strided against contiguous inputs are bit for bit.  The whole result is
compared at every shape.  Every regression and albedo-scale input first passes the margin condition (each branch quantity a factor 2 from
its threshold in fp32 and in fp64), so no bound above is ever asked to decide a discontinuity.

The worst measured values per family are printed at the end of the module (``-s``), and written to the file ``SGR_LIGHT_GLUE_WORST`` names
if it is set; profiles/r13_light_glue_worst.txt is such a file."""
import os

import numpy as np
import pytest
import torch

import light_glue_checker as LG
from conftest import GOLDEN_DIR, rel_l2, scalar_close

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


WORST = {}      # family -> (measured / bound, measured, bound, case)


def note(family, measured, bound, case):
    ratio = measured / bound if bound > 0 else (0.0 if measured == 0 else float("inf"))
    if family not in WORST or ratio > WORST[family][0]:
        WORST[family] = (ratio, measured, bound, case)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    lines = ["worst measured value per family, against the fp64 checker (tests/light_glue_checker.py): family, measured, bound, case"]
    lines += [f"{k:28s} {v[1]:.3e}  <= {v[2]:.3e}   {v[3]}" for k, v in sorted(WORST.items())]
    print("\n" + "\n".join(lines))
    path = os.environ.get("SGR_LIGHT_GLUE_WORST")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g18_lightglue_{name}.npz"))


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


def check_scalar(family, case, got, ref64, ref32):
    got, ref64, e_ref = float(got), float(ref64), abs(float(ref32) - float(ref64))
    lim = max(2.0 * e_ref, 1e-5 * abs(ref64))
    print(f"{family} {case}: got {got!r} ref64 {ref64!r} |diff| {abs(got - ref64):.3e} bound {lim:.3e}")
    note(family, abs(got - ref64), lim, case)
    assert np.isfinite(got) and scalar_close(got, ref64, e_ref, rtol=1e-5), (family, case, got, ref64, lim)


# =========================================================================================================================================
# light_encoder_input
# =========================================================================================================================================
ENCODER_SHAPES = [((1, 1), (4, 6)), ((5, 7), (11, 13)), ((6, 10), (6, 10)), ((12, 20), (5, 7)), ((3, 50), (7, 300)), ((32, 48), (480, 640)),
                  ((74, 74), (37, 37)), ((130, 127), (9, 8))]


def encoder_inputs(h, w, seed):
    """bn = 3 distinct random images; image 1 has an all-zero albedo, image 2 a depth of mean 1e-12 (both below the 1e-10 mean floor)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda c: torch.rand(3, c, h, w, generator=g)
    im, albedo, normal, rough, depth = r(3), r(3), 2 * r(3) - 1, 2 * r(1) - 1, 3 * r(1) + 1
    albedo[1] = 0.0
    depth[2] = 2e-12 * torch.rand(1, h, w, generator=g)
    return [im, albedo, normal, rough, depth]


def compare_encoder(tag, got, ref64, ref32):
    out, alb_n, dep_n = [t.cpu() for t in got]
    assert all(bool(torch.isfinite(t).all()) for t in (out, alb_n, dep_n)), tag
    parts = [(g, out[:, a:b], ref64[0][:, a:b], ref32[0][:, a:b]) for g, (a, b) in LG.GROUPS.items()]
    parts += [("albedo_n", alb_n, ref64[1], ref32[1]), ("depth_n", dep_n, ref64[2], ref32[2])]
    for g, x, r64, r32 in parts:
        assert x.shape == r64.shape
        for b in range(x.shape[0]):
            if float(r64[b].abs().max()) == 0.0:
                assert float(x[b].abs().max()) == 0.0, (tag, g, b)
                continue
            e, lim = err(x[b], r64[b]), max(2.0 * err(r32[b], r64[b]), 1e-6)
            note("encoder_input " + g, e, lim, f"{tag} image {b}")
            assert e <= lim, (tag, g, b, e, lim)


@pytest.mark.parametrize("src,dst", ENCODER_SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in ENCODER_SHAPES])
def test_encoder_input_whole_tensor_vs_checker(sgr, src, dst):
    args = encoder_inputs(src[0], src[1], 100 + src[0])
    dev = [t.cuda() for t in args]
    got = sgr.light_encoder_input(*dev, size=dst)
    assert tuple(got[0].shape) == (3, 11) + dst and got[1].shape == args[1].shape and got[2].shape == args[4].shape
    ref64, ref32 = LG.encoder_input(*args, size=dst, dtype=F64), LG.encoder_input(*args, size=dst, dtype=F32)
    assert float(ref64[1][1].abs().max()) == 0.0 and float(args[4][2].mean()) < 1e-11          # both floors are live
    compare_encoder(f"{src}->{dst}", got, ref64, ref32)
    again = sgr.light_encoder_input(*dev, size=dst)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                                   # determinism
    for b in range(3):                                                                          # batch independence
        alone = sgr.light_encoder_input(*[t[b:b + 1] for t in dev], size=dst)
        assert all(torch.equal(a[0], x[b]) for a, x in zip(alone, got)), b


def test_encoder_input_vs_reference_fixture_whole_lattice(sgr):
    z = load("encoder")
    args = [torch.from_numpy(z[k]) for k in ("im", "albedo_raw", "normalPred", "roughPred", "depth_raw")]
    out, alb_n, _ = sgr.light_encoder_input(*[t.cuda() for t in args])
    lat = out.cpu()[:, :, torch.from_numpy(z["rows"])][:, :, :, torch.from_numpy(z["cols"])]
    assert float(alb_n[1].abs().max()) == 0.0
    for g, (a, b) in LG.GROUPS.items():
        for img in range(2):
            r64, r32 = z["ref64_light_in"][img, a:b], z["ref32_light_in"][img, a:b]
            if np.abs(r64).max() == 0.0:
                assert float(lat[img, a:b].abs().max()) == 0.0
                continue
            e, lim = err(lat[img, a:b], r64), max(2.0 * err(r32, r64), 1e-6)
            note("encoder_input " + g, e, lim, f"fixture image {img}")
            assert e <= lim, (g, img, e, lim)
    for k, power in ((0, 1), (1, 2)):                                                           # the whole tensor through its channel sums
        got = (out.double() ** power).sum(dim=(2, 3)).cpu().numpy()
        assert np.allclose(got, z["ref64_sum"][k], rtol=1e-5, atol=0.0)      # the rule of tests/test_gpu_glue.py


@pytest.mark.parametrize("src,dst", [((5, 7), (11, 13)), ((74, 74), (37, 37))])
def test_encoder_input_strided_inputs_give_the_same_bits(sgr, src, dst):
    args = [t.cuda() for t in encoder_inputs(src[0], src[1], 200 + src[0])]
    want = sgr.light_encoder_input(*args, size=dst)
    cl = [t.contiguous(memory_format=torch.channels_last) for t in args]
    assert not cl[0].is_contiguous()
    got = sgr.light_encoder_input(*cl, size=dst)
    assert all(torch.equal(a.contiguous(), b) for a, b in zip(got, want))
    padded = [torch.full((3, t.shape[1] + 1, src[0] + 3, src[1] + 5), float("nan"), device="cuda") for t in args]
    views = []
    for p, t in zip(padded, args):
        v = p[:, 1:, 1:-2, 2:-3]
        v.copy_(t)
        assert not v.is_contiguous()
        views.append(v)
    got = sgr.light_encoder_input(*views, size=dst)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# =========================================================================================================================================
# light_albedo_scale
# =========================================================================================================================================
SCALE_NAMES = ("cLight", "cAlbedo", "cDiff", "cSpec")


def run_scale(sgr, args):
    dev = [torch.as_tensor(a).cuda() for a in args]
    out4 = torch.ops.sgrender.light_albedo_scale(*dev)
    cLight, cAlbedo = sgr.light_albedo_scale(*dev)
    assert tuple(out4.shape) == (4,) and cLight.dim() == 0 and cLight.is_cuda
    assert torch.equal(out4[0], cLight) and torch.equal(out4[1], cAlbedo)                      # and two runs are bit-identical
    return out4.cpu().tolist()


@pytest.mark.parametrize("tag", ["nospec", "clip_lo", "clip_hi", "noclip", "clip_hi_dark", "big"])
def test_albedo_scale_vs_reference_fixture(sgr, tag):
    z = load("scale")
    args = [z[f"{tag}_{k}"] for k in ("diffuseNew", "diffuse", "specNew", "spec", "albedo")]
    ok, rep = LG.albedo_scale_margins_ok(*args)
    assert ok, rep
    got = run_scale(sgr, args)
    for name, g, r64, r32 in zip(SCALE_NAMES, got, z[tag + "_ref64"], z[tag + "_ref32"]):
        check_scalar("albedo_scale " + name, "fixture " + tag, g, r64, r32)


@pytest.mark.parametrize("n,where,branch", LG.SCALE_CASES)
def test_albedo_scale_vs_checker(sgr, n, where, branch):
    args = LG.scale_case(n, where, branch, 7000 + n)
    ok, rep = LG.albedo_scale_margins_ok(*args)
    assert ok, rep
    (ref64, br64), (ref32, br32) = LG.albedo_scale(*args, dtype=F64), LG.albedo_scale(*args, dtype=F32)
    assert br64 == br32
    got = run_scale(sgr, args)
    for name, g, r64, r32 in zip(SCALE_NAMES, got, ref64, ref32):
        check_scalar("albedo_scale " + name, f"n={n} max {where} {br64}", g, r64, r32)


# =========================================================================================================================================
# predToShading
# =========================================================================================================================================
def shading_pred(bn, K, R, C, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(bn, K, 3, R, C, generator=g)
    a = a / a.norm(dim=2, keepdim=True)
    return torch.cat([a.reshape(bn, 3 * K, R, C), torch.rand(bn, K, R, C, generator=g), torch.rand(bn, 3 * K, R, C, generator=g)], 1)


def check_shading(tag, got, ref64, ref32):
    got = torch.as_tensor(got).cpu()
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0
    for b in range(got.shape[0]):
        e, lim = err(got[b], ref64[b]), max(2.0 * err(ref32[b], ref64[b]), 1e-5)
        note("shading", e, lim, f"{tag} image {b}")
        assert e <= lim, (tag, b, e, lim)


@pytest.mark.parametrize("tag", ["k13", "k24w", "k24", "k24one", "k1", "k1one"])
def test_shading_vs_reference_fixture(sgr, tag):
    z = load("shading")
    K, R, C, eh, ew = [int(v) for v in z[tag + "_cfg"]]
    got = sgr.predToShading(z[tag + "_pred"], envWidth=ew, envHeight=eh, SGNum=K)
    assert got.shape == (3, R, C)
    check_shading("fixture " + tag, got[None], torch.from_numpy(z[tag + "_ref64"])[None], torch.from_numpy(z[tag + "_ref32"])[None])


SHADING_GRIDS = [((1, 1), 4), ((7, 9), 8), ((8, 8), 16), ((5, 13), 8), ((9, 14), 16), ((5, 13), 4)]      # R*C = 1, 63, 64, 65, 126; envHeight


@pytest.mark.parametrize("ew", [16, 32])
@pytest.mark.parametrize("K", [1, 12, 13, 24])
def test_shading_three_distinct_images_vs_checker(sgr, K, ew):
    """both lobe-count instantiations either side of their boundary (12 | 13) and at their ends, both direction-grid widths; cell counts
    around one 64-lane workgroup; premap 1 through the Python layer, premap 0 (lamb / weight already mapped) through the operator"""
    for j, ((R, C), eh) in enumerate(SHADING_GRIDS):
        pred = shading_pred(3, K, R, C, 900 + 10 * K + j)
        for premap in ((1, 0) if (R, C) == (5, 13) else (j % 2,)):
            p = pred.clone()
            if premap == 0:
                p[:, 3 * K:] = torch.tan(np.pi / 2.0 * (p[:, 3 * K:] * 0.999))
            ref64, ref32 = LG.shading(p, eh, ew, K, premap, F64), LG.shading(p, eh, ew, K, premap, F32)
            d = p.cuda()
            if premap:
                got = sgr.predToShading(d, envWidth=ew, envHeight=eh, SGNum=K)
            else:
                got = torch.ops.sgrender.sg_shading(d[:, :3 * K].reshape(3, K, 3, R, C), d[:, 3 * K:4 * K], d[:, 4 * K:], eh, ew, 0)
            assert tuple(got.shape) == (3, 3, R, C)
            check_shading(f"K={K} {eh}x{ew} grid {R}x{C} premap={premap}", got, ref64, ref32)
            alone = sgr.predToShading(d[1:2], envWidth=ew, envHeight=eh, SGNum=K) if premap else None
            assert alone is None or torch.equal(alone[0], got[1])


def test_shading_refuses_what_it_has_no_kernel_for(sgr):
    with pytest.raises(RuntimeError):
        sgr.predToShading(shading_pred(1, 25, 2, 3, 1).cuda(), envWidth=16, envHeight=8, SGNum=25)
    with pytest.raises(RuntimeError):
        sgr.predToShading(shading_pred(1, 12, 2, 3, 2).cuda(), envWidth=8, envHeight=4, SGNum=12)
    torch.cuda.synchronize()


# =========================================================================================================================================
# lsregress_coef / lsregress_diffspec_coef
# =========================================================================================================================================
LO32, HI32 = float(np.float32(0.001)), 1000.0


def check_diffspec(sgr, tag, d, s, i):
    ok, rep = LG.diffspec_margins_ok(d, s, i)
    assert ok, rep
    (c64, i64), (c32, i32) = LG.diffspec_coef(d, s, i, F64), LG.diffspec_coef(d, s, i, F32)
    assert torch.equal(i64["two"], i32["two"]) and LG.diffspec_raw_clear(i64) and LG.diffspec_raw_clear(i32)
    dev = [t.cuda() for t in (d, s, i)]
    got = torch.ops.sgrender.lsregress_diffspec_coef(*dev)
    assert tuple(got.shape) == (d.shape[0], 2)
    assert torch.equal(got, torch.ops.sgrender.lsregress_diffspec_coef(*dev))                   # determinism
    g = got.cpu()
    for b in range(d.shape[0]):
        alone = torch.ops.sgrender.lsregress_diffspec_coef(*[t[b:b + 1] for t in dev])
        assert torch.equal(alone[0], got[b]), (tag, b)                                          # batch independence
        clamp = {0.001: LO32, 1000.0: HI32}
        cd, cs, cim = float(i64["cd"][b]), float(i64["cs"][b]), float(i64["cim"][b])
        if cs == 0.0:
            assert float(g[b, 1]) == 0.0, (tag, b, g[b])
        else:
            check_scalar("diffspec_coef", f"{tag} image {b} spec", g[b, 1], c64[b, 1], c32[b, 1])
        if cd in clamp and cim in clamp:
            assert float(g[b, 0]) == float(np.float32(clamp[cim]) * np.float32(clamp[cd])), (tag, b, g[b])
        else:
            check_scalar("diffspec_coef", f"{tag} image {b} diffuse", g[b, 0], c64[b, 0], c32[b, 0])
    return got


@pytest.mark.parametrize("kinds,R,C,seed", LG.DIFFSPEC_BATCHES, ids=[f"{R}x{C}-" + "-".join(k) for k, R, C, _ in LG.DIFFSPEC_BATCHES])
def test_diffspec_coef_vs_checker(sgr, kinds, R, C, seed):
    d, s, i = LG.diffspec_batch(kinds, R, C, seed)
    check_diffspec(sgr, f"{R}x{C}", d, s, i)


def test_diffspec_through_the_python_layer_on_the_reference_fixtures(sgr):
    z = load("regress")
    for tag in z["ds_tags"].tolist():
        d, s, i = [torch.from_numpy(z[f"{tag}_{k}"]) for k in ("diff", "spec", "im")]
        coef = check_diffspec(sgr, tag, d, s, i)
        dS, sS = sgr.LSregressDiffSpec(d.cuda(), s.cuda(), i.cuda(), d.cuda(), s.cuda())
        assert torch.equal(dS, coef[:, 0].reshape(-1, 1, 1, 1) * d.cuda()) and torch.equal(sS, coef[:, 1].reshape(-1, 1, 1, 1) * s.cuda())
        for name, x in (("diffScaled", dS), ("specScaled", sS)):
            r64, r32 = z[f"{tag}_{name}64"], z[f"{tag}_{name}32"]
            if np.abs(r64).max() == 0.0:
                assert float(x.abs().max()) == 0.0, (tag, name)
                continue
            e, lim = err(x, r64), max(2.0 * err(r32, r64), 1e-5)
            note("LSregressDiffSpec images", e, lim, tag + " " + name)
            assert e <= lim, (tag, name, e, lim)


@pytest.mark.parametrize("kinds,n,seed", LG.LSREGRESS_BATCHES, ids=[f"n{n}-" + "-".join(k) for k, n, _ in LG.LSREGRESS_BATCHES])
def test_lsregress_coef_vs_checker(sgr, kinds, n, seed):
    p, g = LG.lsregress_batch(kinds, n, seed)
    ok, rep = LG.lsregress_margins_ok(p, g)
    assert ok, rep
    (c64, i64), (c32, _) = LG.lsregress_coef(p, g, F64), LG.lsregress_coef(p, g, F32)
    dp, dg = p.cuda(), g.cuda()
    got = torch.ops.sgrender.lsregress_coef(dp, dg)
    assert tuple(got.shape) == (3,) and torch.equal(got, torch.ops.sgrender.lsregress_coef(dp, dg))
    for b, k in enumerate(kinds):
        assert torch.equal(torch.ops.sgrender.lsregress_coef(dp[b:b + 1], dg[b:b + 1])[0], got[b])
        if float(c64[b]) in (0.001, 1000.0):
            assert k in ("clamp_lo", "clamp_hi") and float(got[b]) == (LO32 if k == "clamp_lo" else HI32), (k, float(got[b]))
        else:
            check_scalar("lsregress_coef", f"n={n} image {b} {k}", got[b], c64[b], c32[b])


def test_lsregress_through_the_python_layer_on_the_reference_fixtures(sgr):
    z = load("regress")
    for tag in z["ls_tags"].tolist():
        p, g = torch.from_numpy(z[tag + "_pred"]).cuda(), torch.from_numpy(z[tag + "_gt"]).cuda()
        assert LG.lsregress_margins_ok(p, g)[0]
        coef = sgr.LSregress(p, g, torch.ones_like(p))[0, 0, 0, 0]
        r64, r32 = z[tag + "_coef64"][0], z[tag + "_coef32"][0]
        if r64 in (0.001, 1000.0):
            assert float(coef) == float(np.float32(r64)), (tag, float(coef))
        else:
            check_scalar("lsregress_coef", "fixture " + tag, coef, r64, r32)
        scaled = sgr.LSregress(p, g, p)
        e, lim = err(scaled, z[tag + "_scaled64"]), max(2.0 * err(z[tag + "_scaled32"], z[tag + "_scaled64"]), 1e-5)
        note("LSregress images", e, lim, tag)
        assert e <= lim, (tag, e, lim)
