"""CPU: the cascade-1 BRDF encoder input without a GPU.

  * tests/brdf_input_checker.py (the contract of DESIGN.md section 8c in torch, own code) is pinned at 1e-12, in fp64, to the fixtures
    the UNMODIFIED reference produced (tests/golden/g15_brdfin_*.npz, tools/make_golden_brdf_input.py), and for the flag combination of
    testReal.py:439-449 to the three ``F.interpolate`` / ``0.5 (x + 1)`` steps composed here; at the seven geometries no fixture holds
    (tests/brdf_input_cases.py) to ``F.interpolate``, ``F.adaptive_avg_pool2d`` and the regression written out here, again at 1e-12;
  * every input set the GPU edge tests draw (same module, same seeds) decides neither discontinuity by rounding;
  * the C ABI refuses NULL tensors, non-positive sizes and an illegal source size before anything is dereferenced, and its workspace
    query is a pure host function;
  * ``torch.ops.sgrender.brdf_encoder_input`` is registered by the C++ extension with a Meta kernel of the documented shapes;
  * the Python wrapper raises on a CPU tensor, on unequal BRDF-map sizes and on an oversize map."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import brdf_input_cases as K
import brdf_input_checker as C
from conftest import GOLDEN_DIR

import inverserenderingofindoorscene_amd as sgr
from inverserenderingofindoorscene_amd import _lib

CASES = ["small", "same", "fallback", "meanfloor", "tiny", "full"]
PIN = 1e-12


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g15_brdfin_{name}.npz"))


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


@pytest.mark.parametrize("name", CASES)
def test_checker_is_pinned_to_the_reference_fixture(name):
    z = load(name)
    inp = C.load_inputs(z)
    out, coef = C.brdf_encoder_input(*[torch.from_numpy(inp[k]).double() for k in C.INPUTS])
    st = int(z["stride"])
    for g, (a, b) in C.GROUPS.items():
        got = out[:, a:b]
        if st > 1:
            e = err(got.sum((2, 3)), z["sum64_" + g])
            assert e <= PIN, (name, g, "sums", e)
            got = got[:, :, ::st, ::st]
        e = err(got, z["ref64_" + g])
        assert e <= PIN, (name, g, e)
    assert err(coef, z["ref64_coef"]) <= PIN, (name, coef, z["ref64_coef"])


def test_fixtures_reach_the_paths_they_are_named_for():
    z = load("fallback")
    assert z["det_over_n"][0] == 0.0 and z["ref64_coef"][0, 1] == 0.0                # specular all zero: the diffuse-only branch
    assert z["det_over_n"][1] < 1e-2 and z["ref64_coef"][1, 0] > 1e3                 # c_d at its 1e3 clamp, times c_im
    assert 0.5 < z["bright_share"][2] < 1.0 and z["det_over_n"][2] > 1e-2            # most pooled cells at or above 0.9
    z = load("meanfloor")
    assert np.abs(z["ref64_albedo"][0]).max() == 0.0 and z["depthPre"][0].mean() < 1e-10
    z = load("tiny")
    assert z["diffusePre"][0].size < 64 * 1                                          # fewer cells per channel than workgroups per image
    z = load("small")
    assert z["im"].shape[2] * z["im"].shape[3] % 4 != 0 and z["im"].shape[3] % z["diffusePre"].shape[3] != 0
    for name in CASES:      # no fixture decides a discontinuity by rounding
        assert (np.abs(load(name)["det_over_n"] - 1e-2) >= 1e-5).all(), name


def test_checker_matches_the_inference_form_composed_from_torch():
    """testReal.py:439-449: six bilinear resizes, then 0.5 (x + 1) on normal and rough -- the remap AFTER the resize, where the contract
    (one order for every call site) has it before; bilinear weights sum to one, so the two differ in rounding only"""
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    im, al, nr, ro, dp, df, sp = r(2, 3, 30, 41), r(2, 3, 15, 21), 2 * r(2, 3, 15, 21) - 1, 2 * r(2, 1, 15, 21) - 1, r(2, 1, 15, 21), r(2, 3, 10, 13), r(2, 3, 10, 13)
    up = lambda t: F.interpolate(t, [30, 41], mode="bilinear")
    want = torch.cat([im, up(al), 0.5 * (up(nr) + 1), 0.5 * (up(ro) + 1), up(dp), up(df), up(sp)], 1)
    out, coef = C.brdf_encoder_input(im, al, nr, ro, dp, df, sp, regress=False, normalize=False, remap=True)
    assert err(out, want) <= PIN and bool((coef == 1).all())
    # and the pooling rule against torch's, at a non-integer ratio in both directions
    assert err(C.pooled(im, 7, 9), F.adaptive_avg_pool2d(im, (7, 9))) <= PIN


def _torch_composition(im, al, nr, ro, dp, df, sp):
    """the default call (regress, normalize, no remap) composed from torch's own resize and pooling, the regression of DESIGN.md section
    8c written out image by image with plain branches"""
    bn, _, H, W = im.shape
    up = lambda t: t if tuple(t.shape[2:]) == (H, W) else F.interpolate(t, [H, W], mode="bilinear", align_corners=False)
    small = F.adaptive_avg_pool2d(im, (df.shape[2], df.shape[3]))
    n = df[0].numel()
    dfs, sps, coef = [], [], []
    for b in range(bn):
        keep = (small[b] < 0.9).to(im.dtype)
        d, s, i = df[b] * keep, sp[b] * keep, small[b] * keep
        a11, a22, a12, b1, b2 = float((d * d).sum()), float((s * s).sum()), float((d * s).sum()), float((d * i).sum()), float((s * i).sum())
        det = a11 * a22 - a12 * a12
        if det / n > 1e-2:
            cd, cs = (b1 * a22 - b2 * a12) / max(det, 1e-2), (a11 * b2 - b1 * a12) / max(det, 1e-2)
        else:
            cd, cs = min(max(b1 / max(a11, 1e-5), 1e-3), 1e3), 0.0
        cd, cs = min(max(cd, 0.0), 1e3), min(max(cs, 0.0), 1e3)
        render = torch.clamp(cd * df[b] + cs * sp[b], 0, 1)
        cim = min(max(float((render * small[b]).sum()) / max(float((render * render).sum()), 1e-5), 1e-3), 1e3)
        dfs.append(cim * (cd * df[b]))
        sps.append(cim * (cs * sp[b]))
        coef.append([cim * cd, cim * cs])
    unit = lambda t: t / torch.clamp(t.flatten(1).mean(1), min=1e-10).reshape(-1, 1, 1, 1) / 3.0
    out = torch.cat([im, unit(up(al)), up(nr), up(ro), unit(up(dp)), up(torch.stack(dfs)), up(torch.stack(sps))], 1)
    return out, torch.tensor(coef, dtype=im.dtype)


@pytest.mark.parametrize("name", list(K.GEOMETRIES))
def test_checker_matches_torch_on_the_geometries_no_fixture_holds(name):
    """maps equal along one axis only, a down-sample along one axis, an env grid at image size and one taller than the image, 1 x 1 maps:
    the checker's own interpolation / pooling matrices against ``F.interpolate`` and ``F.adaptive_avg_pool2d``, in fp64 at PIN"""
    inp = K.build(*K.GPU_CASES["geometry " + name])
    args = K.tensors(inp, dtype=torch.float64)
    H, W, h, w, R, Cc = K.GEOMETRIES[name]
    assert tuple(args[0].shape[2:]) == (H, W) and tuple(args[1].shape[2:]) == (h, w) and tuple(args[5].shape[2:]) == (R, Cc)
    out, coef = C.brdf_encoder_input(*args)
    want, cw = _torch_composition(*args)
    for g, (a, b) in C.GROUPS.items():
        e = err(out[:, a:b], want[:, a:b])
        assert e <= PIN, (name, g, e)
    assert err(coef, cw) <= PIN, (name, coef, cw)
    # and the inference form: remap, no regression, no normalisation (the remap before the resize: rounding only)
    up = lambda t: t if tuple(t.shape[2:]) == (H, W) else F.interpolate(t, [H, W], mode="bilinear", align_corners=False)
    im, al, nr, ro, dp, df, sp = args
    want = torch.cat([im, up(al), 0.5 * (up(nr) + 1), 0.5 * (up(ro) + 1), up(dp), up(df), up(sp)], 1)
    out, coef = C.brdf_encoder_input(*args, regress=False, normalize=False, remap=True)
    assert err(out, want) <= PIN and bool((coef == 1).all())


@pytest.mark.parametrize("tag", list(K.GPU_CASES))
def test_inputs_of_the_gpu_edge_tests_decide_nothing_by_rounding(tag):
    """every input set of tests/test_gpu_brdf_input_edges.py, built here from the same seeds: each pooled cell at least 1e-4 from the 0.9
    mask, ``det / n`` at least 1e-5 from 1e-2 and on one side of it in fp32 and in fp64 -- what tools/make_golden_brdf_input.py asserts
    of a fixture"""
    inp = K.build(*K.GPU_CASES[tag])
    gap, det = K.assert_settled(tag, inp)
    assert all(v.dtype == np.float32 for v in inp.values())
    assert (inp["diffusePre"][:, 0, 0, 0] == 1.0).all() and (inp["specularPre"][:, 0, 0, 0] == 0.25).all()
    assert np.allclose(np.linalg.norm(inp["normalPre"], axis=1), 1.0, atol=1e-6)
    assert inp["depthPre"].min() >= 0.5 and inp["depthPre"].max() <= 4.5
    if tag == "tiny":
        assert inp["diffusePre"][0].size < 64 and det[0] > 1e-2      # workgroups with no element; the two-coefficient branch


def test_c_abi_refusals_and_workspace_without_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused before a launch
    ok_sizes = (2, 24, 32, 12, 16, 12, 16)

    def call(ptrs=None, sizes=ok_sizes):
        p = [fake] * 10 if ptrs is None else ptrs
        return lib.sgr_brdf_input_fwd(*p, *sizes, 1, 1, 0, None)
    for k in range(10):      # each tensor in turn
        p = [fake] * 10
        p[k] = None
        assert call(p) == -1 and b"NULL" in lib.sgr_last_error(), k
    for k in range(7):       # each size in turn, zero and negative
        for bad in (0, -3):
            s = list(ok_sizes)
            s[k] = bad
            assert call(sizes=s) == -1 and b"non-positive" in lib.sgr_last_error(), (k, bad)
    # a source larger than the output along both axes, or as high and wider: the reference would fail in its cat
    for s in ((2, 24, 32, 25, 33, 12, 16), (2, 24, 32, 24, 33, 12, 16), (2, 24, 32, 12, 16, 30, 32), (2, 24, 32, 12, 16, 24, 40)):
        assert call(sizes=s) == -1 and b"illegal source size" in lib.sgr_last_error(), s
    n1, n2, n16 = (lib.sgr_brdf_input_workspace_floats(b) for b in (1, 2, 16))
    assert 0 < n1 < n2 < n16 and n16 == 16 * n1
    assert lib.sgr_brdf_input_workspace_floats(0) == 0


def m(*shape):
    return torch.empty(*shape, device="meta")


def test_operator_is_registered_with_meta_shapes():
    op = torch.ops.sgrender.brdf_encoder_input
    schema = str(op.default._schema)
    assert schema.startswith("sgrender::brdf_encoder_input(") and "bool regress=True" in schema and "bool remap=False" in schema
    for key in ("Meta", "CUDA"):      # registered from C++ (TORCH_LIBRARY), not by a Python torch.library.custom_op
        assert torch._C._dispatch_has_kernel_for_dispatch_key("sgrender::brdf_encoder_input", key), key
    bn, H, W = 3, 30, 41
    for h, w, R, Cc in ((15, 21, 15, 21), (30, 41, 10, 13), (30, 41, 30, 41), (40, 30, 15, 21)):      # the last: larger along one axis only
        out, coef = op(m(bn, 3, H, W), m(bn, 3, h, w), m(bn, 3, h, w), m(bn, 1, h, w), m(bn, 1, h, w), m(bn, 3, R, Cc), m(bn, 3, R, Cc))
        assert tuple(out.shape) == (bn, 17, H, W) and tuple(coef.shape) == (bn, 2) and out.dtype == torch.float32
    out, _ = op(m(bn, 3, H, W), m(bn, 3, 15, 21), m(bn, 3, 15, 21), m(bn, 1, 15, 21), m(bn, 1, 15, 21), m(bn, 3, 15, 21), m(bn, 3, 15, 21), False, False, True)
    assert tuple(out.shape) == (bn, 17, H, W) and not out.requires_grad
    # the Meta kernel refuses what the device kernel refuses
    with pytest.raises(RuntimeError, match="smaller along an axis"):
        op(m(bn, 3, H, W), m(bn, 3, 31, 42), m(bn, 3, 31, 42), m(bn, 1, 31, 42), m(bn, 1, 31, 42), m(bn, 3, 15, 21), m(bn, 3, 15, 21))
    with pytest.raises(RuntimeError, match="share one size"):
        op(m(bn, 3, H, W), m(bn, 3, 15, 21), m(bn, 3, 15, 21), m(bn, 1, 15, 20), m(bn, 1, 15, 21), m(bn, 3, 15, 21), m(bn, 3, 15, 21))
    with pytest.raises(RuntimeError, match="fp32"):
        op(m(bn, 3, H, W).double(), m(bn, 3, 15, 21), m(bn, 3, 15, 21), m(bn, 1, 15, 21), m(bn, 1, 15, 21), m(bn, 3, 15, 21), m(bn, 3, 15, 21))


def test_wrapper_raises_on_cpu_tensors_and_illegal_sizes():
    z = torch.zeros
    args = lambda h=12, w=16: (z(2, 3, 24, 32), z(2, 3, h, w), z(2, 3, h, w), z(2, 1, h, w), z(2, 1, h, w), z(2, 3, 12, 16), z(2, 3, 12, 16))
    assert "brdf_encoder_input" in sgr.__all__
    with pytest.raises(RuntimeError, match="no CPU path"):
        sgr.brdf_encoder_input(*args())
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.sgrender.brdf_encoder_input(*args())
    a = list(args())
    a[3] = z(2, 1, 12, 15)                                  # roughPre of another size
    with pytest.raises(RuntimeError, match="share one size"):
        sgr.brdf_encoder_input(*a)
    dev = lambda ts: [t.to("meta") for t in ts]             # sizes are checked before any launch, for fake tensors as for device tensors
    with pytest.raises(RuntimeError, match="smaller along an axis"):
        sgr.brdf_encoder_input(*dev(args(25, 33)))          # an oversize map
    with pytest.raises(RuntimeError, match="image's"):
        sgr.brdf_encoder_input(*dev(args()), size=(48, 64))
    out, coef = sgr.brdf_encoder_input(*dev(args()), size=(24, 32))
    assert tuple(out.shape) == (2, 17, 24, 32) and tuple(coef.shape) == (2, 2)
