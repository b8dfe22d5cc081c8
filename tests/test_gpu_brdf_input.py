"""GPU: sgr.brdf_encoder_input (csrc/sgr_brdf_input.hip behind torch.ops.sgrender.brdf_encoder_input) against the fixtures the UNMODIFIED
reference produced (tests/golden/g15_brdfin_*.npz, tools/make_golden_brdf_input.py) and against tests/brdf_input_checker.py, which
tests/test_brdf_input.py pins to those fixtures at 1e-12.

Bounds.  Per channel group of the 17-channel tensor, rel-L2 against the fp64 reference: ``max(2 e_ref, 1e-6)`` -- the rule of the g13 /
g14 tests: ``e_ref`` is the reference's own fp32-vs-fp64 distance (stored in the fixture; for the flag combinations no fixture covers,
the checker evaluated in fp32 on the same inputs), and 1e-6 is the floor for groups the reference reproduces almost exactly.  The
coefficients: ``|got - ref| <= max(2 e_ref_coef, 1e-6 |ref|)`` each.  A plane that is zero in the reference is zero exactly.  The
per-channel sums of the full-size case: the same scalar rule.  Everything else here (two runs, one image against its batch, strided
inputs, a graph replay) is bit for bit."""
import os

import numpy as np
import pytest
import torch

import brdf_input_checker as C
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

CASES = ["small", "same", "fallback", "meanfloor", "tiny", "full"]


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


_cache = {}


def case(name):
    """(fixture, the seven inputs as device tensors); loaded once, never written to"""
    if name not in _cache:
        z = np.load(os.path.join(GOLDEN_DIR, f"g15_brdfin_{name}.npz"))
        inp = C.load_inputs(z)
        _cache[name] = (z, [torch.from_numpy(inp[k]).cuda() for k in C.INPUTS])
    return _cache[name]


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


def bound(e_ref):
    return max(2.0 * float(e_ref), 1e-6)


def check_coef(tag, got, ref, e_ref):
    got, ref, e_ref = np.asarray(got.cpu(), np.float64), np.asarray(ref, np.float64), np.asarray(e_ref, np.float64)
    lim = np.maximum(2.0 * e_ref, 1e-6 * np.abs(ref))
    print(f"{tag} coef: got {got.ravel()} ref {ref.ravel()} |diff| {np.abs(got - ref).ravel()} bound {lim.ravel()}")
    assert np.isfinite(got).all() and (np.abs(got - ref) <= lim).all(), (tag, got, ref, lim)


@pytest.mark.parametrize("name", CASES)
def test_input_matches_the_reference_fixture(sgr, name):
    z, args = case(name)
    out, coef = sgr.brdf_encoder_input(*args)
    bn, _, H, W = args[0].shape
    assert tuple(out.shape) == (bn, 17, H, W) and tuple(coef.shape) == (bn, 2) and out.is_contiguous() and not out.requires_grad
    assert torch.isfinite(out).all()
    st = int(z["stride"])
    for g, (a, b) in C.GROUPS.items():
        got, lim = out[:, a:b], bound(z["e_ref_" + g])
        if st > 1:      # the full-size case: every st-th pixel, and all of them through the per-channel sums
            s_got, s64, s32 = got.double().sum((2, 3)).cpu().numpy(), z["sum64_" + g], z["sum32_" + g]
            s_lim = np.maximum(2.0 * np.abs(s32 - s64), 1e-6 * np.abs(s64))
            print(f"{name} {g} sums: |diff| {np.abs(s_got - s64).ravel()} bound {s_lim.ravel()}")
            assert (np.abs(s_got - s64) <= s_lim).all(), (name, g, s_got, s64, s_lim)
            got = got[:, :, ::st, ::st]
        ref = z["ref64_" + g]
        e = err(got, ref)
        print(f"{name} {g}: {e:.2e} (bound {lim:.1e}, e_ref {float(z['e_ref_' + g]):.2e})")
        assert e <= lim, (name, g, e, lim)
        zero = np.abs(ref).reshape(ref.shape[0], ref.shape[1], -1).max(-1) == 0      # [bn, channels of the group]
        if zero.any():
            assert float(got[torch.from_numpy(zero).cuda()].abs().max()) == 0.0, (name, g)
    check_coef(name, coef, z["ref64_coef"], z["e_ref_coef"])


FLAGS = [dict(remap=True), dict(regress=False, normalize=False), dict(regress=False, normalize=False, remap=True), dict(regress=False), dict(normalize=False)]


@pytest.mark.parametrize("name", ["small", "same"])
@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "-".join(f"{k}={int(v)}" for k, v in f.items()))
def test_flag_combinations_match_the_checker(sgr, name, flags):
    _, args = case(name)
    out, coef = sgr.brdf_encoder_input(*args, **flags)
    r64, c64 = C.brdf_encoder_input(*[a.double() for a in args], **flags)
    r32, c32 = C.brdf_encoder_input(*args, **flags)
    for g, (a, b) in C.GROUPS.items():
        e_ref = err(r32[:, a:b], r64[:, a:b])
        e, lim = err(out[:, a:b], r64[:, a:b]), bound(e_ref)
        print(f"{name} {flags} {g}: {e:.2e} (bound {lim:.1e}, checker's own fp32 distance {e_ref:.2e})")
        assert e <= lim, (name, flags, g, e, lim)
    check_coef(f"{name} {flags}", coef, c64.cpu().numpy(), (c32.double() - c64).abs().cpu().numpy())
    if not flags.get("regress", True):
        assert bool((coef == 1).all())


@pytest.mark.parametrize("name", ["small", "same", "tiny"])
def test_two_calls_are_bit_identical(sgr, name):
    _, args = case(name)
    a, ca = sgr.brdf_encoder_input(*args)
    b, cb = sgr.brdf_encoder_input(*args)
    assert torch.equal(a, b) and torch.equal(ca, cb)


@pytest.mark.parametrize("name", ["small", "fallback"])
def test_an_image_does_not_depend_on_its_batch(sgr, name):
    _, args = case(name)
    out, coef = sgr.brdf_encoder_input(*args)
    for i in range(args[0].shape[0]):
        one, c1 = sgr.brdf_encoder_input(*[a[i:i + 1].clone() for a in args])
        assert torch.equal(one[0], out[i]) and torch.equal(c1[0], coef[i]), (name, i)


def test_non_contiguous_inputs_give_the_contiguous_result(sgr):
    _, args = case("same")
    want, cw = sgr.brdf_encoder_input(*args)
    im = torch.zeros(args[0].shape[:3] + (args[0].shape[3] + 5,), device="cuda")[..., 2:-3]      # a window of a wider tensor
    im.copy_(args[0])
    albedo = args[1].contiguous(memory_format=torch.channels_last)
    spec = args[6].transpose(2, 3).contiguous().transpose(2, 3)
    assert not im.is_contiguous() and not albedo.is_contiguous() and not spec.is_contiguous()
    got, cg = sgr.brdf_encoder_input(im, albedo, *args[2:6], spec)
    assert got.is_contiguous() and torch.equal(got, want) and torch.equal(cg, cw)


def test_graph_capture_and_replay(sgr):
    _, args = case("small")
    static = [a.clone() for a in args]
    eager, ce = sgr.brdf_encoder_input(*static)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):      # torch's capture recipe: first uses (allocator growth) on a side stream
        sgr.brdf_encoder_input(*static)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, coef = sgr.brdf_encoder_input(*static)
    out.zero_()
    coef.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(coef, ce)
    # the replay reads its inputs where they lie: new data, same graph
    _, other = case("small")
    static[0].copy_(other[0].flip(0))
    want, cw = sgr.brdf_encoder_input(*static)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(coef, cw)
