"""GPU: sgr.brdf_encoder_input (csrc/sgr_brdf_input.hip) where the fixtures of tests/test_gpu_brdf_input.py never go: resize geometries
other than "half size along both axes", pass C's grid-stride loop and both branches of its cap, the alignment half of the V = 4 / V = 1
dispatch, and reads and writes at the edges of the tensors.

Inputs come from tests/brdf_input_cases.py (seeded; tests/test_brdf_input.py asserts on the CPU that none of them decides the 0.9 mask or
the ``det / n`` branch by rounding, and pins the checker to torch's own resize and pooling at the seven geometries).

Bounds: those of tests/test_gpu_brdf_input.py, imported.  Per channel group, rel-L2 against the checker in fp64 ``<= max(2 e_ref, 1e-6)``
with ``e_ref`` the checker in fp32 on the same inputs; coefficients ``|got - ref| <= max(2 e_ref_coef, 1e-6 |ref|)``; a plane that is zero
in the reference is zero exactly.  The checker runs on the device, a few images at a time.  Everything else is bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import brdf_input_cases as K
import brdf_input_checker as C
from test_gpu_brdf_input import bound, check_coef

pytestmark = pytest.mark.gpu

DEFAULT = dict(regress=True, normalize=True, remap=False)
INFERENCE = dict(regress=False, normalize=False, remap=True)      # testReal.py:439-449


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


_cache = {}


def case(tag):
    """the seven inputs of a case of brdf_input_cases.GPU_CASES as device tensors; made once, never written to"""
    if tag not in _cache:
        _cache[tag] = K.tensors(K.build(*K.GPU_CASES[tag]), device="cuda")
        assert all(t.data_ptr() % 16 == 0 and t.is_contiguous() for t in _cache[tag])
    return _cache[tag]


def against_the_checker(tag, out, coef, args, flags, chunk=4):
    """the bounds of the module docstring; the checker is evaluated `chunk` images at a time and the squared norms are added up, which
    gives the rel-L2 over the batch; the worst single image is printed beside it"""
    bn, _, H, W = args[0].shape
    assert tuple(out.shape) == (bn, 17, H, W) and tuple(coef.shape) == (bn, 2) and out.is_contiguous()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(coef).all())
    sq = {g: torch.zeros(3, bn, dtype=torch.float64, device=out.device) for g in C.GROUPS}      # |got - r64|^2, |r32 - r64|^2, |r64|^2 per image
    c64, c32 = [], []
    for b0 in range(0, bn, chunk):
        sl = slice(b0, min(b0 + chunk, bn))
        r64, k64 = C.brdf_encoder_input(*[a[sl].double() for a in args], **flags)
        r32, k32 = C.brdf_encoder_input(*[a[sl] for a in args], **flags)
        c64.append(k64)
        c32.append(k32.double())
        for g, (a, b) in C.GROUPS.items():
            got, ref = out[sl, a:b].double(), r64[:, a:b]
            sq[g][0, sl] = ((got - ref) ** 2).sum((1, 2, 3))
            sq[g][1, sl] = ((r32[:, a:b].double() - ref) ** 2).sum((1, 2, 3))
            sq[g][2, sl] = (ref ** 2).sum((1, 2, 3))
            zero = ref.abs().amax((2, 3)) == 0      # [images, channels of the group]
            if bool(zero.any()):
                assert float(out[sl, a:b][zero].abs().max()) == 0.0, (tag, g, "a plane that is zero in the reference")
    for g, (a, b) in C.GROUPS.items():
        d2, e2, r2 = (float(v) for v in sq[g].sum(1))
        if r2 > 0:
            e, e_ref = (d2 / r2) ** 0.5, (e2 / r2) ** 0.5
            live = sq[g][2] > 0
            worst = float((sq[g][0][live] / sq[g][2][live]).max()) ** 0.5
        else:      # the group is zero in every image: exactly zero was asserted above
            e, e_ref, worst = float(out[:, a:b].abs().max()), e2 ** 0.5, 0.0
        lim = bound(e_ref)
        print(f"{tag} {g}: {e:.2e} (bound {lim:.1e}, e_ref {e_ref:.2e}; worst single image {worst:.2e})")
        assert e <= lim, (tag, g, e, lim)
    c64, c32 = torch.cat(c64).cpu().numpy(), torch.cat(c32).cpu().numpy()
    if bn > 4:      # thirty-two rows of figures say no more than their worst
        got, lim = coef.double().cpu().numpy(), np.maximum(2.0 * np.abs(c32 - c64), 1e-6 * np.abs(c64))
        k = np.unravel_index(np.argmax(np.abs(got - c64) - lim), lim.shape)
        print(f"{tag} coef nearest its bound: image {k[0]} coefficient {k[1]}: got {got[k]:.9g} ref {c64[k]:.9g} |diff| {abs(got[k] - c64[k]):.2e} bound {lim[k]:.2e}")
        assert np.isfinite(got).all() and (np.abs(got - c64) <= lim).all(), (tag, got, c64, lim)
    else:
        check_coef(tag, coef, c64, np.abs(c32 - c64))
    if not flags["regress"]:
        assert bool((coef == 1).all())


def shifted(t):
    """the same values one float off every 16-byte boundary: contiguous, so the operator takes it as it is"""
    buf = torch.empty(t.numel() + 1, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def banded(t, band, fill, shift=0):
    """-> (buffer, the view of `t`'s shape in its middle): `band + shift` floats of `fill` before the values and `band` after"""
    n = t.numel()
    buf = torch.full((n + 2 * band + shift,), fill, device=t.device)
    v = buf[band + shift:band + shift + n].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous()
    return buf, v


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def raw_call(args, out, coef, ws, flags):
    from inverserenderingofindoorscene_amd import _lib
    bn, _, H, W = args[0].shape
    (h, w), (R, Cc) = args[1].shape[2:], args[5].shape[2:]
    _lib.call("sgr_brdf_input_fwd", *[_ptr(a) for a in args], _ptr(out), _ptr(coef), _ptr(ws), bn, H, W, h, w, R, Cc, int(flags["regress"]), int(flags["normalize"]),
              int(flags["remap"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def workspace_floats(bn):
    from inverserenderingofindoorscene_amd import _lib
    return _lib.load().sgr_brdf_input_workspace_floats(bn)


# ---- a. geometries ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [DEFAULT, INFERENCE], ids=["default", "inference"])
@pytest.mark.parametrize("name", list(K.GEOMETRIES))
def test_resize_geometries_against_the_checker(sgr, name, flags):
    """maps equal along one axis and smaller along the other, larger along one axis (a down-sample: scale > 1 in src_index), an env grid
    of the image's size (1 x 1 pooling windows, diffuse / specular read as they are) and one taller than the image, 1 x 1 maps"""
    args = case("geometry " + name)
    out, coef = sgr.brdf_encoder_input(*args, **flags)
    against_the_checker(f"{name} {'default' if flags is DEFAULT else 'inference'}", out, coef, args, flags)


# ---- b. the striding grid --------------------------------------------------------------------------------------------------------------
# rounds of pass C's loop at the busiest thread; each shape is the smallest that reaches its branch: bn = 32 is where the cap reaches its
# floor of 64 workgroups per image, and more than 64 (256 at bn = 8) workgroups of 256 threads need more than 16384 V (65536 V) pixels
ROUNDS = {"32x129x131": (1, 2), "32x200x201": (1, 3), "32x260x256": (4, 2), "8x257x259": (1, 2), "32x260x256_same": (4, 2)}


@pytest.mark.parametrize("name", list(K.STRIDING))
def test_pass_c_strides_against_the_checker(sgr, name):
    """more workgroups wanted per image than the cap allows, so every thread of pass C takes a second (third) trip: with a cap of 64
    (its floor, bn = 32) and of 2048 / bn = 256 (bn = 8), element-wise and 128-bit, resized and identity maps.  16.6 to 36 million output
    values per case; the checker goes four images at a time"""
    args = case("striding " + name)
    bn, _, H, W = args[0].shape
    V, rounds = ROUNDS[name]
    assert V == (4 if W % 4 == 0 else 1)      # the tensors are aligned (asserted in case())
    want, cap = K.pass_c_grid(bn, H, W, V)
    print(f"{name}: V {V}, want {want} workgroups per image, cap {cap}, rounds {-(-want // cap)}")
    assert want > cap and -(-want // cap) == rounds, (name, want, cap)
    assert cap == (64 if bn == 32 else 2048 // bn)
    if name.endswith("_same"):      # pass A's two contiguous streams: 65536 elements per round
        assert tuple(args[1].shape[2:]) == (H, W) and 3 * H * W > 65536 and H * W > 65536
    out, coef = sgr.brdf_encoder_input(*args)
    against_the_checker(name, out, coef, args, DEFAULT)


def test_identity_branch_at_batch_32_in_one_round(sgr):
    """32 x 132 x 128 with maps of 132 x 128: the identity branch under V = 4 with the cap at its floor.  It does NOT stride: 16896 / 4 / 256
    = 17 workgroups wanted against a cap of 64, and pass A's streams (50688 and 16896 elements) stay below the 65536 of one round.  The
    striding partner is 32x260x256_same above"""
    args = case("same 32x132x128")
    bn, _, H, W = args[0].shape
    want, cap = K.pass_c_grid(bn, H, W, 4)
    assert (want, cap) == (17, 64) and 3 * H * W < 65536
    out, coef = sgr.brdf_encoder_input(*args)
    against_the_checker("32x132x128 same", out, coef, args, DEFAULT)


# ---- c. alignment, bit for bit ---------------------------------------------------------------------------------------------------------
# Which kernels a run takes (sgr_brdf_input_fwd): pass A is <4> when the maps are read as they are, h w % 4 == 0 and albedoPre / depthPre
# are aligned, <1> otherwise (with resized maps it always is <1>: the taps are formed element by element);  pass C is <4> when W % 4 == 0,
# `out` and `im` are aligned, the four maps are aligned IF they are read as they are, diffusePre / specularPre IF the env grid has the
# image's size.  `out` comes from the allocator here: aligned.
ALIGNMENT = [
    # geometry, the inputs shifted by one float, (pass A, pass C) of the shifted run;  the aligned run: (4, 4) for same*, (1, 4) for half*
    ("same", ("im",), (4, 1)),                       # im is not read by pass A's streams; pass C loses its 128-bit accesses
    ("same", ("albedoPre",), (1, 1)),                # read as it is by both passes
    ("same", ("depthPre",), (1, 1)),                 # the same, through the second stream
    ("same", ("diffusePre",), (4, 4)),               # resized: read tap by tap, the alignment is not asked for -- the same kernels on an odd address
    ("same_env", ("diffusePre",), (4, 1)),           # env grid at image size: read as it is, so pass C goes element-wise
    ("same", C.INPUTS, (1, 1)),
    ("half", ("im",), (1, 1)),
    ("half", ("albedoPre",), (1, 4)),                # resized maps: an offset albedoPre must still take pass_c<4>
    ("half", ("depthPre",), (1, 4)),
    ("half", ("diffusePre",), (1, 4)),
    ("half_env_same", ("diffusePre",), (1, 1)),
    ("half", C.INPUTS, (1, 1)),
]


def expected_kernels(args):
    """(V of pass A, V of pass C) by the host's rule, from the tensors' sizes and addresses; `out` aligned"""
    ok = lambda *ts: all(t.data_ptr() % 16 == 0 for t in ts)
    H, W = args[0].shape[2:]
    same_m, same_e = tuple(args[1].shape[2:]) == (H, W), tuple(args[5].shape[2:]) == (H, W)
    va = 4 if same_m and H * W % 4 == 0 and ok(args[1], args[4]) else 1
    vc = 4 if W % 4 == 0 and ok(args[0]) and (not same_m or ok(*args[1:5])) and (not same_e or ok(*args[5:7])) else 1
    return va, vc


@pytest.mark.parametrize("geometry,which,kernels", ALIGNMENT, ids=[f"{g}-{'all' if len(w) == 7 else w[0]}" for g, w, _ in ALIGNMENT])
def test_the_128_bit_and_the_element_wise_path_give_the_same_bits(sgr, geometry, which, kernels):
    args = case("aligned " + geometry)
    assert expected_kernels(args) == ((4, 4) if geometry.startswith("same") else (1, 4))
    moved = [shifted(a) if k in which else a for k, a in zip(C.INPUTS, args)]
    assert expected_kernels(moved) == kernels      # the comment beside the case, checked against the host's rule
    want, cw = sgr.brdf_encoder_input(*args)
    got, cg = sgr.brdf_encoder_input(*moved)
    assert torch.equal(got, want) and torch.equal(cg, cw), (geometry, which, float((got - want).abs().max()), int((got != want).sum()))
    for flags in (INFERENCE, dict(regress=True, normalize=False, remap=True)):
        want, cw = sgr.brdf_encoder_input(*args, **flags)
        got, cg = sgr.brdf_encoder_input(*moved, **flags)
        assert torch.equal(got, want) and torch.equal(cg, cw), (geometry, which, flags)


# ---- d. the raw C entry with `out` off its boundary -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["same", "half", "same_env"])
def test_raw_c_entry_with_an_offset_output(sgr, geometry):
    """`out` is the one tensor the operator always allocates itself: here it lies one float off, so pass C goes element-wise on aligned inputs"""
    args = case("aligned " + geometry)
    bn, _, H, W = args[0].shape
    want, cw = sgr.brdf_encoder_input(*args)
    out = shifted(torch.zeros(bn, 17, H, W, device="cuda"))
    coef, ws = torch.zeros(bn, 2, device="cuda"), torch.zeros(workspace_floats(bn), device="cuda")
    raw_call(args, out, coef, ws, DEFAULT)
    assert torch.equal(out, want) and torch.equal(coef, cw)
    aligned = torch.zeros(bn, 17, H, W, device="cuda")      # and the raw entry itself, aligned, is the operator
    raw_call(args, aligned, coef, ws, DEFAULT)
    assert torch.equal(aligned, want) and torch.equal(coef, cw)


# ---- e. reads stay inside the inputs -----------------------------------------------------------------------------------------------------
EDGE_GEOMETRIES = {"half": "aligned half", "11x13": "geometry non_integer_ratios", "down_sample": "geometry maps_larger_along_H"}


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one_float_off"])
@pytest.mark.parametrize("geometry", list(EDGE_GEOMETRIES))
@pytest.mark.parametrize("flags", [DEFAULT, INFERENCE], ids=["default", "inference"])
def test_reads_stay_inside_the_inputs(sgr, geometry, shift, flags):
    """every input in the middle of a larger buffer, one full plane of guard band on either side (as far as the last vector of a plane or
    the last tap of a row or column could reach): the bands zero, then NaN, at the same addresses.  A NaN read with weight 0 still shows"""
    args = case(EDGE_GEOMETRIES[geometry])
    held = [banded(a, a.shape[2] * a.shape[3], 0.0, shift) for a in args]
    views = [v for _, v in held]
    clean, cc = sgr.brdf_encoder_input(*views, **flags)
    for (buf, v), a in zip(held, args):
        buf.fill_(float("nan"))
        v.copy_(a)
    dirty, cd = sgr.brdf_encoder_input(*views, **flags)
    assert bool(torch.isfinite(dirty).all()) and bool(torch.isfinite(cd).all())
    assert torch.equal(dirty, clean) and torch.equal(cd, cc)
    want, cw = sgr.brdf_encoder_input(*args, **flags)      # and the placement changes nothing
    assert torch.equal(clean, want) and torch.equal(cc, cw)


# ---- f. writes stay inside the outputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one_float_off"])
@pytest.mark.parametrize("geometry", list(EDGE_GEOMETRIES) + ["tiny"])
@pytest.mark.parametrize("flags", [DEFAULT, dict(regress=False, normalize=False, remap=False)], ids=["default", "no_reduction"])
def test_writes_stay_inside_the_outputs(sgr, geometry, shift, flags):
    """through the raw C entry: `out`, `coef` and the workspace are the middles of NaN-filled buffers.  Afterwards the bands are NaN still
    and the outputs are finite throughout -- with the default flags that also says every workspace slot was written before it was folded,
    those of workgroups that received no element included (`tiny`: 36 env cells, 64 workgroups)"""
    args = case(EDGE_GEOMETRIES.get(geometry, geometry))
    bn, _, H, W = args[0].shape
    nan = float("nan")
    obuf, out = banded(torch.empty(bn, 17, H, W, device="cuda"), H * W, nan, shift)
    cbuf, coef = banded(torch.empty(bn, 2, device="cuda"), 64, nan, shift)
    nws = workspace_floats(bn)
    wbuf, ws = banded(torch.empty(nws, device="cuda"), 1024, nan, shift)
    for buf in (obuf, cbuf, wbuf):
        buf.fill_(nan)
    raw_call(args, out, coef, ws, flags)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(coef).all())
    for name, buf, inner, band in (("out", obuf, out, H * W), ("coef", cbuf, coef, 64), ("workspace", wbuf, ws, 1024)):
        lo, hi = buf[:band + shift], buf[band + shift + inner.numel():]
        assert lo.numel() == band + shift and hi.numel() == band
        assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all()), (name, int((~torch.isnan(lo)).sum()), int((~torch.isnan(hi)).sum()))
    want, cw = sgr.brdf_encoder_input(*args, **flags)
    assert torch.equal(out, want) and torch.equal(coef, cw)
    if flags["regress"]:
        assert bool(torch.isfinite(ws).all())      # every slot of both passes
    else:
        assert bool((coef == 1).all()) and bool(torch.isnan(ws).all())      # no reducing pass ran: the workspace is not touched at all


# ---- g. invariants under striding --------------------------------------------------------------------------------------------------------
def test_striding_runs_are_bit_identical_and_an_image_does_not_depend_on_its_batch(sgr):
    args = case("striding 32x129x131")
    a, ca = sgr.brdf_encoder_input(*args)
    b, cb = sgr.brdf_encoder_input(*args)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    one, c1 = sgr.brdf_encoder_input(*[t[31:32].clone() for t in args])      # alone: 67 workgroups, one round
    assert torch.equal(one[0], a[31]) and torch.equal(c1[0], ca[31])
