"""GPU: the real-image loader operators (sgr.nyu_prepare_batch, sgr.nyu_augmentation, sgr.iiw_image) on the device -- values against the
fixtures the unmodified reference loaders produced and against the fp64 checker (rel-L2 within max(2 e_ref, 1e-6); segDepth with == outside
the pixels within 1e-5 t of a threshold t, 1 % at most), shapes no fixture holds, the crop border, the exact properties (batch, rerun, mirror,
TEST as a TRAIN call, alignment, the two forms of the kernel), the raw C entries and HIP-graph capture with device-side augmentation."""
import ctypes
import os

import numpy as np
import pytest
import torch

import real_loader_checker as K
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

NYU_CASES = ("tiny", "up", "down", "corner", "corner2", "mixed", "test", "w1", "w7", "ratio", "quarter")
IIW_CASES = ("tiny", "odd", "black")


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


_cache = {}


def fixture(name):
    if name not in _cache:
        _cache[name] = np.load(os.path.join(GOLDEN_DIR, f"g27_{name}.npz"))
    return _cache[name]


def args_of(z):
    raw = {k: z[k] for k in ("im", "normal", "seg", "depth")}
    H, W, _, _, train = (int(v) for v in z["cfg"])
    return (raw, z["crop"], z["flip"], z["colour"], H, W) if train else (raw, None, None, None, H, W)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(sgr, raw, crop, flip, colour, H, W, on_device=True):
    """the wrapper on a numpy batch -> dict of device tensors; the augmentation as device tensors or as host values"""
    d = {k: dev(v) for k, v in raw.items()}
    if crop is None:
        return sgr.nyu_prepare_batch(d, "TEST", imHeight=H, imWidth=W)
    aug = (dev(np.asarray(crop, np.int32)), dev(np.asarray(flip, bool)), dev(np.asarray(colour, np.float64))) if on_device else (crop, flip, colour)
    return sgr.nyu_prepare_batch(d, "TRAIN", *aug, imHeight=H, imWidth=W)


def host(out):
    return {k: out[k].cpu().numpy() for k in K.NYU_KEYS}


def same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in K.NYU_KEYS)


_sets = {}


def gpu_set(i):
    """(raw, crop, flip, colour, H, W, the fp32 and the fp64 checker's outputs) of K.GPU_SHAPES[i], computed once"""
    if i not in _sets:
        _, bn, Hs, Ws, H, W, side = K.GPU_SHAPES[i]
        raw = K.draw_raw(bn, Hs, Ws, 2800 + i)
        crop, flip, colour = K.draw_aug(bn, Hs, Ws, 2900 + i, side)
        _sets[i] = (raw, crop, flip, colour, H, W, K.nyu_prepare(raw, crop, flip, colour, H, W, np.float32), K.nyu_prepare(raw, crop, flip, colour, H, W, np.float64))
    return _sets[i]


# ---- values -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NYU_CASES)
def test_nyu_against_the_reference_fixtures(sgr, name):
    z = fixture("nyu_" + name)
    raw, crop, flip, colour, H, W = args_of(z)
    out = run(sgr, raw, crop, flip, colour, H, W)
    for k in K.NYU_KEYS:
        assert out[k].dtype == torch.float32 and tuple(out[k].shape) == z["ref_" + k].shape and out[k].is_contiguous(), (name, k)
    e_ref = {k: float(z["e_ref_" + k]) for k in K.NYU_KEYS}
    want64 = K.nyu_prepare(raw, crop, flip, colour, H, W, np.float64)      # the checker, which the CPU tests pin to the fixture's fp64 run
    K.check_nyu(host(out), {k: z["ref64_" + k] for k in K.NYU_KEYS}, e_ref, name + " (fixture)", seg_depth_everywhere=name == "quarter")
    K.check_nyu(host(out), want64, e_ref, name + " (checker)", seg_depth_everywhere=name == "quarter")
    if crop is not None:      # host values go through the wrapper's checks and give the same bits
        assert same_bits(run(sgr, raw, crop, flip, colour, H, W, on_device=False), out), name


@pytest.mark.parametrize("i", range(len(K.GPU_SHAPES)), ids=[s[0] for s in K.GPU_SHAPES])
def test_nyu_against_the_checker(sgr, i):
    raw, crop, flip, colour, H, W, w32, w64 = gpu_set(i)
    got = host(run(sgr, raw, crop, flip, colour, H, W))
    e_ref = {k: K.rel_l2(w32[k], w64[k]) for k in K.NYU_KEYS}      # the fp32 checker's own distance from fp64 on these inputs
    K.check_nyu(got, w64, e_ref, K.GPU_SHAPES[i][0])
    for k in ("normal", "depth", "segNormal", "im"):      # and the fp32 checker itself: two fp32 evaluations, each within e_ref of fp64
        assert K.rel_l2(got[k], w32[k]) <= K.bound_of(e_ref[k]), (K.GPU_SHAPES[i][0], k, K.rel_l2(got[k], w32[k]))


def test_unit_normals_and_the_floor(sgr):
    """|normal| = 1 after the second normalisation; a normal of all 127.5-neighbours (|n|^2 below 1e-5 is out of a byte's reach: the smallest
    is 3 / 255^2 = 4.6e-5) stays finite"""
    raw = K.draw_raw(1, 6, 8, 5)
    raw["normal"][:] = (127, 128, 127)
    out = run(sgr, raw, None, None, None, 9, 11)["normal"]
    assert torch.isfinite(out).all() and ((out.double() ** 2).sum(1).sqrt() - 1).abs().max() < 1e-6


# ---- the crop border ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("up", "down", "corner", "corner2", "mixed", "ratio"))
def test_nothing_outside_the_crop_is_read(sgr, name):
    z = fixture("nyu_" + name)
    raw, crop, flip, colour, H, W = args_of(z)
    dirty = {k: v.copy() for k, v in raw.items()}
    for b, (rs, cs, ch, cw) in enumerate(crop.tolist()):
        inside = np.zeros(raw["depth"].shape[1:], bool)
        inside[rs:rs + ch, cs:cs + cw] = True
        dirty["depth"][b][~inside] = np.nan
        for k in ("im", "normal", "seg"):
            dirty[k][b][~inside] = 255
    assert any(np.isnan(dirty["depth"][b]).any() for b in range(len(crop)))
    got, clean = run(sgr, dirty, crop, flip, colour, H, W), run(sgr, raw, crop, flip, colour, H, W)
    assert same_bits(got, clean) and torch.isfinite(got["depth"]).all(), name


def test_a_bad_device_rectangle_is_clamped_into_the_source(sgr):
    """a rectangle from device memory cannot be refused: the kernel uses clamp_rect's rectangle (the host build pins the rule under ASan)"""
    raw = K.draw_raw(3, 6, 9, 31)
    flip, colour = np.array([False, True, False]), 1 + 0.1 * np.arange(9).reshape(3, 3)
    bad = np.array([[-3, -2, 4, 5], [4, 7, 9, 9], [99, 99, 0, -4]], np.int32)
    used = np.array([[0, 0, 4, 5], [4, 7, 2, 2], [5, 8, 1, 1]], np.int32)
    assert same_bits(run(sgr, raw, bad, flip, colour, 5, 7), run(sgr, raw, used, flip, colour, 5, 7))
    with pytest.raises(RuntimeError, match="leaves the source"):
        run(sgr, raw, bad, flip, colour, 5, 7, on_device=False)


# ---- exact properties ---------------------------------------------------------------------------------------------------------------------

def test_an_image_alone_equals_the_image_in_its_batch_and_two_runs_agree(sgr):
    z = fixture("nyu_mixed")
    raw, crop, flip, colour, H, W = args_of(z)
    whole = run(sgr, raw, crop, flip, colour, H, W)
    assert same_bits(whole, run(sgr, raw, crop, flip, colour, H, W))
    for b in range(3):
        alone = run(sgr, {k: v[b:b + 1] for k, v in raw.items()}, crop[b:b + 1], flip[b:b + 1], colour[b:b + 1], H, W)
        assert all(torch.equal(alone[k][0], whole[k][b]) for k in K.NYU_KEYS), b
    raw, crop, flip, colour, H, W, _, _ = gpu_set(6)
    whole = run(sgr, raw, crop, flip, colour, H, W)
    alone = run(sgr, {k: v[1:2] for k, v in raw.items()}, crop[1:2], flip[1:2], colour[1:2], H, W)
    assert all(torch.equal(alone[k][0], whole[k][1]) for k in K.NYU_KEYS) and same_bits(whole, run(sgr, raw, crop, flip, colour, H, W))


@pytest.mark.parametrize("i", (0, 1, 6), ids=[K.GPU_SHAPES[i][0] for i in (0, 1, 6)])
def test_a_flipped_call_is_the_unflipped_call_mirrored(sgr, i):
    raw, crop, _, colour, H, W, _, _ = gpu_set(i)
    bn = len(crop)
    plain, flipped = run(sgr, raw, crop, np.zeros(bn, bool), colour, H, W), run(sgr, raw, crop, np.ones(bn, bool), colour, H, W)
    for k in K.NYU_KEYS:
        want = plain[k].flip(-1)
        if k == "normal":
            want = torch.cat([-want[:, 0:1], want[:, 1:]], 1)
        assert torch.equal(flipped[k], want), (i, k)


@pytest.mark.parametrize("name", ("test", "ratio"))
def test_the_test_phase_is_a_train_call_with_the_full_rectangle(sgr, name):
    z = fixture("nyu_" + name)
    raw, _, _, _, H, W = args_of(z)
    bn, Hs, Ws = raw["depth"].shape
    full = np.tile(np.array([0, 0, Hs, Ws], np.int32), (bn, 1))
    assert same_bits(run(sgr, raw, None, None, None, H, W), run(sgr, raw, full, np.zeros(bn, bool), np.ones((bn, 3)), H, W))


def test_inputs_off_a_16_byte_boundary_and_strided_inputs_give_the_same_bits(sgr):
    raw, crop, flip, colour, H, W, _, _ = gpu_set(0)
    want = run(sgr, raw, crop, flip, colour, H, W)
    aug = (dev(crop), dev(flip), dev(colour))

    def off_by_one(x):      # the same values, starting one element into a fresh buffer
        x = dev(x)
        flat = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
        flat[1:] = x.reshape(-1)
        v = flat[1:].view(x.shape)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v
    assert same_bits(sgr.nyu_prepare_batch({k: off_by_one(v) for k, v in raw.items()}, "TRAIN", *aug, imHeight=H, imWidth=W), want)
    wide = {k: dev(np.concatenate([v, v], axis=2))[:, :, :v.shape[2]] for k, v in raw.items()}      # column slices of a wider batch
    assert not wide["im"].is_contiguous() and same_bits(sgr.nyu_prepare_batch(wide, "TRAIN", *aug, imHeight=H, imWidth=W), want)
    depth4 = dict({k: dev(v) for k, v in raw.items()}, depth=dev(raw["depth"])[:, None], name=["x"] * len(crop))
    out = sgr.nyu_prepare_batch(depth4, "TRAIN", *aug, imHeight=H, imWidth=W)
    assert same_bits(out, want) and out["name"] == ["x"] * len(crop)


@pytest.mark.parametrize("i", range(len(K.GPU_SHAPES)), ids=[s[0] for s in K.GPU_SHAPES])
def test_the_staged_and_the_direct_form_give_the_same_bits(sgr, i, monkeypatch):
    raw, crop, flip, colour, H, W, _, _ = gpu_set(i)
    monkeypatch.setenv("SGR_NYU_STAGE", "0")
    direct = run(sgr, raw, crop, flip, colour, H, W)
    monkeypatch.setenv("SGR_NYU_STAGE", "1")
    staged = run(sgr, raw, crop, flip, colour, H, W)
    assert same_bits(direct, staged), K.GPU_SHAPES[i][0]


def raw_nyu(lib, d, aug, H, W, offset):
    """sgr_nyu_prepare itself; every output `offset` floats into its own buffer"""
    bn, Hs, Ws = d["depth"].shape
    bufs = [torch.zeros(bn * C * H * W + offset + 4, device="cuda") for C in (3, 1, 1, 1, 3)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = lib.sgr_nyu_prepare(ptr(d["im"]), ptr(d["normal"]), ptr(d["seg"]), ptr(d["depth"]), *(ptr(a) for a in aug), *(ctypes.c_void_p(b.data_ptr() + 4 * offset) for b in bufs),
                             bn, Hs, Ws, H, W, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.sgr_last_error()
    torch.cuda.synchronize()
    out = {k: b[offset:offset + bn * C * H * W].view(bn, C, H, W) for k, b, C in zip(K.NYU_KEYS, bufs, (3, 1, 1, 1, 3))}
    assert all(float(b[offset + bn * C * H * W:].abs().max()) == 0 and float(b[:offset].abs().sum()) == 0 for b, C in zip(bufs, (3, 1, 1, 1, 3)))      # nothing past the ends
    return out


def test_raw_c_entry_with_aligned_and_unaligned_outputs(sgr):
    from inverserenderingofindoorscene_amd import _lib
    lib = _lib.load()
    for i in (0, 2):      # W = 130 (scalar stores) and W = 4 (128-bit stores when aligned)
        raw, crop, flip, colour, H, W, _, _ = gpu_set(i)
        d = {k: dev(v) for k, v in raw.items()}
        aug = (dev(crop), dev(flip).to(torch.uint8), dev(colour))
        want = run(sgr, raw, crop, flip, colour, H, W)
        for offset in (0, 1):
            assert same_bits(raw_nyu(lib, d, aug, H, W, offset), want), (i, offset)
    raw, _, _, _, H, W = args_of(fixture("nyu_test"))
    assert same_bits(raw_nyu(lib, {k: dev(v) for k, v in raw.items()}, (None, None, None), H, W, 0), run(sgr, raw, None, None, None, H, W))


# ---- HIP graph ----------------------------------------------------------------------------------------------------------------------------

def test_graph_replay_with_device_side_augmentation(sgr):
    Hs, Ws, H, W, wmax, wmin, bn = 24, 32, 12, 16, 28, 20, 3
    raw = {k: dev(v) for k, v in K.draw_raw(bn, Hs, Ws, 77).items()}
    rng = np.random.default_rng(78)
    u = dev(rng.random((bn, 7)))

    def step():
        crop, flip, colour = sgr.nyu_augmentation(u, H, W, wmax, wmin, srcHeight=Hs, srcWidth=Ws)
        return sgr.nyu_prepare_batch(raw, "TRAIN", crop, flip, colour, imHeight=H, imWidth=W)
    eager = {k: v.clone() for k, v in step().items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):      # torch's capture recipe: first uses (allocator growth) on a side stream
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    for k in K.NYU_KEYS:
        out[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager)
    # new draws written in place: the replay forms the new rectangles on the device
    u.copy_(dev(rng.random((bn, 7))))
    g.replay()
    torch.cuda.synchronize()
    want = step()
    assert same_bits(out, want) and not torch.equal(want["im"], eager["im"])
    crop = sgr.nyu_augmentation(u, H, W, wmax, wmin, srcHeight=Hs, srcWidth=Ws)[0].cpu().numpy()
    assert (crop[:, 0] + crop[:, 2] <= Hs).all() and (crop[:, 1] + crop[:, 3] <= Ws).all() and len({tuple(c) for c in crop.tolist()}) > 1


def test_autocast_keeps_fp32_and_the_double_colour(sgr):
    z = fixture("nyu_mixed")
    raw, crop, flip, colour, H, W = args_of(z)
    want = run(sgr, raw, crop, flip, colour, H, W)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = run(sgr, raw, crop, flip, colour, H, W)
        im = sgr.iiw_image(dev(fixture("iiw_odd")["im_u8"]))
    assert same_bits(got, want) and im.dtype == torch.float32


# ---- iiw_image ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", IIW_CASES)
def test_iiw_against_the_reference_fixtures(sgr, name):
    z = fixture("iiw_" + name)
    out = sgr.iiw_image(dev(z["im_u8"]))
    assert out.dtype == torch.float32 and tuple(out.shape) == z["ref_im"].shape and out.is_contiguous()
    if name == "black":
        assert torch.isnan(out).all()
        return
    e = K.rel_l2(out.cpu().numpy(), z["ref64_im"])
    print(f"iiw {name}: rel-L2 {e:.2e}, bound {K.bound_of(z['e_ref_im']):.2e}")
    assert e <= K.bound_of(z["e_ref_im"])
    assert all(float(out[b].max()) == 1.0 for b in range(out.shape[0]))      # the image's largest byte divided by itself


@pytest.mark.parametrize("shape", [(2, 4, 6), (3, 5, 7), (1, 1, 3), (2, 33, 40), (1, 64, 129)], ids=str)
def test_iiw_against_the_checker_alone_in_a_batch_and_twice(sgr, shape):
    bn, H, W = shape
    rng = np.random.default_rng(sum(shape))
    im = rng.integers(0, 256, (bn, H, W, 3), dtype=np.uint8)
    im[0] //= 3      # another maximum per image
    w32, w64 = K.iiw_image(im, np.float32), K.iiw_image(im, np.float64)
    out = sgr.iiw_image(dev(im))
    assert K.rel_l2(out.cpu().numpy(), w64) <= K.bound_of(K.rel_l2(w32, w64))
    assert all(float(out[b].max()) == 1.0 for b in range(bn)) and torch.equal(out, sgr.iiw_image(dev(im)))
    for b in range(bn):
        assert torch.equal(sgr.iiw_image(dev(im[b:b + 1]))[0], out[b]), b
    flat = torch.empty(im.size + 1, dtype=torch.uint8, device="cuda")      # one byte off: the byte-load form
    flat[1:] = dev(im).reshape(-1)
    assert torch.equal(sgr.iiw_image(flat[1:].view(im.shape)), out)
    black = im.copy()
    black[-1] = 0
    got = sgr.iiw_image(dev(black))
    assert torch.isnan(got[-1]).all() and (bn == 1 or torch.equal(got[:-1], out[:-1]))      # a black image does not touch its neighbours


def test_opcheck(sgr):
    z = fixture("nyu_mixed")
    raw, crop, flip, colour, H, W = args_of(z)
    d = {k: dev(v) for k, v in raw.items()}
    torch.library.opcheck(torch.ops.sgrender.nyu_prepare.default, (d["im"], d["normal"], d["seg"], d["depth"], dev(crop), dev(flip), dev(colour), H, W),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.sgrender.iiw_image.default, (dev(fixture("iiw_odd")["im_u8"]),), test_utils=("test_schema", "test_faketensor"))
