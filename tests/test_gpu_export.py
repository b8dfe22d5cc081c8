"""GPU: the export operators (csrc/sgr_export.hip behind torch.ops.sgrender.export_*) against the fixtures made from the reference's own
statements (tests/golden/g26_export_*.npz, tools/make_golden_export.py) and against tests/export_checker.py, which tests/test_export.py pins
to those fixtures.

The bound on bytes (export_checker.check_bytes).  Truncation is discontinuous, so a byte is judged against the fp64 value t it truncates:
delta = max(4 e_t, 1e-3), e_t the reference's own fp32 distance from fp64 (stored in the fixture; at shapes no fixture holds, the checker
evaluated in fp32 on the same inputs).  Where t is farther than delta from every integer 1..255 the byte must equal (uint8) clip(t, 0, 255);
elsewhere it may differ by one; at most 1 % of a case's bytes may lie there (tests/test_export.py asserts that of every input set used
here, and that the reference's fp32 bytes have no mismatch outside).  export_env_hwc and every layout, batch, rerun and graph comparison
are bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

import export_checker as K
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

IMAGE_CASES = ("tiny", "row", "odd", "down", "same")
BLOCK_KINDS = ("albedo", "normal", "rough", "depth", "rendered", "shading")


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


_cache = {}


def fixture(name):
    if name not in _cache:
        _cache[name] = np.load(os.path.join(GOLDEN_DIR, f"g26_export_{name}.npz"))
    return _cache[name]


def fixture_sets(name):
    z = fixture(name)
    size = tuple(int(v) for v in z["size"])
    for kind in BLOCK_KINDS:
        yield z, kind, kind, z["x_" + kind], (size if kind in K.RESIZED else None), (z["scale"] if kind == "albedo" and "scale" in z.files else None)
    if name == "same":
        for C in (1, 3):
            for kind in ("image", "image_gamma"):
                yield z, kind, f"{kind}{C}", z[f"x_image{C}"], None, None


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def t64_of(x, kind, size, scale):
    return K.image_t(x, kind, size, scale, dtype=np.float64, clip=False)


def e_t_of(x, kind, size, scale):
    return float(np.abs(K.image_t(x, kind, size, scale, dtype=np.float32, clip=False).astype(np.float64) - t64_of(x, kind, size, scale)).max())


def run(sgr, x, kind, size, scale, bgr=False):
    return sgr.export_image(x, kind, size, dev(scale) if isinstance(scale, np.ndarray) else scale, bgr)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", IMAGE_CASES)
def test_images_against_the_reference_fixtures(sgr, name):
    for z, kind, key, x, size, scale in fixture_sets(name):
        got = run(sgr, dev(x), kind, size, scale)
        assert got.dtype == torch.uint8 and tuple(got.shape) == z["ref_" + key].shape and got.is_contiguous()
        K.check_bytes(got.cpu().numpy(), t64_of(x, kind, size, scale), float(z["e_t_" + key]), f"{name} {key}")
        diff = np.abs(got.cpu().numpy().astype(int) - z["ref_" + key].astype(int))
        print(f"{name} {key}: {np.count_nonzero(diff)} of {diff.size} bytes differ from the reference's fp32 run, by at most {diff.max()}")
        assert diff.max() <= 1
        assert torch.equal(run(sgr, dev(x), kind, size, scale, bgr=True), got.flip(-1))


def raw_image(sgr, lib, x, kind, size, scale, bgr):
    B, C, h, w = x.shape
    nh, nw = size if size is not None else (h, w)
    k = sgr.EXPORT_KINDS[kind]
    out = torch.empty(B, nh, nw, 3 if k >= 6 else C, dtype=torch.uint8, device="cuda")
    need = lib.sgr_export_image_workspace_floats(k, B)
    ws = torch.empty(max(need, 1), device="cuda")
    st = (ctypes.c_longlong * 4)(*x.stride())
    rc = lib.sgr_export_image(x.data_ptr(), st, None if scale is None else scale.data_ptr(), out.data_ptr(), ws.data_ptr() if need else None, k, B, C, h, w, nh, nw, int(bgr),
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.sgr_last_error().decode()
    return out


def test_raw_c_entries_against_the_fixtures(sgr):
    from inverserenderingofindoorscene_amd import _lib
    lib = _lib.load()
    for name in IMAGE_CASES:
        for z, kind, key, x, size, scale in fixture_sets(name):
            xd, sd = dev(x), None if scale is None else dev(scale)
            got = raw_image(sgr, lib, xd, kind, size, sd, True)
            K.check_bytes(got.flip(-1).cpu().numpy(), t64_of(x, kind, size, scale), float(z["e_t_" + key]), f"C ABI {name} {key}")
            assert torch.equal(got, run(sgr, xd, kind, size, scale, bgr=True))
    z = fixture("env")
    for tag in ("a", "b"):
        env = dev(z["env_" + tag])
        nrows, ncols, gap = (int(v) for v in z["cfg_" + tag])
        B, _, R, C, eh, ew = env.shape
        Hm, Wm = K.mosaic_geometry(R, C, eh, ew, nrows, ncols, gap)[4:]
        out = torch.empty(B, Hm, Wm, 3, dtype=torch.uint8, device="cuda")
        st = (ctypes.c_longlong * 6)(*env.stride())
        assert lib.sgr_export_env_mosaic(env.data_ptr(), st, out.data_ptr(), B, R, C, eh, ew, nrows, ncols, gap, 0, torch.cuda.current_stream().cuda_stream) == 0
        assert torch.equal(out, sgr.export_env_mosaic(env, nrows, ncols, gap))
        hwc = torch.empty(B, R, C, eh, ew, 3, device="cuda")
        assert lib.sgr_export_env_hwc(env.data_ptr(), hwc.data_ptr(), B, R, C, eh, ew, 1, torch.cuda.current_stream().cuda_stream) == 0
        assert np.array_equal(hwc.cpu().numpy(), z["ref_hwc_" + tag])


def test_env_against_the_reference_fixture(sgr):
    z = fixture("env")
    for tag in ("a", "b"):
        env = dev(z["env_" + tag])
        nrows, ncols, gap = (int(v) for v in z["cfg_" + tag])
        got = sgr.export_env_mosaic(env, nrows, ncols, gap)
        assert got.dtype == torch.uint8 and tuple(got.shape) == z["ref_mosaic_" + tag].shape
        K.check_bytes(got.cpu().numpy(), K.env_mosaic_t(z["env_" + tag], nrows, ncols, gap, clip=False), float(z["e_t_mosaic_" + tag]), f"mosaic {tag}")
        assert torch.equal(sgr.export_env_mosaic(env, nrows, ncols, gap, bgr=True), got.flip(-1))
        hwc = sgr.export_env_hwc(env)
        assert hwc.dtype == torch.float32 and np.array_equal(hwc.cpu().numpy(), z["ref_hwc_" + tag])
        assert torch.equal(sgr.export_env_hwc(env, flip=False), env.permute(0, 2, 3, 4, 5, 1).contiguous())


# ---- the checker at shapes no fixture holds ---------------------------------------------------------------------------------------------

SETS = {tag: rest for tag, *rest in K.gpu_input_sets()}


@pytest.mark.parametrize("tag", list(SETS))
def test_images_against_the_checker(sgr, tag):
    kind, x, size, scale = SETS[tag]
    got = run(sgr, dev(x), kind, size, scale)
    K.check_bytes(got.cpu().numpy(), t64_of(x, kind, size, scale), e_t_of(x, kind, size, scale), tag)
    assert torch.equal(run(sgr, dev(x), kind, size, scale, bgr=True), got.flip(-1))


def test_depth_floor_and_a_maximum_in_the_last_element(sgr):
    rng = np.random.default_rng(2790)
    depth = (0.3 + 3 * rng.random((3, 1, 6, 10))).astype(np.float32)
    depth[1] = 0.0      # mean 0: the 1e-10 floor is live, d = 0, t = 255 exactly
    got = sgr.export_image(dev(depth), "depth", (9, 13)).cpu().numpy()
    assert (got[1] == 255).all()
    for b in (0, 2):
        alone = sgr.export_image(dev(depth[b:b + 1]), "depth", (9, 13)).cpu().numpy()
        assert np.array_equal(alone[0], got[b])
    x = K.draw_ok("rendered", 2, 3, 7, 9, (11, 12), 2791)
    x[1] *= np.float32(0.5)
    x[1, 2, 6, 8] = np.float32(9.0)      # the maximum sits in the last element of image 1
    got = sgr.export_image(dev(x), "rendered", (11, 12)).cpu().numpy()
    t64 = t64_of(x, "rendered", (11, 12), None)
    K.check_bytes(got, t64, e_t_of(x, "rendered", (11, 12), None), "rendered, maximum last")
    assert got[1, -1, -1, 2] == 255 and got[1].astype(int).sum() < got[0].astype(int).sum()
    # NaN -> 0, saturation both ways
    edge = np.array([np.nan, -3.0, 0.0, 1.0, 7.0, np.inf], np.float32).reshape(1, 1, 2, 3)
    assert sgr.export_image(dev(edge), "rough").cpu().numpy().reshape(-1).tolist() == [0, 0, 127, 255, 255, 255]
    assert sgr.export_image(dev(edge), "image").cpu().numpy()[..., 0].reshape(-1).tolist() == [0, 0, 0, 255, 255, 255]


@pytest.mark.parametrize("tag", [s[0] for s in K.gpu_env_sets()])
def test_env_mosaic_reads_only_the_sampled_cells(sgr, tag):
    env, nrows, ncols, gap = {s[0]: s[1:] for s in K.gpu_env_sets()}[tag]
    t64 = K.env_mosaic_t(env, nrows, ncols, gap, clip=False)
    e_t = float(np.abs(K.env_mosaic_t(env, nrows, ncols, gap, dtype=np.float32, clip=False).astype(np.float64) - t64).max())
    iy, ix = K.mosaic_geometry(*env.shape[2:], nrows, ncols, gap)[:2]
    guarded = np.full_like(env, np.nan)      # a guard band of NaN in every cell the mosaic does not sample
    guarded[:, :, ::iy, ::ix] = env[:, :, ::iy, ::ix]
    got = sgr.export_env_mosaic(dev(guarded), nrows, ncols, gap)
    K.check_bytes(got.cpu().numpy(), t64, e_t, "mosaic " + tag)
    assert torch.equal(got, sgr.export_env_mosaic(dev(env), nrows, ncols, gap))
    assert torch.equal(sgr.export_env_mosaic(dev(guarded), nrows, ncols, gap, bgr=True), got.flip(-1))


@pytest.mark.parametrize("shape", [(2, 3, 3, 4, 8, 16), (1, 3, 2, 3, 3, 5), (2, 3, 1, 1, 1, 1), (1, 3, 5, 2, 2, 2), (1, 3, 2, 2, 16, 32)])
def test_env_hwc_is_the_permutation(sgr, shape):
    env = torch.randn(*shape, device="cuda")      # eh ew = 15, 1: not a multiple of four -- the element-wise path
    for flip in (True, False):
        want = env.permute(0, 2, 3, 4, 5, 1)
        want = (want.flip(-1) if flip else want).contiguous()
        got = sgr.export_env_hwc(env, flip)
        assert got.is_contiguous() and torch.equal(got, want)
    # a view that starts off a 16-byte boundary and a sliced grid: the same values
    buf = torch.randn(env.numel() + 1, device="cuda")
    off = buf[1:].view(*shape)
    assert torch.equal(sgr.export_env_hwc(off), off.permute(0, 2, 3, 4, 5, 1).flip(-1).contiguous())
    wide = torch.randn(shape[0], 3, shape[2] + 1, shape[3] + 2, shape[4], shape[5], device="cuda")[:, :, 1:, 1:-1]
    assert torch.equal(sgr.export_env_hwc(wide), wide.permute(0, 2, 3, 4, 5, 1).flip(-1).contiguous())


# ---- layouts, batches, reruns, graphs ---------------------------------------------------------------------------------------------------

def calls(sgr):
    """(tag, call on device inputs, inputs): every operator, every statistic, both paths of the image kernel"""
    picks = ("albedo 30x41->45x60", "depth 30x41->45x60", "rendered 30x41->45x60", "rough one pixel wide", "normal 40x90->3x5: far past it", "depth 40x90->3x5: far past it",
             "shading C=3 9x13", "image C=1 9x13")
    out = []
    for tag in picks:
        kind, x, size, scale = SETS[tag]
        on_dev = None if scale is None else dev(scale)      # uploaded once: the call itself must stay free of host work (graph capture)
        out.append((tag, (lambda kind, size, scale: lambda x: run(sgr, x, kind, size, scale))(kind, size, on_dev), x))
    tag, env, nrows, ncols, gap = K.gpu_env_sets()[0]
    out.append(("mosaic", lambda e: sgr.export_env_mosaic(e, nrows, ncols, gap), env))
    out.append(("hwc", lambda e: sgr.export_env_hwc(e), env))
    return out


def test_two_runs_and_an_image_against_its_batch(sgr):
    for tag, call, x in calls(sgr):
        xd = dev(x)
        a = call(xd)
        assert torch.equal(a, call(xd)), tag
        for b in range(x.shape[0]):
            if "albedo" in tag:
                kind, _, size, scale = SETS[tag]
                alone = run(sgr, xd[b:b + 1], kind, size, None if scale is None else scale[b:b + 1])
            else:
                alone = call(xd[b:b + 1])
            assert torch.equal(alone[0], a[b]), (tag, b)


def test_strided_inputs_give_the_same_bits(sgr):
    for tag, call, x in calls(sgr):
        xd = dev(x)
        want = call(xd)
        if xd.dim() == 4:
            cl = xd.contiguous(memory_format=torch.channels_last)
            assert not cl.is_contiguous() or xd.shape[1] == 1 or xd.shape[2] * xd.shape[3] == 1
            assert torch.equal(call(cl), want), tag
            big = torch.full((xd.shape[0], xd.shape[1] + 2, xd.shape[2] + 3, 2 * xd.shape[3] + 1), float("nan"), device="cuda")
            big[:, 1:-1, 2:-1, 1::2] = xd
            view = big[:, 1:-1, 2:-1, 1::2]
            assert not view.is_contiguous() and torch.equal(call(view), want), tag
        else:
            big = torch.full((xd.shape[0], 3, xd.shape[2] + 1, xd.shape[3], xd.shape[4], xd.shape[5] + 3), float("nan"), device="cuda")
            big[:, :, 1:, :, :, 2:-1] = xd
            view = big[:, :, 1:, :, :, 2:-1]
            assert not view.is_contiguous() and torch.equal(call(view), want), tag
            assert torch.equal(call(xd.permute(0, 2, 3, 4, 5, 1).contiguous().permute(0, 5, 1, 2, 3, 4)), want), tag


def test_graph_replay(sgr):
    todo = calls(sgr)
    static = [dev(x) for _, _, x in todo]
    eager = [call(s) for (_, call, _), s in zip(todo, static)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):      # torch's capture recipe: first uses (allocator growth) on a side stream
        for (_, call, _), t in zip(todo, static):
            call(t)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = [call(t) for (_, call, _), t in zip(todo, static)]
    for o in out:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(out, eager))
    # the replay reads its inputs where they lie: new data, same graph
    for t in static:
        t.copy_(t.flip(-1) * 0.9)
    want = [call(t) for (_, call, _), t in zip(todo, static)]
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o, w) for o, w in zip(out, want))
    assert not torch.equal(want[0], eager[0])


def test_export_predictions(sgr):
    z = fixture("odd")
    size = tuple(int(v) for v in z["size"])
    one = lambda key: [dev(z["x_" + key][:1])]
    env = dev(K.gpu_env_sets()[3][1])
    preds = dict(albedo=one("albedo") * 2, normal=one("normal"), rough=one("rough"), depth=one("depth"), albedoBS=one("albedo"), roughBS=one("rough"), depthBS=one("depth"),
                 rendered=one("rendered"), shading=one("shading"), envmaps=[env])
    out = sgr.export_predictions(preds, size, cAlbedos=[float(z["scale"][0])])
    for key in ("albedo", "normal", "rough", "depth", "rendered", "shading"):
        kind_size = size if key in K.RESIZED else None
        want = sgr.export_image(preds[key][0], key, kind_size, [float(z["scale"][0])] if key == "albedo" else None, bgr=True)
        assert torch.equal(out[key + "0.png"], want), key
        K.check_bytes(out[key + "0.png"].flip(-1).cpu().numpy(), t64_of(z["x_" + key][:1], key, kind_size, z["scale"][:1] if key == "albedo" else None), float(z["e_t_" + key]),
                      "export_predictions " + key)
    assert torch.equal(out["albedoBS0.png"], out["albedo0.png"]) and torch.equal(out["depthBS0.png"], out["depth0.png"])
    assert torch.equal(out["albedo1.png"], sgr.export_image(preds["albedo"][1], "albedo", size, bgr=True))      # beyond cAlbedos: no scale
    assert not torch.equal(out["albedo1.png"], out["albedo0.png"])
    assert torch.equal(out["envmap0.npz"], env.permute(0, 2, 3, 4, 5, 1).flip(-1).contiguous())
    assert torch.equal(out["envmap0.png"], sgr.export_env_mosaic(env, 24, 16, bgr=True)) and tuple(out["envmap0.png"].shape) == (1, 217, 273, 3)


def test_autocast_keeps_fp32(sgr):
    kind, x, size, scale = SETS["albedo 2x3->5x7"]
    xd = dev(x)
    want = run(sgr, xd, kind, size, scale)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert torch.equal(run(sgr, xd, kind, size, scale), want)
        half = run(sgr, xd.to(torch.bfloat16), kind, size, scale)      # a bf16 tensor is cast up, not refused
    assert torch.equal(half, run(sgr, xd.to(torch.bfloat16).float(), kind, size, scale))


def test_opcheck(sgr):
    ops = torch.ops.sgrender
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    x3, x1 = dev(K.draw("albedo", 2, 3, 4, 6, 1)), dev(K.draw("depth", 2, 1, 4, 6, 2))
    torch.library.opcheck(ops.export_image, (x3, 0, [5, 7], torch.ones(2, device="cuda"), True), test_utils=tests)
    torch.library.opcheck(ops.export_image, (x1, 3, None, None, False), test_utils=tests)
    torch.library.opcheck(ops.export_image, (x1, 6, None, None, False), test_utils=tests)
    env = dev(K.gpu_env_sets()[0][1])
    torch.library.opcheck(ops.export_env_mosaic, (env, 2, 3, 2, False), test_utils=tests)
    torch.library.opcheck(ops.export_env_hwc, (env, True), test_utils=tests)
