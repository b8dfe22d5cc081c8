"""GPU: the loader-preparation operators (csrc/sgr_loader_prep.hip behind torch.ops.sgrender.loader_*) against the fixtures the UNMODIFIED
reference produced (tests/golden/g25_loader_*.npz, tools/make_golden_loader_prep.py) and against tests/loader_prep_checker.py, which
tests/test_loader_prep.py pins to those fixtures.

Bounds.  The masks and the order statistic ``v`` are compared with ``==``: 0 / 1 decisions and an element of the data.  ``im``, ``albedo``,
``normal``, ``rough`` and ``envmaps``: rel-L2 against the fp64 evaluation within ``max(2 e_ref, 1e-6)``, the project's standing bound for
values -- ``e_ref`` is the reference's own fp32 distance from fp64 (stored in the fixture; at shapes no fixture holds, the checker evaluated
in fp32 on the same inputs).  Exact cases (integer data, one-hot cells, images without env map), two runs, one image against its batch and
a graph replay are bit for bit."""
import os

import numpy as np
import pytest
import torch

import loader_prep_checker as K
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

CASES = ("tiny", "cell", "odd", "wide", "ratio1")
VALUE_KEYS = ("albedo", "normal", "rough", "im", "envmaps")
EXACT_KEYS = ("segArea", "segEnv", "segObj", "depth", "envmapsInd")


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


_cache = {}


def case(name):
    """(fixture, raw arrays, raw device tensors, cfg); loaded once, never written to"""
    if name not in _cache:
        z = np.load(os.path.join(GOLDEN_DIR, f"g25_loader_{name}.npz"))
        bn, H, W, R, C, eh, ew, k, is_light = (int(x) for x in z["cfg"])
        raw = {key[4:]: z[key] for key in z.files if key.startswith("raw_")}
        raw["envmaps"] = raw["envmaps"].astype(np.float32)
        phase = str(z["phase"])
        cfg = dict(bn=bn, H=H, W=W, R=R, C=C, eh=eh, ew=ew, k=k, isLight=bool(is_light), phase=phase, u=None if phase == "TEST" else z["u"])
        _cache[name] = (z, raw, {k_: torch.from_numpy(v_).cuda() for k_, v_ in raw.items()}, cfg)
    return _cache[name]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bound(e_ref):
    return max(2.0 * float(e_ref), 1e-6)


def close(tag, got, ref64, e_ref):
    e = K.rel(got.cpu().numpy(), ref64)
    print(f"{tag}: rel-L2 {e:.2e}  e_ref {float(e_ref):.2e}  bound {bound(e_ref):.2e}")
    assert np.isfinite(e) and e <= bound(e_ref), (tag, e, bound(e_ref))


def same(got, want):
    return np.array_equal(got.cpu().numpy(), np.asarray(want))


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_operators_against_the_reference_fixtures(sgr, name):
    z, raw, d, cfg = case(name)
    c64 = K.prepare_batch(raw, cfg["phase"], cfg["isLight"], cfg["u"], cfg["eh"], cfg["ew"], np.float64)
    area, env, obj = sgr.loader_masks(d["seg"], erode=cfg["isLight"])
    assert same(area, z["ref_segArea"]) and same(env, z["ref_segEnv"]) and same(obj, z["ref_segObj"])
    im, scale, v = sgr.loader_scale_hdr(d["im"], d["seg"], cfg["u"], return_v=True)
    assert same(v, z["v"]), (v.cpu().numpy(), z["v"])
    assert im.dtype == torch.float32 and tuple(scale.shape) == (cfg["bn"],)
    assert np.abs(scale.cpu().numpy().astype(np.float64) - z["scale"]).max() <= 1e-6 * np.abs(z["scale"]).max()
    close(name + " im", im, c64["im"], z["e_ref_im"])
    albedo, normal, rough = sgr.loader_brdf_maps(d["albedo"], d["normal"], d["rough"])
    for key, got in (("albedo", albedo), ("normal", normal), ("rough", rough)):
        assert tuple(got.shape) == z["ref_" + key].shape
        close(f"{name} {key}", got, c64[key], z["e_ref_" + key])
    if cfg["isLight"]:
        got = sgr.loader_envmaps(d["envmaps"], scale, d["envmapsInd"], cfg["eh"], cfg["ew"])
        assert tuple(got.shape) == z["ref_envmaps"].shape
        close(name + " envmaps", got, c64["envmaps"], z["e_ref_envmaps"])
        dead = raw["envmapsInd"] == 0
        assert not got.cpu().numpy()[dead].any()


@pytest.mark.parametrize("name", CASES)
def test_prepare_batch_returns_the_fixtures_dict_key_for_key(sgr, name):
    z, raw, d, cfg = case(name)
    c64 = K.prepare_batch(raw, cfg["phase"], cfg["isLight"], cfg["u"], cfg["eh"], cfg["ew"], np.float64)
    batch = sgr.prepare_batch(d, cfg["phase"], cfg["isLight"], cfg["u"], cfg["eh"], cfg["ew"])
    want = [key[4:] for key in z.files if key.startswith("ref_")]
    assert sorted(batch) == sorted(want)
    for key in want:
        assert tuple(batch[key].shape) == z["ref_" + key].shape and batch[key].dtype == torch.float32, key
        if key in EXACT_KEYS:
            assert same(batch[key], z["ref_" + key]), key
        else:
            close(f"{name} batch[{key}]", batch[key], c64[key], z["e_ref_" + key])


# ---- the fp64 checker at shapes no fixture holds ---------------------------------------------------------------------------------------

def draw_plane(seed, bn, H, W, cin=3):
    rng = np.random.default_rng(seed)
    q = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
    seg = np.where(rng.random((bn, H, W, cin)) < 0.7, 255, q(bn, H, W, cin)).astype(np.uint8)
    return dict(seg=seg, im=(rng.random((bn, H, W, 3)) ** 3 * 6).astype(np.float32) - np.float32(0.05), albedo=q(bn, H, W, 3), normal=q(bn, H, W, 3), rough=q(bn, H, W, 1))


@pytest.mark.parametrize("H,W", [(1, 1), (7, 1), (1, 9), (33, 65)])
def test_planes_against_the_fp64_checker(sgr, H, W):
    bn = 2
    raw = draw_plane(2600 + H * W, bn, H, W)
    u = [0.25, 0.75]
    d = {k: dev(v) for k, v in raw.items()}
    area, env, obj = sgr.loader_masks(d["seg"])
    for got, want in zip((area, env, obj), K.masks(raw["seg"])):
        assert same(got, want)
    assert same(sgr.loader_masks(d["seg"], erode=False)[2], K.masks(raw["seg"], erode=False)[2])
    im, scale, v = sgr.loader_scale_hdr(d["im"], d["seg"], u, return_v=True)
    im64, scale64, _ = K.scale_hdr(raw["im"], raw["seg"], u, np.float64)
    im32, scale32, v32 = K.scale_hdr(raw["im"], raw["seg"], u, np.float32)
    assert same(v, v32)
    close(f"{H}x{W} im", im, im64, K.rel(im32, im64))
    close(f"{H}x{W} scale", scale, scale64, K.rel(scale32, scale64))
    c64, c32 = K.brdf_maps(raw["albedo"], raw["normal"], raw["rough"], np.float64), K.brdf_maps(raw["albedo"], raw["normal"], raw["rough"], np.float32)
    for key, got, r64, r32 in zip(("albedo", "normal", "rough"), sgr.loader_brdf_maps(d["albedo"], d["normal"], d["rough"]), c64, c32):
        close(f"{H}x{W} {key}", got, r64, K.rel(r32, r64))
    # a map on its own gives the same bits as in company
    alone = sgr.loader_brdf_maps(None, d["normal"], None)
    assert alone[0] is None and alone[2] is None and torch.equal(alone[1], sgr.loader_brdf_maps(d["albedo"], d["normal"], d["rough"])[1])


@pytest.mark.parametrize("eh,ew", [(8, 16), (16, 32)])
@pytest.mark.parametrize("R,C", [(1, 1), (5, 3), (4, 37)])
def test_env_grids_against_the_fp64_checker(sgr, R, C, eh, ew):
    rng = np.random.default_rng(2700 + R * C + eh)
    bn = 2
    raw = (rng.random((bn, R * 16, C * 32, 3)) ** 2 * 8).astype(np.float32)
    scale = np.array([0.37, 1.9], np.float32)
    got = sgr.loader_envmaps(dev(raw), dev(scale), None, eh, ew)
    r64, r32 = K.envmaps(raw, scale, None, eh, ew, np.float64), K.envmaps(raw, scale, None, eh, ew, np.float32)
    assert tuple(got.shape) == (bn, 3, R, C, eh, ew)
    close(f"{R}x{C} {eh}x{ew}", got, r64, K.rel(r32, r64))
    assert same(got, r32)      # the contract's expression, bit for bit


# ---- select edges -------------------------------------------------------------------------------------------------------------------------

def select(sgr, values, H, W):
    """v of loader_scale_hdr over `values` [bn, H*W*3] with an all-object mask (seg = 1 exactly: the products are the values)"""
    bn = values.shape[0]
    seg = torch.full((bn, H, W, 1), 255, dtype=torch.uint8, device="cuda")
    _, _, v = sgr.loader_scale_hdr(dev(values.reshape(bn, H, W, 3)), seg, None, return_v=True)
    return v.cpu().numpy()


def test_select_all_values_equal(sgr):
    for val in (0.75, 0.0, -2.0, 1e-40):
        x = np.full((1, 8 * 16 * 3), val, np.float32)
        assert np.array_equal(select(sgr, x, 8, 16), x[:, 0])


def key_to_float(key):
    key = np.asarray(key, np.uint32)
    bits = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7FFFFFFF), ~key)
    return bits.astype(np.uint32).view(np.float32)


def float_to_key(x):
    u = np.asarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


@pytest.mark.parametrize("digit", [0, 255])
@pytest.mark.parametrize("p", [0, 1, 2, 3])
def test_select_answer_in_the_lowest_and_highest_bucket_of_every_pass(sgr, p, digit):
    """the element of rank k carries `digit` in the eight bits radix pass p looks at; its neighbours in rank lie within a few buckets of it at
    that pass, on both sides, so the walk over the histogram must stop in the first / last bucket, with the carried-over rank right"""
    H, W = 4, 8
    n, k = H * W * 3, K.rank_k(H, W)
    rng = np.random.default_rng(2800 + 10 * p + digit)
    answer = np.array([0x40, 0x37, 0x9A, 0x5C], np.int64)
    answer[p] = digit
    if p == 0:
        answer[1] = 0x9A if digit == 0 else 0x37      # keep the float finite: keys 0x00800000 .. 0xFF7FFFFF
    a = int((answer[0] << 24) | (answer[1] << 16) | (answer[2] << 8) | answer[3])
    span = 1 << (8 * (3 - p) + 2)      # four buckets of pass p
    below = a - rng.integers(1, span, k)
    above = a + rng.integers(1, span, n - k - 1)
    keys = np.clip(np.concatenate([below, [a], above]), 0x00800000, 0xFF7FFFFF).astype(np.uint32)
    assert (keys[:k] < a).all() and (keys[k + 1:] > a).all()
    x = key_to_float(rng.permutation(keys))[None]
    assert np.isfinite(x).all() and np.array_equal(np.sort(float_to_key(x[0])), np.sort(keys))
    want = np.sort(x[0])[k]
    assert (int(float_to_key(want)) >> (8 * (3 - p))) & 255 == digit and want == key_to_float(a)
    assert np.array_equal(select(sgr, x, H, W), [want])


@pytest.mark.parametrize("HW", [1023, 1024, 1025])
def test_select_element_counts_around_the_workgroups_stride(sgr, HW):
    """the select's workgroup strides over the pixels by its 1024 threads"""
    rng = np.random.default_rng(2900 + HW)
    x = (rng.standard_normal((2, HW * 3)) * 3).astype(np.float32)
    x[1, : HW] = 0.0
    got = select(sgr, x, 1, HW)
    assert np.array_equal(got, np.sort(x, axis=1)[:, K.rank_k(1, HW)])


def test_select_at_the_training_size_once(sgr):
    rng = np.random.default_rng(2950)
    H, W = 120, 160
    raw = draw_plane(2951, 1, H, W)
    raw["seg"][0, :, : W // 3, 0] = 0      # a masked third: a long run of equal products
    d = {k: dev(v) for k, v in raw.items()}
    im, scale, v = sgr.loader_scale_hdr(d["im"], d["seg"], [float(rng.random())], return_v=True)
    prod = raw["im"][0] * K.seg_value(raw["seg"][0, ..., 0])[..., None]
    assert np.array_equal(v.cpu().numpy(), [np.sort(prod.reshape(-1))[K.rank_k(H, W)]])


def test_nan_and_inf_in_hdr_do_not_fault(sgr):
    """outside the domain: the result is unspecified, the run is clean"""
    x = np.random.default_rng(2960).random((1, 4, 8, 3)).astype(np.float32)
    x[0, 0, 0] = [np.nan, np.inf, -np.inf]
    seg = torch.full((1, 4, 8, 1), 255, dtype=torch.uint8, device="cuda")
    im, scale, v = sgr.loader_scale_hdr(dev(x), seg, None, return_v=True)
    torch.cuda.synchronize()
    assert tuple(im.shape) == (1, 3, 4, 8)


# ---- erosion edges ------------------------------------------------------------------------------------------------------------------------

def eroded(sgr, obj):
    """segObj of loader_masks for a [H,W] bool plane (codes 255 / 0)"""
    seg = dev(np.where(obj, 255, 0).astype(np.uint8)[None, ..., None])
    return sgr.loader_masks(seg)[2][0, 0].cpu().numpy().astype(bool)


def test_erosion_single_unset_pixel_at_each_corner_and_edge(sgr):
    H, W = 20, 70      # two tiles of the mask kernel along each axis
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (15, 63), (16, 64), (H // 2, W // 2)]
    for y, x in spots:
        obj = np.ones((H, W), bool)
        obj[y, x] = False
        want = K.scipy_erosion(obj)
        got = eroded(sgr, obj)
        assert np.array_equal(got, want), (y, x)
        assert (~got).sum() == (min(y + 3, H - 1) - max(y - 3, 0) + 1) * (min(x + 3, W - 1) - max(x - 3, 0) + 1)
    assert eroded(sgr, np.ones((H, W), bool)).all()      # border_value=1: a full plane stays full


@pytest.mark.parametrize("H,W", [(1, 1), (3, 4), (6, 6), (2, 9), (7, 7)])
def test_erosion_on_planes_smaller_than_the_box(sgr, H, W):
    rng = np.random.default_rng(3000 + H * 10 + W)
    for p in (0.8, 0.95, 1.0):
        obj = rng.random((H, W)) < p
        assert np.array_equal(eroded(sgr, obj), K.scipy_erosion(obj)), (H, W, p)


def test_all_byte_values_through_the_mask_kernel(sgr):
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)
    got = sgr.loader_masks(dev(u8), erode=False)
    seg = 0.5 * ((u8.astype(np.float32)[..., 0] - 127.5) / 127.5 + 1)      # numpy's fp32 evaluation of dataLoader.py:120
    assert same(got[0][:, 0], np.logical_and(seg > 0.49, seg < 0.51).astype(np.float32))
    assert same(got[1][:, 0], (seg < 0.1).astype(np.float32)) and same(got[2][:, 0], (seg > 0.9).astype(np.float32))
    # the continuous value, through the order statistic: one byte value per image, hdr = 1
    hdr = torch.ones(256, 1, 1, 3, device="cuda")
    _, _, v = sgr.loader_scale_hdr(hdr, dev(u8.reshape(256, 1, 1, 1)), None, return_v=True)
    assert same(v, seg.reshape(256))


# ---- env map ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eh,ew", [(8, 16), (16, 32)])
def test_env_integer_data_with_unit_scale_is_exact(sgr, eh, ew):
    rng = np.random.default_rng(3100 + eh)
    raw = rng.integers(-50, 200, (2, 3 * 16, 6 * 32, 3)).astype(np.float32)
    got = sgr.loader_envmaps(dev(raw), torch.ones(2, device="cuda"), None, eh, ew)
    e = raw.astype(np.float64).reshape(2, 3, 16, 6, 32, 3).transpose(0, 5, 1, 3, 2, 4)
    want = e if eh == 16 else e.reshape(2, 3, 3, 6, 8, 2, 16, 2).mean(axis=(5, 7))
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want)


@pytest.mark.parametrize("eh,ew", [(8, 16), (16, 32)])
def test_env_one_hot_inputs_cover_every_position_of_a_cell(sgr, eh, ew):
    """image t of the batch holds a single 1 at position t of its one cell: 16 x 32 x 3 images"""
    n = 16 * 32 * 3
    raw = torch.zeros(n, 16 * 32 * 3, device="cuda")
    raw[torch.arange(n), torch.arange(n)] = 1.0
    got = sgr.loader_envmaps(raw.view(n, 16, 32, 3), torch.ones(n, device="cuda"), None, eh, ew).cpu().numpy()
    t = np.arange(n)
    i, j, k = t // 96, (t // 3) % 32, t % 3
    want = np.zeros((n, 3, 1, 1, eh, ew), np.float32)
    if eh == 8:
        want[t, k, 0, 0, i // 2, j // 2] = 0.25
    else:
        want[t, k, 0, 0, i, j] = 1.0
    assert np.array_equal(got, want)


def test_env_image_without_env_map_is_zero_and_guard_bands_stay(sgr):
    rng = np.random.default_rng(3200)
    bn, R, C = 3, 2, 5
    per = R * 16 * C * 32 * 3
    for guard in (64, 3):      # 3: the view is not 16-byte aligned, the operator reads an aligned copy
        buf = torch.full((guard + bn * per + guard,), -777.0, device="cuda")
        body = rng.random((bn, R * 16, C * 32, 3)).astype(np.float32)
        body[1] = np.nan      # never read: env_ind[1] == 0
        buf[guard:guard + bn * per] = dev(body).reshape(-1)
        before = buf.clone()
        raw = buf[guard:guard + bn * per].view(bn, R * 16, C * 32, 3)
        ind = torch.tensor([1.0, 0.0, 1.0], device="cuda")
        scale = dev(np.array([0.5, 2.0, 1.25], np.float32))
        got = sgr.loader_envmaps(raw, scale, ind.view(bn, 1, 1, 1))
        want = K.envmaps(np.nan_to_num(body), scale.cpu().numpy(), ind.cpu().numpy())
        assert same(got, want) and not got[1].any().item()
        assert torch.equal(buf.view(torch.int32), before.view(torch.int32))


# ---- across the operators -----------------------------------------------------------------------------------------------------------------

def run_all(sgr, d, cfg):
    b = sgr.prepare_batch(d, cfg["phase"], True, cfg["u"], cfg["eh"], cfg["ew"])
    return [b[k] for k in VALUE_KEYS + EXACT_KEYS]


def test_two_runs_are_bit_identical_and_an_image_does_not_depend_on_its_batch(sgr):
    _, raw, d, cfg = case("odd")
    first, second = run_all(sgr, d, cfg), run_all(sgr, d, cfg)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for b in range(cfg["bn"]):
        one = {k: v[b:b + 1].clone() for k, v in d.items()}
        alone = run_all(sgr, one, dict(cfg, u=cfg["u"][b:b + 1]))
        assert all(torch.equal(a[0], f[b]) for a, f in zip(alone, first)), b


def test_graph_capture_and_replay(sgr):
    _, raw, d, cfg = case("odd")
    static = {k: v.clone() for k, v in d.items()}
    u = dev(np.asarray(cfg["u"], np.float32))      # a device tensor: nothing of the call runs on the host
    call = lambda: sgr.prepare_batch(static, "TRAIN", True, u, cfg["eh"], cfg["ew"])
    eager = call()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):      # torch's capture recipe: first uses (allocator growth) on a side stream
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for k in VALUE_KEYS + ("segObj",):
        out[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager[k]) for k in VALUE_KEYS + EXACT_KEYS)
    # the replay reads its inputs where they lie: new data, same graph
    for k in ("im", "envmaps", "seg", "albedo"):
        static[k].copy_(d[k].flip(0))
    want = call()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], want[k]) for k in VALUE_KEYS + EXACT_KEYS)
    assert not torch.equal(want["im"], eager["im"])


def test_opcheck(sgr):
    ops = torch.ops.sgrender
    _, raw, d, cfg = case("cell")
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(ops.loader_masks, (d["seg"], True), test_utils=tests)
    torch.library.opcheck(ops.loader_scale_hdr, (d["im"], d["seg"], None, cfg["k"]), test_utils=tests)
    torch.library.opcheck(ops.loader_scale_hdr, (d["im"], d["seg"], torch.full((1,), 0.9, device="cuda"), cfg["k"]), test_utils=tests)
    torch.library.opcheck(ops.loader_brdf_maps, (d["albedo"], d["normal"], d["rough"]), test_utils=tests)
    torch.library.opcheck(ops.loader_brdf_maps, (None, d["normal"], None), test_utils=tests)
    torch.library.opcheck(ops.loader_envmaps, (d["envmaps"], torch.ones(1, device="cuda"), d["envmapsInd"], 8, 16), test_utils=tests)
    torch.library.opcheck(ops.loader_envmaps, (d["envmaps"], torch.ones(1, device="cuda"), None, 16, 32), test_utils=tests)
