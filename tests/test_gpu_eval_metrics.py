"""GPU: the evaluation-metric operators (sgr.whdr, sgr.whdr_from_ranking, sgr.normal_angle_error, sgr.depth_log_rmse) on the device -- values
against the fixtures made from the reference's own statements and against the fp64 checker (sums within max(2 e_ref, 1e-12 |ref|); reported
values within max(2 e_ref, 1e-5 |ref|); theta rel-L2 within max(2 e_ref, 1e-6); classifications and counts with == under the margin condition
that tests/test_eval_metrics.py proves on these very inputs, nothing left out; the median == numpy's median of the kernel's own angles), the
edge sizes no fixture holds, and the exact properties: reruns, an image against its batch, strided inputs, a replayed HIP graph, autocast.
Every measured distance is printed beside its bound (profiles/r30_eval_metrics_gpu_tests.txt is this output)."""
import os

import numpy as np
import pytest
import torch

import eval_metrics_checker as K
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

WHDR_CASES = ("mix", "floor")
NORMAL_CASES = ("id", "up", "odd", "one", "ties", "none")
DEPTH_CASES = ("id", "up", "zeros", "edge", "none", "one")


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


def fixture(kind, name):
    return np.load(os.path.join(GOLDEN_DIR, f"g28_evalmetrics_{kind}_{name}.npz"))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(out):
    return [host(t).tobytes() for t in out]


def close(got, ref, e_ref, rel, what):
    """|got - ref| <= max(2 e_ref, rel |ref|) elementwise, NaN matching NaN; prints the worst distance beside its bound"""
    got, ref, e_ref = (np.atleast_1d(np.asarray(v, np.float64)) for v in (got, ref, e_ref))
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    ok = ~np.isnan(ref)
    e_ref = np.broadcast_to(np.nan_to_num(e_ref), ref.shape)
    dist, bound = np.abs(got - ref)[ok], np.maximum(2 * e_ref[ok], rel * np.abs(ref)[ok])
    if dist.size:
        i = int(np.argmax(dist - bound))
        print(f"{what}: worst |got - ref| = {dist[i]:.3e}, bound {bound[i]:.3e}")
    assert np.all(dist <= bound), (what, dist, bound)


# ---- WHDR -----------------------------------------------------------------------------------------------------------------------------------

def run_whdr(sgr, im, point, weight, label, num, delta=0.1):
    return sgr.whdr(dev(im), dev(point), dev(weight), dev(label), dev(num), delta)


def check_whdr(out, im_u8, point, weight, label, num, what, ref64=None, e=None):
    """against the fp64 checker (and, with ref64, the reference's fp64 run and its own fp32 error)"""
    c64 = K.whdr(K.reflectance_of(im_u8, np.float64), point, weight, label, num)
    if e is None:      # the reference's fp32-vs-fp64 distance by the checker's two evaluations
        e = np.abs(K.whdr(K.reflectance_of(im_u8, np.float32), point, weight, label, num, dtype=np.float32)["ratios"] - c64["ratios"])
        ref64 = c64["ratios"]
    # every classification ==: a flipped class moves an error sum by that judgement's weight (>= 0.01), far beyond the bound of the sums
    close(host(out.sums), c64["sums"], 0.0, 1e-12, what + " sums")
    close(np.stack([host(out.whdr), host(out.equal), host(out.inequal)], axis=1), K.whdr_expected(ref64), np.nan_to_num(e), 1e-5, what + " ratios")
    assert out.sums.dtype == torch.float64 and out.whdr.dtype == torch.float32


@pytest.mark.parametrize("name", WHDR_CASES)
def test_whdr_fixtures_bytes_and_fp32(sgr, name):
    z = fixture("whdr", name)
    a = (z["point"], z["weight"], z["label"], z["num"])
    out = run_whdr(sgr, z["im_u8"], *a)
    check_whdr(out, z["im_u8"], *a, f"whdr {name}", z["ref64_ratios"], z["e_ratios"])
    close(host(out.sums), z["sums64"], 0.0, 1e-12, f"whdr {name} sums (fixture)")
    f32 = K.reflectance_of(z["im_u8"], np.float32).transpose(0, 3, 1, 2)      # the same image as fp32 [B,3,H,W]
    assert bits(run_whdr(sgr, f32, *a)) == bits(out)
    assert bits(run_whdr(sgr, z["im_u8"], a[0].astype(np.int64), a[1], a[2].astype(np.uint8 if name == "floor" else np.int64), a[3].astype(np.int64))) == bits(out)
    if name == "mix":
        assert np.isnan(host(out.whdr)[1]) and host(out.equal)[1] == 0 and host(out.inequal)[1] == 0 and not host(out.sums)[1].any()      # num == 0


@pytest.mark.parametrize("i", range(5), ids=[s[0] for s in K.GPU_WHDR_SHAPES[:5]])
def test_whdr_sizes_around_the_workgroup(sgr, i):
    im, *a = K.gpu_whdr_set(i)
    out = run_whdr(sgr, im, *a)
    check_whdr(out, im, *a, "whdr " + K.GPU_WHDR_SHAPES[i][0])
    assert bits(run_whdr(sgr, im, *a)) == bits(out)      # two runs
    one = run_whdr(sgr, im[1:], *(v[1:] for v in a))      # an image against its batch
    assert bits(one) == [host(t[1:]).tobytes() for t in out]


def test_whdr_guard_bands_strides_ranking_and_export_chain(sgr):
    im, point, weight, label, num = K.gpu_whdr_set(2)
    B, H, W, _ = im.shape
    want = run_whdr(sgr, im, point, weight, label, num)
    # the image inside guard bands of NaN: out-of-image and garbage entries never reach them
    f32 = K.reflectance_of(im, np.float32).transpose(0, 3, 1, 2)
    big = torch.full((B + 2, 5, H + 4, W + 6), float("nan"), device="cuda")
    big[1:-1, 1:4, 2:-2, 3:-3] = dev(f32)
    p2, w2 = point.copy(), weight.copy()
    p2[:, :8] = [[-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, H, 0], [0, 0, 0, W], [H, W, H, W], [-2 ** 31, 0, 0, 2 ** 31 - 1], [0, 0, -1, -1], [H - 1, W - 1, H, W - 1]]
    ref = K.whdr(K.reflectance_of(im, np.float64), p2, w2, label, num)
    out = sgr.whdr(big[1:-1, 1:4, 2:-2, 3:-3], dev(p2), dev(w2), dev(label), dev(num))
    close(host(out.sums), ref["sums"], 0.0, 1e-12, "whdr guard bands sums")
    assert (ref["cls"][:, :8] == -1).all()
    # channels-last and sliced inputs: the same bits as the contiguous call
    cl = dev(f32).contiguous(memory_format=torch.channels_last)
    assert bits(sgr.whdr(cl, dev(point), dev(weight), dev(label), dev(num))) == bits(want)
    assert bits(sgr.whdr(big[1:-1, 1:4, 2:-2, 3:-3], dev(point), dev(weight), dev(label), dev(num))) == bits(want)
    wide = torch.zeros(B, H, W + 3, 3, dtype=torch.uint8, device="cuda")
    wide[:, :, :W] = dev(im)
    assert bits(sgr.whdr(wide[:, :, :W], dev(point)[:, :, :], dev(weight), dev(label), dev(num))) == bits(want)
    # the ranking loss's arrays
    from inverserenderingofindoorscene_amd import eval_metrics as EM
    rng = np.random.default_rng(5)
    eq = (dev(point[:, :100]), dev(np.abs(weight[:, :100])), dev(np.array([100, 40], np.int32)))
    dk = (dev(point[:, 100:250].astype(np.int64)), dev(np.nan_to_num(weight[:, 100:250], nan=1.0)), dev(np.array([150, 0], np.int64)))
    got = sgr.whdr_from_ranking(dev(im), *eq, *dk)
    mapped = EM.ranking_to_whdr(*eq, *dk)
    assert bits(got) == bits(sgr.whdr(dev(im), *mapped)) and host(mapped[2]).tolist() == [[0] * 100 + [2] * 150] * 2
    check_whdr(got, im, *(host(t) for t in mapped), "whdr_from_ranking")
    # the chain from export_image
    albedo = torch.rand(2, 3, 9, 11, generator=torch.Generator().manual_seed(7)).cuda()
    png = sgr.export_image(albedo, "albedo")
    assert png.dtype == torch.uint8 and tuple(png.shape) == (2, 9, 11, 3)
    pt = np.stack([rng.integers(0, 9, (2, 50)), rng.integers(0, 11, (2, 50)), rng.integers(0, 9, (2, 50)), rng.integers(0, 11, (2, 50))], axis=2).astype(np.int32)
    args = (pt, np.ones((2, 50), np.float32), rng.integers(0, 3, (2, 50)).astype(np.int32), np.array([50, 50], np.int32))
    assert K.whdr_margin_violations(host(png), *args) == 0      # the bytes come from the device: the margin condition is checked here
    check_whdr(sgr.whdr(png, *(dev(v) for v in args)), host(png), *args, "whdr of export_image")


# ---- normal angle ---------------------------------------------------------------------------------------------------------------------------

def run_normal(sgr, pred, gt, mask):
    return sgr.normal_angle_error(dev(pred), dev(gt), dev(mask), return_map=True)


def check_normal(out, pred, gt, mask, what, ref=None):
    """ref: the fixture (the reference's runs); otherwise the checker's fp32 and fp64 evaluations"""
    c64 = K.normal_angle(pred, gt, mask, np.float64)
    if ref is None:
        c32 = K.normal_angle(pred, gt, mask, np.float32)
        ref = dict(ref64_theta=c64["theta"], ref64_mean=c64["mean"], count=c64["count"], e_theta=K.rel_l2(c32["theta"], c64["theta"]), e_mean=np.abs(c32["mean"] - c64["mean"]))
    theta, m = host(out.theta), c64["mask"]
    assert np.array_equal(host(out.count), ref["count"]) and out.count.dtype == torch.int32
    e, bound = K.rel_l2(theta, ref["ref64_theta"]), max(2 * float(ref["e_theta"]), 1e-6)
    print(f"{what}: theta rel-L2 {e:.3e}, bound {bound:.3e}")
    assert e <= bound
    close(host(out.mean), ref["ref64_mean"], ref["e_mean"], 1e-5, what + " mean")
    for b in range(theta.shape[0]):      # the select alone: numpy's median of the kernel's own angles
        v = theta[b][m[b]]
        want = np.median(v) if v.size else np.float32(np.nan)
        got = host(out.median)[b]
        assert (np.isnan(want) and np.isnan(got)) or got == want, (what, b, got, want)


@pytest.mark.parametrize("name", NORMAL_CASES)
def test_normal_fixtures(sgr, name):
    z = fixture("normal", name)
    out = run_normal(sgr, z["pred"], z["gt_u8"], z["mask_u8"])
    check_normal(out, z["pred"], z["gt_u8"], z["mask_u8"], f"normal {name}", z)
    one = sgr.normal_angle_error(dev(z["pred"]), dev(z["gt_u8"]), dev(z["mask_u8"].min(axis=3)))      # the one-channel mask
    assert one._fields == ("mean", "median", "count") and bits(one) == bits(out[:3])
    if name == "none":
        assert np.isnan(host(out.mean)).all() and np.isnan(host(out.median)).all() and host(out.count).tolist() == [0]
    if name == "ties":
        assert (host(out.theta)[1] == 0).all() and host(out.median)[1] == 0


@pytest.mark.parametrize("i", range(4), ids=[s[0] for s in K.GPU_MAP_SHAPES[:4]])
def test_normal_shapes_beyond_the_fixtures(sgr, i):
    pred, gt, mask = K.gpu_normal_set(i)
    if K.GPU_MAP_SHAPES[i][0] == "one":
        mask[:] = 255
    out = run_normal(sgr, pred, gt, mask)
    check_normal(out, pred, gt, mask, "normal " + K.GPU_MAP_SHAPES[i][0])
    assert bits(run_normal(sgr, pred, gt, mask)) == bits(out)      # two runs
    b = pred.shape[0] - 1      # an image against its batch
    assert bits(run_normal(sgr, pred[b:], gt[b:], mask[b:])) == [host(t[b:]).tobytes() for t in out]
    # channels-last and sliced inputs
    p = dev(pred)
    big = torch.full((p.shape[0], 5, p.shape[2] + 2, p.shape[3] + 3), float("nan"), device="cuda")
    big[:, 1:4, 1:-1, 2:-1] = p
    assert bits(sgr.normal_angle_error(big[:, 1:4, 1:-1, 2:-1], dev(gt), dev(mask), return_map=True)) == bits(out)
    assert bits(sgr.normal_angle_error(p.contiguous(memory_format=torch.channels_last), dev(gt)[:, :, :], dev(mask), return_map=True)) == bits(out)


def test_normal_select_edges(sgr):
    """all-equal angles; counts n and n + 1 around a digit boundary of the select (256 and 257 counted pixels, 65536 and 65537 keys below and
    above); a NaN prediction"""
    H, W = 20, 20
    gt = np.full((1, H, W, 3), 128, np.uint8)
    gt[..., 2] = 255
    pred = np.zeros((1, 3, H, W), np.float32)
    pred[0, 0] = 1.0
    for n in (255, 256, 257, 399, 400):
        mask = np.zeros((1, H, W), np.uint8)
        mask.reshape(-1)[:n] = 255
        out = run_normal(sgr, pred, gt, mask)
        check_normal(out, pred, gt, mask, f"normal all-equal n={n}")
        assert len(np.unique(host(out.theta))) == 1 and host(out.count).tolist() == [n]
    rng = np.random.default_rng(9)
    H, W = 258, 256
    pred, gt, _ = K.draw_normal(1, 129, 128, H, W, 41)
    for n in (65535, 65536, 65537):
        mask = np.zeros((1, H, W), np.uint8)
        mask.reshape(-1)[rng.permutation(H * W)[:n]] = 255
        check_normal(run_normal(sgr, pred, gt, mask), pred, gt, mask, f"normal n={n}")
    pred, gt, mask = K.gpu_normal_set(1)
    pred[0, 1, 2, 3] = np.nan
    out = run_normal(sgr, pred, gt, mask)
    assert np.isnan(host(out.mean)[0]) and np.isnan(host(out.median)[0]) and not np.isnan(host(out.mean)[1]) and not np.isnan(host(out.median)[1])


# ---- log-depth RMSE -------------------------------------------------------------------------------------------------------------------------

def check_depth(out, pred, gt, what, ref=None):
    c64 = K.depth_log_rmse(pred, gt, np.float64)
    if ref is None:
        ref = dict(ref64_rmse=c64["rmse"], count=c64["count"], e_rmse=np.abs(K.depth_log_rmse(pred, gt, np.float32)["rmse"] - c64["rmse"]))
    assert np.array_equal(host(out.count), ref["count"]) and out.count.dtype == torch.int32 and out.rmse.dtype == torch.float32
    close(host(out.rmse), ref["ref64_rmse"], ref["e_rmse"], 1e-5, what + " rmse")


@pytest.mark.parametrize("name", DEPTH_CASES)
def test_depth_fixtures(sgr, name):
    z = fixture("depth", name)
    out = sgr.depth_log_rmse(dev(z["pred"]), dev(z["gt"]))
    check_depth(out, z["pred"], z["gt"], f"depth {name}", z)
    assert bits(sgr.depth_log_rmse(dev(z["pred"])[:, None], dev(z["gt"])[:, None])) == bits(out)      # [B,1,h,w] and [B,1,H,W]
    if name == "none":
        assert np.isnan(host(out.rmse)).all() and host(out.count).tolist() == [0]
    if name == "edge":      # ground truth exactly 1 and 10 is excluded
        assert (z["gt"] == 1).sum() == 5 and (z["gt"] == 10).sum() == 5 and int(host(out.count)[0]) == int(((z["gt"] > 1) & (z["gt"] < 10)).sum())


@pytest.mark.parametrize("i", range(4), ids=[s[0] for s in K.GPU_MAP_SHAPES[:4]])
def test_depth_shapes_beyond_the_fixtures(sgr, i):
    pred, gt = K.gpu_depth_set(i)
    out = sgr.depth_log_rmse(dev(pred), dev(gt))
    check_depth(out, pred, gt, "depth " + K.GPU_MAP_SHAPES[i][0])
    assert bits(sgr.depth_log_rmse(dev(pred), dev(gt))) == bits(out)      # two runs
    b = pred.shape[0] - 1      # an image against its batch
    assert bits(sgr.depth_log_rmse(dev(pred[b:]), dev(gt[b:]))) == [host(t[b:]).tobytes() for t in out]
    # sliced inputs, off every 16-byte boundary
    bp = torch.full((pred.shape[0], pred.shape[1] + 2, pred.shape[2] + 3), float("nan"), device="cuda")
    bg = torch.full((gt.shape[0], 2, gt.shape[1] + 1, gt.shape[2] + 5), float("nan"), device="cuda")
    bp[:, 1:-1, 1:-2] = dev(pred)
    bg[:, 1, 1:, 3:-2] = dev(gt)
    assert bits(sgr.depth_log_rmse(bp[:, 1:-1, 1:-2], bg[:, 1:2, 1:, 3:-2])) == bits(out)


# ---- all three ------------------------------------------------------------------------------------------------------------------------------

def test_replayed_hip_graph(sgr):
    im, point, weight, label, num = (dev(v) for v in K.gpu_whdr_set(3))
    pred, gt, mask = (dev(v) for v in K.gpu_normal_set(3))
    dpred, dgt = (dev(v) for v in K.gpu_depth_set(3))

    def step():
        return tuple(sgr.whdr(im, point, weight, label, num)) + tuple(sgr.normal_angle_error(pred, gt, mask, return_map=True)) + tuple(sgr.depth_log_rmse(dpred, dgt))
    want = bits(step())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):      # torch's capture recipe: first uses (allocator growth) on a side stream
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert bits(out) == want
    # new values in the captured inputs
    pred.copy_(pred.flip(0))
    dpred.mul_(1.5)
    want = bits(step())
    g.replay()
    torch.cuda.synchronize()
    assert bits(out) == want


def test_bf16_inside_autocast_equals_the_upcast_fp32_call(sgr):
    im, point, weight, label, num = K.gpu_whdr_set(1)
    a = (dev(point), dev(weight), dev(label), dev(num))
    r16 = dev(K.reflectance_of(im, np.float32).transpose(0, 3, 1, 2)).bfloat16()
    pred, gt, mask = K.gpu_normal_set(3)
    dpred, dgt = K.gpu_depth_set(3)
    p16, d16, g16 = dev(pred).bfloat16(), dev(dpred).bfloat16(), dev(dgt).bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = (sgr.whdr(r16, *a), sgr.normal_angle_error(p16, dev(gt), dev(mask), return_map=True), sgr.depth_log_rmse(d16, g16), sgr.whdr(dev(im), *a))
    want = (sgr.whdr(r16.float(), *a), sgr.normal_angle_error(p16.float(), dev(gt), dev(mask), return_map=True), sgr.depth_log_rmse(d16.float(), g16.float()), sgr.whdr(dev(im), *a))
    for g, w in zip(got, want):
        assert bits(g) == bits(w) and [t.dtype for t in g] == [t.dtype for t in w]
    with pytest.raises(RuntimeError, match="must be fp32"):
        sgr.depth_log_rmse(d16, g16)


def test_full_size_against_the_fp64_checker(sgr):
    """480 x 640, batch 2: NYU's normals and depth from 240 x 320, an IIW-sized albedo with 800 + 800 judgements"""
    i = len(K.GPU_MAP_SHAPES) - 1
    pred, gt, mask = K.gpu_normal_set(i)
    check_normal(run_normal(sgr, pred, gt, mask), pred, gt, mask, "normal full")
    dpred, dgt = K.gpu_depth_set(i)
    check_depth(sgr.depth_log_rmse(dev(dpred), dev(dgt)), dpred, dgt, "depth full")
    im, *a = K.gpu_whdr_set(len(K.GPU_WHDR_SHAPES) - 1)
    check_whdr(run_whdr(sgr, im, *a), im, *a, "whdr full")
