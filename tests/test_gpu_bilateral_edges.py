"""GPU: the paths of the bilateral solver (csrc/sgr_bilateral.hip) that the fixtures of tests/test_gpu_bilateral.py never take, against
tests/bilateral_checker.py on inputs made on the spot:

* PCG systems that stop in mid-run, at different iterations per (image, channel): the sticky stop flag, the masked updates and the
  early returns between iteration 1 and the last one.  The checker's record of its own stop tests is asserted first -- distinct stop
  iterations, and a stop margin (smallest |ln(|r| / atol)| over all stop tests) that a summation order different at ~1e-13 cannot flip;
* cg_maxiter at its limits (0, 64, 65), C = 2, images of more than 262144 vertices (a second pass of the grid-stride loops), maps of
  one pixel / row / column, pixel counts around the scan chunk (1023 / 1024 / 1025), a batch of very unlike vertex counts;
* the grid's structure itself (nbr, seg, perm), non-contiguous and misaligned inputs, every host-side rejection, the layer's modes 1, 2, 4.

Bounds, everywhere: the inputs keep every scaled colour coordinate >= 1e-9 from an integer (asserted), so pixel->vertex map, nvertices
and nbr are demanded EXACTLY; out, grad_pred, grad_conf: rel-L2 <= 1e-6 per image, absolute 1e-6 where the reference is zero -- the
bound test_gpu_bilateral.py uses for fp64 against fp64 (what is left is the fp32 cast of the result, 6e-8, and summation order).  The
fp64 distance of yhat from the checker's is printed, not asserted."""
import numpy as np
import pytest
import torch

import bilateral_checker as BC
from test_gpu_bilateral import SOLVER_CASES, _synthetic, err, load, nchw, run, sgr  # noqa: F401  (sgr: the module's fixture)

pytestmark = pytest.mark.gpu

LIM = 1e-6
M0 = BC.MODES[0]


def with_cg(params, tol, maxiter):
    return tuple(params[:5]) + (tol, maxiter)


def maps(B, C, H, W, seed, noise=0.0015):
    """_synthetic's images for any size down to one pixel: smooth colour with a darker right half plus a little noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    u, v = x / max(W - 1, 1), y / max(H - 1, 1)
    ims = []
    for _ in range(B):
        ph = rng.random(3) * 3
        im = np.stack([0.45 + 0.25 * np.sin(2.1 * u + 0.7 * v + p) + 0.1 * np.cos(3.3 * v + p) for p in ph], 0)
        im[:, :, W // 2:] *= 0.7
        im += noise * rng.standard_normal(im.shape)
        ims.append(np.clip(im, 0.05, 0.95))
    image = np.stack(ims).astype(np.float32)
    base = image if C == 3 else image[:, :C] if C == 2 else image.mean(1, keepdims=True)
    pred = np.clip(base + 0.05 * rng.standard_normal((B, C, H, W)), 0, 1).astype(np.float32)
    conf = (0.05 + 0.95 * rng.random((B, 1, H, W))).astype(np.float32)
    grad = rng.standard_normal((B, C, H, W)).astype(np.float32)
    return image, pred, conf, grad


def stop_inputs(seed=2):
    """B = 2, C = 3, 40 x 56: channel 0 constant with a zero cotangent (stops at 0; |b| = 0 backward), channel 1 the guide's mean plus
    2e-3 of noise (a small residual at the start: stops early), channel 2 uniform noise (stops late).  The cotangents of channels 1
    and 2 are smooth plus noise (1 +- 0.1, the guide's mean +- 0.05): white noise needs about 30 iterations for cg_tol = 1e-2 on
    this grid, and every system here is to stop before that."""
    image, pred, conf, grad = _synthetic(2, 3, 40, 56, seed)
    rng = np.random.default_rng(1000 + seed)
    plane = image[:, 0].shape
    pred[:, 0] = 0.4
    pred[:, 1] = image.mean(1) + 2e-3 * rng.standard_normal(plane)
    pred[:, 2] = rng.random(plane)
    rng = np.random.default_rng(2000 + seed)
    grad[:, 0] = 0.0
    grad[:, 1] = 1.0 + 0.1 * rng.standard_normal(plane)
    grad[:, 2] = image.mean(1) + 0.05 * rng.standard_normal(plane)
    return image, pred, conf, grad


def bands_inputs(C=2, H=513, W=512, seed=3):
    """four vertical bands of constant colour: with sigma_spatial = 1 every pixel is a vertex with its spatial neighbours"""
    rng = np.random.default_rng(seed)
    colours = np.array([[0.21, 0.43, 0.35], [0.62, 0.33, 0.54], [0.37, 0.71, 0.26], [0.83, 0.58, 0.67]], np.float32)
    image = np.repeat(colours.T[None, :, None, :], W // 4, axis=3).repeat(H, axis=2)          # [1,3,H,W]
    pred = rng.random((1, C, H, W)).astype(np.float32)
    conf = (0.05 + 0.95 * rng.random((1, 1, H, W))).astype(np.float32)
    grad = rng.standard_normal((1, C, H, W)).astype(np.float32)
    return np.ascontiguousarray(image), pred, conf, grad


BANDS_PARAMS = (8.0, 2.0, 1.0, 50.0, 1e-5, 1e-5, 12)
EDGE_SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (31, 33), (32, 32), (25, 41)]
EDGE_CASES = [(H, W, ss, 1 + (2 * i + j) % 3) for i, (H, W) in enumerate(EDGE_SIZES) for j, ss in enumerate((1.0, 7.0))]


def edge_inputs(H, W, ss, C):
    return maps(2, C, H, W, seed=100 * H + W), (M0[0], M0[1], ss) + tuple(M0[3:])


def assert_fair(image, params):
    for b in range(image.shape[0]):
        sc = BC.scaled_colour(np.moveaxis(image[b], 0, -1), params[0], params[1])
        assert np.abs(sc - np.round(sc)).min() >= 1e-9, b


_REF = {}


def reference(key, inputs, params):
    """the checker's result, computed once per case and shared (never modified)"""
    k = (key, tuple(params))
    if k not in _REF:
        assert_fair(inputs[0], params)
        _REF[k] = BC.run_batch(*inputs, params)
    return _REF[k]


def grid_of(image, params):
    return torch.ops.sgrender.bilateral_grid(image, *[float(p) for p in params[:3]])


def check_grid_structure(grid, ref_idx, ref_nv, ref_nbr):
    """map and nvert exactly; nbr equal to the checker's (same column order 2 d + {0: -1, 1: +1}); seg strictly ascending from 0; perm
    strictly ascending inside each segment (the stable sort, which the splat's summation order rests on) and pix2vert[perm[i]] the
    segment's vertex"""
    p2v, perm, seg, nbr, nvert = [t.cpu().numpy() for t in grid[:5]]
    B, N = p2v.shape
    assert np.array_equal(nvert, np.asarray(ref_nv, np.int32))
    assert np.array_equal(p2v, np.asarray(ref_idx).reshape(B, N))
    for b in range(B):
        nv = int(nvert[b])
        assert np.array_equal(nbr[b, :nv], ref_nbr[b]), b
        s = seg[b, :nv].astype(np.int64)
        assert s[0] == 0 and np.all(np.diff(s) > 0) and s[-1] < N, b
        assert np.array_equal(np.sort(perm[b]), np.arange(N)), b
        vert_of_pos = np.repeat(np.arange(nv), np.diff(np.append(s, N)))        # sorted position -> vertex
        assert np.array_equal(p2v[b][perm[b]], vert_of_pos), b
        inside = vert_of_pos[1:] == vert_of_pos[:-1]
        assert np.all(np.diff(perm[b].astype(np.int64))[inside] > 0), b


def compare(sgr, name, inputs, params, ref):
    """grid structure exactly, then out / grad_pred / grad_conf per image against the checker; yhat's distance is printed"""
    image, pred, conf, grad = inputs
    B, C = pred.shape[:2]
    t = [torch.from_numpy(a).cuda() for a in inputs]
    grid = grid_of(t[0], params)
    check_grid_structure(grid, ref["idx"], ref["nvertices"], ref["nbr"])
    print(f"EDGE {name}: nvertices {ref['nvertices'].tolist()} stops fwd {ref['stops_fwd'].tolist()} bwd {ref['stops_bwd'].tolist()} margin {ref['margin']:.3g}")
    _, yhat = torch.ops.sgrender.bilateral_solve_fwd(*grid, t[1], t[2], *[float(p) for p in params[3:6]], int(params[6]))
    got = dict(zip(("out", "grad_pred", "grad_conf"), run(sgr, *t, params)))
    errs = {}
    for b in range(B):                                    # every figure is printed before anything is asserted
        nv = int(ref["nvertices"][b])
        errs[b] = {k: err(got[k][b].cpu().numpy(), ref[k][b]) for k in ("out", "grad_pred", "grad_conf")}
        print(f"EDGE {name}[{b}]: yhat {err(yhat[b, :nv].cpu().numpy(), ref['yhat'][b]):.2e}  " + "  ".join(f"{k} {e:.2e}" for k, e in errs[b].items()))
    for b in range(B):
        for k in ("out", "grad_pred", "grad_conf"):
            g, r = got[k][b].cpu().numpy(), ref[k][b]
            assert np.isfinite(g).all(), (name, b, k)
            assert errs[b][k] <= LIM, (name, b, k, errs[b][k])
            for c in range(r.shape[0]):
                if not r[c].any():                        # a channel the reference leaves at zero: absolute
                    assert np.abs(g[c]).max() <= LIM, (name, b, k, c)
    return got


# ---- a. stops in mid-run ---------------------------------------------------------------------------------------------------------
def test_systems_stop_in_mid_run_at_different_iterations(sgr):
    inputs = stop_inputs()
    params = with_cg(M0, 1e-2, 30)
    ref = reference("stop", inputs, params)
    stops = np.concatenate([ref["stops_fwd"], ref["stops_bwd"]], 1)                 # [B, 2 C]: the 12 solves
    mid = stops[(stops > 0) & (stops < 30)]
    assert stops.size == 12 and len(np.unique(mid)) >= 3, stops
    assert any(len(np.unique(ref[k][b])) > 1 for k in ("stops_fwd", "stops_bwd") for b in range(2)), stops
    assert (stops == 0).any() and (stops == BC.B_ZERO).any(), stops
    assert not (stops == 30).any(), stops                                          # every system has stopped by 30
    assert ref["margin"] >= 1e-3, ref["margin"]
    got = compare(sgr, "stop tol 1e-2 maxiter 30", inputs, params, ref)
    # the flag is sticky: 34 more iterations are no-ops
    t = [torch.from_numpy(a).cuda() for a in inputs]
    for a, b in zip(run(sgr, *t, with_cg(M0, 1e-2, 64)), (got["out"], got["grad_pred"], got["grad_conf"])):
        assert torch.equal(a, b)


# ---- b. iteration limits ---------------------------------------------------------------------------------------------------------
def test_cg_maxiter_64(sgr):
    inputs = stop_inputs()
    params = with_cg(M0, 1e-4, 64)
    ref = reference("stop", inputs, params)
    stops = np.concatenate([ref["stops_fwd"], ref["stops_bwd"]], 1)
    assert stops.max() > 30 and ref["margin"] >= 1e-3, (stops, ref["margin"])      # runs past the other tests' iteration counts
    compare(sgr, "stop tol 1e-4 maxiter 64", inputs, params, ref)


def test_cg_maxiter_0_returns_the_start_vector(sgr):
    inputs = stop_inputs()
    params = with_cg(M0, 1e-5, 0)
    ref = reference("stop", inputs, params)
    assert ref["margin"] == float("inf")                  # no stop test is ever made
    compare(sgr, "maxiter 0", inputs, params, ref)


def test_cg_maxiter_65_is_rejected(sgr):
    t = [torch.from_numpy(a).cuda() for a in maps(1, 1, 6, 9, seed=2)]
    with pytest.raises(RuntimeError, match="cg_maxiter above 64"):
        sgr.bilateral_solve(*t[:3], *M0[:6], 65)
    assert torch.isfinite(sgr.bilateral_solve(*t[:3], *M0[:6], 64)).all()


# ---- c. two channels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 4])
def test_two_channels(sgr, mode):
    inputs = maps(2, 2, 25, 41, seed=21)
    compare(sgr, f"C=2 mode {mode}", inputs, BC.MODES[mode], reference("c2", inputs, BC.MODES[mode]))


# ---- d. more than 262144 vertices in one image: the grid-stride loops make a second pass --------------------------------------------
def test_more_than_262144_vertices_with_neighbours(sgr):
    inputs = bands_inputs()
    ref = reference("bands", inputs, BANDS_PARAMS)
    assert ref["nvertices"][0] == 513 * 512 > 262144
    assert (ref["nbr"][0] >= 0).sum(1).mean() >= 3
    compare(sgr, "513x512 bands", inputs, BANDS_PARAMS, ref)


def test_more_than_262144_vertices_every_pixel_alone(sgr):
    """mode 1 (the normal refinement) on a noisy guide: bandwidths of 0.5 make every pixel its own vertex, none with a neighbour"""
    rng = np.random.default_rng(11)
    H, W = 513, 512
    image = (0.05 + 0.9 * rng.random((1, 3, H, W))).astype(np.float32)
    inputs = (image, rng.random((1, 1, H, W)).astype(np.float32), (0.05 + 0.95 * rng.random((1, 1, H, W))).astype(np.float32),
              rng.standard_normal((1, 1, H, W)).astype(np.float32))
    ref = reference("alone", inputs, BC.MODES[1])
    assert ref["nvertices"][0] > 262144
    compare(sgr, "513x512 mode 1", inputs, BC.MODES[1], ref)


# ---- e. degenerate and chunk-edge maps -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,ss,C", EDGE_CASES)
def test_degenerate_and_chunk_edge_maps(sgr, H, W, ss, C):
    inputs, params = edge_inputs(H, W, ss, C)
    ref = reference(("edge", H, W, C), inputs, params)
    if ss == 1.0:
        assert np.all(ref["nvertices"] == H * W)           # a segment head at every sorted position
    assert ref["margin"] >= 1e-6, ref["margin"]
    compare(sgr, f"{H}x{W} sigma_spatial {ss:g} C={C}", inputs, params, ref)


# ---- f. grid structure, exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOLVER_CASES)
def test_grid_structure_of_the_fixtures(sgr, name):
    z = load(name)
    params = tuple(z["params"])
    nbr = [BC.Grid(z["image"][b], *params[:3]).nbr for b in range(z["image"].shape[0])]
    check_grid_structure(grid_of(nchw(z["image"]), params), z["idx"], z["nvertices"], nbr)
# (the shapes of d and e go through check_grid_structure inside compare)


# ---- g. a batch of unlike images -------------------------------------------------------------------------------------------------
def test_batch_of_unlike_images(sgr):
    B, C, H, W = 3, 3, 24, 40
    params = (M0[0], M0[1], 64.0) + tuple(M0[3:])
    image, pred, conf, grad = maps(B, C, H, W, seed=31)
    rng = np.random.default_rng(32)
    image[0] = np.array([0.31, 0.52, 0.43], np.float32)[:, None, None]              # one colour, one spatial cell: one vertex
    image[2] = (0.05 + 0.9 * rng.random((3, H, W))).astype(np.float32)              # per-pixel noise
    inputs = (image, pred, conf, grad)
    ref = reference("unlike", inputs, params)
    nv = ref["nvertices"]
    assert nv[0] == 1 and nv.max() >= 10 * nv.min() and len(set(nv.tolist())) == 3, nv
    whole = compare(sgr, "unlike batch", inputs, params, ref)
    t = [torch.from_numpy(a).cuda() for a in inputs]
    for i in range(B):
        s = slice(i, i + 1)
        for k, one in zip(("out", "grad_pred", "grad_conf"), run(sgr, *[x[s] for x in t], params)):
            assert torch.equal(whole[k][s], one), (i, k)


# ---- h. layouts ------------------------------------------------------------------------------------------------------------------
def _solve_raw(sgr, image, pred, conf, grad, params):
    """forward and backward on the tensors AS GIVEN (no clone: their strides reach the operators), through the operators and through autograd"""
    grid = grid_of(image, params)
    sp = [float(p) for p in params[3:6]] + [int(params[6])]
    out, yhat = torch.ops.sgrender.bilateral_solve_fwd(*grid, pred, conf, *sp)
    gp, gc = torch.ops.sgrender.bilateral_solve_bwd(*grid, grad, pred, conf, yhat, *sp)
    p, c = pred.detach().requires_grad_(True), conf.detach().requires_grad_(True)
    assert p.stride() == pred.stride() and c.stride() == conf.stride()
    o2 = sgr.bilateral_solve(image, p, c, *params[:6], int(params[6]))
    gp2, gc2 = torch.autograd.grad(o2, [p, c], grad_outputs=grad)
    live = torch.arange(yhat.shape[1], device=yhat.device)[None, :, None] < grid[4][:, None, None]
    return grid[0], out, torch.where(live, yhat, 0.0), gp, gc, o2.detach(), gp2, gc2      # yhat's rows past nvert[b] are never written


def _channels_last(x):
    return x.contiguous(memory_format=torch.channels_last)


def _sliced_off_alignment(x):
    """a view into a larger buffer that starts one float past a 16-byte boundary, rows and planes strided"""
    B, C, H, W = x.shape
    pad = 2 + (-(W + 2)) % 4                              # a row length that is a multiple of 4 puts element [0,0,1,1] at 4 bytes mod 16
    big = torch.zeros(B, C, H + 1, W + pad, device=x.device)
    v = big[:, :, 1:, 1:W + 1]
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and not v.is_contiguous()
    return v


def _contiguous_off_alignment(x):
    """contiguous, so the kernels read it in place, but one float past a 16-byte boundary"""
    buf = torch.zeros(x.numel() + 1, device=x.device)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("layout", ["channels_last", "sliced", "offset", "expanded_conf"])
def test_layouts_give_the_bits_of_the_contiguous_call(sgr, layout):
    B, C, H, W = 2, 3, 25, 41
    image, pred, conf, grad = [torch.from_numpy(a).cuda() for a in maps(B, C, H, W, seed=41)]
    if layout == "expanded_conf":
        conf = conf[:, :, :, :1].expand(B, 1, H, W)
        given = (image, pred, conf, grad)
        assert conf.stride(3) == 0
    else:
        f = dict(channels_last=_channels_last, sliced=_sliced_off_alignment, offset=_contiguous_off_alignment)[layout]
        given = tuple(f(x) for x in (image, pred, conf, grad))
        if layout != "offset":
            assert not given[0].is_contiguous() and not given[1].is_contiguous() and not given[3].is_contiguous()
    want = _solve_raw(sgr, *[x.contiguous().clone() for x in given], M0)
    got = _solve_raw(sgr, *given, M0)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
        assert a.is_contiguous(), i
    assert torch.isfinite(got[1]).all()


# ---- i. rejections: all in host code, before any launch of the rejected operator ------------------------------------------------------
def test_host_side_rejections_leave_the_operators_usable(sgr):
    image, pred, conf, _ = [torch.from_numpy(a).cuda() for a in maps(1, 3, 6, 9, seed=51)]
    p = list(M0)

    def call(image=image, pred=pred, conf=conf, **kw):
        q = dict(zip(("sl", "sc", "ss", "lam", "amin", "tol", "mi"), p), **kw)
        return sgr.bilateral_solve(image, pred, conf, q["sl"], q["sc"], q["ss"], q["lam"], q["amin"], q["tol"], q["mi"])

    good = call()
    torch.cuda.synchronize()
    grid = grid_of(image, M0)
    other = grid_of(torch.cat([image, image], 3), M0)
    bad = [("C in 1..3", lambda: call(pred=torch.cat([pred, pred[:, :1]], 1))),
           ("0.25", lambda: call(sl=0.2)),
           ("0.25", lambda: call(sc=0.2)),
           ("must be positive", lambda: call(ss=0.0)),
           ("must be positive", lambda: call(sl=-8.0)),
           ("bad solver parameter", lambda: call(lam=-1.0)),
           ("bad solver parameter", lambda: call(amin=0.0)),
           ("confidence must be", lambda: call(conf=conf[:, :, :, :-1])),
           ("confidence must be", lambda: call(conf=torch.cat([conf, conf], 1))),
           ("fp32 tensors required", lambda: call(pred=pred.double())),
           ("built for another shape", lambda: torch.ops.sgrender.bilateral_solve_fwd(*other, pred, conf, 200.0, 1e-5, 1e-5, 12))]
    for msg, f in bad:
        with pytest.raises(RuntimeError, match=msg):
            f()
        assert torch.equal(call(), good), msg
    assert torch.equal(torch.ops.sgrender.bilateral_solve_fwd(*grid, pred, conf, 200.0, 1e-5, 1e-5, 12)[0], good)


# ---- j. the layer's other modes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 4])
def test_layer_modes_call_the_solver_with_their_own_table(sgr, mode):
    torch.manual_seed(60 + mode)
    layer = sgr.BilateralLayer(mode=mode).cuda()
    C = 3 if mode == 1 else 1
    assert layer.conv1.in_channels == 3 + C
    image, pred, _, _ = [torch.from_numpy(a).cuda() for a in maps(2, C, 24, 32, seed=61)]
    feature = torch.from_numpy(maps(2, 3, 24, 32, seed=62)[0]).cuda()
    with torch.no_grad():
        out, conf = layer(image, feature, pred)
        guide = layer._scaled(image, feature)[1]
        want = sgr.bilateral_solve(guide, pred, conf, *BC.MODES[mode][:6], int(BC.MODES[mode][6]))
    assert tuple(out.shape) == tuple(pred.shape) and tuple(conf.shape) == (2, 1, 24, 32)
    assert torch.isfinite(out).all() and torch.equal(out, want)
