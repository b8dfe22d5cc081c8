"""GPU: sgr.light_final_conv (csrc/sgr_light_final_conv.hip behind torch.ops.sgrender.light_final_conv) against the fixtures the UNMODIFIED
reference produced (tests/golden/g21_lightconv_*.npz, tools/make_golden_light_final_conv.py) and against tests/light_final_conv_checker.py,
which tests/test_light_final_conv.py pins to those fixtures at 1e-12.

Bounds: the project's rule.  Values against fp64 in rel-L2: ``max(2 e_ref, 1e-6)``; gradients: ``max(4 e_ref, 1e-6)``.  ``e_ref`` is the
reference's own fp32-vs-fp64 distance: stored in the fixture, or -- where no fixture fits -- the distance of torch's own composition
(``F.pad(mode='replicate')`` + ``F.conv2d`` under autograd) in fp32 on the same inputs from the fp64 checker.

The lane-map cases use integer data small enough that every fp32 sum is exact, so the comparison is ``==``: a transposed accumulator write or
a permuted k index passes none of them."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import light_final_conv_checker as C
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

FIXTURES = ["ax", "lam", "one", "row", "col", "two", "k1m0", "k1m1", "k5", "plain"]
GRADS = ("dy", "dW", "db")


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


def value_bound(e_ref):
    return max(2.0 * float(e_ref), 1e-6)


def grad_bound(e_ref):
    return max(4.0 * float(e_ref), 1e-6)


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


def load(name):
    """-> ((y, Wt, bias, ct) on the device, the fixture)"""
    z = np.load(os.path.join(GOLDEN_DIR, f"g21_lightconv_{name}.npz"))
    return tuple(torch.from_numpy(z[k]).cuda() for k in ("y", "Wt", "bias", "ct")), z


def run(sgr, y, Wt, bias, ct, need=(True, True, True)):
    """-> (out, [dy, dW, db]), None where not required"""
    leaves = [t.detach().requires_grad_(n) for t, n in zip((y, Wt, bias), need)]
    out = sgr.light_final_conv(*leaves)
    live = [t for t in leaves if t.requires_grad]
    gs = list(torch.autograd.grad(out, live, grad_outputs=ct)) if live else []
    return out.detach(), [gs.pop(0) if t.requires_grad else None for t in leaves]


def draw(B, Cc, O, H, W, seed, device="cuda"):
    """a signed N(0,1) map, convolution weights N(0, 1/(9 C)), an N(0,1) cotangent"""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, Cc, H, W, generator=g)
    Wt = torch.randn(O, Cc, 3, 3, generator=g) / (9.0 * Cc) ** 0.5
    bias = 0.1 * torch.randn(O, generator=g)
    ct = torch.randn(B, O, H, W, generator=g)
    return tuple(t.to(device) for t in (y, Wt, bias, ct))


def check_against(tag, out, gs, out64, g64, e_out, e_g):
    assert out.is_contiguous() and torch.isfinite(out).all()
    e, lim = err(out, out64), value_bound(e_out)
    print(f"{tag}: values {e:.2e} (bound {lim:.1e}, e_ref {float(e_out):.1e})")
    assert e <= lim, (tag, "values", e, lim)
    for k, g, gr, eg in zip(GRADS, gs, g64, e_g):
        e, lim = err(g, gr), grad_bound(eg)
        print(f"{tag}: {k} {e:.2e} (bound {lim:.1e}, e_ref {float(eg):.1e})")
        assert g.is_contiguous() and torch.isfinite(g).all() and e <= lim, (tag, k, e, lim)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def raw_abi(y, Wt, bias, ct, wants=(True, True, True)):
    """sgr_light_final_conv_fwd / _bwd alone, outputs pre-filled with NaN -> (out, [dy, dW, db] or None)"""
    from inverserenderingofindoorscene_amd import _lib
    lib = _lib.load()
    B, Cc, H, W = y.shape
    O = Wt.shape[0]
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ys = (ctypes.c_longlong * 4)(*y.stride())
    out, ws = f(B, O, H, W), f(lib.sgr_light_final_conv_workspace_floats(B, Cc, O, H, W))
    _lib.call("sgr_light_final_conv_fwd", _ptr(y), _ptr(Wt), _ptr(bias), _ptr(out), B, Cc, O, H, W, ys, stream)
    dy, dW, db = (f(B, Cc, H, W) if wants[0] else None), (f(O, Cc, 3, 3) if wants[1] else None), (f(O) if wants[2] else None)
    _lib.call("sgr_light_final_conv_bwd", _ptr(ct), _ptr(y), _ptr(Wt), _ptr(dy), _ptr(dW), _ptr(db), _ptr(ws), B, Cc, O, H, W, ys, stream)
    torch.cuda.synchronize()
    return out, [dy, dW, db]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_the_operator_and_the_raw_c_abi(sgr, name):
    """values and every gradient against the reference's fp64 run; the C ABI alone gives the operator's bits; the module form too"""
    args, z = load(name)
    refs = (z["out64"], [z[f"{k}64"] for k in GRADS], z["e_ref_out"], [z[f"e_ref_{k}"] for k in GRADS])
    out, gs = run(sgr, *args)
    check_against(name, out, gs, *refs)
    raw_out, raw_gs = raw_abi(*args)
    check_against(name + " C ABI", raw_out, raw_gs, *refs)
    assert torch.equal(raw_out, out) and all(torch.equal(p, q) for p, q in zip(raw_gs, gs))
    y, Wt, bias, ct = args
    conv = sgr.LightFinalConv(in_channels=y.shape[1], out_channels=Wt.shape[0]).cuda()
    conv.load_state_dict({"weight": Wt, "bias": bias})
    with torch.no_grad():
        assert torch.equal(conv(y), out)


def test_a_null_gradient_is_not_written_and_changes_nothing_else(sgr):
    args, _ = load("lam")
    _, full = raw_abi(*args)
    for wants in ((True, False, False), (False, False, True), (False, True, False), (True, False, True)):
        _, gs = raw_abi(*args, wants=wants)
        for got, ref, w in zip(gs, full, wants):
            assert (got is None) if not w else torch.equal(got, ref), wants


def test_ax_composed_with_light_heads_gives_the_decoders_return(sgr):
    (y, Wt, bias, _), z = load("ax")
    B, _, H, W = y.shape
    with torch.no_grad():
        x_orig = sgr.light_final_conv(y, Wt, bias)
        axis = sgr.light_heads(x_orig, torch.zeros(B, 12, H, W, device="cuda"), torch.zeros(B, 36, H, W, device="cuda"))[0]
    e, lim = err(axis, z["ret64"]), value_bound(z["e_ref_ret"])
    print(f"ax + light_heads: {e:.2e} (bound {lim:.1e}, e_ref {float(z['e_ref_ret']):.1e})")
    assert tuple(axis.shape) == (B, 12, 3, H, W) and e <= lim, (e, lim)


# ---- lane maps, exact ------------------------------------------------------------------------------------------------------------------
# (B, C, H, W, O, o, c, tap): every N tile with its first and last column (o = 0, 15 | 16, 31 | 32, 35), every tap, channels in the chunks
# 0 .. 3 of 8, on both shapes and both output counts
A, Bs = (2, 32, 5, 7), (1, 16, 9, 13)
ONE_HOT = ([A + (36, o, c, t) for t, (o, c) in enumerate([(0, 0), (15, 9), (16, 17), (31, 31), (32, 8), (35, 15), (7, 16), (20, 24), (33, 5)])] +
           [Bs + (17, o, c, t) for t, (o, c) in enumerate([(0, 0), (15, 7), (16, 8), (1, 15), (14, 3), (16, 12), (8, 9), (15, 1), (0, 14)])] +
           [A + (17, 16, 23, 4), A + (17, 15, 30, 8), Bs + (36, 35, 15, 0), Bs + (36, 32, 8, 6), Bs + (36, 31, 0, 2)])


@pytest.mark.parametrize("case", ONE_HOT, ids=lambda c: "x".join(map(str, c[:4])) + f"-O{c[4]}-o{c[5]}c{c[6]}t{c[7]}")
def test_lane_maps_with_a_one_hot_weight_are_exact(sgr, case):
    B, Cc, H, W, O, o, c, tap = case
    kh, kw = divmod(tap, 3)
    y = torch.arange(B * Cc * H * W, dtype=torch.float32, device="cuda").reshape(B, Cc, H, W) - 1000.0      # distinct small integers
    Wt = torch.zeros(O, Cc, 3, 3, device="cuda")
    Wt[o, c, kh, kw] = 1.0
    bias = torch.arange(O, dtype=torch.float32, device="cuda") * 3.0 - 7.0
    g = torch.Generator().manual_seed(2300 + tap)
    ct = torch.randint(-3, 4, (B, O, H, W), generator=g).float().cuda()
    out, (dy, dW, db) = run(sgr, y, Wt, bias, ct)
    want = bias.view(1, O, 1, 1).expand(B, O, H, W).clone()
    want[:, o] += C._shifted(y[:, c], kh, kw)      # the clamped shift of plane c; every other plane is its bias
    assert torch.equal(out, want), (out - want).abs().max()
    _, (dy64, dW64, db64) = C.light_final_conv(y.double(), Wt.double(), bias.double(), cotangent=ct.double())
    assert torch.equal(dy.double(), dy64) and int((dy64[:, c] != 0).sum()) > 0 and int((dy64 != 0).sum()) == int((dy64[:, c] != 0).sum())
    assert torch.equal(dW.double(), dW64)      # integer g and y: every fp32 partial sum is exact
    assert torch.equal(db.double(), db64)


@pytest.mark.parametrize("shape", [A + (36,), Bs + (17,)], ids=lambda s: "x".join(map(str, s)))
def test_integer_data_equal_the_checker_exactly(sgr, shape):
    """dense integer weights: all N tiles, taps and chunks at once, forward and all three gradients"""
    B, Cc, H, W, O = shape
    g = torch.Generator().manual_seed(2320 + O)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g).float().cuda()
    y, Wt, bias, ct = ri(-9, 10, B, Cc, H, W), ri(-3, 4, O, Cc, 3, 3), ri(-5, 6, O), ri(-3, 4, B, O, H, W)
    out, gs = run(sgr, y, Wt, bias, ct)
    o64, g64 = C.light_final_conv(y.double(), Wt.double(), bias.double(), cotangent=ct.double())
    assert torch.equal(out.double(), o64)
    for k, p, q in zip(GRADS, gs, g64):
        assert torch.equal(p.double(), q), k


# ---- shapes no fixture covers ------------------------------------------------------------------------------------------------------------
def against_the_checker(sgr, tag, args):
    y, Wt, bias, ct = args
    d = lambda t: t.double()
    out, gs = run(sgr, *args)
    o64, g64 = C.light_final_conv(d(y), d(Wt), d(bias), cotangent=d(ct))
    o32, g32 = C.composition(y, Wt, bias, cotangent=ct)      # what eager executes, in fp32
    check_against(tag, out, gs, o64, g64, err(o32, o64), [err(a, c) for a, c in zip(g32, g64)])


# 9 x 13 inside one tile: the channel counts 16, 32, 256 (two passes of the data gradient) with 1, 2 and 3 N tiles, full and ragged;
# 30 x 41 and 37 x 70: several 32 x 8 / 32 x 4 tiles per axis, ragged both ways; 120 x 160: the training plane
SHAPES = [(3, 16, 1, 9, 13), (3, 16, 17, 9, 13), (3, 32, 12, 9, 13), (3, 32, 48, 9, 13), (3, 256, 16, 9, 13), (3, 256, 36, 9, 13),
          (1, 128, 36, 30, 41), (2, 16, 36, 37, 70), (2, 128, 36, 120, 160)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_no_fixture_covers_against_the_checker(sgr, shape):
    against_the_checker(sgr, "x".join(map(str, shape)), draw(*shape, seed=2340 + shape[1] + shape[2] + shape[3]))


# ---- bit-exact comparisons ---------------------------------------------------------------------------------------------------------------
# (5, 7) / (6, 12): element-wise and 128-bit paths of one tile; (37, 70): several tiles per axis, odd sizes; (12, 132): 128-bit stores over
# five tiles per row
@pytest.mark.parametrize("shape", [(3, 16, 17, 5, 7), (3, 16, 12, 6, 12), (3, 32, 36, 37, 70), (3, 16, 36, 12, 132)], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bit_identical_and_an_image_does_not_depend_on_its_batch(sgr, shape):
    y, Wt, bias, ct = draw(*shape, seed=2360 + shape[4])
    o1, g1 = run(sgr, y, Wt, bias, ct)
    o2, g2 = run(sgr, y, Wt, bias, ct)
    assert torch.equal(o1, o2) and all(torch.equal(p, q) for p, q in zip(g1, g2))
    for i in range(3):
        ob, gb = run(sgr, y[i:i + 1], Wt, bias, ct[i:i + 1])
        assert torch.equal(ob, o1[i:i + 1]), i
        assert torch.equal(gb[0], g1[0][i:i + 1]), i


@pytest.mark.parametrize("name", ["ax", "lam", "row", "col", "plain"])
def test_channels_last_and_sliced_inputs_give_the_same_bits(sgr, name):
    (y, Wt, bias, ct), _ = load(name)
    oa, ga = run(sgr, y, Wt, bias, ct)

    def sliced(t):      # a view into a larger buffer: one float off every 16-byte boundary, padded rows, planes and images
        B, Cc, H, W = t.shape
        buf = torch.zeros(B + 1, Cc + 2, H + 1, W + 4, device="cuda")
        v = buf[1:, 1:Cc + 1, :H, 1:W + 1]
        v.copy_(t)
        assert not v.is_contiguous() and v.data_ptr() % 16 != 0
        return v
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    for tag, f in (("channels_last", cl), ("sliced", sliced)):
        ob, gb = run(sgr, f(y), Wt, bias, ct)
        assert ob.is_contiguous() and torch.equal(oa, ob), tag
        for p, q in zip(ga, gb):
            assert torch.equal(p, q) and p.shape == q.shape and q.is_contiguous(), tag
    # a non-contiguous cotangent and non-contiguous weights
    ob, gb = run(sgr, y, cl(Wt), bias.repeat_interleave(2)[::2], cl(ct))
    assert torch.equal(oa, ob) and all(torch.equal(p, q) for p, q in zip(ga, gb))


@pytest.mark.parametrize("name", ["ax", "k1m1"])
def test_a_subset_of_requires_grad_gives_the_same_numbers(sgr, name):
    args, _ = load(name)
    out, full = run(sgr, *args)
    for need in itertools.product((False, True), repeat=3):
        ok, gk = run(sgr, *args, need=need)
        assert torch.equal(ok, out)
        for j in range(3):
            assert (gk[j] is None) if not need[j] else torch.equal(gk[j], full[j]), (need, j)
    with torch.no_grad():
        y0 = sgr.light_final_conv(*[t.detach().requires_grad_(True) for t in args[:3]])
    assert y0.grad_fn is None and torch.equal(y0, out)


def test_deterministic_mode_runs_and_gives_the_usual_bits(sgr):
    """torch's own replicate pad raises in its backward under this flag; this operator has nothing to refuse"""
    args = draw(2, 32, 36, 11, 37, seed=2380)
    out, gs = run(sgr, *args)
    before = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        out_d, gs_d = run(sgr, *args)
    finally:
        torch.use_deterministic_algorithms(before)
    assert torch.equal(out, out_d) and all(torch.equal(p, q) for p, q in zip(gs, gs_d))


def test_a_captured_step_replays_to_the_same_bits(sgr):
    """forward + backward captured in a HIP graph on a single stream (the recipe of tests/test_gpu_graph.py), replayed after the inputs were
    overwritten in place"""
    shape = (2, 32, 36, 11, 37)
    static = [t.clone() for t in draw(*shape, seed=2390)]

    def step(a):
        leaves = [t.detach().requires_grad_(True) for t in a[:3]]
        out = sgr.light_final_conv(*leaves)
        return [out.detach(), *torch.autograd.grad(out, leaves, grad_outputs=a[3])]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step(static)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(static)
    for seed in (2391, 2392):
        fresh = draw(*shape, seed=seed)
        for dst, src in zip(static, fresh):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = step(list(fresh))
        assert all(torch.equal(p, q) for p, q in zip(got, want)), seed


def test_opcheck(sgr):
    ops = torch.ops.sgrender
    y, Wt, bias, ct = draw(2, 16, 5, 3, 5, seed=2395)
    live = [t.requires_grad_(True) for t in (y, Wt, bias)]
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")      # aot_dispatch compares gradients through a second path
    torch.library.opcheck(ops.light_final_conv, tuple(live), test_utils=tests)
    torch.library.opcheck(ops.light_final_conv, (live[0], live[1].detach(), live[2]), test_utils=tests)
    d = [t.detach() for t in live]
    torch.library.opcheck(ops.light_final_conv_bwd, (ct, d[0], d[1], True, True, True), test_utils=tests)
    torch.library.opcheck(ops.light_final_conv_bwd, (ct, None, d[1], True, False, True), test_utils=tests)
