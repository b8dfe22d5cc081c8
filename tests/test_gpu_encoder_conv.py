"""GPU: sgr.encoder_conv (csrc/sgr_encoder_conv.hip behind torch.ops.sgrender.encoder_conv) against the fixtures the UNMODIFIED reference
produced (tests/golden/g22_encconv_*.npz, tools/make_golden_encoder_conv.py) and against tests/encoder_conv_checker.py, which
tests/test_encoder_conv.py pins to those fixtures at 1e-12.

Bounds: the project's rule.  Values against fp64 in rel-L2: ``max(2 e_ref, 1e-6)``; gradients: ``max(4 e_ref, 1e-6)``.  ``e_ref`` is the
reference's own fp32-vs-fp64 distance: stored in the fixture, or -- where no fixture fits -- the distance of torch's own composition
(``F.pad`` + ``F.conv2d(stride=2)`` under autograd) in fp32 on the same inputs from the fp64 checker.

The lane-map and border cases use integer data small enough that every fp32 sum is exact, so the comparison is ``==``: a transposed
accumulator write, a swapped ``kh`` / ``kw`` or a wrong column parity passes none of them."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import encoder_conv_checker as C
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

# name -> pad
FIXTURES = {"rgb": "replicate", "c17": "replicate", "pre": "replicate", "two": "replicate", "three": "replicate", "row": "replicate", "col": "replicate",
            "zero": "zeros", "zero3": "zeros"}
GRADS = ("dx", "dW", "db")


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
    """-> ((x, Wt, bias, ct) on the device, the fixture)"""
    z = np.load(os.path.join(GOLDEN_DIR, f"g22_encconv_{name}.npz"))
    return tuple(torch.from_numpy(z[k]).cuda() for k in ("x", "Wt", "bias", "ct")), z


def run(sgr, x, Wt, bias, ct, mode, need=(True, True, True)):
    """-> (out, [dx, dW, db]), None where not required"""
    leaves = [t.detach().requires_grad_(n) for t, n in zip((x, Wt, bias), need)]
    out = sgr.encoder_conv(*leaves, padding=mode)
    live = [t for t in leaves if t.requires_grad]
    gs = list(torch.autograd.grad(out, live, grad_outputs=ct)) if live else []
    return out.detach(), [gs.pop(0) if t.requires_grad else None for t in leaves]


def draw(B, Cc, O, H, W, seed, device="cuda"):
    """a signed N(0,1) map, convolution weights N(0, 1/(16 C)), an N(0,1) cotangent"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cc, H, W, generator=g)
    Wt = torch.randn(O, Cc, 4, 4, generator=g) / (16.0 * Cc) ** 0.5
    bias = 0.1 * torch.randn(O, generator=g)
    ct = torch.randn(B, O, H // 2, W // 2, generator=g)
    return tuple(t.to(device) for t in (x, Wt, bias, ct))


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


def raw_abi(x, Wt, bias, ct, mode, wants=(True, True, True)):
    """sgr_encoder_conv_fwd / _bwd alone, outputs pre-filled with NaN -> (out, [dx, dW, db] or None)"""
    from inverserenderingofindoorscene_amd import _lib
    lib = _lib.load()
    B, Cc, H, W = x.shape
    O, pm = Wt.shape[0], C.MODES.index(mode)
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    xs = (ctypes.c_longlong * 4)(*x.stride())
    out, ws = f(B, O, H // 2, W // 2), f(lib.sgr_encoder_conv_workspace_floats(B, Cc, O, H, W))
    _lib.call("sgr_encoder_conv_fwd", _ptr(x), _ptr(Wt), _ptr(bias), _ptr(out), B, Cc, O, H, W, xs, pm, stream)
    dx, dW, db = (f(B, Cc, H, W) if wants[0] else None), (f(O, Cc, 4, 4) if wants[1] else None), (f(O) if wants[2] else None)
    _lib.call("sgr_encoder_conv_bwd", _ptr(ct), _ptr(x), _ptr(Wt), _ptr(dx), _ptr(dW), _ptr(db), _ptr(ws), B, Cc, O, H, W, xs, pm, stream)
    torch.cuda.synchronize()
    return out, [dx, dW, db]


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixture_through_the_operator_the_raw_c_abi_and_the_module(sgr, name):
    """values and every gradient against the reference's fp64 run; the C ABI alone and the module form give the operator's bits"""
    args, z = load(name)
    mode = FIXTURES[name]
    refs = (z["out64"], [z[f"{k}64"] for k in GRADS], z["e_ref_out"], [z[f"e_ref_{k}"] for k in GRADS])
    out, gs = run(sgr, *args, mode)
    check_against(name, out, gs, *refs)
    raw_out, raw_gs = raw_abi(*args, mode)
    check_against(name + " C ABI", raw_out, raw_gs, *refs)
    assert torch.equal(raw_out, out) and all(torch.equal(p, q) for p, q in zip(raw_gs, gs))
    x, Wt, bias, ct = args
    conv = sgr.EncoderConv(x.shape[1], Wt.shape[0], padding=mode).cuda()
    conv.load_state_dict({"weight": Wt, "bias": bias})
    xl = x.detach().requires_grad_(True)
    om = conv(xl)
    gm = torch.autograd.grad(om, [xl, conv.weight, conv.bias], grad_outputs=ct)
    assert torch.equal(om.detach(), out) and all(torch.equal(p, q) for p, q in zip(gm, gs))


def test_a_null_gradient_is_not_written_and_changes_nothing_else(sgr):
    args, _ = load("pre")
    _, full = raw_abi(*args, "replicate")
    for wants in ((True, False, False), (False, False, True), (False, True, False), (True, False, True)):
        _, gs = raw_abi(*args, "replicate", wants=wants)
        for got, ref, w in zip(gs, full, wants):
            assert (got is None) if not w else torch.equal(got, ref), wants


# ---- lane maps, exact ------------------------------------------------------------------------------------------------------------------
# (mode, B, C, H, W, O, o, c, tap): every kh and kw, the first and last column of every N tile of both output passes (o = 0, 15 | 16, 31 |
# .. | 112, 127), the first and last channel of the chunks of 4 (c = 0, 3, 4, 7, 8), on two shapes
_O128 = [0, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 127]
_C9 = [0, 3, 4, 7, 8, 0, 3, 4, 7, 8, 0, 3, 4, 7, 8, 3]
_O32 = [0, 15, 16, 31, 7, 24, 15, 16, 0, 31, 1, 30, 16, 15, 31, 0]
_C17 = [0, 16, 3, 4, 15, 12, 7, 8, 11, 16, 0, 13, 3, 4, 16, 15]
ONE_HOT = ([("replicate", 2, 9, 5, 7, 128, _O128[t], _C9[t], t) for t in range(16)] + [("zeros", 1, 17, 9, 13, 32, _O32[t], _C17[t], t) for t in range(16)] +
           [("zeros", 2, 9, 5, 7, 128, 64, 8, 5), ("replicate", 1, 17, 9, 13, 32, 16, 16, 10), ("replicate", 1, 3, 18, 70, 16, 15, 2, 12)])


@pytest.mark.parametrize("case", ONE_HOT, ids=lambda c: c[0][:3] + "-" + "x".join(map(str, c[1:5])) + f"-O{c[5]}-o{c[6]}c{c[7]}t{c[8]}")
def test_lane_maps_with_a_one_hot_weight_are_exact(sgr, case):
    mode, B, Cc, H, W, O, o, c, tap = case
    kh, kw = divmod(tap, 4)
    x = torch.arange(B * Cc * H * W, dtype=torch.float32, device="cuda").reshape(B, Cc, H, W) - 1000.0      # distinct small integers
    Wt = torch.zeros(O, Cc, 4, 4, device="cuda")
    Wt[o, c, kh, kw] = 1.0
    bias = torch.arange(O, dtype=torch.float32, device="cuda") * 3.0 - 7.0
    g = torch.Generator().manual_seed(2300 + tap)
    ct = torch.randint(-3, 4, (B, O, H // 2, W // 2), generator=g).float().cuda()
    out, (dx, dW, db) = run(sgr, x, Wt, bias, ct, mode)
    want = bias.view(1, O, 1, 1).expand(B, O, H // 2, W // 2).clone()
    want[:, o] += C._shifted(x[:, c], kh, kw, mode)      # the strided shift of plane c under the border rule; every other plane is its bias
    assert torch.equal(out, want), (out - want).abs().max()
    _, (dx64, dW64, db64) = C.encoder_conv(x.double(), Wt.double(), bias.double(), mode, cotangent=ct.double())
    assert torch.equal(dx.double(), dx64) and int((dx64 != 0).sum()) == int((dx64[:, c] != 0).sum())
    assert torch.equal(dW.double(), dW64)      # integer g and x: every fp32 partial sum is exact
    assert torch.equal(db.double(), db64)


# several tiles of every kernel per axis, ragged; two output passes; three channel passes of the data gradient; two strips of the weight gradient
DENSE = [("replicate", 2, 9, 128, 5, 7), ("zeros", 1, 17, 32, 9, 13), ("replicate", 1, 5, 80, 19, 70), ("zeros", 1, 148, 16, 18, 67), ("replicate", 1, 3, 16, 9, 420)]


@pytest.mark.parametrize("shape", DENSE, ids=lambda s: "x".join(map(str, s)))
def test_integer_data_equal_the_checker_exactly(sgr, shape):
    """dense integer weights: all N tiles, taps and chunks at once, forward and all three gradients"""
    mode, B, Cc, O, H, W = shape
    g = torch.Generator().manual_seed(2320 + O)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g).float().cuda()
    x, Wt, bias, ct = ri(-9, 10, B, Cc, H, W), ri(-3, 4, O, Cc, 4, 4), ri(-5, 6, O), ri(-3, 4, B, O, H // 2, W // 2)
    out, gs = run(sgr, x, Wt, bias, ct, mode)
    o64, g64 = C.encoder_conv(x.double(), Wt.double(), bias.double(), mode, cotangent=ct.double())
    assert torch.equal(out.double(), o64)
    for k, p, q in zip(GRADS, gs, g64):
        assert torch.equal(p.double(), q), k


# ---- borders, exact --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("size", [(6, 8), (7, 9), (6, 9), (2, 2), (3, 3)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("where", ["first_row", "last_row", "first_col", "last_col"])
def test_a_map_that_lives_on_one_border_is_exact(sgr, mode, size, where):
    """in zeros mode the pad contributes nothing; in replicate mode the border counts twice exactly where R_n says"""
    H, W = size
    B, Cc, O = 2, 3, 16
    g = torch.Generator().manual_seed(2330 + H + W)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g).float().cuda()
    full = ri(1, 6, B, Cc, H, W)
    x = torch.zeros_like(full)
    sel = dict(first_row=(slice(0, 1), slice(None)), last_row=(slice(H - 1, H), slice(None)), first_col=(slice(None), slice(0, 1)),
               last_col=(slice(None), slice(W - 1, W)))[where]
    x[:, :, sel[0], sel[1]] = full[:, :, sel[0], sel[1]]
    Wt, bias, ct = ri(-3, 4, O, Cc, 4, 4), ri(-5, 6, O), ri(-3, 4, B, O, H // 2, W // 2)
    out, gs = run(sgr, x, Wt, bias, ct, mode)
    o64, g64 = C.encoder_conv(x.double(), Wt.double(), bias.double(), mode, cotangent=ct.double())
    assert torch.equal(out.double(), o64)
    for k, p, q in zip(GRADS, gs, g64):
        assert torch.equal(p.double(), q), k
    # the count itself, with unit weights on a unit border: how many taps of an output next to the border read it
    ones = torch.zeros(1, 1, H, W, device="cuda")
    ones[:, :, sel[0], sel[1]] = 1.0
    cnt = sgr.encoder_conv(ones, torch.ones(16, 1, 4, 4, device="cuda"), torch.zeros(16, device="cuda"), padding=mode)[0, 0]
    n, axis = (H, 0) if where.endswith("row") else (W, 1)
    edge = cnt.select(axis, 0 if where.startswith("first") else n // 2 - 1)      # the outputs nearest the border
    m = W if axis == 0 else H                                                       # the length of the border line
    taps = len([k for i, k in C.pairs(0 if where.startswith("first") else n - 1, n, mode)])
    along = torch.tensor([sum(1 for k in range(4) if C.src(2 * j + k - 1, m, mode) is not None) for j in range(m // 2)], device="cuda").float()
    assert taps == ((2 if where.startswith("first") or n % 2 == 0 else 1) if mode == "replicate" else 1)
    assert torch.equal(edge, taps * along), (edge, taps, along)


# ---- shapes no fixture covers ------------------------------------------------------------------------------------------------------------
def against_the_checker(sgr, tag, mode, args):
    x, Wt, bias, ct = args
    d = lambda t: t.double()
    out, gs = run(sgr, *args, mode)
    o64, g64 = C.encoder_conv(d(x), d(Wt), d(bias), mode, cotangent=d(ct))
    o32, g32 = C.composition(x, Wt, bias, mode, cotangent=ct)      # what eager executes, in fp32
    check_against(tag, out, gs, o64, g64, err(o32, o64), [err(a, c) for a, c in zip(g32, g64)])


# Ho one below, at and one above 4 and 8 (the tile heights of the weight gradient and of the forward; the data gradient's tile is 4 rows of
# ceil(H / 2)), Wo likewise around 16 and 32, each with an even and an odd map
EDGES = [(6, 30), (7, 31), (8, 32), (9, 33), (10, 34), (11, 35), (14, 62), (15, 63), (16, 64), (17, 65), (18, 66), (19, 67)]


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("size", EDGES, ids=lambda s: "x".join(map(str, s)))
def test_tile_edges_against_the_checker(sgr, mode, size):
    H, W = size
    against_the_checker(sgr, f"{mode} 2x5x{H}x{W}", mode, draw(2, 5, 16, H, W, seed=2340 + H))


# every channel count of the issue with every output count; the two largest planes of the file: 64 -> 128 on 120 x 160 (three strips of the
# weight gradient) and 11 -> 32 on 240 x 320
SHAPES = [("replicate", 3, 1, 16, 9, 13), ("zeros", 3, 3, 32, 9, 13), ("replicate", 3, 17, 64, 9, 13), ("zeros", 3, 64, 128, 9, 13), ("replicate", 2, 148, 128, 9, 13),
          ("zeros", 2, 160, 16, 9, 13), ("zeros", 2, 1, 128, 8, 12), ("replicate", 2, 160, 64, 8, 12), ("replicate", 2, 64, 128, 120, 160),
          ("replicate", 1, 11, 32, 240, 320), ("zeros", 1, 32, 64, 37, 70)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_no_fixture_covers_against_the_checker(sgr, shape):
    mode = shape[0]
    against_the_checker(sgr, "x".join(map(str, shape)), mode, draw(*shape[1:], seed=2360 + shape[2] + shape[3] + shape[4]))


# ---- bit-exact comparisons ---------------------------------------------------------------------------------------------------------------
# (5, 7) / (8, 16): element-wise and 128-bit paths of one tile; (37, 70): several tiles per axis, odd sizes; (24, 264): 128-bit stores over
# several tiles per row
@pytest.mark.parametrize("shape", [("replicate", 3, 17, 32, 5, 7), ("zeros", 3, 3, 16, 8, 16), ("replicate", 3, 11, 32, 37, 70), ("zeros", 3, 5, 80, 24, 264),
                                   ("replicate", 3, 5, 16, 24, 264)], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bit_identical_and_an_image_does_not_depend_on_its_batch(sgr, shape):
    mode = shape[0]
    x, Wt, bias, ct = draw(*shape[1:], seed=2380 + shape[3])
    o1, g1 = run(sgr, x, Wt, bias, ct, mode)
    o2, g2 = run(sgr, x, Wt, bias, ct, mode)
    assert torch.equal(o1, o2) and all(torch.equal(p, q) for p, q in zip(g1, g2))
    for i in range(3):
        ob, gb = run(sgr, x[i:i + 1], Wt, bias, ct[i:i + 1], mode)
        assert torch.equal(ob, o1[i:i + 1]), i
        assert torch.equal(gb[0], g1[0][i:i + 1]), i


@pytest.mark.parametrize("name", ["rgb", "c17", "pre", "row", "col", "zero"])
def test_channels_last_and_sliced_inputs_give_the_same_bits(sgr, name):
    (x, Wt, bias, ct), _ = load(name)
    mode = FIXTURES[name]
    oa, ga = run(sgr, x, Wt, bias, ct, mode)

    def sliced(t):      # a view into a larger buffer: one float off every 16-byte boundary, padded rows, planes and images
        B, Cc, H, W = t.shape
        buf = torch.zeros(B + 1, Cc + 2, H + 1, W + 4, device="cuda")
        v = buf[1:, 1:Cc + 1, :H, 1:W + 1]
        v.copy_(t)
        assert not v.is_contiguous() and v.data_ptr() % 16 != 0
        return v
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    for tag, f in (("channels_last", cl), ("sliced", sliced)):
        ob, gb = run(sgr, f(x), Wt, bias, ct, mode)
        assert ob.is_contiguous() and torch.equal(oa, ob), tag
        for p, q in zip(ga, gb):
            assert torch.equal(p, q) and p.shape == q.shape and q.is_contiguous(), tag
    # a non-contiguous cotangent and non-contiguous weights
    ob, gb = run(sgr, x, cl(Wt), bias.repeat_interleave(2)[::2], cl(ct), mode)
    assert torch.equal(oa, ob) and all(torch.equal(p, q) for p, q in zip(ga, gb))


@pytest.mark.parametrize("name", ["c17", "zero"])
def test_a_subset_of_requires_grad_gives_the_same_numbers(sgr, name):
    """dbias among them: its bits do not change when dWt is dropped"""
    args, _ = load(name)
    mode = FIXTURES[name]
    out, full = run(sgr, *args, mode)
    for need in itertools.product((False, True), repeat=3):
        ok, gk = run(sgr, *args, mode, need=need)
        assert torch.equal(ok, out)
        for j in range(3):
            assert (gk[j] is None) if not need[j] else torch.equal(gk[j], full[j]), (need, j)
    with torch.no_grad():
        y0 = sgr.encoder_conv(*[t.detach().requires_grad_(True) for t in args[:3]], padding=mode)
    assert y0.grad_fn is None and torch.equal(y0, out)


@pytest.mark.parametrize("mode", C.MODES)
def test_deterministic_mode_runs_and_gives_the_usual_bits(sgr, mode):
    """torch's own replicate pad raises in its backward under this flag; this operator has nothing to refuse"""
    args = draw(2, 11, 32, 11, 37, seed=2400)
    out, gs = run(sgr, *args, mode)
    before = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        out_d, gs_d = run(sgr, *args, mode)
    finally:
        torch.use_deterministic_algorithms(before)
    assert torch.equal(out, out_d) and all(torch.equal(p, q) for p, q in zip(gs, gs_d))


def test_a_captured_step_replays_to_the_same_bits(sgr):
    """forward + backward captured in a HIP graph on a single stream (the recipe of tests/test_gpu_graph.py), replayed after the inputs were
    overwritten in place"""
    shape = (2, 11, 32, 11, 37)
    static = [t.clone() for t in draw(*shape, seed=2410)]

    def step(a):
        leaves = [t.detach().requires_grad_(True) for t in a[:3]]
        out = sgr.encoder_conv(*leaves)
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
    for seed in (2411, 2412):
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
    x, Wt, bias, ct = draw(2, 3, 16, 5, 7, seed=2420)
    live = [t.requires_grad_(True) for t in (x, Wt, bias)]
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")      # aot_dispatch compares gradients through a second path
    torch.library.opcheck(ops.encoder_conv, (*live, 0), test_utils=tests)
    torch.library.opcheck(ops.encoder_conv, (live[0], live[1].detach(), live[2], 1), test_utils=tests)
    d = [t.detach() for t in live]
    torch.library.opcheck(ops.encoder_conv_bwd, (ct, d[0], d[1], 5, 7, 0, True, True, True), test_utils=tests)
    torch.library.opcheck(ops.encoder_conv_bwd, (ct, None, d[1], 5, 7, 1, True, False, True), test_utils=tests)


def test_the_chain_from_the_step_wrapper_into_the_encoder(sgr):
    """sgr.light_encoder_input -> EncoderConv(11, 32) -> sgr.group_norm_relu against the eager chain on the same input batch"""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(2430)
    r = lambda *s: torch.rand(*s, generator=g).cuda()
    B, h, w = 2, 12, 16
    batch = sgr.light_encoder_input(r(B, 3, h, w), r(B, 3, h, w), r(B, 3, h, w) - 0.5, r(B, 1, h, w), r(B, 1, h, w) + 0.1, size=(24, 32))[0]
    assert tuple(batch.shape) == (B, 11, 24, 32)
    conv = sgr.EncoderConv(11, 32).cuda()
    gn = torch.nn.GroupNorm(2, 32).cuda()
    with torch.no_grad():
        got = sgr.group_norm_relu(conv(batch), gn.weight, gn.bias, 2)

        def eager(dt):
            y = F.conv2d(F.pad(batch.to(dt), (1, 1, 1, 1), mode="replicate"), conv.weight.to(dt), conv.bias.to(dt), stride=2)
            return F.relu(F.group_norm(y, 2, gn.weight.to(dt), gn.bias.to(dt)))
        ref64, ref32 = eager(torch.float64), eager(torch.float32)
    e, lim = err(got, ref64), value_bound(err(ref32, ref64))
    print(f"chain: values {e:.2e} (bound {lim:.1e}, e_ref {err(ref32, ref64):.1e})")
    assert tuple(got.shape) == (B, 32, 12, 16) and e <= lim, (e, lim)
