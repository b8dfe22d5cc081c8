"""GPU: sgr.group_norm_relu_resize / sgr.group_norm_relu_resize_upcat (the resize kernels of csrc/sgr_gn_stage.hip behind
torch.ops.sgrender.gn_resize) against the fixtures the UNMODIFIED reference produced (tests/golden/g19_gnresize_*.npz,
tools/make_golden_gn_resize.py) and against tests/gn_resize_checker.py, which tests/test_gn_resize.py pins to those fixtures and to torch's
own composition at 1e-12.

Bounds: the project's rule for these operators.  Values against fp64 in rel-L2: ``max(2 e_ref, 1e-6)``; gradients: ``max(4 e_ref, 1e-6)``.
``e_ref`` is the reference's own fp32-vs-fp64 distance: stored in the fixture, or -- where no fixture fits -- the checker evaluated in fp32
(``scale`` formed in fp32, as the kernel and torch form it) on the same inputs.  Inputs drawn here keep every ReLU argument 1e-5 away from
zero, as the fixtures do (asserted), so that a 1-ulp difference cannot flip a branch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gn_resize_checker as R
import gn_stage_checker as C
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

PARTS = [("h1", "s"), ("hw", "s"), ("dbl", "s"), ("one", "w"), ("one", "hw"), ("fin", "d0"), ("fin", "dl")]
IDS = [f"{n}-{p}" for n, p in PARTS]
GRADS = ("dx", "dw", "db", "ds")


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


def load(name, part):
    """-> (x, weight, bias, G, size, skip, ct) on the device and the fixture"""
    z = np.load(os.path.join(GOLDEN_DIR, f"g19_gnresize_{name}.npz"))
    dev = lambda k: torch.from_numpy(z[f"{part}_{k}"]).cuda() if f"{part}_{k}" in z.files else None
    return (dev("x"), dev("weight"), dev("bias"), int(z[f"{part}_G"]), tuple(int(v) for v in z[f"{part}_size"]), dev("skip"), dev("ct")), z


def call(sgr, x, w, b, G, size, skip):
    return sgr.group_norm_relu_resize(x, w, b, G, size) if skip is None else sgr.group_norm_relu_resize_upcat(x, w, b, G, skip)


def run(sgr, x, w, b, G, size, skip, ct, need=(True, True, True, True)):
    """-> (out, [dx, dw, db, ds]) with None where not required or absent"""
    leaves = [t.detach().requires_grad_(n) if t is not None else None for t, n in zip((x, w, b, skip), need)]
    xl, wl, bl, sl = leaves
    y = call(sgr, xl, wl, bl, G, size, sl)
    live = [t for t in leaves if t is not None and t.requires_grad]
    gs = list(torch.autograd.grad(y, live, grad_outputs=ct)) if live else []
    return y.detach(), [gs.pop(0) if t is not None and t.requires_grad else None for t in leaves]


def draw(B, Cc, G, H, W, Hs, Ws, Cs, seed, offset=0.0):
    """as tests/test_gpu_gn_stage.py draws: x = offset + N(0,1) with every ReLU argument at least 1e-5 from zero (elements nearer than 1e-4
    are moved by 1e-2 standard deviations, asserted afterwards), scales with negative ones and an exact zero, N(0,1) skip [B,Cs,Hs,Ws] and
    cotangent, on the device"""
    g = torch.Generator().manual_seed(seed)
    x = offset + torch.randn(B, Cc, H, W, generator=g)
    w = torch.randn(Cc, generator=g)
    w[Cc // 3] = 0.0
    b = 0.3 * torch.randn(Cc, generator=g)
    b[b.abs() < 1e-3] = 0.05
    skip = torch.randn(B, Cs, Hs, Ws, generator=g) if Cs else None
    ct = torch.randn(B, Cc + Cs, 2 * Hs, 2 * Ws, generator=g) if Cs else torch.randn(B, Cc, Hs, Ws, generator=g)
    for _ in range(8):
        pre, _, _ = C.pre_relu(x.double(), w.double(), b.double(), G)
        bad = pre.abs() < 1e-4
        if not bool(bad.any()):
            break
        x = torch.where(bad, x + 1e-2, x)
    pre, _, _ = C.pre_relu(x.double(), w.double(), b.double(), G)
    assert float(pre.abs().min()) >= 1e-5
    cu = lambda t: None if t is None else t.cuda()
    return cu(x), cu(w), cu(b), G, (Hs, Ws), cu(skip), cu(ct)


def check_against(tag, y, gs, y64, g64, e_y, e_g):
    assert y.is_contiguous() and torch.isfinite(y).all()
    e, lim = err(y, y64), value_bound(e_y)
    print(f"{tag}: values {e:.2e} (bound {lim:.1e}, e_ref {float(e_y):.1e})")
    assert e <= lim, (tag, "values", e, lim)
    for k, g, gr, eg in zip(GRADS, gs, g64, e_g):
        if gr is None:
            assert g is None, (tag, k)
            continue
        e, lim = err(g, gr), grad_bound(eg)
        print(f"{tag}: {k} {e:.2e} (bound {lim:.1e}, e_ref {float(eg):.1e})")
        assert torch.isfinite(g).all() and e <= lim, (tag, k, e, lim)
    assert torch.equal(gs[0].cpu() == 0, torch.as_tensor(g64[0]).cpu() == 0), (tag, "zero pattern of dx")


def fixture_refs(z, part):
    has = lambda k: f"{part}_{k}" in z.files
    return (z[f"{part}_y64"], [z[f"{part}_{k}64"] if has(f"{k}64") else None for k in GRADS], z[f"{part}_e_ref_y"],
            [z[f"{part}_e_ref_{k}"] if has(f"e_ref_{k}") else None for k in GRADS])


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _strides(t):
    return (ctypes.c_longlong * 4)(*t.stride()) if t is not None else None


def raw_abi(x, w, b, G, size, skip, ct, want=(True, True, True, True)):
    """forward + backward through the C ABI alone -> (out, stats, [dx, dw, db, ds])"""
    from inverserenderingofindoorscene_amd import _lib
    lib = _lib.load()
    B, Cc, H, W = x.shape
    Hs, Ws = size
    Cs = 0 if skip is None else skip.shape[1]
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    out = f(B, Cc + Cs, 2 * Hs, 2 * Ws) if Cs else f(B, Cc, Hs, Ws)
    stats = f(B, G, 4)
    q = lib.sgr_gn_resize_workspace_floats
    ws = f(max(q(B, Cc, G, H, W, Hs, Ws, int(Cs > 0), 0), q(B, Cc, G, H, W, Hs, Ws, int(Cs > 0), 1)))
    _lib.call("sgr_gn_resize_fwd", _ptr(x), _ptr(w), _ptr(b), _ptr(skip), _ptr(out), _ptr(stats), _ptr(ws), B, Cc, G, Cs, H, W, Hs, Ws, _strides(x), _strides(skip),
              ctypes.c_float(1e-5), _stream())
    gs = [f(B, Cc, H, W) if want[0] else None, f(Cc) if want[1] else None, f(Cc) if want[2] else None, f(B, Cs, Hs, Ws) if Cs and want[3] else None]
    _lib.call("sgr_gn_resize_bwd", _ptr(ct), _ptr(x), _ptr(w), _ptr(b), _ptr(stats), *[_ptr(g) for g in gs], _ptr(ws), B, Cc, G, Cs, H, W, Hs, Ws, _strides(x),
              _stream())
    torch.cuda.synchronize()
    return out, stats, gs


@pytest.mark.parametrize("name,part", PARTS, ids=IDS)
def test_fixture_through_the_operator_and_the_raw_c_abi(sgr, name, part):
    """values and the gradients against the reference's fp64 run, the zero pattern of dx exactly the reference's; the C ABI gives the
    operator's bits; a NULL gradient changes nothing else"""
    args, z = load(name, part)
    y, gs = run(sgr, *args)
    check_against(f"{name} {part}", y, gs, *fixture_refs(z, part))
    out, stats, raw = raw_abi(*args)
    check_against(f"{name} {part} C ABI", out, raw, *fixture_refs(z, part))
    assert torch.equal(out, y)
    for a, b in zip(raw, gs):
        assert (a is None and b is None) or torch.equal(a, b)
    x, w, b, G, size, skip, ct = args
    mean, rstd = C.moments(x.double(), G, 1e-5)
    assert err(stats[..., 0].double() + stats[..., 1].double(), mean.reshape(stats.shape[:2])) <= 1e-12
    assert err(stats[..., 2], rstd.reshape(stats.shape[:2])) <= 1e-7
    _, _, only = raw_abi(*args, want=(True, False, False, False))
    assert torch.equal(only[0], raw[0]) and only[1] is None and only[2] is None and only[3] is None
    if skip is not None:
        _, _, only = raw_abi(*args, want=(False, False, False, True))
        assert torch.equal(only[3], raw[3]) and only[0] is None
    # the module form is the same call
    mod = sgr.GroupNormReLU(G, x.shape[1], resize=True).cuda()
    mod.load_state_dict({"weight": w, "bias": b})
    with torch.no_grad():
        assert torch.equal(mod(x, skip) if skip is not None else mod(x, size=size), y)


def against_the_checker(sgr, tag, args):
    x, w, b, G, size, skip, ct = args
    y, gs = run(sgr, *args)
    d = lambda t: None if t is None else t.double().cpu()
    f = lambda t: None if t is None else t.cpu()
    y64, g64 = R.gn_resize(d(x), d(w), d(b), G, size, d(skip), cotangent=d(ct))
    y32, g32 = R.gn_resize(f(x), f(w), f(b), G, size, f(skip), cotangent=f(ct))
    check_against(tag, y, gs, y64, g64, err(y32, y64), [None if a is None else err(a, c) for a, c in zip(g32, g64)])


# (B, C, G, H, W, Hs, Ws, Cs): decoder0 stage 2 and decoderLight stage 2 at the training size; several workgroups per plane at a
# testReal-like size; the top of the domain with odd widths; the final-stage form at the training size
CHECKER_SHAPES = [(2, 256, 16, 14, 20, 15, 20, 256), (2, 512, 32, 6, 10, 7, 10, 512), (2, 64, 4, 106, 160, 107, 160, 64), (1, 32, 2, 33, 41, 66, 82, 5),
                  (2, 64, 4, 212, 320, 213, 320, 0)]


@pytest.mark.parametrize("shape", CHECKER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_checker(sgr, shape):
    against_the_checker(sgr, "x".join(map(str, shape)), draw(*shape, seed=1900 + shape[3]))


@pytest.mark.parametrize("Cs", [64, 0], ids=["upcat", "final"])
def test_a_mean_far_from_zero_at_30_by_41_against_the_checker(sgr, Cs):
    against_the_checker(sgr, f"mean 100 Cs={Cs}", draw(1, 64, 4, 30, 41, 31, 41, Cs, seed=1980, offset=100.0))


def test_equal_sizes_give_the_bits_of_the_existing_operators(sgr):
    x, w, b, G, _, skip, ct = draw(2, 16, 4, 6, 10, 6, 10, 8, seed=1985)
    ya, ga = run(sgr, x, w, b, G, (6, 10), skip, ct)
    xl, wl, bl, sl = [t.detach().requires_grad_(True) for t in (x, w, b, skip)]
    yb = sgr.group_norm_relu_upcat(xl, wl, bl, G, sl)
    gb = torch.autograd.grad(yb, (xl, wl, bl, sl), grad_outputs=ct)
    assert torch.equal(ya, yb.detach()) and all(torch.equal(a, c) for a, c in zip(ga, gb))
    with torch.no_grad():
        assert torch.equal(sgr.group_norm_relu_resize(x, w, b, G, (6, 10)), sgr.group_norm_relu(x, w, b, G))


@pytest.mark.parametrize("name,part", [("h1", "s"), ("hw", "s"), ("fin", "d0"), ("fin", "dl")], ids=["h1", "hw", "fin-d0", "fin-dl"])
def test_channels_last_and_sliced_inputs_give_the_same_bits(sgr, name, part):
    (x, w, b, G, size, skip, ct), _ = load(name, part)
    ya, ga = run(sgr, x, w, b, G, size, skip, ct)

    def sliced(t):      # a view into a larger buffer: one float off every 16-byte boundary (padded rows of a multiple of four floats, so
        if t is None:   # every row, plane and image starts one float past one), padded planes and images
            return None
        B, Cc, H, W = t.shape
        buf = torch.zeros(B + 1, Cc + 2, H + 1, (W + 6) // 4 * 4, device="cuda")
        v = buf[1:, 1:Cc + 1, :H, 1:W + 1]
        v.copy_(t)
        assert not v.is_contiguous() and v.data_ptr() % 16 != 0
        return v
    cl = lambda t: None if t is None else t.contiguous(memory_format=torch.channels_last)
    for tag, f in (("channels_last", cl), ("sliced", sliced)):
        xv, sv = f(x), f(skip)
        assert not xv.is_contiguous()
        yb, gb = run(sgr, xv, w, b, G, size, sv, ct)
        assert yb.is_contiguous() and torch.equal(ya, yb), tag
        for a, c in zip(ga, gb):
            assert (a is None and c is None) or (torch.equal(a, c) and a.shape == c.shape), tag
    # a non-contiguous cotangent and non-contiguous scales
    y = call(sgr, x.requires_grad_(True), w.repeat_interleave(2)[::2], b, G, size, skip)
    gx, = torch.autograd.grad(y, x, grad_outputs=ct.contiguous(memory_format=torch.channels_last))
    assert torch.equal(gx, ga[0])


# both forms at an element-wise shape (odd widths, one workgroup) and at a multi-workgroup shape (75x52 -> 76x104: 3952 positions of the
# skip's grid forward and 3900 source pixels backward, on workgroups of 256 threads x 8 rounds: two each)
@pytest.mark.parametrize("shape", [(3, 8, 2, 5, 7, 6, 9, 3), (3, 8, 2, 5, 7, 6, 9, 0), (3, 16, 2, 75, 52, 76, 104, 5), (3, 16, 2, 75, 52, 76, 104, 0)],
                         ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bit_identical_and_an_image_does_not_depend_on_its_batch(sgr, shape):
    x, w, b, G, size, skip, ct = draw(*shape, seed=1940 + shape[3])
    y1, g1 = run(sgr, x, w, b, G, size, skip, ct)
    y2, g2 = run(sgr, x, w, b, G, size, skip, ct)
    assert torch.equal(y1, y2)
    for a, c in zip(g1, g2):
        assert (a is None and c is None) or torch.equal(a, c)
    for i in range(3):
        s1 = None if skip is None else skip[i:i + 1]
        yb, gb = run(sgr, x[i:i + 1], w, b, G, size, s1, ct[i:i + 1])
        assert torch.equal(yb, y1[i:i + 1]), i
        assert torch.equal(gb[0], g1[0][i:i + 1]), i
        assert skip is None or torch.equal(gb[3], g1[3][i:i + 1]), i


@pytest.mark.parametrize("name,part", [("h1", "s"), ("hw", "s"), ("fin", "d0")], ids=["h1", "hw", "fin-d0"])
def test_a_subset_of_requires_grad_gives_the_same_numbers(sgr, name, part):
    args, _ = load(name, part)
    y, full = run(sgr, *args)
    for k in range(4):
        if args[5] is None and k == 3:
            continue
        need = tuple(j == k for j in range(4))
        yk, gk = run(sgr, *args, need=need)
        assert torch.equal(yk, y)
        for j in range(4):
            assert (gk[j] is None) if j != k else torch.equal(gk[j], full[j]), (k, j)
    with torch.no_grad():
        x, w, b, G, size, skip, _ = args
        y0 = call(sgr, x.requires_grad_(True), w, b, G, size, skip)
    assert y0.grad_fn is None and torch.equal(y0, y)


def test_captured_in_a_hip_graph(sgr):
    """forward + backward of both forms captured; replays on overwritten inputs equal eager runs bit for bit"""
    shape = (2, 16, 4, 6, 10, 7, 10, 8)
    x, w, b, G, size, skip, ct = draw(*shape, seed=1960)
    ct0 = ct[:, :16, ::2, ::2].contiguous()
    static = [t.requires_grad_(True) for t in (x, w, b, skip)]

    def step(x, w, b, skip):
        up = sgr.group_norm_relu_resize_upcat(x, w, b, G, skip)
        y = sgr.group_norm_relu_resize(x, w, b, G, size)
        return (up, y) + tuple(torch.autograd.grad(up, (x, w, b, skip), grad_outputs=ct)) + tuple(torch.autograd.grad(y, (x, w, b), grad_outputs=ct0))
    captured = sgr.capture_step(lambda: step(*static))
    for seed in (1961, 1962):
        fx, fw, fb, _, _, fs, _ = draw(*shape, seed=seed)
        with torch.no_grad():
            for s, f in zip(static, (fx, fw, fb, fs)):
                s.copy_(f)
        got = [o.clone() for o in captured()]
        torch.cuda.synchronize()
        want = step(*[f.requires_grad_(True) for f in (fx, fw, fb, fs)])
        torch.cuda.synchronize()
        for a, c in zip(got, want):
            assert torch.equal(a, c) and torch.isfinite(a).all()


def test_opcheck(sgr):
    ops = torch.ops.sgrender
    x, w, b, G, size, skip, ct = draw(2, 8, 2, 3, 5, 4, 6, 3, seed=1995)
    live = [t.requires_grad_(True) for t in (x, w, b, skip)]
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")      # aot_dispatch compares gradients through a second path
    torch.library.opcheck(ops.gn_resize, (live[0], live[1], live[2], live[3], G, 4, 6, 1e-5), test_utils=tests)
    torch.library.opcheck(ops.gn_resize, (live[0], live[1].detach(), live[2], None, G, 4, 6, 1e-5), test_utils=tests)
    stats = ops.gn_resize(x.detach(), w.detach(), b.detach(), skip.detach(), G, 4, 6, 1e-5)[1]
    torch.library.opcheck(ops.gn_resize_bwd, (ct, x.detach(), w.detach(), b.detach(), stats, 8, 3, G, 3, 5, True, True, True, True), test_utils=tests)
    torch.library.opcheck(ops.gn_resize_bwd, (ct, None, None, None, None, 8, 3, G, 3, 5, False, False, False, True), test_utils=tests)
