"""GPU: sgr.brdf_heads / sgr.brdf_head (csrc/sgr_brdf_heads.hip behind torch.ops.sgrender.brdf_heads) against the fixtures the UNMODIFIED
reference produced (tests/golden/g16_brdfheads_*.npz, tools/make_golden_brdf_heads.py) and against tests/brdf_heads_checker.py, which
tests/test_brdf_heads.py pins to those fixtures at 1e-12.

Bounds: the project's rule for the BRDF operators.  Values against fp64 in rel-L2: ``max(2 e_ref, 1e-6)``; gradients: ``max(4 e_ref, 1e-6)``.
``e_ref`` is the reference's own fp32-vs-fp64 distance: stored in the fixture, or -- where no fixture fits -- the checker evaluated in
fp32 on the same inputs.  Inputs drawn here are kept 1e-5 away from the clamp's kink, as the fixtures are (asserted), so that a 1-ulp
tanh cannot flip a branch.

This file was written in a session that could not obtain a GPU: it has not run on one yet.  The conditions it asserts on its own inputs
(kink distances, the objective's clamp) were checked on the CPU with the checkers."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import brdf_heads_checker as C
import brdf_objective_checker as CO
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

CASES = ["vec", "odd", "sat", "nyu"]
OUT_CH = (3, 3, 1, 1)
SUBSETS = [s for s in itertools.product((False, True), repeat=4) if any(s)]


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g16_brdfheads_{name}.npz"))


def value_bound(e_ref):
    return max(2.0 * float(e_ref), 1e-6)


def grad_bound(e_ref):
    return max(4.0 * float(e_ref), 1e-6)


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


def dev(z, key):
    return [torch.from_numpy(z[f"{key}_{t}"]).cuda() if f"{key}_{t}" in z.files else None for t in C.TERMS]


def run(sgr, xs, cts, unit, need=(True, True, True, True)):
    """-> (outputs, gradients at the x that are present and needed), None elsewhere"""
    live = [x.detach().clone().requires_grad_(n) if x is not None else None for x, n in zip(xs, need)]
    ys = sgr.brdf_heads(*live, unit=unit)
    pairs = [(x, y, g) for x, y, g in zip(live, ys, cts) if x is not None and x.requires_grad]
    gs = list(torch.autograd.grad([y for _, y, _ in pairs], [x for x, _, _ in pairs], grad_outputs=[g for _, _, g in pairs])) if pairs else []
    return ys, [gs.pop(0) if x is not None and x.requires_grad else None for x in live]


def draw(B, H, W, seed, terms=(True, True, True, True), device="cuda"):
    """pre-activations 2 N(0,1) (depth: 2 sqrt(3) N(0,1), whose channel mean is 2 N(0,1)) and N(0,1) cotangents, on the device; a triplet
    within 1e-4 of the clamp's kink is halved, and a distance of at least 1e-5 is asserted"""
    g = torch.Generator().manual_seed(seed)
    xs, cts = [], []
    for k, (term, on) in enumerate(zip(C.TERMS, terms)):
        x = (2.0 * 3 ** 0.5 if term == "depth" else 2.0) * torch.randn(B, 3, H, W, generator=g)
        ct = torch.randn(B, OUT_CH[k], H, W, generator=g)
        if not on:
            xs.append(None)
            cts.append(None)
            continue
        for _ in range(8):      # a halved triplet may land near the kink in its turn
            t = x.double() if term != "depth" else ((x[:, 0:1] + x[:, 1:2]) + x[:, 2:3]).double() / 3
            bad = (((1.01 * torch.tanh(t)).abs() - 1).abs() < 1e-4).any(1, keepdim=True).expand_as(x)
            if not bool(bad.any()):
                break
            x = torch.where(bad, 0.5 * x, x)
        assert C.kink_distance(x, term) >= 1e-5
        xs.append(x.to(device))
        cts.append(ct.to(device))
    return xs, cts


def check_against(name, ys, gs, y64, g64, e_y, e_g):
    for term, y, g, yr, gr, ey, eg in zip(C.TERMS, ys, gs, y64, g64, e_y, e_g):
        if yr is None:
            assert y is None and g is None, (name, term)
            continue
        assert y.is_contiguous() and torch.isfinite(y).all() and torch.isfinite(g).all()
        ev, lv, eg_, lg = err(y, yr), value_bound(ey), err(g, gr), grad_bound(eg)
        print(f"{name} {term}: values {ev:.2e} (bound {lv:.1e}, e_ref {ey:.1e})  gradients {eg_:.2e} (bound {lg:.1e}, e_ref {eg:.1e})")
        assert ev <= lv, (name, term, "values", ev, lv)
        assert eg_ <= lg, (name, term, "gradients", eg_, lg)
        assert torch.equal(g.cpu() == 0, torch.as_tensor(gr).cpu() == 0), (name, term, "zero pattern")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("name", CASES)
def test_fixture_through_the_operator(sgr, name):
    """1. and 2.: values and gradients against the reference's fp64 run, and the gradients' zero pattern exactly the reference's"""
    z = load(name)
    xs, cts = dev(z, "x"), dev(z, "ct")
    y64 = [z[f"y64_{t}"] if f"x_{t}" in z.files else None for t in C.TERMS]
    g64 = [z[f"gx64_{t}"] if f"x_{t}" in z.files else None for t in C.TERMS]
    e_y = [float(z[f"e_ref_y_{t}"]) if f"x_{t}" in z.files else None for t in C.TERMS]
    e_g = [float(z[f"e_ref_gx_{t}"]) if f"x_{t}" in z.files else None for t in C.TERMS]
    ys, gs = run(sgr, xs, cts, unit=False)
    check_against(name, ys, gs, y64, g64, e_y, e_g)
    # the wrappers' form: 0.5 (y + 1) and half the gradient for albedo and depth, normal and roughness unchanged
    half = (True, False, False, True)
    yu, gu = run(sgr, xs, cts, unit=True)
    check_against(name + " unit", yu, gu, [0.5 * (y + 1) if h and y is not None else y for y, h in zip(y64, half)],
                  [0.5 * g if h and g is not None else g for g, h in zip(g64, half)], e_y, e_g)
    for y, y1, h in zip(ys, yu, half):
        if y is not None and not h:
            assert torch.equal(y, y1)
    # one decoder at a time is decoder0's own return value, and the same bits
    for k, term in enumerate(C.TERMS):
        if xs[k] is not None:
            assert torch.equal(sgr.brdf_head(xs[k], C.MODES[term]), ys[k]), term


@pytest.mark.parametrize("name", CASES)
def test_fixture_through_the_raw_c_abi(sgr, name):
    from inverserenderingofindoorscene_amd import _lib
    z = load(name)
    xs, cts = dev(z, "x"), dev(z, "ct")
    B, _, H, W = next(x for x in xs if x is not None).shape
    ys = [torch.empty(B, OUT_CH[k], H, W, device="cuda") if x is not None else None for k, x in enumerate(xs)]
    gs = [torch.empty_like(x) if x is not None else None for x in xs]
    _lib.call("sgr_brdf_heads_fwd", *[_ptr(x) for x in xs], *[_ptr(y) for y in ys], B, H, W, 0, _stream())
    _lib.call("sgr_brdf_heads_bwd", *[_ptr(x) for x in xs], *[_ptr(c) for c in cts], *[_ptr(g) for g in gs], B, H, W, 0, _stream())
    torch.cuda.synchronize()
    present = lambda key: [z[f"{key}_{t}"] if f"x_{t}" in z.files else None for t in C.TERMS]
    check_against(name + " C ABI", ys, gs, present("y64"), present("gx64"), [None if v is None else float(v) for v in present("e_ref_y")],
                  [None if v is None else float(v) for v in present("e_ref_gx")])
    want_y, want_g = run(sgr, xs, cts, unit=False)
    for a, b in zip(ys + gs, list(want_y) + want_g):
        assert (a is None and b is None) or torch.equal(a, b)
    # a NULL cotangent is a zero cotangent: a zero gradient, written; a NULL gx leaves its plane alone
    k = 1 if xs[0] is None else 0
    gs2 = [torch.full_like(x, 7.0) if x is not None else None for x in xs]
    cts2 = list(cts)
    cts2[k] = None
    gptr = [_ptr(g) for g in gs2]
    gptr[3] = None
    _lib.call("sgr_brdf_heads_bwd", *[_ptr(x) for x in xs], *[_ptr(c) for c in cts2], *gptr, B, H, W, 0, _stream())
    torch.cuda.synchronize()
    assert float(gs2[k].abs().max()) == 0.0 and bool((gs2[3] == 7.0).all())
    for j in (1, 2):
        if j != k and xs[j] is not None:
            assert torch.equal(gs2[j], gs[j])


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "".join(c for c, on in zip("anrd", s) if on))
def test_every_subset_of_terms(sgr, subset):
    """3.: an absent term gives None and changes nothing else; an x that does not require grad receives no gradient"""
    z = load("odd")
    xs, cts = dev(z, "x"), dev(z, "ct")
    full_y, full_g = run(sgr, xs, cts, unit=True)
    sub_x = [x if on else None for x, on in zip(xs, subset)]
    ys, gs = run(sgr, sub_x, cts, unit=True)
    for on, y, g, fy, fg in zip(subset, ys, gs, full_y, full_g):
        if on:
            assert torch.equal(y, fy) and torch.equal(g, fg)
        else:
            assert y is None and g is None
    # of the terms present, only every other one requires grad
    present = [k for k in range(4) if subset[k]]
    need = tuple(k in present[::2] for k in range(4))
    ys, gs = run(sgr, sub_x, cts, unit=True, need=need)
    for k in range(4):
        if not subset[k]:
            continue
        assert torch.equal(ys[k], full_y[k])
        assert ys[k].requires_grad == need[k]
        if need[k]:
            assert torch.equal(gs[k], full_g[k])
        else:
            assert gs[k] is None


def test_no_grad_saves_nothing_and_an_unused_output_does_not_break_the_backward(sgr):
    z = load("vec")
    xs, cts = dev(z, "x"), dev(z, "ct")
    full_y, full_g = run(sgr, xs, cts, unit=True)
    live = [x.clone().requires_grad_(True) for x in xs]
    with torch.no_grad():
        ys = sgr.brdf_heads(*live)
    for y, fy in zip(ys, full_y):
        assert y.grad_fn is None and not y.requires_grad and torch.equal(y, fy)
    # only the albedo and the depth prediction are used: the other two decoders get a zero gradient (a zero cotangent through NULL)
    ys = sgr.brdf_heads(*live)
    assert all(y.grad_fn is not None for y in ys)
    loss = (ys[0] * cts[0]).sum() + (ys[3] * cts[3]).sum()
    loss.backward()
    assert torch.equal(live[0].grad, full_g[0]) and torch.equal(live[3].grad, full_g[3])
    for k in (1, 2):
        assert live[k].grad is None or float(live[k].grad.abs().max()) == 0.0
    ga, gn = torch.autograd.grad((sgr.brdf_heads(*live)[0] * cts[0]).sum(), [live[0], live[1]], allow_unused=True)
    assert torch.equal(ga, full_g[0]) and (gn is None or float(gn.abs().max()) == 0.0)


def test_two_runs_are_bit_identical_and_an_image_does_not_depend_on_its_batch(sgr):
    """4."""
    xs, cts = draw(5, 37, 52, seed=1640)
    y1, g1 = run(sgr, xs, cts, unit=True)
    y2, g2 = run(sgr, xs, cts, unit=True)
    for a, b in zip(list(y1) + g1, list(y2) + g2):
        assert torch.equal(a, b)
    for b in (0, 3, 4):
        yb, gb = run(sgr, [x[b:b + 1].contiguous() for x in xs], [c[b:b + 1].contiguous() for c in cts], unit=True)
        for a, full in zip(list(yb) + gb, list(y1) + g1):
            assert torch.equal(a, full[b:b + 1]), b


@pytest.mark.parametrize("shape", [(2, 6, 10), (3, 16, 20), (2, 64, 68)])
def test_the_128_bit_and_the_element_wise_path_give_the_same_bits(sgr, shape):
    """5.: the same data in an aligned tensor and through a view shifted by one float (off every 16-byte boundary)"""
    B, H, W = shape
    assert H * W % 4 == 0
    xs, cts = draw(B, H, W, seed=1650 + H)
    assert all(x.data_ptr() % 16 == 0 for x in xs)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    ya, ga = run(sgr, xs, cts, unit=True)
    from inverserenderingofindoorscene_amd import _lib
    xo = [shifted(x) for x in xs]
    co = [shifted(c) for c in cts]
    yo = [shifted(torch.zeros_like(y)) for y in ya]
    go = [shifted(torch.zeros_like(g)) for g in ga]
    _lib.call("sgr_brdf_heads_fwd", *[_ptr(x) for x in xo], *[_ptr(y) for y in yo], B, H, W, 1, _stream())
    _lib.call("sgr_brdf_heads_bwd", *[_ptr(x) for x in xo], *[_ptr(c) for c in co], *[_ptr(g) for g in go], B, H, W, 1, _stream())
    torch.cuda.synchronize()
    for a, b in zip(list(ya) + ga, yo + go):
        assert torch.equal(a, b)
    # and through the operator, where only the inputs are shifted
    live = [x.requires_grad_(True) for x in xo]
    yb = sgr.brdf_heads(*live, unit=True)
    gb = torch.autograd.grad(yb, live, grad_outputs=co)
    for a, b in zip(list(ya) + ga, list(yb) + list(gb)):
        assert torch.equal(a, b)


# (2,120,160) and (1,250,333): one round of the grid, 128-bit and element-wise; (32,260,256) and (32,129,131): more workgroups wanted than
# the cap of 64 per image allows, so the threads stride, 128-bit and element-wise
@pytest.mark.parametrize("shape", [(2, 120, 160), (1, 250, 333), (32, 260, 256), (32, 129, 131)])
def test_larger_planes_and_the_striding_grid_against_the_checker(sgr, shape):
    """6.: against the fp64 checker evaluated on the device, e_ref from the checker's own fp32 run"""
    B, H, W = shape
    xs, cts = draw(B, H, W, seed=1660 + W)
    ys, gs = run(sgr, xs, cts, unit=True)
    y64, g64 = C.brdf_heads(*[x.double() for x in xs], unit=True, cotangents=[c.double() for c in cts])
    y32, g32 = C.brdf_heads(*xs, unit=True, cotangents=cts)
    check_against(f"{B}x{H}x{W}", ys, gs, y64, g64, [err(a, b) for a, b in zip(y32, y64)], [err(a, b) for a, b in zip(g32, g64)])


def test_a_channels_last_input_gives_the_same_bits(sgr):
    """7."""
    xs, cts = draw(2, 12, 20, seed=1670)
    ya, ga = run(sgr, xs, cts, unit=True)
    cl = [x.contiguous(memory_format=torch.channels_last) for x in xs]
    assert not any(x.is_contiguous() for x in cl)
    yb, gb = run(sgr, cl, cts, unit=True)
    for a, b in zip(list(ya) + ga, list(yb) + gb):
        assert torch.equal(a, b) and a.shape == b.shape
    assert all(y.is_contiguous() for y in yb)


def test_captured_in_a_hip_graph_without_host_synchronisation(sgr):
    """8.: forward + backward captured; replays on overwritten inputs equal eager runs bit for bit"""
    static, cts = draw(2, 24, 36, seed=1680)
    for x in static:
        x.requires_grad_(True)

    def step(xs):
        ys = sgr.brdf_heads(*xs, unit=True)
        return tuple(ys) + tuple(torch.autograd.grad(ys, xs, grad_outputs=cts))
    captured = sgr.capture_step(lambda: step(static))
    for seed in (1681, 1682):
        fresh, _ = draw(2, 24, 36, seed=seed)
        with torch.no_grad():
            for s, f in zip(static, fresh):
                s.copy_(f)
        got = [o.clone() for o in captured()]
        torch.cuda.synchronize()
        want = step([f.requires_grad_(True) for f in fresh])
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b) and torch.isfinite(a).all()


def test_heads_into_the_brdf_objective(sgr):
    """9.: brdf_heads -> brdf_objective(...).total.backward() at 2 x 30 x 41: the gradients at the four x against the fp64 composition of
    the two checkers; e_ref is the same composition in fp32"""
    B, H, W = 2, 30, 41
    xs, _ = draw(B, H, W, seed=1690)
    g = torch.Generator().manual_seed(1691)
    u = lambda *s: torch.rand(*s, generator=g)
    n = torch.randn(B, 3, H, W, generator=g)
    obj = u(B, 1, H, W) < 0.7
    gt = [u(B, 3, H, W), n / n.norm(dim=1, keepdim=True), u(B, 1, H, W), 0.5 + 4 * u(B, 1, H, W), obj.float(), obj.float() + (~obj & (u(B, 1, H, W) < 0.5)).float()]
    gt = [t.cuda() for t in gt]
    kw = dict(weights=(6.0, 1.0, 0.5, 0.5), depth_offset=1.0)

    def composed(dtype):
        x = [t.to(dtype) for t in xs]
        ys, _ = C.brdf_heads(*x, unit=True)
        o = CO.brdf_objective(*ys, *[t.to(dtype) for t in gt], **kw)
        _, gx = C.brdf_heads(*x, unit=True, cotangents=[o[k] for k in ("g_albedo", "g_normal", "g_rough", "g_depth")])
        return o, ys, gx
    o64, y64, g64 = composed(torch.float64)
    o32, _, g32 = composed(torch.float32)
    # a condition on the inputs: no scaled albedo near a kink of the objective's clamp.  A saturated albedo head is EXACTLY 0 in every
    # precision (0.5 (-1 + 1)), on the closed side of that clamp for the fp32 and the fp64 evaluation alike: those are left out
    prod = (y64[0] * o64["coef"][:, 0].reshape(-1, 1, 1, 1))[(gt[4] > 0).expand_as(y64[0])]
    prod = prod[prod != 0]
    assert float(torch.minimum(prod.abs(), (prod - 1).abs()).min()) > 1e-6
    live = [x.clone().requires_grad_(True) for x in xs]
    out = sgr.brdf_objective(*sgr.brdf_heads(*live, unit=True), *gt, **kw)
    out.total.backward()
    assert abs(float(out.total) - float(o64["total"])) <= max(2 * abs(float(o32["total"]) - float(o64["total"])), 1e-5 * abs(float(o64["total"])))
    for term, x, gr, g3 in zip(C.TERMS, live, g64, g32):
        e, lim = err(x.grad, gr), grad_bound(err(g3, gr))
        print(f"heads -> objective {term}: {e:.2e} (bound {lim:.1e}, e_ref {err(g3, gr):.2e})")
        assert torch.isfinite(x.grad).all() and e <= lim, (term, e, lim)


def test_an_all_zero_normal_triplet_is_finite_and_has_the_stated_gradient(sgr):
    """10.: output 0, gradient g / 1e-6 * 1.01 where the reference gives NaN"""
    x = torch.randn(1, 3, 4, 6, generator=torch.Generator().manual_seed(1700)).cuda()
    x[0, :, 1, 2] = 0.0
    x[0, :, 3, 5] = 0.0
    ct = torch.randn(1, 3, 4, 6, generator=torch.Generator().manual_seed(1701)).cuda()
    live = x.clone().requires_grad_(True)
    y = sgr.brdf_head(live, 1)
    gx, = torch.autograd.grad(y, live, grad_outputs=ct)
    y64, g64 = C.head(x.double(), "normal", ct.double())
    assert torch.isfinite(y).all() and torch.isfinite(gx).all()
    for r, c in ((1, 2), (3, 5)):
        assert float(y[0, :, r, c].abs().max()) == 0.0
        assert err(gx[0, :, r, c], g64[0, :, r, c]) <= 1e-6 and err(g64[0, :, r, c], 1.01e6 * ct[0, :, r, c].double()) <= 1e-14
    assert err(y, y64) <= 1e-6 and err(gx, g64) <= 1e-6


def test_opcheck(sgr):
    """11."""
    ops = torch.ops.sgrender
    xs, cts = draw(2, 6, 10, seed=1710)
    live = [x.requires_grad_(True) for x in xs]
    torch.library.opcheck(ops.brdf_heads, (live[0], live[1], live[2], live[3], True))
    torch.library.opcheck(ops.brdf_heads, (live[0], live[1], live[2], live[3], False))
    torch.library.opcheck(ops.brdf_heads, (None, live[1], None, live[3].detach(), True))
    raw = [x.detach() for x in xs]
    torch.library.opcheck(ops.brdf_heads_bwd, (*raw, *cts, True, True, True, True, True))
    torch.library.opcheck(ops.brdf_heads_bwd, (raw[0], None, raw[2], None, None, None, cts[2], None, False, True, False, True, False))
