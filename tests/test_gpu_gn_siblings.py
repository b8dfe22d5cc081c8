"""GPU: the sibling forms of the decoders' upcat stage (sgr.group_norm_relu_upcat_siblings / sgr.group_norm_relu_resize_upcat_siblings,
torch.ops.sgrender.gn_stage_siblings / gn_resize_siblings).

Two yardsticks:

  * the single operators, bit for bit: ``outs[d]``, ``dx[d]``, ``dweight[d]``, ``dbias[d]`` and the statistics are what
    ``group_norm_relu_upcat`` / ``group_norm_relu_resize_upcat`` return for sibling ``d``; ``dskip`` is ``((s_0 + s_1) + s_2) + ...`` in fp32, in
    sibling order, over the single operators' ``dskip``.  In bf16 a single operator's ``dskip`` is already rounded, so the sum is formed from
    the fp32 operator on the upcast tensors (which section 8j defines the bf16 operator by) and rounded once;
  * the fixtures the UNMODIFIED reference produced (tests/golden/g23_gnsib_{brdf,light}.npz, tools/make_golden_gn_siblings.py): four
    ``decoder0`` / three ``decoderLight`` instances driven at one stage from one shared skip leaf, whose ``.grad`` the reference's autograd
    accumulated.  Bounds, the project's rule: values within ``max(2 e_ref, 1e-6)`` rel-L2 of the fp64 arrays, gradients within
    ``max(4 e_ref, 1e-6)``, ``e_ref`` the reference's own fp32-vs-fp64 distance stored in the fixture."""
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DS = (1, 2, 3, 4, 8)
# B, C, G, H, W, Cs: the vector path; nothing on a 16-byte boundary; one pixel; one row; Cs = 7 != C throughout
SAME = [(2, 64, 4, 6, 10, 7), (3, 256, 16, 3, 5, 7), (1, 512, 32, 1, 1, 7), (2, 128, 8, 1, 7, 7)]
# B, C, G, H, W, Hs, Ws, Cs
RESIZE = [(2, 64, 4, 5, 8, 6, 8, 7), (3, 64, 4, 3, 5, 4, 6, 7), (1, 64, 4, 2, 3, 4, 6, 64), (2, 128, 8, 1, 1, 2, 2, 7)]


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


def draw(D, B, C, H, W, Hs, Ws, Cs, seed, dtype=torch.float32):
    """xs (sibling 1 at 100 + N(0,1): statistics swapped between siblings cannot pass), scales with negative ones and an exact zero, a
    skip and one cotangent per sibling, on the device"""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    xs = [((100.0 if d == 1 else 0.0) + n(B, C, H, W)).to(dtype).cuda() for d in range(D)]
    ws = [n(C) for _ in range(D)]
    for w in ws:
        w[C // 3] = 0.0
    bs = [0.3 * n(C) for _ in range(D)]
    skip = n(B, Cs, Hs, Ws).to(dtype).cuda()
    cts = [n(B, C + Cs, 2 * Hs, 2 * Ws).to(dtype).cuda() for _ in range(D)]
    return xs, [w.cuda() for w in ws], [b.cuda() for b in bs], skip, cts


def single(sgr, x, w, b, G, skip):
    return sgr.group_norm_relu_upcat(x, w, b, G, skip) if x.shape[2:] == skip.shape[2:] else sgr.group_norm_relu_resize_upcat(x, w, b, G, skip)


def siblings(sgr, xs, ws, bs, G, skip):
    f = sgr.group_norm_relu_upcat_siblings if xs[0].shape[2:] == skip.shape[2:] else sgr.group_norm_relu_resize_upcat_siblings
    return f(xs, ws, bs, G, skip)


def leaf(t, need=True):
    return t.detach().requires_grad_(need)


def run_single(sgr, x, w, b, G, skip, ct):
    """-> (y, dx, dw, db, ds) of the single operator"""
    l = [leaf(t) for t in (x, w, b, skip)]
    y = single(sgr, *l[:3], G, l[3])
    return (y.detach(),) + tuple(torch.autograd.grad(y, l, grad_outputs=ct))


def ordered_dskip(sgr, xs, ws, bs, G, skip, cts, live=None):
    """((s_0 + s_1) + s_2) + ... over the siblings in `live`, in fp32 and in the cotangents' dtype at the end"""
    total = None
    for d in range(len(xs)):
        if live is not None and d not in live:
            continue
        s = run_single(sgr, xs[d].float(), ws[d], bs[d], G, skip.float(), cts[d].float())[4]
        total = s if total is None else total + s
    return total.to(skip.dtype)


def run_siblings(sgr, xs, ws, bs, G, skip, cts, need=None, live=None):
    """-> (outs, dxs, dws, dbs, ds); `need`: (xs, ws, bs, skip) flags per sibling; `live`: the siblings whose result enters the loss"""
    D = len(xs)
    need = need or ([True] * D, [True] * D, [True] * D, True)
    lx, lw, lb = ([leaf(t, n) for t, n in zip(ts, ns)] for ts, ns in zip((xs, ws, bs), need[:3]))
    ls = leaf(skip, need[3])
    outs = siblings(sgr, lx, lw, lb, G, ls)
    live = list(range(D)) if live is None else live
    wrt = [t for t in lx + lw + lb + [ls] if t.requires_grad]
    got = list(torch.autograd.grad([outs[d] for d in live], wrt, grad_outputs=[cts[d] for d in live], allow_unused=True)) if wrt else []
    take = lambda ts: [got.pop(0) if t.requires_grad else None for t in ts]
    dx, dw, db = take(lx), take(lw), take(lb)
    return [o.detach() for o in outs], dx, dw, db, take([ls])[0]


def same(a, b):
    return a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b) and bool(torch.isfinite(a.float()).all())


def against_the_single_operators(sgr, args, G):
    xs, ws, bs, skip, cts = args
    D = len(xs)
    outs, dx, dw, db, ds = run_siblings(sgr, xs, ws, bs, G, skip, cts)
    op = torch.ops.sgrender.gn_stage_siblings if xs[0].shape[2:] == skip.shape[2:] else torch.ops.sgrender.gn_resize_siblings
    stats = op(xs, ws, bs, skip, G, 1e-5)[1]
    assert stats.shape == (D, xs[0].shape[0], G, 4) and stats.dtype == torch.float32
    for d in range(D):
        y1, dx1, dw1, db1, ds1 = run_single(sgr, xs[d], ws[d], bs[d], G, skip, cts[d])
        assert same(outs[d], y1) and same(dx[d], dx1) and same(dw[d], dw1) and same(db[d], db1), d
        if xs[0].shape[2:] == skip.shape[2:]:
            st1 = torch.ops.sgrender.gn_stage(xs[d], ws[d], bs[d], skip, G, 1e-5)[1]
        else:
            st1 = torch.ops.sgrender.gn_resize(xs[d], ws[d], bs[d], skip, G, skip.shape[2], skip.shape[3], 1e-5)[1]
        assert same(stats[d], st1), d
        if D == 1:
            assert same(ds, ds1)      # one sibling: the single operator in every output
    assert same(ds, ordered_dskip(sgr, xs, ws, bs, G, skip, cts))
    return outs, dx, dw, db, ds


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SAME, ids=lambda s: "x".join(map(str, s)))
def test_same_size_bits_are_the_single_operators(sgr, shape, dtype):
    B, C, G, H, W, Cs = shape
    for D in DS:
        against_the_single_operators(sgr, draw(D, B, C, H, W, H, W, Cs, 2300 + D, dtype), G)


@pytest.mark.parametrize("shape", RESIZE, ids=lambda s: "x".join(map(str, s)))
def test_resize_bits_are_the_single_operators(sgr, shape):
    B, C, G, H, W, Hs, Ws, Cs = shape
    for D in DS:
        against_the_single_operators(sgr, draw(D, B, C, H, W, Hs, Ws, Cs, 2320 + D), G)


def test_equal_sizes_through_the_resize_wrapper_are_the_same_size_operator(sgr):
    xs, ws, bs, skip, cts = draw(3, 2, 16, 3, 5, 3, 5, 7, 2330)
    a = sgr.group_norm_relu_resize_upcat_siblings(xs, ws, bs, 4, skip)
    b = sgr.group_norm_relu_upcat_siblings(xs, ws, bs, 4, skip)
    assert all(same(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("form", ["same", "resize"])
def test_every_subset_of_requires_grad(sgr, form):
    """the sixteen subsets of (xs, weights, biases, skip) for all siblings alike, then flags that differ between the siblings: what is
    computed equals the full run's bits, the rest is None, and without any flag there is no node"""
    D, G = 3, 4
    args = draw(D, 2, 16, 3, 5, *((3, 5) if form == "same" else (4, 6)), 7, 2340)
    xs, ws, bs, skip, cts = args
    full = run_siblings(sgr, *args[:3], G, skip, cts)
    masks = [([a] * D, [b] * D, [c] * D, s) for a, b, c, s in itertools.product([False, True], repeat=4)]
    masks += [([True, False, False], [False, True, False], [False, False, False], False), ([False, False, True], [False, False, True], [True, False, False], True)]
    for need in masks:
        if not (any(need[0]) or any(need[1]) or any(need[2]) or need[3]):
            outs = siblings(sgr, xs, ws, bs, G, skip)
            assert all(o.grad_fn is None and same(o, f) for o, f in zip(outs, full[0]))
            continue
        got = run_siblings(sgr, xs, ws, bs, G, skip, cts, need=need)
        assert all(same(o, f) for o, f in zip(got[0], full[0]))
        for k in range(3):
            for d in range(D):
                assert same(got[1 + k][d], full[1 + k][d]) if need[k][d] else got[1 + k][d] is None, (need, k, d)
        assert same(got[4], full[4]) if need[3] else got[4] is None, need


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("live", [(0, 2, 3), (1, 2, 3), (0, 1, 2), (2,)], ids=["middle-out", "first-out", "last-out", "one-in"])
def test_a_sibling_left_out_of_the_loss(sgr, live, dtype):
    """an undefined cotangent: no gradients for that sibling, and it is skipped in dskip's sum"""
    D, G = 4, 4
    xs, ws, bs, skip, cts = draw(D, 2, 16, 3, 5, 3, 5, 7, 2350, dtype)
    full = run_siblings(sgr, xs, ws, bs, G, skip, cts)
    outs, dx, dw, db, ds = run_siblings(sgr, xs, ws, bs, G, skip, cts, live=list(live))
    for d in range(D):
        if d in live:
            assert same(dx[d], full[1][d]) and same(dw[d], full[2][d]) and same(db[d], full[3][d]), d
        else:
            assert dx[d] is None and dw[d] is None and db[d] is None, d
    assert same(ds, ordered_dskip(sgr, xs, ws, bs, G, skip, cts, live=live))
    # the resize form's adjoint kernel takes the same table
    xs, ws, bs, skip, cts = draw(D, 2, 16, 3, 5, 4, 6, 7, 2351)
    if dtype == torch.float32:
        got = run_siblings(sgr, xs, ws, bs, G, skip, cts, live=list(live))
        assert same(got[4], ordered_dskip(sgr, xs, ws, bs, G, skip, cts, live=live))
        assert all((got[1][d] is None) == (d not in live) for d in range(D))


@pytest.mark.parametrize("form", ["same", "resize"])
def test_two_runs_an_image_against_its_batch_and_other_layouts(sgr, form):
    D, G = 3, 4
    hs = (6, 10) if form == "same" else (7, 12)
    xs, ws, bs, skip, cts = draw(D, 3, 16, 6, 10, *hs, 7, 2360)
    torch.use_deterministic_algorithms(True)
    try:
        a = run_siblings(sgr, xs, ws, bs, G, skip, cts)
        b = run_siblings(sgr, xs, ws, bs, G, skip, cts)
    finally:
        torch.use_deterministic_algorithms(False)
    flat = lambda r: list(r[0]) + r[1] + r[2] + r[3] + [r[4]]
    assert all(same(p, q) for p, q in zip(flat(a), flat(b)))
    # image 1 alone: its results and its part of dx and dskip (dweight and dbias are sums over the batch)
    one = run_siblings(sgr, [x[1:2] for x in xs], ws, bs, G, skip[1:2], [c[1:2] for c in cts])
    for d in range(D):
        assert same(one[0][d], a[0][d][1:2]) and same(one[1][d], a[1][d][1:2]), d
    assert same(one[4], a[4][1:2])
    # channels-last and sliced xs and skip are read in place: the same bits
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    wide = lambda t: torch.cat([torch.zeros_like(t), t, torch.zeros_like(t)], 1)[:, t.shape[1]:2 * t.shape[1]]
    odd = lambda t: torch.nn.functional.pad(t, (1, 2, 0, 1))[:, :, :t.shape[2], 1:1 + t.shape[3]]
    for lay_x, lay_s in ((cl, cl), (wide, odd), (odd, wide)):
        lx, ls = [lay_x(x) for x in xs], lay_s(skip)
        assert not lx[0].is_contiguous() and torch.equal(lx[0], xs[0]) and torch.equal(ls, skip)
        c = run_siblings(sgr, lx, ws, bs, G, ls, cts)
        assert all(same(p, q) for p, q in zip(flat(a), flat(c)))
    # one sibling in another layout than the rest
    c = run_siblings(sgr, [xs[0], cl(xs[1]), odd(xs[2])], ws, bs, G, skip, cts)
    assert all(same(p, q) for p, q in zip(flat(a), flat(c)))


def test_captured_in_a_hip_graph(sgr):
    """forward + backward of both forms, one chain: replays on overwritten inputs equal eager runs bit for bit"""
    D, G = 3, 4
    xs, ws, bs, skip, cts = draw(D, 2, 16, 4, 6, 4, 6, 7, 2370)
    skip2 = draw(D, 2, 16, 4, 6, 5, 8, 7, 2371)[3]
    cts2 = draw(D, 2, 16, 4, 6, 5, 8, 7, 2371)[4]
    static = [[leaf(t) for t in ts] for ts in (xs, ws, bs)] + [[leaf(skip), leaf(skip2)]]

    def step(lx, lw, lb, ls):
        a = sgr.group_norm_relu_upcat_siblings(lx, lw, lb, G, ls[0])
        ga = torch.autograd.grad(a, lx + lw + lb + [ls[0]], grad_outputs=cts)
        b = sgr.group_norm_relu_resize_upcat_siblings(lx, lw, lb, G, ls[1])
        gb = torch.autograd.grad(b, lx + lw + lb + [ls[1]], grad_outputs=cts2)
        return tuple(a) + tuple(ga) + tuple(b) + tuple(gb)
    captured = sgr.capture_step(lambda: step(*static))
    for seed in (2372, 2373):
        fx, fw, fb, fs, _ = draw(D, 2, 16, 4, 6, 4, 6, 7, seed)
        fs2 = draw(D, 2, 16, 4, 6, 5, 8, 7, seed + 10)[3]
        with torch.no_grad():
            for s, f in zip(static[0] + static[1] + static[2] + static[3], fx + fw + fb + [fs, fs2]):
                s.copy_(f)
        got = [o.clone() for o in captured()]
        torch.cuda.synchronize()
        want = step([leaf(t) for t in fx], [leaf(t) for t in fw], [leaf(t) for t in fb], [leaf(fs), leaf(fs2)])
        torch.cuda.synchronize()
        assert len(got) == len(want) and all(same(p, q) for p, q in zip(got, want))


def test_opcheck(sgr):
    ops = torch.ops.sgrender
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")      # aot_dispatch compares gradients through a second path
    for hs, fwd, bwd in (((3, 5), ops.gn_stage_siblings, ops.gn_stage_siblings_bwd), ((4, 6), ops.gn_resize_siblings, ops.gn_resize_siblings_bwd)):
        xs, ws, bs, skip, cts = draw(3, 2, 8, 3, 5, *hs, 3, 2380)
        lx, lw, lb, ls = [leaf(t) for t in xs], [leaf(t) for t in ws], [leaf(t, False) for t in bs], leaf(skip)
        torch.library.opcheck(fwd, (lx, lw, lb, ls, 2, 1e-5), test_utils=tests)
        stats = fwd(xs, ws, bs, skip, 2, 1e-5)[1]
        torch.library.opcheck(bwd, (cts, xs, ws, bs, stats, 8, 3, 2, 3, 5, 7, 7, 7, True), test_utils=tests)
        none = torch.empty(0, device="cuda")
        torch.library.opcheck(bwd, ([cts[0], none, cts[2]], [none] * 3, [none] * 3, [none] * 3, None, 8, 3, 2, 3, 5, 0, 0, 0, True), test_utils=tests)


def test_the_module_and_cpu_tensors(sgr):
    stages = [sgr.GroupNormReLU(4, 16).cuda() for _ in range(4)]
    xs, ws, bs, skip, _ = draw(4, 2, 16, 3, 5, 3, 5, 7, 2390)
    with torch.no_grad():
        for m, w, b in zip(stages, ws, bs):
            m.weight.copy_(w)
            m.bias.copy_(b)
    outs = sgr.SiblingGroupNormReLU(stages)(xs, skip)
    assert all(same(o.detach(), m(x, skip).detach()) for o, m, x in zip(outs, stages, xs))
    with pytest.raises(RuntimeError, match="no CPU path"):
        sgr.group_norm_relu_upcat_siblings([x.cpu() for x in xs], [w.cpu() for w in ws], [b.cpu() for b in bs], 4, skip.cpu())


# ---- the reference's fixtures ------------------------------------------------------------------------------------------------------------------

def value_bound(e_ref):
    return max(2.0 * float(e_ref), 1e-6)


def grad_bound(e_ref):
    return max(4.0 * float(e_ref), 1e-6)


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


@pytest.mark.parametrize("name", ["brdf", "light"])
def test_against_the_reference_fixtures(sgr, name):
    z = np.load(os.path.join(GOLDEN_DIR, f"g23_gnsib_{name}.npz"))
    D, G = int(z["D"]), int(z["G"])
    dev = lambda k: torch.from_numpy(z[k]).cuda()
    xs, ws, bs, cts = ([dev(f"s{d}_{k}") for d in range(D)] for k in ("x", "weight", "bias", "ct"))
    skip = dev("skip")
    outs, dx, dw, db, ds = run_siblings(sgr, xs, ws, bs, G, skip, cts)
    worst = []
    for d in range(D):
        e, lim = err(outs[d], z[f"s{d}_y64"]), value_bound(z[f"s{d}_e_ref_y"])
        print(f"{name} sibling {d}: values {e:.2e} (bound {lim:.1e})")
        worst.append((e <= lim, f"y{d}", e, lim))
        for k, g in (("dx", dx[d]), ("dw", dw[d]), ("db", db[d])):
            e, lim = err(g, z[f"s{d}_{k}64"]), grad_bound(z[f"s{d}_e_ref_{k}"])
            print(f"{name} sibling {d}: {k} {e:.2e} (bound {lim:.1e})")
            worst.append((e <= lim, f"{k}{d}", e, lim))
        assert torch.equal(dx[d].cpu() == 0, torch.from_numpy(z[f"s{d}_dx64"]) == 0), (name, d, "zero pattern of dx")
    e, lim = err(ds, z["ds64"]), grad_bound(z["e_ref_ds"])
    print(f"{name}: dskip {e:.2e} (bound {lim:.1e})")
    worst.append((e <= lim, "ds", e, lim))
    assert all(w[0] for w in worst), [w for w in worst if not w[0]]
