"""GPU: sgr.brdf_objective and sgr.batch_ranking_loss (csrc/sgr_brdf_loss.hip behind torch.ops.sgrender.*) against the fixtures the
UNMODIFIED reference produced (tests/golden/g14_brdfobj_*.npz, tools/make_golden_brdf_objective.py) and against
tests/brdf_objective_checker.py, which tests/test_brdf_objective_checker.py pins to those fixtures at 1e-12.

Bounds.  Reported values (the five errors, angleMean, the two ranking losses): ``conftest.scalar_close(got, ref64, e_ref)``, the
project-wide ``max(2 e_ref, 1e-5 |ref|)``.  Gradients against the fp64 reference in rel-L2: ``max(4 e_ref, 1e-6)``, never above 1e-4
-- the bound of tests/test_gpu_bilateral.py, for the same reason: the GPU's reduction order differs from both reference runs, and
the floor covers the fp32 cast.  ``e_ref`` is the reference's own fp32-vs-fp64 distance: stored in the fixture, or -- at full size,
where no fixture fits -- the checker evaluated in fp32 on the same inputs.  Sharded against unsharded: 1e-6 relative, about eight
fp32 ulps -- the two evaluations differ only in the order in which fp32 partial totals are added (per rank, then across ranks)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import brdf_objective_checker as C
from conftest import GOLDEN_DIR, scalar_close

pytestmark = pytest.mark.gpu

SYN = ["syn_small", "syn_clip", "syn_softmask", "syn_coefclamp", "syn_odd"]
VALUES = ("total", "albedoErr", "normalErr", "roughErr", "depthErr")
GRADS = ("g_albedo", "g_normal", "g_rough", "g_depth")
ARGS = ("albedoPred", "normalPred", "roughPred", "depthPred", "albedo", "normal", "rough", "depth", "segBRDF", "segAll")


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g14_brdfobj_{name}.npz"))


def grad_bound(e_ref):
    return min(max(4.0 * float(e_ref), 1e-6), 1e-4)


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


def fixture_args(z):
    """positional arguments (device fp32 tensors, None for absent terms) and keyword arguments of sgr.brdf_objective / the checker"""
    args = [torch.from_numpy(z[k]).cuda() if k in z.files else None for k in ARGS]
    for i in range(4):
        if args[i] is None:
            args[i + 4] = None
    seg_depth = torch.from_numpy(z["segDepth"]).cuda() if "segDepth" in z.files else None
    return args, dict(weights=tuple(float(w) for w in z["weights"]), depth_offset=float(z["depth_offset"])), seg_depth


def run(sgr, args, kw, seg_depth=None, upstream=(1.0, 0.0, 0.0, 0.0, 0.0), group=None):
    """-> (BRDFObjective, gradients of sum_k upstream[k] * scalar_k with respect to the predictions present, in GRADS order with None)"""
    live = [a.detach().clone().requires_grad_(True) if a is not None else None for a in args[:4]]
    out = sgr.brdf_objective(*live, *args[4:], segDepthBatch=seg_depth, group=group, **kw)
    obj = sum(float(u) * getattr(out, k) for u, k in zip(upstream, VALUES) if u != 0.0)
    present = [t for t in live if t is not None]
    g = list(torch.autograd.grad(obj, present))
    return out, [g.pop(0) if t is not None else None for t in live]


def checker(args, kw, seg_depth, dtype, upstream=(1.0, 0.0, 0.0, 0.0, 0.0)):
    cast = lambda t: t.to(dtype) if t is not None else None
    return C.brdf_objective(*[cast(a) for a in args], segDepth=cast(seg_depth), upstream=upstream, **kw)


@pytest.mark.parametrize("name", SYN + ["nyu_small"])
def test_objective_matches_the_reference_fixture(sgr, name):
    z = load(name)
    args, kw, seg_depth = fixture_args(z)
    out, grads = run(sgr, args, kw, seg_depth)
    c64, c32 = checker(args, kw, seg_depth, torch.float64), checker(args, kw, seg_depth, torch.float32)
    for k in VALUES + ("angleMean",):
        if "ref64_" + k in z.files:
            got, ref, e = float(getattr(out, k).detach()), float(z["ref64_" + k]), float(z["e_ref_" + k])
        elif k == "angleMean":      # wrapperBRDF.py does not report it: the checker (pinned to wrapperNYU's by nyu_small) stands in
            got, ref, e = float(out.angleMean), float(c64[k]), abs(float(c32[k]) - float(c64[k]))
        else:
            assert float(getattr(out, k).detach()) == 0.0, k      # an absent term
            continue
        print(f"{name} {k}: got {got:.9g} ref {ref:.9g} |diff| {abs(got - ref):.2e} (e_ref {e:.1e})")
        assert scalar_close(got, ref, e), (name, k, got, ref, e)
    for k, g in zip(GRADS, grads):
        if g is None:
            assert "ref64_" + k not in z.files
            continue
        assert torch.isfinite(g).all()
        e, lim = err(g, z["ref64_" + k]), grad_bound(z["e_ref_" + k])
        print(f"{name} {k}: {e:.2e} (bound {lim:.1e}, e_ref {float(z['e_ref_' + k]):.2e})")
        assert e <= lim, (name, k, e, lim)
    assert err(out.coef, c64["coef"]) <= 1e-6


def rank_args(z):
    return [torch.from_numpy(z[k]).cuda() for k in ("albedoPred", "eqPoint", "eqWeight", "eqNum", "darkerPoint", "darkerWeight", "darkerNum")]


def run_rank(sgr, a, upstream=(1.0, 1.0), tau=0.5):
    x = a[0].detach().clone().requires_grad_(True)
    eq, dk = sgr.batch_ranking_loss(x, *a[1:], tau=tau)
    g, = torch.autograd.grad(upstream[0] * eq + upstream[1] * dk, [x])
    return eq.detach(), dk.detach(), g


def test_ranking_loss_matches_the_reference_fixture(sgr):
    z = load("rank_small")
    a = rank_args(z)
    for up, key in (((1.0, 0.0), "g_eq"), ((0.0, 1.0), "g_darker")):
        eq, dk, g = run_rank(sgr, a, up, float(z["tau"]))
        for k, got in (("eqLoss", eq), ("darkerLoss", dk)):
            ref, e = float(z["ref64_" + k]), float(z["e_ref_" + k])
            print(f"rank_small {k}: got {float(got):.9g} ref {ref:.9g} (e_ref {e:.1e})")
            assert scalar_close(float(got), ref, e), (k, float(got), ref)
        e, lim = err(g, z["ref64_" + key]), grad_bound(z["e_ref_" + key])
        print(f"rank_small {key}: {e:.2e} (bound {lim:.1e})")
        assert e <= lim, (key, e, lim)
    # int64 index tensors (what the data loader yields) give the same bits as int32
    b = [a[0]] + [t.long() if t.dtype == torch.int32 else t for t in a[1:]]
    for x, y in zip(run_rank(sgr, a), run_rank(sgr, b)):
        assert torch.equal(x, y)


def full_size_inputs(B=16, H=240, W=320, seed=2024, nyu=False):
    """Seeded inputs at the trainBRDF.py defaults: albedo / roughness U(0,1), unit normals, depth in [0.5, 4.5], segObj Bernoulli(0.7) with
    a disjoint segArea.  The albedo prediction is drawn in two bands, [0.05, 0.55] and [0.9, 1], with a ground truth about 1.3x as
    bright: the clamp is live for the upper band and no product comes near its kink (asserted by the test on the inputs)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    unit = lambda t: t / t.norm(dim=1, keepdim=True)
    band = u(B, 3, H, W) < 0.8
    aP = torch.where(band, 0.05 + 0.5 * u(B, 3, H, W), 0.9 + 0.1 * u(B, 3, H, W))
    a = torch.clamp(1.3 * aP * (0.95 + 0.1 * u(B, 3, H, W)), 0, 1)
    n = unit(torch.randn(B, 3, H, W, generator=g))
    nP = unit(n + 0.4 * torch.randn(B, 3, H, W, generator=g))
    r, rP = u(B, 1, H, W), 2 * u(B, 1, H, W) - 1
    d, dP = 0.5 + 4 * u(B, 1, H, W), 0.05 + 0.9 * u(B, 1, H, W)
    obj = u(B, 1, H, W) < 0.7
    seg_obj = obj.float()
    seg_area = (~obj & (u(B, 1, H, W) < 0.5)).float()
    seg_depth = (u(B, 1, H, W) < 0.6).float()
    if nyu:
        return [None, nP, None, dP, None, n, None, d, None, seg_obj + seg_area], seg_depth
    return [aP, nP, rP, dP, a, n, r, d, seg_obj, seg_obj + seg_area], None


@pytest.mark.parametrize("mode", ["synthetic_offset_1", "nyu_offset_0.1"])
def test_full_size_against_the_checker(sgr, mode):
    """16 x 240 x 320 (trainBRDF.py's batch and image size) against the checker in fp64 on the device; the checker in fp32 is e_ref"""
    nyu = mode.startswith("nyu")
    args, seg_depth = full_size_inputs(nyu=nyu)
    args = [a.cuda() if a is not None else None for a in args]
    seg_depth = seg_depth.cuda() if seg_depth is not None else None
    kw = dict(weights=(6.0, 1.0, 0.5, 0.5), depth_offset=0.1 if nyu else 1.0)
    r64, r32 = checker(args, kw, seg_depth, torch.float64), checker(args, kw, seg_depth, torch.float32)
    if not nyu:      # a condition on the inputs: the clamp is live and nothing sits on its kink
        prod = (args[0].double() * r64["coef"][:, 0].reshape(-1, 1, 1, 1))[(args[8] > 0).expand_as(args[0])]
        share = float((prod > 1).double().mean())
        kink = float(torch.minimum(prod.abs(), (prod - 1).abs()).min())
        print(f"full size: clipped share {share:.3f}, distance to the kink {kink:.2e}")
        assert 0.05 <= share <= 0.5 and kink > 1e-4
    out, grads = run(sgr, args, kw, seg_depth)
    for k in VALUES + ("angleMean",):
        got, ref, e = float(getattr(out, k).detach()), float(r64[k]), abs(float(r32[k]) - float(r64[k]))
        print(f"{mode} {k}: got {got:.9g} ref {ref:.9g} |diff| {abs(got - ref):.2e} (e_ref {e:.1e})")
        assert scalar_close(got, ref, e), (mode, k, got, ref, e)
    for k, g in zip(GRADS, grads):
        if g is None:
            assert r64[k] is None
            continue
        e_ref = err(r32[k], r64[k])
        e, lim = err(g, r64[k]), grad_bound(e_ref)
        print(f"{mode} {k}: {e:.2e} (bound {lim:.1e}, e_ref {e_ref:.2e})")
        assert e <= lim, (mode, k, e, lim)


UPSTREAMS = [(1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (0.7, -1.3, 2.0, 0.25, 3.0)]


@pytest.mark.parametrize("up", UPSTREAMS)
def test_gradient_routing_of_each_scalar_and_of_a_mix(sgr, up):
    """back-propagating each of the five scalars alone, and a weighted mix with non-unit upstream gradients, equals the checker"""
    z = load("syn_clip")
    args, kw, seg_depth = fixture_args(z)
    _, grads = run(sgr, args, kw, seg_depth, upstream=up)
    r64, r32 = checker(args, kw, seg_depth, torch.float64, up), checker(args, kw, seg_depth, torch.float32, up)
    for k, g in zip(GRADS, grads):
        e, lim = err(g, r64[k]), grad_bound(err(r32[k], r64[k]))
        print(f"upstream {up} {k}: {e:.2e} (bound {lim:.1e})")
        assert e <= lim, (up, k, e, lim)


def test_prediction_subsets_and_forward_only(sgr):
    """only the predictions that require grad get a gradient (the others' planes are not read in backward), values unchanged"""
    z = load("syn_small")
    args, kw, _ = fixture_args(z)
    full, grads = run(sgr, args, kw)
    live = [a.detach().clone() for a in args[:4]]
    live[1].requires_grad_(True)
    live[3].requires_grad_(True)
    out = sgr.brdf_objective(*live, *args[4:], **kw)
    gn, gd = torch.autograd.grad(out.total, [live[1], live[3]])
    assert torch.equal(gn, grads[1]) and torch.equal(gd, grads[3])
    with torch.no_grad():
        plain = sgr.brdf_objective(*args, return_scaled=True, **kw)
    for k in VALUES + ("angleMean", "coef"):
        assert torch.equal(getattr(plain, k), getattr(full, k)), k
    ref = checker(args, kw, None, torch.float64)
    a_s = torch.clamp(args[0].double() * ref["coef"][:, 0].reshape(-1, 1, 1, 1), 0, 1)
    assert err(plain.albedoScaled, a_s) <= 1e-6 and err(plain.depthScaled, args[3].double() * ref["coef"][:, 1].reshape(-1, 1, 1, 1)) <= 1e-6


def test_two_runs_are_bit_identical(sgr):
    args, seg_depth = full_size_inputs(B=4, H=120, W=160, seed=7)
    args = [a.cuda() for a in args]
    kw = dict(weights=(6.0, 1.0, 0.5, 0.5), depth_offset=1.0)
    o1, g1 = run(sgr, args, kw, upstream=(1.0, 0.5, 0, 0, 2.0))
    o2, g2 = run(sgr, args, kw, upstream=(1.0, 0.5, 0, 0, 2.0))
    for k in VALUES + ("angleMean", "coef"):
        assert torch.equal(getattr(o1, k), getattr(o2, k)), k
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    # the ranking loss, gradient included, with many judgements on few pixels
    B, H, W, N = 4, 60, 80, 800
    g = torch.Generator().manual_seed(11)
    hot = torch.stack([torch.randint(0, H, (50,), generator=g), torch.randint(0, W, (50,), generator=g)], 1)
    pick = lambda: hot[torch.randint(0, 50, (B, N), generator=g)]
    a = [(0.05 + 0.9 * torch.rand(B, 3, H, W, generator=g)).cuda(), torch.cat([pick(), pick()], -1).int().cuda(), torch.rand(B, N, generator=g).cuda(),
         torch.tensor([800, 650, 1, 300], dtype=torch.int32).cuda(), torch.cat([pick(), pick()], -1).int().cuda(), torch.rand(B, N, generator=g).cuda(),
         torch.tensor([0, 800, 799, 20], dtype=torch.int32).cuda()]
    r1, r2 = run_rank(sgr, a, (1.0, 2.0)), run_rank(sgr, a, (1.0, 2.0))
    for x, y in zip(r1, r2):
        assert torch.equal(x, y) and torch.isfinite(x).all()
    ref = C.batch_ranking_loss(a[0].double(), *a[1:], upstream=(1.0, 2.0))
    ref32 = C.batch_ranking_loss(a[0], *a[1:], upstream=(1.0, 2.0))
    assert scalar_close(float(r1[0]), float(ref["eqLoss"]), abs(float(ref32["eqLoss"]) - float(ref["eqLoss"])))
    assert scalar_close(float(r1[1]), float(ref["darkerLoss"]), abs(float(ref32["darkerLoss"]) - float(ref["darkerLoss"])))
    e, lim = err(r1[2], ref["g_albedo"]), grad_bound(err(ref32["g_albedo"], ref["g_albedo"]))
    print(f"ranking 4 x 800 judgements on 50 pixels, gradient: {e:.2e} (bound {lim:.1e})")
    assert e <= lim
    assert int((r1[2][:, 0] != 0).sum()) <= 4 * 50      # zero off the judged pixels


def test_empty_masks_give_zero_not_nan(sgr):
    z = load("syn_small")
    args, kw, _ = fixture_args(z)
    args[8], args[9] = torch.zeros_like(args[8]), torch.zeros_like(args[9])
    out, grads = run(sgr, args, kw, upstream=(1.0, 1.0, 1.0, 1.0, 1.0))
    for k in VALUES + ("angleMean",):
        assert float(getattr(out, k).detach()) == 0.0, k
    for g in grads:
        assert torch.isfinite(g).all() and float(g.abs().max()) == 0.0
    assert torch.all(out.coef == 1e-3)
    # one empty term next to live ones: segBRDF empty, segAll not
    args2, _, _ = fixture_args(z)
    args2[8] = torch.zeros_like(args2[8])
    out2, grads2 = run(sgr, args2, kw)
    ref = checker(args2, kw, None, torch.float64)
    assert float(out2.albedoErr) == 0.0 and float(out2.roughErr) == 0.0 and scalar_close(float(out2.normalErr), float(ref["normalErr"]))
    assert all(torch.isfinite(g).all() for g in grads2)


def test_ranking_edge_cases(sgr):
    z = load("rank_small")
    a = rank_args(z)
    base = run_rank(sgr, a)
    # padding garbage changes nothing: other garbage, same bits
    b = [t.clone() for t in a]
    for pt, wt, num in ((b[1], b[2], b[3]), (b[4], b[5], b[6])):
        for m in range(pt.shape[0]):
            pt[m, int(num[m]):] = 7
            wt[m, int(num[m]):] = -3.0
    for x, y in zip(base, run_rank(sgr, b)):
        assert torch.equal(x, y)
    # num == 0 for every image: 0, no NaN; for one image: that image's gradient is zero, the others' unchanged
    c = [t.clone() for t in a]
    c[3].zero_()
    c[6].zero_()
    eq, dk, g = run_rank(sgr, c)
    assert float(eq) == 0.0 and float(dk) == 0.0 and float(g.abs().max()) == 0.0
    d = [t.clone() for t in a]
    d[3][1] = 0
    d[6][1] = 0
    eq, dk, g = run_rank(sgr, d)
    assert torch.isfinite(eq) and torch.isfinite(dk) and float(g[1].abs().max()) == 0.0 and torch.equal(g[0], base[2][0]) and torch.equal(g[2], base[2][2])
    # a num beyond N is clamped to N; a negative one counts as 0
    e = [t.clone() for t in a]
    e[3][1] = 10 ** 6
    for x, y in zip(base, run_rank(sgr, e)):      # image 1's eqNum is N already
        assert torch.equal(x, y)
    # judgements outside the image change nothing beyond their own absence: the same bits as with their weight set to 0
    f, h = [t.clone() for t in a], [t.clone() for t in a]
    f[1][0, 3] = torch.tensor([0, 0, 24, 5], dtype=f[1].dtype)         # row == H
    f[1][0, 5] = torch.tensor([3, 32, 2, 2], dtype=f[1].dtype)         # column == W
    f[4][2, 0] = torch.tensor([-1, 3, 2, 2], dtype=f[4].dtype)
    f[4][2, 1] = torch.tensor([1, 3, 2, 2 ** 30], dtype=f[4].dtype)
    h[2][0, 3] = 0.0
    h[2][0, 5] = 0.0
    h[5][2, 0] = 0.0
    h[5][2, 1] = 0.0
    rf, rh = run_rank(sgr, f), run_rank(sgr, h)
    want = C.batch_ranking_loss(f[0].double(), *f[1:])
    assert scalar_close(float(rf[0]), float(want["eqLoss"])) and scalar_close(float(rf[1]), float(want["darkerLoss"]))
    for x, y in zip(rf, rh):
        assert torch.equal(x, y)


def test_captured_in_a_hip_graph_without_host_synchronisation(sgr):
    """forward + backward of both objectives captured in a HIP graph: a host synchronisation, a device-to-host copy or a device value
    read on the host anywhere in the path would fail the capture; replays on overwritten inputs equal eager runs bit for bit"""
    def make(seed):
        args, _ = full_size_inputs(B=2, H=48, W=64, seed=seed)
        return [a.cuda() for a in args]
    z = load("rank_small")
    rank = rank_args(z)
    static = make(1)
    for t in static[:4]:
        t.requires_grad_(True)
    rank[0] = rank[0].clone().requires_grad_(True)

    def step(x, ra):
        out = sgr.brdf_objective(*x, weights=(6.0, 1.0, 0.5, 0.5), depth_offset=1.0)
        g = torch.autograd.grad(out.total + 0.5 * out.normalErr, x[:4])
        eq, dk = sgr.batch_ranking_loss(*ra)
        gr, = torch.autograd.grad(eq + dk, [ra[0]])
        return (out.total, out.albedoErr, out.angleMean, eq, dk, gr) + g

    captured = sgr.capture_step(lambda: step(static, rank))
    for seed in (1, 2, 3):
        fresh = make(seed)
        with torch.no_grad():
            for s, f in zip(static, fresh):
                s.copy_(f)
            rank[0].copy_(torch.roll(rank[0], seed, 3))
        got = [o.clone() for o in captured()]
        torch.cuda.synchronize()
        for t in fresh[:4]:
            t.requires_grad_(True)
        want = step(fresh, [rank[0].detach().clone().requires_grad_(True)] + rank[1:])
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b) and torch.isfinite(a).all()


# --------------------------------------------------------------------------- #
# two ranks on one GPU over four images = the single-process batch             #
# --------------------------------------------------------------------------- #
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_inputs():
    args, _ = full_size_inputs(B=4, H=30, W=41, seed=99)
    args[8][1] = 0.0      # uneven denominators across the shards: image 1 has no object pixels
    return args


def _shard_run(sl, group):
    import inverserenderingofindoorscene_amd as pkg
    args = [a[sl].cuda().contiguous() for a in _shard_inputs()]
    out, grads = run(pkg, args, dict(weights=(6.0, 1.0, 0.5, 0.5), depth_offset=1.0), upstream=(1.0, 0.0, 0.5, 0.0, 0.0), group=group)
    torch.cuda.synchronize()
    return dict(values={k: float(getattr(out, k).detach()) for k in VALUES + ("angleMean",)}, coef=out.coef.cpu(), grads=[g.cpu() for g in grads])


def _shard_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out[rank] = _shard_run(slice(rank * 2, rank * 2 + 2), dist.group.WORLD)
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_on_one_gpu_match_the_full_batch():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    full = _shard_run(slice(0, 4), None)
    for r in range(world):
        o = out[r]
        for k, v in full["values"].items():
            print(f"rank {r} {k}: {o['values'][k]:.9g} vs {v:.9g}")
            assert abs(o["values"][k] - v) <= 1e-6 * abs(v), (r, k, o["values"][k], v)
        assert torch.equal(o["coef"], full["coef"][2 * r:2 * r + 2])      # per image: the same workgroups add the same numbers
        for k, a, b in zip(GRADS, o["grads"], full["grads"]):
            e = err(a, b[2 * r:2 * r + 2])
            print(f"rank {r} {k}: {e:.2e}")
            assert torch.isfinite(a).all() and e <= 1e-6, (r, k, e)
