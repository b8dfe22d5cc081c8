"""GPU: ``light_objective(..., brdf_grads=True)`` -- the trainLight objective differentiated w.r.t. the BRDF maps as well (the objective's
backward pass, then the render layer's BRDF backward from the SG lobes driven by the render cotangents), against the reference's own gradients of
renderErr + 10 reconstErr with every input live (the golden fixtures' ``ref{32,64}_gtot_{albedo,normal,rough}``), the fp64 oracle, the
unfused HIP route (forwardSG + render_loss + recon_loss) and the default route (SG gradients), one rank and sharded."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import layer_kwargs, rel_l2, scalar_close, tol2

pytestmark = pytest.mark.gpu

NAMES = ("albedo", "normal", "rough", "axis", "lamb", "weight")
MAPS = ("albedo", "normal", "rough")
SG = ("axis", "lamb", "weight")


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


def _t(z, k):
    return torch.from_numpy(np.ascontiguousarray(z[k])).cuda()


def _live(x, names):
    return {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in x.items()}


def _objective(sgr, layer, x, ind, heads=False, group=None, brdf_grads=True):
    return sgr.light_objective(layer, x["albedo"], x["normal"], x["rough"], x["axis"], x["lamb"], x["weight"], x["im"], x["seg"], x["env_gt"], ind,
                               1.0, 10.0, group=group, decoder_outputs=heads, brdf_grads=brdf_grads)


def _route_d(sgr, layer, x, ind, heads=False):
    """The same gradients through forwardSG + render_loss + recon_loss (env image materialised): the arbiter where the normals sit on the
    |N|^2 == 1 clamp kink (unit normals at ratio 1), since both routes take the kink's side from the same pooled normal."""
    y = {k: (v.detach().clone().requires_grad_(True) if k in NAMES else v) for k, v in x.items()}
    axis, lamb, weight = y["axis"], y["lamb"], y["weight"]
    if heads:
        axis, lamb, weight, _ = sgr.light_heads(axis, lamb, weight)
    R, C = layer.imHeight, layer.imWidth
    env, d, s = layer.forwardSG(y["albedo"], y["normal"], y["rough"], axis, lamb, weight, need_env=True)
    err, _ = sgr.render_loss(d, s, y["im"], y["seg"], R, C)
    rec = sgr.recon_loss(env, y["env_gt"], y["seg"], ind, R, C)
    return dict(zip(NAMES, torch.autograd.grad(err + 10.0 * rec, [y[k] for k in NAMES])))


def _oracle(inp, ind, R, C, eh, ew, fov=57.0, F0=0.05, cam=(0.0, 0.0, 0.0), heads=False, dtype=torch.float64, device="cuda"):
    """renderErr + 10 reconstErr from the oracle's pieces with all six inputs live: (objective, render_err, recon_err, grads of NAMES)."""
    from oracle import sg_oracle as O
    x = {k: v.to(device=device, dtype=dtype).clone().requires_grad_(k in NAMES) for k, v in inp.items()}
    axis, lamb, weight = x["axis"], x["lamb"], x["weight"]
    if heads:
        axis, lamb, weight, _ = O.light_heads(axis, lamb, weight)
    env, d, s = O.render_from_sg(x["albedo"], x["normal"], x["rough"], axis, lamb, weight, eh, ew, fov, F0, cam)
    rerr, _, _, _ = O.render_loss(d, s, x["im"], x["seg"], R, C)
    cerr, _, _, _ = O.recon_loss(env, x["env_gt"], x["seg"], ind.to(device=device, dtype=dtype), R, C)
    tot = rerr + 10.0 * cerr
    g = torch.autograd.grad(tot, [x[k] for k in NAMES])
    return tot.item(), rerr.item(), cerr.item(), {k: t.detach().cpu() for k, t in zip(NAMES, g)}


# --------------------------------------------------------------------------- #
# 1. against the reference's gradients (fused route: g1, g3, g10_*; fallback: g2)
# --------------------------------------------------------------------------- #
def test_brdf_gradients_vs_golden(sgr, golden):
    name, z, cfg = golden
    x = {k: _t(z, "in_" + k) for k in NAMES}
    x.update(im=_t(z, "in_im"), seg=_t(z, "in_seg"), env_gt=_t(z, "in_env_gt"))
    x = _live(x, NAMES)
    layer = sgr.renderingLayer(**layer_kwargs(cfg))
    ind = torch.ones(cfg["bn"], 1, 1, 1, device="cuda")
    obj, rerr, cerr, _, _ = _objective(sgr, layer, x, ind)
    r64, c64 = float(z["ref64_render_err"][0]), float(z["ref64_recon_err"][0])
    r32, c32 = float(z["ref32_render_err"][0]), float(z["ref32_recon_err"][0])
    assert scalar_close(rerr.item(), r64, r32 - r64), (name, rerr.item(), r64)
    assert scalar_close(cerr.item(), c64, c32 - c64), (name, cerr.item(), c64)
    grads = torch.autograd.grad(obj, [x[k] for k in NAMES])
    report = {}
    for k, g in zip(NAMES, grads):
        ref32, ref64 = z["ref32_gtot_" + k], z["ref64_gtot_" + k]
        e_ref, e = rel_l2(ref32, ref64), rel_l2(g.cpu(), ref64)
        report[k] = (e, e_ref)
        assert e <= tol2(e_ref), (name, k, e, e_ref)
    if cfg["imH"] == cfg["R"]:
        # ratio 1, unit normals: the normal gradient sits on the |N|^2 == 1 kink and e_ref is ~0.9 -- the unfused route arbitrates instead
        e_d = rel_l2(grads[1].cpu(), _route_d(sgr, layer, x, ind)["normal"].cpu())
        report["normal vs unfused route"] = (e_d, 0.0)
        assert e_d < 1e-4, (name, e_d)
    print(f"\n{name}: (rel-L2 vs ref64, reference's own fp32 error)", {k: tuple(f"{v:.2e}" for v in t) for k, t in report.items()})


# --------------------------------------------------------------------------- #
# 2. against the fp64 oracle, the fp32 oracle on the GPU as the yardstick
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("heads", [False, True], ids=["plain", "decoder_outputs"])
@pytest.mark.parametrize("bn,imH,imW,R,C,K,benign,eh,ew", [
    (2, 12, 20, 12, 20, 12, True, 8, 16),      # ratio 1, NG = 2, EW = 16
    (3, 18, 26, 9, 13, 12, False, 8, 16),      # ratio 2, ragged tiles, stress lobes
    (2, 10, 14, 10, 14, 5, True, 8, 16),       # five lobes
    (2, 12, 20, 6, 10, 12, True, 16, 32),      # 16x32 grid, NG = 2 on virtual rows
    (2, 18, 26, 9, 13, 24, False, 16, 32),     # 24 lobes, 16x32: NG = 4, ragged 16-pixel tiles, stress lobes
    (1, 14, 22, 7, 11, 24, True, 8, 16),       # 24 lobes on the 8x16 grid: NG = 4, EW = 16
    (2, 10, 14, 10, 14, 17, True, 5, 32),      # odd envHeight, a partly empty fourth lobe group
    (2, 36, 48, 12, 16, 12, True, 8, 16),      # maps at 3x the env grid: torch's pooling in front, autograd through it
    (1, 25, 35, 10, 14, 9, False, 8, 16),      # an odd ratio (2.5): the same
])
def test_brdf_gradients_vs_oracle(sgr, heads, bn, imH, imW, R, C, K, benign, eh, ew):
    from oracle import sg_oracle as O
    if heads and not (sgr.light_objective_supported(K, R, C, eh, ew) and K > 6):
        K = 12 if K <= 6 else K      # decoder heads as the prologue need 6 < SGNum
    inp = O.synthetic_inputs(bn, imH, imW, R, C, K, eh, ew, seed=700 + K + R, benign=benign)
    if heads:
        g = torch.Generator().manual_seed(17)
        inp["axis"] = torch.randn(bn, 3 * K, R, C, generator=g)
        inp["lamb"] = torch.randn(bn, K, R, C, generator=g)
        inp["weight"] = torch.randn(bn, 3 * K, R, C, generator=g)
    ind = torch.ones(bn, 1, 1, 1)
    if bn > 2:
        ind[1] = 0.0
    x = _live({k: v.cuda() for k, v in inp.items()}, NAMES)
    layer = sgr.renderingLayer(imWidth=C, imHeight=R, envWidth=ew, envHeight=eh)
    obj, rerr, cerr, _, _ = _objective(sgr, layer, x, ind.cuda(), heads=heads)
    grads = torch.autograd.grad(obj, [x[k] for k in NAMES])
    t64, r64, c64, g64 = _oracle(inp, ind, R, C, eh, ew, heads=heads)
    t32, r32, c32, g32 = _oracle(inp, ind, R, C, eh, ew, heads=heads, dtype=torch.float32)
    assert scalar_close(rerr.item(), r64, r32 - r64) and scalar_close(cerr.item(), c64, c32 - c64), (rerr.item(), r64, cerr.item(), c64)
    report = {}
    for k, g in zip(NAMES, grads):
        assert tuple(g.shape) == tuple(inp[k].shape), k
        e, e_ref = rel_l2(g.cpu(), g64[k]), rel_l2(g32[k], g64[k])
        report[k] = (e, e_ref)
        assert e <= tol2(e_ref), (k, e, e_ref)
    if imH == R:      # ratio 1, unit normals on the clamp kink (e_ref ~0.4-1): the unfused route arbitrates the normal gradient
        e_d = rel_l2(grads[1].cpu(), _route_d(sgr, layer, x, ind.cuda(), heads)["normal"].cpu())
        report["normal vs unfused route"] = (e_d, 0.0)
        assert e_d < 1e-4, e_d
    print("\n(rel-L2 vs fp64 oracle, fp32 oracle's own)", {k: tuple(f"{v:.2e}" for v in t) for k, t in report.items()})


# --------------------------------------------------------------------------- #
# 3. config 2 at size: 16 images, batch-global denominators, env_ind == 0 and seg == 0 images
# --------------------------------------------------------------------------- #
def test_config2_full_batch_vs_unfused_route_and_oracle(sgr):
    from oracle import sg_oracle as O
    bn, imH, imW, R, C, K = 16, 240, 320, 120, 160, 12
    inp = O.synthetic_inputs(bn, imH, imW, R, C, K, seed=1602)
    inp["seg"][6] = 0.0
    ind = torch.ones(bn, 1, 1, 1)
    ind[3] = ind[10] = 0.0
    dev = {k: v.cuda() for k, v in inp.items()}
    layer = sgr.renderingLayer(imWidth=C, imHeight=R)
    x = _live(dev, NAMES)
    obj = _objective(sgr, layer, x, ind.cuda())[0]
    g = torch.autograd.grad(obj, [x[k] for k in NAMES])
    # (d): forwardSG + render_loss + recon_loss, the maps live
    y = _live(dev, NAMES)
    env, d, s = layer.forwardSG(y["albedo"], y["normal"], y["rough"], y["axis"], y["lamb"], y["weight"], need_env=True)
    err, _ = sgr.render_loss(d, s, y["im"], y["seg"], R, C)
    rec = sgr.recon_loss(env, y["env_gt"], y["seg"], ind.cuda(), R, C)
    gu = torch.autograd.grad(err + 10.0 * rec, [y[k] for k in NAMES])
    worst = {}
    for k, a, b in zip(NAMES, g, gu):
        e = rel_l2(a.cpu(), b.cpu())
        worst[k] = e
        assert e < 1e-4, (k, e)
    # per image against the fp64 oracle (the whole batch in one oracle call: its denominators are the batch's)
    _, _, _, g64 = _oracle(inp, ind, R, C, 8, 16)
    _, _, _, g32 = _oracle(inp, ind, R, C, 8, 16, dtype=torch.float32)
    per = {}
    for k, a in zip(MAPS, g[:3]):
        a = a.cpu()
        for i in range(bn):
            if g64[k][i].norm() == 0:
                assert a[i].abs().max() == 0, (k, i)
                continue
            e, e_ref = rel_l2(a[i], g64[k][i]), rel_l2(g32[k][i], g64[k][i])
            per[(k, i)] = (e, e_ref)
            assert e <= tol2(e_ref) or e <= 2.0 * e_ref, (k, i, e, e_ref)
    print("\nconfig 2: vs the unfused route", {k: f"{v:.2e}" for k, v in worst.items()},
          "worst per-image vs fp64 (err, fp32 oracle's own):", {k: max(((e, r) for (kk, _), (e, r) in per.items() if kk == k)) for k in MAPS})


# --------------------------------------------------------------------------- #
# 4. the adjoint leaves everything else alone; determinism
# --------------------------------------------------------------------------- #
def _small(sgr, seed=5, K=12, heads=False):
    from oracle import sg_oracle as O
    bn, imH, imW, R, C = 3, 24, 32, 12, 16
    inp = O.synthetic_inputs(bn, imH, imW, R, C, K, seed=seed)
    dev = {k: v.cuda() for k, v in inp.items()}
    return dev, torch.ones(bn, 1, 1, 1, device="cuda"), sgr.renderingLayer(imWidth=C, imHeight=R)


def test_brdf_adjoint_leaves_values_and_sg_gradients_alone(sgr):
    dev, ind, layer = _small(sgr)
    x = _live(dev, SG)
    ref = _objective(sgr, layer, x, ind, brdf_grads=False)
    gref = torch.autograd.grad(ref[0], [x[k] for k in SG])
    runs = []
    for _ in range(2):
        y = _live(dev, NAMES)
        out = _objective(sgr, layer, y, ind)
        runs.append((out, torch.autograd.grad(out[0], [y[k] for k in NAMES])))
    out, g = runs[0]
    for a, b in zip(out[:3], ref[:3]):
        assert abs(a.item() - b.item()) <= 1e-6 * abs(b.item()), (a.item(), b.item())
    assert torch.equal(out[3], ref[3]) and torch.equal(out[4], ref[4])
    for a, b in zip(g[3:], gref):
        assert rel_l2(a.cpu(), b.cpu()) <= 1e-6
    bitwise = all(torch.equal(a, b) for a, b in zip(out[:3], ref[:3])) and all(torch.equal(a, b) for a, b in zip(g[3:], gref))
    print(f"\nwith the BRDF adjoint vs without: loss values and SG gradients bit-identical: {bitwise}")
    (o2, g2) = runs[1]
    assert all(torch.equal(a, b) for a, b in zip(out, o2)) and all(torch.equal(a, b) for a, b in zip(g, g2))      # two runs, bit for bit


# --------------------------------------------------------------------------- #
# 5. subsets
# --------------------------------------------------------------------------- #
def test_only_live_maps_get_gradients_and_wrapper_pattern(sgr):
    dev, ind, layer = _small(sgr, seed=8)
    x = _live(dev, ("rough",) + SG)
    obj = _objective(sgr, layer, x, ind)[0]
    obj.backward()
    assert x["rough"].grad is not None and torch.isfinite(x["rough"].grad).all() and x["rough"].grad.abs().sum() > 0
    assert x["albedo"].grad is None and x["normal"].grad is None
    # wrapperBRDFLight.py:194: albedoPred detached, normal and rough live -- the same normal / rough gradients as with all three live
    y = _live(dev, ("normal", "rough") + SG)
    gy = torch.autograd.grad(_objective(sgr, layer, y, ind)[0], [y["normal"], y["rough"]])
    z = _live(dev, NAMES)
    gz = torch.autograd.grad(_objective(sgr, layer, z, ind)[0], [z["normal"], z["rough"]])
    assert all(torch.equal(a, b) for a, b in zip(gy, gz))
    # only a map live, no SG parameter: the map's gradient is still there
    w = _live(dev, ("normal",))
    gw = torch.autograd.grad(_objective(sgr, layer, w, ind)[0], [w["normal"]])[0]
    assert torch.equal(gw, gz[0])


def test_no_live_map_launches_the_default_kernels(sgr):
    from torch.profiler import ProfilerActivity, profile
    dev, ind, layer = _small(sgr, seed=9)

    def kernels(brdf_grads, maps=()):
        x = _live(dev, SG + tuple(maps))
        _objective(sgr, layer, x, ind, brdf_grads=brdf_grads)      # warm-up
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            out = _objective(sgr, layer, x, ind, brdf_grads=brdf_grads)
            torch.autograd.grad(out[0], [x[k] for k in SG])
            torch.cuda.synchronize()
        return out, sorted(e.key for e in prof.key_averages() if "sgr::" in e.key)

    o_def, n_def = kernels(False)
    o_new, n_new = kernels(True)
    assert all(torch.equal(a, b) for a, b in zip(o_def, o_new))
    if n_def:      # the profiler reports device kernels on this box
        assert n_new == n_def, (n_new, n_def)
        _, n_brdf = kernels(True, ("rough",))
        assert all(n in n_brdf for n in n_def), (n_brdf, n_def)      # the default route's kernels, plus the BRDF backward
        brdf = [n for n in n_brdf if "brdf_bwd" in n]
        assert brdf and all(n not in n_def for n in brdf), (brdf, n_def)


# --------------------------------------------------------------------------- #
# 6. cotangent scaling and a second backward through the same node
# --------------------------------------------------------------------------- #
def test_cotangent_scaling_and_second_backward(sgr):
    dev, ind, layer = _small(sgr, seed=11)
    x = _live(dev, NAMES)
    g1 = torch.autograd.grad(_objective(sgr, layer, x, ind)[0], [x[k] for k in NAMES])
    y = _live(dev, NAMES)
    obj = _objective(sgr, layer, y, ind)[0]
    g3 = torch.autograd.grad(3.0 * obj, [y[k] for k in NAMES], retain_graph=True)
    for a, b in zip(g3, g1):
        assert rel_l2(a.cpu(), 3.0 * b.cpu()) < 1e-6
    g3 = [t.clone() for t in g3]
    g_half = torch.autograd.grad(-0.5 * obj, [y[k] for k in NAMES])      # second backward through the node
    for a, b in zip(g_half, g1):
        assert rel_l2(a.cpu(), -0.5 * b.cpu()) < 1e-6
    # .backward() accumulation: gradients of 2 * obj land in .grad of all six
    z = _live(dev, NAMES)
    (2.0 * _objective(sgr, layer, z, ind)[0]).backward()
    for k, b in zip(NAMES, g1):
        assert rel_l2(z[k].grad.cpu(), 2.0 * b.cpu()) < 1e-6, k


# --------------------------------------------------------------------------- #
# 7. sharded: two ranks on one GPU over gloo
# --------------------------------------------------------------------------- #
CASES = {
    "k12_8x16": dict(bn=4, imH=24, imW=32, R=12, C=16, K=12, eh=8, ew=16, heads=False),
    "k12_8x16_decoder_outputs": dict(bn=4, imH=24, imW=32, R=12, C=16, K=12, eh=8, ew=16, heads=True),
    "k24_16x32_ragged": dict(bn=4, imH=10, imW=14, R=5, C=7, K=24, eh=16, ew=32, heads=False),
    "cfg2_8img": dict(bn=8, imH=240, imW=320, R=120, C=160, K=12, eh=8, ew=16, heads=False),
}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_inputs(c):
    from oracle import sg_oracle as O
    inp = O.synthetic_inputs(c["bn"], c["imH"], c["imW"], c["R"], c["C"], c["K"], c["eh"], c["ew"], seed=4243)
    inp["seg"][1] = 0.0
    ind = torch.ones(c["bn"])
    ind[2::4] = 0.0
    inp["ind"] = ind.reshape(c["bn"], 1, 1, 1)
    if c["heads"]:
        g = torch.Generator().manual_seed(98)
        bn, K, R, C = c["bn"], c["K"], c["R"], c["C"]
        inp["axis"] = torch.randn(bn, 3 * K, R, C, generator=g)
        inp["lamb"] = torch.randn(bn, K, R, C, generator=g)
        inp["weight"] = torch.randn(bn, 3 * K, R, C, generator=g)
    return inp


def _shard_run(case, sl, group):
    import inverserenderingofindoorscene_amd as sgr
    c = CASES[case]
    x = {k: v[sl].cuda().contiguous() for k, v in _shard_inputs(c).items()}
    x = _live(x, NAMES)
    layer = sgr.renderingLayer(imWidth=c["C"], imHeight=c["R"], envWidth=c["ew"], envHeight=c["eh"])
    obj = sgr.light_objective(layer, x["albedo"], x["normal"], x["rough"], x["axis"], x["lamb"], x["weight"], x["im"], x["seg"], x["env_gt"],
                              x["ind"], 1.0, 10.0, group=group, decoder_outputs=c["heads"], brdf_grads=True)
    g = torch.autograd.grad(obj[0], [x[k] for k in NAMES])
    torch.cuda.synchronize()
    return dict(obj=obj[0].item(), g=[t.cpu() for t in g])


def _shard_worker(rank, world, port, case, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    per = CASES[case]["bn"] // world
    out[rank] = _shard_run(case, slice(rank * per, (rank + 1) * per), dist.group.WORLD)
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("case", list(CASES))
def test_two_ranks_brdf_gradients_match_the_full_batch(case):
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_shard_worker, args=(world, _free_port(), case, out), nprocs=world, join=True)
    full = _shard_run(case, slice(0, CASES[case]["bn"]), None)
    per = CASES[case]["bn"] // world
    worst = 0.0
    for r in range(world):
        o = out[r]
        assert abs(o["obj"] - full["obj"]) <= 2e-6 * abs(full["obj"]), (case, r, o["obj"], full["obj"])
        for name, a, b in zip(NAMES, o["g"], full["g"]):
            b = b[r * per:(r + 1) * per]
            assert torch.isfinite(a).all()
            rel = rel_l2(a, b)
            assert rel < 5e-6, (case, r, name, rel)
            worst = max(worst, rel)
    print(f"\n{case}: two ranks vs the full batch with brdf_grads=True, worst gradient {worst:.2e} (bound 5e-6)")


# --------------------------------------------------------------------------- #
# 8. the image-side inputs are still refused
# --------------------------------------------------------------------------- #
def test_image_gradients_still_refused(sgr):
    dev, ind, layer = _small(sgr, seed=12)

    class _Group:      # any explicit group selects the sharded route; the refusal comes before any collective
        pass
    for group in (None, _Group()):
        x = _live(dev, ("rough", "im") + SG)
        with pytest.raises(RuntimeError, match="BRDF maps only"):
            _objective(sgr, layer, x, ind, group=group)
