"""GPU: every rung of the render layer's launch ladders (POOL x envWidth x lobe count x vector width x decoder heads), at the smallest
shapes that still tell the rungs apart, against the fp64 oracle.

Two images (the batch index matters) of a 5 x 7 env grid: 35 cells are one full 32-pixel tile plus a 3-pixel tail, inside one partial
64-lane wave.  BRDF maps at 1x and at 2x the grid (POOL 1 / 2).  Direction grids 8x16 and 16x32 (the packed kernels: SGNum 3, 6 | 7, 12 |
13, 24 are the two sides of each boundary of their ladders), 4x8 (generic kernels, J % 4 == 0: vector env access) and 3x6 (generic,
J % 4 != 0: scalar env access; SGNum 3 | 8 | 12 | 16 | 24 | 32 walks the register-group rungs of the generic forward, backward and BRDF
backward).  The layer refuses none of these grids.  Per combination: forwardSG with and without the env image and its backward to all six
inputs, forwardEnv and its backward, sg_shading and the fused light objective (plain and from decoder outputs) where the layer offers them.

The oracle runs on the GPU, as in the other parity tests (its direction loop is launch-bound there and slower still on the host).
Tolerances: max(2 e_ref, 1e-4) rel-L2 with e_ref the fp32 oracle's own distance from the fp64 one on the same inputs (conftest.tol2); the reported loss values through
conftest.scalar_close with the fp32 oracle's own error.  The input normals are scaled to length 0.98: the
layer renormalises them, and |N|^2 stays clear of the kink of the reference's two-sided clamp at 1, where fp64 is no arbiter for the normal
and roughness gradients (tests/test_gpu_parity.py::test_shapes_vs_oracle deals with that case).  The roughness maps are drawn from
[-0.6, 1] instead of [-1, 1]: towards -1 the GGX term alpha^2 / (ndh^2 (alpha^2 - 1) + 1)^2 becomes singular at ndh = 1, and with 70 cells
one near-mirror cell then carries half the norm of the specular image and most of every fp32 evaluation's rounding error on it (on the
3x6 grid at 8 lobes: 47 % of the norm, 83 % of the fp32 oracle's error in one cell), so the comparison would be about that cell alone."""
import functools

import pytest
import torch

from conftest import NAMES6, oracle_with_noise, rel_l2, scalar_close, tol2

pytestmark = pytest.mark.gpu

BN, R, C = 2, 5, 7
SG = ("axis", "lamb", "weight")
BRDF = ("albedo", "normal", "rough")
PACKED = [(eh, ew, K) for eh, ew in ((8, 16), (16, 32)) for K in (3, 6, 7, 12, 13, 24)]
GENERIC = [(eh, ew, K) for eh, ew in ((4, 8), (3, 6)) for K in (3, 8, 12, 16, 24, 32)]
POOLS = [1, 2]


def _id(v):
    return f"{v[0]}x{v[1]}_K{v[2]}" if isinstance(v, tuple) else None


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


@functools.lru_cache(maxsize=None)
def _inputs(eh, ew, K, pool):
    from oracle import sg_oracle as O
    inp = O.synthetic_inputs(BN, pool * R, pool * C, R, C, K, eh, ew, seed=1600 + 100 * pool + ew + K, benign=True)
    inp["normal"] = inp["normal"] * 0.98
    inp["rough"] = inp["rough"] * 0.8 + 0.2
    g = torch.Generator().manual_seed(ew + K)
    cts = (torch.randn(BN, 3, R, C, eh, ew, generator=g), torch.randn(BN, 3, R, C, generator=g), torch.randn(BN, 3, R, C, generator=g))
    return inp, cts


@functools.lru_cache(maxsize=None)
def _sg_oracle(eh, ew, K, pool, need_env):
    """(ref64, e32) of forwardSG + backward; without the env image its cotangent is zero"""
    from oracle import sg_oracle as O
    inp, cts = _inputs(eh, ew, K, pool)
    cts = cts if need_env else (torch.zeros_like(cts[0]),) + cts[1:]
    r64, _, e32 = oracle_with_noise(O, inp, cts, eh, ew, NAMES6, "cuda")
    return r64, e32


def _layer(sgr, eh, ew):
    return sgr.renderingLayer(imWidth=C, imHeight=R, envWidth=ew, envHeight=eh)


def _check(tag, got, r64, e32):
    for k, v in got.items():
        assert torch.isfinite(v).all(), (tag, k)
        e = rel_l2(v.detach().to(r64[k].device), r64[k])
        print(f"{tag} {k}: rel-L2 {e:.2e}, fp32 oracle {e32[k]:.2e}")
        assert e <= tol2(e32[k]), (tag, k, e, e32[k])


@pytest.mark.parametrize("need_env", [True, False], ids=["env", "noenv"])
@pytest.mark.parametrize("pool", POOLS, ids=["pool1", "pool2"])
@pytest.mark.parametrize("cfg", PACKED + GENERIC, ids=_id)
def test_forward_sg_and_backward(sgr, cfg, pool, need_env):
    eh, ew, K = cfg
    inp, cts = _inputs(eh, ew, K, pool)
    r64, e32 = _sg_oracle(eh, ew, K, pool, need_env)
    x = {k: inp[k].cuda().requires_grad_(True) for k in NAMES6}
    env, d, s = _layer(sgr, eh, ew).forwardSG(*[x[k] for k in NAMES6], need_env=need_env)
    assert (env is not None) == need_env
    outs, ct = ([env, d, s], cts) if need_env else ([d, s], cts[1:])
    grads = torch.autograd.grad(outs, [x[k] for k in NAMES6], grad_outputs=[c.cuda() for c in ct])
    got = dict(diffuse=d, spec=s, **{"g_" + k: g for k, g in zip(NAMES6, grads)})
    if need_env:
        got["env"] = env
    _check(f"forwardSG {cfg} pool {pool} need_env {need_env}", got, r64, e32)


@pytest.mark.parametrize("pool", POOLS, ids=["pool1", "pool2"])
@pytest.mark.parametrize("cfg", [(8, 16, 0), (16, 32, 0), (4, 8, 0), (3, 6, 0)], ids=_id)
def test_forward_env_and_backward(sgr, cfg, pool):
    """forwardEnv takes no lobes: one env image per grid (the oracle's, from the 12-lobe inputs)"""
    from oracle import sg_oracle as O
    eh, ew, _ = cfg
    inp, cts = _inputs(eh, ew, 12, pool)
    env_in = _sg_oracle(eh, ew, 12, pool, True)[0]["env"].float()
    names = BRDF + ("env",)

    def oracle(dtype):
        x = {k: inp[k].to("cuda", dtype).requires_grad_(True) for k in BRDF}
        x["env"] = env_in.to(dtype).clone().requires_grad_(True)
        d, s = O.render_env(x["albedo"], x["normal"], x["rough"], x["env"])
        g = torch.autograd.grad([d, s], [x[k] for k in names], grad_outputs=[c.to("cuda", dtype) for c in cts[1:]])
        return dict(diffuse=d.detach(), spec=s.detach(), **{"g_" + k: t for k, t in zip(names, g)})
    r64, r32 = oracle(torch.float64), oracle(torch.float32)
    e32 = {k: rel_l2(r32[k], r64[k]) for k in r64}
    x = {k: inp[k].cuda().requires_grad_(True) for k in BRDF}
    x["env"] = env_in.clone().requires_grad_(True)
    d, s = _layer(sgr, eh, ew).forwardEnv(x["albedo"], x["normal"], x["rough"], x["env"])
    grads = torch.autograd.grad([d, s], [x[k] for k in names], grad_outputs=[c.cuda() for c in cts[1:]])
    _check(f"forwardEnv {eh}x{ew} pool {pool}", dict(diffuse=d, spec=s, **{"g_" + k: g for k, g in zip(names, grads)}), r64, e32)


@pytest.mark.parametrize("cfg", PACKED, ids=_id)
def test_sg_shading(sgr, cfg):
    """sg_shading has kernels for the packed grids alone (12 | 24 lobe slots x envWidth 16 | 32)"""
    from light_glue_checker import shading
    eh, ew, K = cfg
    inp, _ = _inputs(eh, ew, K, 1)
    pred = torch.cat([inp["axis"].reshape(BN, 3 * K, R, C), inp["lamb"], inp["weight"]], 1)
    ref64, ref32 = shading(pred, eh, ew, K, 1, torch.float64), shading(pred, eh, ew, K, 1, torch.float32)
    got = sgr.predToShading(pred.cuda(), envWidth=ew, envHeight=eh, SGNum=K)
    _check(f"sg_shading {cfg}", dict(shading=got), dict(shading=ref64), dict(shading=rel_l2(ref32, ref64)))


@pytest.mark.parametrize("heads", [False, True], ids=["plain", "decoder_outputs"])
@pytest.mark.parametrize("pool", POOLS, ids=["pool1", "pool2"])
@pytest.mark.parametrize("cfg", PACKED, ids=_id)
def test_light_objective(sgr, cfg, pool, heads):
    """the fused objective, offered on the packed grids alone; from decoder outputs the heads run as the kernels' prologue for
    SGNum > 6 and as a pass of their own below"""
    from oracle import sg_oracle as O
    from test_gpu_objective import _decoder_outputs
    eh, ew, K = cfg
    assert sgr.light_objective_supported(K, R, C, eh, ew)
    inp, _ = _inputs(eh, ew, K, pool)
    ind = torch.ones(BN, 1, 1, 1)
    ren_w, rec_w = 0.7, 3.0
    xs = _decoder_outputs(BN, K, R, C, seed=900 + K) if heads else tuple(inp[k] for k in SG)

    def oracle(dtype):
        o = {k: v.to("cuda", dtype) for k, v in inp.items()}
        x = [t.to("cuda", dtype).requires_grad_(True) for t in xs]
        a, l, w = O.light_heads(*x)[:3] if heads else x
        env, d, s = O.render_from_sg(o["albedo"], o["normal"], o["rough"], a, l, w, eh, ew)
        rerr = O.render_loss(d, s, o["im"], o["seg"], R, C)[0]
        cerr = O.recon_loss(env, o["env_gt"], o["seg"], ind.to("cuda", dtype), R, C, 1.0)[0]
        tot = ren_w * rerr + rec_w * cerr
        return tot.item(), rerr.item(), cerr.item(), torch.autograd.grad(tot, x)
    t64, r64, c64, g64 = oracle(torch.float64)
    t32, r32, c32, g32 = oracle(torch.float32)
    dev = {k: v.cuda() for k, v in inp.items()}
    x = [t.cuda().requires_grad_(True) for t in xs]
    obj, rerr, cerr, _, _ = sgr.light_objective(_layer(sgr, eh, ew), dev["albedo"], dev["normal"], dev["rough"], *x, dev["im"], dev["seg"],
                                                dev["env_gt"], ind.cuda(), ren_w, rec_w, decoder_outputs=heads)
    grads = torch.autograd.grad(obj, x)
    tag = f"light_objective {cfg} pool {pool} heads {heads}"
    print(f"{tag}: objective {obj.item():.7g} / {t64:.7g} ({t32:.7g}), render {rerr.item():.7g} / {r64:.7g} ({r32:.7g}), "
          f"recon {cerr.item():.7g} / {c64:.7g} ({c32:.7g})")
    assert scalar_close(rerr.item(), r64, r32 - r64), (tag, rerr.item(), r64, r32)
    assert scalar_close(cerr.item(), c64, c32 - c64), (tag, cerr.item(), c64, c32)
    assert scalar_close(obj.item(), t64, ren_w * abs(r32 - r64) + rec_w * abs(c32 - c64)), (tag, obj.item(), t64, t32)
    _check(tag, {"g_" + k: g for k, g in zip(SG, grads)}, {"g_" + k: g for k, g in zip(SG, g64)},
           {"g_" + k: rel_l2(a, b) for k, a, b in zip(SG, g32, g64)})
