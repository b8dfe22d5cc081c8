"""GPU: the last, ragged 32-pixel tile of an env grid reads nothing that changes a result.

The env-sized streams (the objective's ground-truth env, the env cotangent of ``forwardSG(need_env=True)``'s backward, the env input of
``forwardEnv``) reach the LDS by buffer loads in 32-pixel tiles (csrc/sgr_common.h: tile32_dma_issue, csrc/sgr_pk.inl:
tile32_dma_issue_vrow).  The second request of a tile carries its +16 rows in the wave-uniform offset, which the buffer range check does not
cover, so on a last tile with ``R*C % 32`` in 1..15 the rows past the grid may be read from beyond the image -- values of masked pixels, which
a parity test cannot see.  Here every env-sized input is a contiguous view at the START of a larger buffer whose tail is NaN: whatever is
read past the end stays inside the allocation, and if any of it reached an output or a gradient the result would differ from the run on
exactly sized tensors (or stop being finite).  Grids with ``R*C % 32`` = 1, 10, 15 and 31, on the 8x16 / 12-lobe and the 16x32 / 24-lobe
kernels."""
import pytest
import torch

pytestmark = pytest.mark.gpu
SG = ("axis", "lamb", "weight")
BRDF = ("albedo", "normal", "rough")
GRIDS = [(3, 11), (6, 7), (11, 13), (7, 9)]            # R*C = 33, 42, 143, 63: R*C % 32 = 1, 10, 15, 31
KERNELS = [(12, 8, 16), (24, 16, 32)]


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


def _poisoned(t):
    """``t`` copied to the start of a buffer with a NaN tail of 32 whole rows of every colour (more than a tile reaches past an image)."""
    tail = 3 * 32 * t.shape[-2] * t.shape[-1]
    buf = torch.full((t.numel() + tail,), float("nan"), device="cuda")
    buf[:t.numel()].copy_(t.reshape(-1))
    return buf, buf[:t.numel()].view(t.shape)


def _run(sgr, inp, cts, ind, R, C, eh, ew, poison):
    env_sized = (lambda t: _poisoned(t)[1]) if poison else (lambda t: t.cuda().clone())
    x = {k: v.cuda() for k, v in inp.items() if k != "env_gt"}
    env_gt = env_sized(inp["env_gt"].cuda())
    out = {}
    layer = sgr.renderingLayer(imWidth=C, imHeight=R, envWidth=ew, envHeight=eh)
    # the fused objective: the ground-truth env stream
    sg = [x[k].clone().requires_grad_(True) for k in SG]
    obj, rerr, cerr, ren, coef = sgr.light_objective(layer, x["albedo"], x["normal"], x["rough"], *sg, x["im"], x["seg"], env_gt, ind, 1.0, 10.0)
    out.update(obj=obj.detach(), rerr=rerr, cerr=cerr, ren=ren, coef=coef)
    out.update({f"obj_g_{k}": g for k, g in zip(SG, torch.autograd.grad(obj, sg))})
    # the fused layer's backward: the env cotangent stream
    xs = {k: x[k].clone().requires_grad_(True) for k in BRDF + SG}
    env, d, s = layer.forwardSG(xs["albedo"], xs["normal"], xs["rough"], xs["axis"], xs["lamb"], xs["weight"], need_env=True)
    ct = [env_sized(cts[0].cuda()), cts[1].cuda(), cts[2].cuda()]
    out.update(env=env.detach(), d=d.detach(), s=s.detach())
    out.update({f"sg_g_{k}": g for k, g in zip(BRDF + SG, torch.autograd.grad([env, d, s], [xs[k] for k in BRDF + SG], grad_outputs=ct))})
    # forwardEnv: the env input stream, forward and backward (the BRDF-map gradients read the env tile by tile)
    if poison:
        buf, env_in = _poisoned(env.detach())
        buf.requires_grad_(True)
        env_in = buf[:env_in.numel()].view(env_in.shape)
    else:
        env_in = env.detach().clone().requires_grad_(True)
    xb = {k: x[k].clone().requires_grad_(True) for k in BRDF}
    d2, s2 = layer.forwardEnv(xb["albedo"], xb["normal"], xb["rough"], env_in)
    out.update(env_d=d2.detach(), env_s=s2.detach())
    g = torch.autograd.grad([d2, s2], [xb[k] for k in BRDF] + [env_in], grad_outputs=[cts[1].cuda(), cts[2].cuda()])
    out.update({f"env_g_{k}": t for k, t in zip(BRDF + ("env",), g)})
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("K,eh,ew", KERNELS, ids=[f"K{k}_{h}x{w}" for k, h, w in KERNELS])
@pytest.mark.parametrize("R,C", GRIDS, ids=[f"{r}x{c}_rc{(r * c) % 32}" for r, c in GRIDS])
def test_ragged_last_tile_ignores_what_lies_past_the_env(sgr, R, C, K, eh, ew):
    from oracle import sg_oracle as O
    bn = 2
    assert sgr.light_objective_supported(K, R, C, eh, ew)
    inp = O.synthetic_inputs(bn, 2 * R, 2 * C, R, C, K, eh, ew, seed=5100 + R * C + K)
    g = torch.Generator().manual_seed(R * C)
    cts = [torch.randn(bn, 3, R, C, eh, ew, generator=g), torch.randn(bn, 3, R, C, generator=g), torch.randn(bn, 3, R, C, generator=g)]
    ind = torch.ones(bn, 1, 1, 1, device="cuda")
    clean = _run(sgr, inp, cts, ind, R, C, eh, ew, poison=False)
    dirty = _run(sgr, inp, cts, ind, R, C, eh, ew, poison=True)
    differ = []
    for k, a in clean.items():
        b = dirty[k]
        assert torch.isfinite(a).all(), (k, "clean run")
        if not (torch.isfinite(b).all() and torch.equal(a, b)):
            differ.append(k)
    print(f"\n{R}x{C} (R*C % 32 = {(R * C) % 32}), K={K}, {eh}x{ew}: NaN tail past the env streams changes", differ or "nothing")
    assert not differ, differ
