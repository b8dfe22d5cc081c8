"""GPU: the training OBJECTIVE at size -- ``light_objective`` = renderErr + 10 reconstErr (wrapperBRDFLight.py:167-207, trainLight.py:237)
at BASELINE config 2 (240x320 -> 120x160, SGNum 12, 8x16) against the reference and the fp64 oracle, not only against itself.

(a) One image against the reference-made fixture g12_cfg2_objective.npz (oracle/make_golden_fullsize.py: the unmodified reference in fp32 and
    fp64, the image of g7), the fused route and the unfused HIP route (forwardSG + render_loss + recon_loss).  The yardstick e_ref is the
    reference's own fp32-vs-fp64 error on each quantity.
(b) All sixteen images of a batch with two env_ind == 0 images, one image without a single segmented pixel and a block of dark ground-truth
    cells, against the fp64 oracle on the GPU: values, the per-image LSregress coefficients, the rendered image and the SG gradients image by
    image.  What only appears at size is in play here: 600 partial tiles per image folded by recon_fold0/1, mask sums over 16 x 19 200 cells x
    128 directions, per-image regressions over 57 600 pixels.
(c) The same batch through ``decoder_outputs=True`` (the heads as the kernels' prologue: sg_bwd_recon_pk_kernel<2,16,2,true,true>).  The
    gradients w.r.t. the sharpness / intensity decoder outputs are compared off the few elements that sit within rounding of an end of the
    heads' [0, 1] clamp, where fp64 is no arbiter (_off_the_head_clamps), and over the whole batch: image by image the fp32 oracle's own
    error on x_weight reaches 1.1e-4 (image 3: next to w = 1 the pre-map tan(pi/2 0.999 w) multiplies the rounding of w by up to 1e3), which
    would put that image's bound above the cap.  The per-image errors are printed.

Every bound is ``tol2`` / ``scalar_close`` (tests/conftest.py) of the yardstick -- e_ref in (a), the fp32 oracle's own error on the same
inputs in (b) and (c) -- and each is printed and asserted to be at most 2e-4, so that an unlucky yardstick cannot loosen a test silently.

The oracle runs image by image: the loss denominators carry no gradient and the LSregress coefficients are per image (oracle/sg_oracle.py:
298-384), so with the batch-global denominators put back in, the gradient of one image's numerators IS that image's share of the batch
gradient."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN_DIR, rel_l2, scalar_close, tol2

pytestmark = pytest.mark.gpu
SG = ("axis", "lamb", "weight")
NAMES6 = ("albedo", "normal", "rough", "axis", "lamb", "weight")
CAP = 2e-4          # no yardstick-derived bound may exceed this
BN, IMH, IMW, R, C, K, EH, EW = 16, 240, 320, 120, 160, 12, 8, 16
ENV_IND0, SEG0, DARK = (3, 10), 6, 12      # images of the batch of (b) / (c) with env_ind == 0, seg == 0, a block of dark env_gt cells


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


def _bound(e_ref, what):
    b = tol2(e_ref)
    assert b <= CAP, (what, "yardstick-derived bound above the cap", b, e_ref)
    return b


def _close(got, ref, e_ref, what):
    """``scalar_close`` for a loss value or a coefficient, its relative bound held to the same cap."""
    assert 2.0 * abs(e_ref) <= CAP * abs(ref), (what, "yardstick-derived bound above the cap", e_ref, ref)
    return scalar_close(got, ref, e_ref)


# --------------------------------------------------------------------------- #
# (a) one image against the reference                                          #
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def g12():
    from oracle import sg_oracle as O
    z = np.load(os.path.join(GOLDEN_DIR, "g12_cfg2_objective.npz"))
    cfg = {k: v for k, v in zip(z["cfg_keys"].tolist(), z["cfg_vals"].tolist())}
    for k in ("bn", "imH", "imW", "R", "C", "K", "eh", "ew", "seed"):
        cfg[k] = int(cfg[k])
    inp = O.synthetic_inputs_np(cfg["bn"], cfg["imH"], cfg["imW"], cfg["R"], cfg["C"], cfg["K"], cfg["eh"], cfg["ew"], seed=cfg["seed"])
    chk = np.array([inp[k].double().sum().item() for k in NAMES6])
    assert np.allclose(chk, z["in_checksums"], rtol=1e-12), ("regenerated inputs differ from the fixture's", chk, z["in_checksums"])
    chk = np.array([inp[k].double().sum().item() for k in ("im", "seg", "env_gt")])
    assert np.allclose(chk, z["in_checksums_loss"], rtol=1e-12), ("regenerated loss inputs differ from the fixture's", chk, z["in_checksums_loss"])
    return z, cfg, inp


def _objective_routes(sgr, layer, x, ind, route):
    """``(total, renderErr, reconstErr, rendered)`` and the SG gradients of ``renderErr + 10 reconstErr`` through one HIP route."""
    sg = [x[k] for k in SG]
    if route == "fused":
        obj, rerr, cerr, ren, _ = sgr.light_objective(layer, x["albedo"], x["normal"], x["rough"], *sg, x["im"], x["seg"], x["env_gt"], ind, 1.0, 10.0)
    else:
        env, d, s = layer.forwardSG(x["albedo"], x["normal"], x["rough"], *sg, need_env=True)
        rerr, ren = sgr.render_loss(d, s, x["im"], x["seg"], layer.imHeight, layer.imWidth)
        cerr = sgr.recon_loss(env, x["env_gt"], x["seg"], ind, layer.imHeight, layer.imWidth)
        obj = rerr + 10.0 * cerr
    grads = torch.autograd.grad(obj, sg)
    return (obj.item(), rerr.item(), cerr.item(), ren.detach()), grads


@pytest.mark.parametrize("route", ["fused", "unfused"])
def test_one_image_objective_vs_reference_fixture(sgr, g12, route):
    z, cfg, inp = g12
    x = {k: v.cuda() for k, v in inp.items()}
    for k in SG:
        x[k].requires_grad_(True)
    layer = sgr.renderingLayer(imWidth=cfg["C"], imHeight=cfg["R"], fov=cfg["fov"], F0=cfg["F0"], envWidth=cfg["ew"], envHeight=cfg["eh"])
    ind = torch.ones(cfg["bn"], 1, 1, 1, device="cuda")
    (tot, rerr, cerr, ren), grads = _objective_routes(sgr, layer, x, ind, route)
    r32, r64 = float(z["ref32_render_err"][0]), float(z["ref64_render_err"][0])
    c32, c64 = float(z["ref32_recon_err"][0]), float(z["ref64_recon_err"][0])
    report = {"renderErr": (abs(rerr - r64) / r64, abs(r32 - r64) / r64), "reconstErr": (abs(cerr - c64) / c64, abs(c32 - c64) / c64)}
    assert _close(rerr, r64, r32 - r64, "renderErr"), (route, "renderErr", rerr, r64, r32)
    assert _close(cerr, c64, c32 - c64, "reconstErr"), (route, "reconstErr", cerr, c64, c32)
    assert _close(tot, r64 + 10.0 * c64, abs(r32 - r64) + 10.0 * abs(c32 - c64), "total"), (route, "total", tot, r64 + 10.0 * c64)
    e_ref = rel_l2(z["ref32_rendered"], z["ref64_rendered"])
    e = rel_l2(ren.cpu(), z["ref64_rendered"])
    report["rendered"] = (e, e_ref)
    assert e <= _bound(e_ref, "rendered"), (route, "rendered", e, e_ref)
    s = int(z["stride_sg"][0])
    for k, g in zip(SG, grads):
        assert torch.isfinite(g).all(), (route, k)
        ref32, ref64 = z["ref32_gtot_" + k], z["ref64_gtot_" + k]
        e_ref = rel_l2(ref32, ref64)
        gs = g[..., ::s, ::s].cpu()
        e64, e32 = rel_l2(gs, ref64), rel_l2(gs, ref32)
        n64 = float(z[f"ref64_gtot_{k}_norm"][0])
        en = abs(g.double().norm().item() - n64) / n64
        report["g_" + k] = (e64, e_ref, e32, en)
        assert e64 <= _bound(e_ref, "g_" + k), (route, k, "vs reference fp64", e64, e_ref)
        assert e32 <= 1e-4, (route, k, "vs reference fp32", e32)
        assert en <= 1e-4, (route, k, "full-tensor norm", en)
    print(f"\nconfig 2, one image, {route} objective vs g12 (error vs ref64, e_ref[, vs ref32, norm]):",
          {k: tuple(f"{v:.2e}" for v in t) for k, t in report.items()})


# --------------------------------------------------------------------------- #
# (b) / (c) sixteen images against the fp64 oracle                             #
# --------------------------------------------------------------------------- #
def _batch_inputs():
    """Config-2 batch with what the objective must get right at size: two images without a ground-truth env (env_ind == 0), one with no
    segmented pixel at all (neither loss sees it: its gradient is exactly zero), and a block of dark ground-truth cells (mean < 1e-3: out of
    the env mask) inside an image that keeps the rest."""
    from oracle import sg_oracle as O
    inp = O.synthetic_inputs(BN, IMH, IMW, R, C, K, EH, EW, seed=20202)
    ind = torch.ones(BN, 1, 1, 1)
    ind[list(ENV_IND0)] = 0.0
    inp["seg"][SEG0] = 0.0
    inp["env_gt"][DARK, :, 30:70, 40:100] = 0.0
    return inp, ind


def _denominators(inp, ind, dtype):
    """The batch-global denominators (no gradient): sum of the pooled segmentation, and the env mask (pooled seg x env_ind x not dark)
    summed over cells -- recomputed from the inputs as wrapperBRDFLight.py:175-192 forms them."""
    seg_s = F.adaptive_avg_pool2d(inp["seg"].to("cuda", dtype), (R, C))
    gt = inp["env_gt"].to("cuda", dtype)
    not_dark = (gt.mean(5).mean(4).mean(1, keepdim=True) > 0.001).to(dtype)
    m = seg_s * ind.to("cuda", dtype) * not_dark
    return max(seg_s.sum().item(), 1e-5), max(m.sum().item(), 1e-5)


def _oracle_per_image(inp, ind, dtype, xs=None, ren_w=1.0, rec_w=10.0):
    """The objective of the whole batch through the oracle, image by image in ``dtype`` on the GPU.  ``xs``: the decoders' last-convolution
    outputs (the heads of models.py:336-346 run first; gradients w.r.t. them), else gradients w.r.t. the SG parameters."""
    from oracle import sg_oracle as O
    Dr, Dc = _denominators(inp, ind, dtype)
    num_r = num_c = den_r = den_c = 0.0
    rendered, coef, grads = [], [], [[], [], []]
    for b in range(BN):
        o = {k: v[b:b + 1].to("cuda", dtype) for k, v in inp.items()}
        if xs is None:
            leaves = [o[k].clone().requires_grad_(True) for k in SG]
            a, l, w = leaves
        else:
            leaves = [t[b:b + 1].to("cuda", dtype).clone().requires_grad_(True) for t in xs]
            a, l, w, _ = O.light_heads(*leaves)
        env, d, s = O.render_from_sg(o["albedo"], o["normal"], o["rough"], a, l, w, EH, EW)
        _, ren, nr, dr = O.render_loss(d, s, o["im"], o["seg"], R, C)
        ib = ind[b:b + 1].to("cuda", dtype)
        _, scaled, nc, dc = O.recon_loss(env, o["env_gt"], o["seg"], ib, R, C)
        obj_b = ren_w * nr / Dr / 3.0 + rec_w * nc / Dc / 3.0 / EW / EH
        for acc, g in zip(grads, torch.autograd.grad(obj_b, leaves)):
            acc.append(g.detach())
        num_r, num_c, den_r, den_c = num_r + nr.item(), num_c + nc.item(), den_r + dr.item(), den_c + dc.item()
        rendered.append(ren.detach())
        e = env.detach().reshape(-1)
        i = e.abs().argmax()
        coef.append((scaled.detach().reshape(-1)[i] / e[i]).item())      # envScale = envmapsPredScaledImage / envmapsPredImage
    # the per-image sums reproduce the batch-global denominators the gradients were formed with
    assert abs(den_r - Dr) <= 1e-9 * Dr + 1e-5 and abs(den_c - Dc) <= 1e-9 * Dc + 1e-5, (den_r, Dr, den_c, Dc)
    rerr, cerr = num_r / Dr / 3.0, num_c / Dc / 3.0 / EW / EH
    return dict(rerr=rerr, cerr=cerr, tot=ren_w * rerr + rec_w * cerr, rendered=torch.cat(rendered), coef=torch.tensor(coef, dtype=torch.float64),
                grads=[torch.cat(g) for g in grads])


@pytest.fixture(scope="module")
def batch():
    return _batch_inputs()


def _off_the_head_clamps(x):
    """Elements of a sharpness / intensity decoder output whose head value clamp(0.5 (1.01 tanh x + 1), 0, 1) (models.py:339-340) lies more
    than 1e-6 from either end of the clamp.  Within a few fp32 ulps of an end the clamp's branch is decided by rounding (the gradient
    passes or is blocked), and next to w = 1 a passed gradient is the largest of the tensor (the pre-map tan(pi/2 0.999 w) has slope 6e5
    there): one element that an fp32 evaluation clamps and fp64 does not is an O(1) share of the tensor's norm.  The fp32 oracle's own
    error is 3.5e-2 on x_weight with them and fp64 is no arbiter there (as on the |N|^2 == 1 kink, fixture g9)."""
    u = 0.5 * (1.01 * torch.tanh(x.double()) + 1.0)
    return ((u - 1.0).abs() > 1e-6) & (u.abs() > 1e-6)


def _check_batch(tag, obj, ren, coef, grads, o64, o32, names, masks=None, per_image=True):
    report = {}
    for k, got, i in (("renderErr", obj[1], "rerr"), ("reconstErr", obj[2], "cerr"), ("total", obj[0], "tot")):
        assert _close(got, o64[i], o32[i] - o64[i], k), (tag, k, got, o64[i], o32[i])
        report[k] = (abs(got - o64[i]) / abs(o64[i]), abs(o32[i] - o64[i]) / abs(o64[i]))
    # the per-image LSregress coefficient of the env reconstruction (envScale): the images outside the env mask have none to compare
    live = [b for b in range(BN) if b not in ENV_IND0 and b != SEG0]
    worst = (0.0, 0.0)
    for b in live:
        c64, c32 = float(o64["coef"][b]), float(o32["coef"][b])
        assert _close(coef[b], c64, c32 - c64, f"envScale {b}"), (tag, "envScale", b, coef[b], c64, c32)
        worst = max(worst, (abs(coef[b] - c64) / c64, abs(c32 - c64) / c64))
    report["envScale"] = worst
    e_ref = rel_l2(o32["rendered"], o64["rendered"])
    e = rel_l2(ren, o64["rendered"])
    report["rendered"] = (e, e_ref)
    assert e <= _bound(e_ref, "rendered"), (tag, "rendered", e, e_ref)
    fails = []
    for i, (k, g, a64, a32) in enumerate(zip(names, grads, o64["grads"], o32["grads"])):
        assert torch.isfinite(g).all(), (tag, k)
        mask = torch.ones_like(g, dtype=torch.bool) if masks is None or masks[i] is None else masks[i].to(g.device).clone()
        per = []
        for b in range(BN):
            if float(a64[b].abs().max()) == 0.0:         # no live pixel, no live env cell: the kernels must produce exact zeros too
                assert float(g[b].abs().max()) == 0.0, (tag, k, b, float(g[b].abs().max()))
                mask[b] = False
                continue
            per.append((rel_l2(g[b][mask[b]], a64[b][mask[b]]), rel_l2(a32[b][mask[b]], a64[b][mask[b]]), b))
        if per_image:
            checks = per
        else:
            checks = [(rel_l2(g[mask], a64[mask]), rel_l2(a32[mask], a64[mask]), "batch")]
        for e, e_ref, b in checks:
            if tol2(e_ref) > CAP or e > tol2(e_ref):
                fails.append((k, b, e, e_ref))
        report[k] = max(checks) if per_image else checks[0] + max(per)
    assert float(o64["grads"][0][SEG0].abs().max()) == 0.0      # the seg == 0 image really has no gradient
    print(f"\n{tag} (error vs fp64 oracle, fp32 oracle's own[, image; worst single image]):",
          {k: tuple(f"{v:.2e}" if isinstance(v, float) else v for v in t) for k, t in report.items()})
    assert not fails, (tag, "(gradient, image, error, e_ref): above max(2 e_ref, 1e-4) or a bound above the cap", fails)


@pytest.mark.timeout(900)
def test_sixteen_images_objective_vs_oracle(sgr, batch):
    inp, ind = batch
    x = {k: v.cuda() for k, v in inp.items()}
    for k in SG:
        x[k].requires_grad_(True)
    layer = sgr.renderingLayer(imWidth=C, imHeight=R, envWidth=EW, envHeight=EH)
    obj, rerr, cerr, ren, coef = sgr.light_objective(layer, x["albedo"], x["normal"], x["rough"], x["axis"], x["lamb"], x["weight"], x["im"], x["seg"],
                                                     x["env_gt"], ind.cuda(), 1.0, 10.0)
    grads = torch.autograd.grad(obj, [x[k] for k in SG])
    o64 = _oracle_per_image(inp, ind, torch.float64)
    o32 = _oracle_per_image(inp, ind, torch.float32)
    _check_batch("config 2, 16 images, fused objective", (obj.item(), rerr.item(), cerr.item()), ren.detach(), coef.reshape(-1).tolist(), grads,
                 o64, o32, tuple("g_" + k for k in SG))


@pytest.mark.timeout(900)
def test_sixteen_images_objective_from_decoder_outputs_vs_oracle(sgr, batch):
    from test_gpu_objective import _decoder_outputs
    inp, ind = batch
    xs = _decoder_outputs(BN, K, R, C, seed=41)
    x = {k: v.cuda() for k, v in inp.items()}
    xd = [t.cuda().requires_grad_(True) for t in xs]
    layer = sgr.renderingLayer(imWidth=C, imHeight=R, envWidth=EW, envHeight=EH)
    obj, rerr, cerr, ren, coef = sgr.light_objective(layer, x["albedo"], x["normal"], x["rough"], *xd, x["im"], x["seg"], x["env_gt"], ind.cuda(),
                                                     1.0, 10.0, decoder_outputs=True)
    grads = torch.autograd.grad(obj, xd)
    o64 = _oracle_per_image(inp, ind, torch.float64, xs)
    o32 = _oracle_per_image(inp, ind, torch.float32, xs)
    masks = [None, _off_the_head_clamps(xs[1]), _off_the_head_clamps(xs[2])]
    print("\nelements within 1e-6 of a head clamp's end, left out of the gradient comparison: x_lamb", int((~masks[1]).sum()), "of", masks[1].numel(),
          ", x_weight", int((~masks[2]).sum()), "of", masks[2].numel(), end="")
    _check_batch("config 2, 16 images, objective from decoder outputs", (obj.item(), rerr.item(), cerr.item()), ren.detach(), coef.reshape(-1).tolist(),
                 grads, o64, o32, ("x_axis", "x_lamb", "x_weight"), masks, per_image=False)
