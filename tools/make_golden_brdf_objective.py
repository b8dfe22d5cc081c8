"""Golden vectors for the BRDF-stage objectives, produced by the UNMODIFIED reference (wrapperBRDF.py, wrapperNYU.py, models.py).
TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout); never runs on the GPU machine:

    python tools/make_golden_brdf_objective.py        # writes tests/golden/g14_brdfobj_<case>.npz

The reference modules are imported where they lie.  ``wrapperBRDF.wrapperBRDF`` and ``wrapperNYU.wrapperNYU`` run as they are, with
stub networks that return fixed seeded tensors and ``torch.Tensor.cuda`` rebound to the identity on a GPU-less machine (SURVEY.md
section 8c); wrapperNYU.py ends in a dangling line continuation and is compiled at run time without it (``load_wrapper_nyu``).  ``wrapperIIW.wrapperIIW`` cannot run (it uses ``np.long``, which current numpy lacks), so the tool calls
``models.BatchRankingLoss`` per image with the slices of wrapperIIW.py:90-100 and applies the two divisions of :108-109 itself.

Each run is made twice, in fp64 (the arbiter) and in fp32; per value and per gradient array the file holds both and ``e_ref_*`` = the
distance between them (absolute for the scalars, rel-L2 for the arrays).  The predictions stored are the tensors the wrappers call
``albedoPred`` ... ``depthPred`` (for NYU the depth BEFORE its LSregress, wrapperNYU.py:97: the stub decoders return tensors of the
ground truth's size, so that the bilinear resize of :94-95 is the identity, and ``0.5 * (x + 1)`` is formed here in the same dtype).
The gradients are those of ``total = sum_i w_i Err_i`` (trainBRDF.py:285) with respect to those predictions."""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("SGR_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
MAX_BYTES = 1 << 20
WEIGHTS = (6.0, 1.0, 0.5, 0.5)      # (4 * albeW, normW, rougW, deptW) at the defaults of trainBRDF.py:36-39,285


def reference():
    if not os.path.isfile(os.path.join(REF, "wrapperBRDF.py")):
        raise SystemExit("reference not mounted")
    if REF not in sys.path:
        sys.path.insert(0, REF)
    if not torch.cuda.is_available():
        torch.Tensor.cuda = lambda self, *a, **k: self      # the wrappers call .cuda() unconditionally
    import models
    import wrapperBRDF
    return models, wrapperBRDF, load_wrapper_nyu()


def load_wrapper_nyu():
    """wrapperNYU.py does not import as it lies: its return statement ends in a line-continuation backslash followed by the end of the file
    (wrapperNYU.py:120-121).  The file is read where it lies and compiled at run time with that one trailing character dropped, which
    closes the statement after ``[depthPred, depthErr]``; every other character runs as written."""
    path = os.path.join(REF, "wrapperNYU.py")
    src = open(path).read().rstrip()
    try:
        compile(src, path, "exec")
    except SyntaxError:
        assert src.endswith("\\"), "wrapperNYU.py fails to compile for another reason than its trailing backslash"
        src = src[:-1]
    mod = types.ModuleType("wrapperNYU")
    mod.__file__ = path
    exec(compile(src, path, "exec"), mod.__dict__)
    return mod


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.abs(a).max())


def save(name, blob):
    path = os.path.join(OUT, f"g14_brdfobj_{name}.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    e = {k[6:]: f"{float(v):.1e}" for k, v in blob.items() if k.startswith("e_ref_")}
    print(f"{name:14s} {size / 1024:7.1f} KiB  e_ref {e}")


class Stub:
    """a network that ignores its inputs and returns what it was given"""

    def __init__(self, *out):
        self.out = out

    def __call__(self, *args):
        return self.out[0] if len(self.out) == 1 else self.out


def decoder_output(pred, dtype, half):
    """the decoder output x whose wrapper-side activation gives ``pred``: x = 2 pred - 1 for the 0.5 (x + 1) heads, pred itself otherwise"""
    x = torch.from_numpy(pred).to(dtype)
    return (2.0 * x - 1.0 if half else x).requires_grad_(True)


def run_synthetic(W, inp, dtype):
    """wrapperBRDF.wrapperBRDF on the stub networks -> values, the predictions it returns, gradients of the weighted total"""
    t = lambda k: torch.from_numpy(inp[k]).to(dtype)
    data = dict(albedo=t("albedo"), normal=t("normal"), rough=t("rough"), depth=t("depth"), segArea=t("segArea"), segEnv=t("segEnv"), segObj=t("segObj"),
                im=torch.zeros(inp["albedo"].shape, dtype=dtype))
    opt = types.SimpleNamespace(cascadeLevel=0)
    x = [decoder_output(inp[k], dtype, h) for k, h in (("albedoPred", True), ("normalPred", False), ("roughPred", False), ("depthPred", True))]
    (aP, aE), (nP, nE), (rP, rE), (dP, dE) = W.wrapperBRDF(data, opt, Stub(*([None] * 6)), Stub(x[0]), Stub(x[1]), Stub(x[2]), Stub(x[3]))
    total = WEIGHTS[0] * aE + WEIGHTS[1] * nE + WEIGHTS[2] * rE + WEIGHTS[3] * dE
    g = torch.autograd.grad(total, [aP, nP, rP, dP])
    vals = dict(total=total, albedoErr=aE, normalErr=nE, roughErr=rE, depthErr=dE)
    return ({k: v.item() for k, v in vals.items()}, dict(albedoPred=aP, normalPred=nP, roughPred=rP, depthPred=dP),
            dict(g_albedo=g[0], g_normal=g[1], g_rough=g[2], g_depth=g[3]))


def run_nyu(N, inp, dtype):
    t = lambda k: torch.from_numpy(inp[k]).to(dtype)
    data = dict(normal=t("normal"), depth=t("depth"), segNormal=t("segNormal"), segDepth=t("segDepth"), im=torch.zeros(inp["normal"].shape, dtype=dtype))
    opt = types.SimpleNamespace(cascadeLevel=0)
    xn, xd = decoder_output(inp["normalPred"], dtype, False), decoder_output(inp["depthPred"], dtype, True)
    dummy = torch.zeros(1, dtype=dtype)
    res = N.wrapperNYU(data, opt, Stub(*([None] * 6)), Stub(dummy), Stub(xn), Stub(dummy), Stub(xd))
    nE, angle, dE = res[1][1], res[1][2], res[3][1]
    total = WEIGHTS[1] * nE + WEIGHTS[3] * dE
    g = torch.autograd.grad(total, [xn, xd])
    depth_pred = 0.5 * (xd.detach() + 1)      # what wrapperNYU.py:92 forms; its return value is already scaled (:97-98)
    # d depthPred / d x = 0.5 exactly, and the identity resize passes gradients through unchanged
    return (dict(total=total.item(), normalErr=nE.item(), depthErr=dE.item(), angleMean=angle.item()), dict(normalPred=xn.detach(), depthPred=depth_pred),
            dict(g_normal=g[0], g_depth=2.0 * g[1]))


def finish(name, inp, r64, r32, extra=None):
    v64, p64, g64 = r64
    v32, p32, g32 = r32
    blob = dict(inp)
    for k, v in p32.items():      # the predictions as the wrapper returns them (fp32 run), and they must be what was asked for to the last bit
        got = v.detach().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, inp[k]), k
        blob[k] = got
    for k in v64:
        blob["ref64_" + k], blob["ref32_" + k], blob["e_ref_" + k] = np.float64(v64[k]), np.float32(v32[k]), np.float64(abs(v32[k] - v64[k]))
    for k in g64:
        blob["ref64_" + k], blob["ref32_" + k] = g64[k].detach().numpy(), g32[k].detach().numpy()
        blob["e_ref_" + k] = np.float64(rel(blob["ref32_" + k], blob["ref64_" + k]))
    blob["weights"] = np.array(WEIGHTS, np.float64)
    blob.update(extra or {})
    save(name, blob)


def q20(p):
    """multiples of 2^-20 in (0, 1): then 2 p - 1 and 0.5 ((2 p - 1) + 1) are exact in fp32, so the fp32 and the fp64 run of a wrapper see
    the same ``albedoPred`` / ``depthPred`` behind their 0.5 (decoder + 1)"""
    return (np.maximum(np.round(np.asarray(p, np.float64) * 2 ** 20), 1.0) / 2 ** 20).astype(np.float32)


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def synthetic_inputs(rng, B, H, W, soft=False, clip=False):
    f = lambda *s: rng.random(s).astype(np.float32)
    inp = dict(albedo=f(B, 3, H, W), normal=unit(rng.standard_normal((B, 3, H, W))).astype(np.float32), rough=f(B, 1, H, W),
               depth=(0.5 + 4.0 * f(B, 1, H, W)), albedoPred=q20(0.02 + 0.96 * f(B, 3, H, W)),
               normalPred=unit(rng.standard_normal((B, 3, H, W))).astype(np.float32), roughPred=(2.0 * f(B, 1, H, W) - 1.0),
               depthPred=q20(0.05 + 0.9 * f(B, 1, H, W)))
    if soft:      # fractional masks; the area mask overlaps the object mask (segAll = segArea + segObj stays within [0, 1])
        inp["segObj"] = q20(0.6 * f(B, 1, H, W))      # multiples of 2^-20: their sum is exact in fp32, so both runs of the wrapper see one segAll
        inp["segArea"] = q20(0.4 * f(B, 1, H, W))
    else:         # the data loader's masks: objects Bernoulli, the area light on a disjoint part of what is left
        obj = rng.random((B, 1, H, W)) < 0.7
        inp["segObj"] = obj.astype(np.float32)
        inp["segArea"] = (~obj & (rng.random((B, 1, H, W)) < 0.5)).astype(np.float32)
    inp["segEnv"] = (1.0 - np.minimum(inp["segObj"] + inp["segArea"], 1.0)).astype(np.float32)
    if clip:      # ground truth brighter than the prediction by a factor that saturates: the regression scales the prediction past 1
        inp["albedo"] = np.minimum(1.7 * inp["albedoPred"], 1.0).astype(np.float32) * (0.9 + 0.1 * f(B, 3, H, W))
    return inp


def masks_of(inp):
    return dict(segBRDF=inp["segObj"], segAll=(torch.from_numpy(inp["segArea"]) + torch.from_numpy(inp["segObj"])).numpy())      # wrapperBRDF.py:30-31, in fp32


def synthetic_case(W, name, B, H, Wd, seed, soft=False, clip=False, coefclamp=False):
    rng = np.random.default_rng(seed)
    inp = synthetic_inputs(rng, B, H, Wd, soft, clip)
    if coefclamp:
        inp["albedoPred"][0] = q20(inp["albedoPred"][0] * 1e-4)      # <p, g> / max(<p, p>, 1e-5) far above 1e3
        inp["segObj"][1] = 0.0                        # an image without object pixels: 0 / max(0, 1e-5) -> the 1e-3 floor
    r64, r32 = run_synthetic(W, inp, torch.float64), run_synthetic(W, inp, torch.float32)
    m = masks_of(inp)
    # reference-only conditions, from the reference's own regression (models.LSregress on the wrapper's arguments, fp64)
    import models
    aP, sB, A = [torch.from_numpy(x).double() for x in (inp["albedoPred"], m["segBRDF"], inp["albedo"])]
    scaled = models.LSregress(aP * sB.expand_as(aP), (sB * A) * sB.expand_as(aP), aP)
    coef = (scaled.flatten(1)[:, 0] / aP.flatten(1)[:, 0]).numpy()
    on = (sB.expand_as(aP) > 0).numpy()
    prod = scaled.numpy()[on]
    frac = float((prod > 1).mean())
    kink = float(min(np.abs(prod).min(), np.abs(prod - 1).min()))
    print(f"  {name}: albedo coefficients {np.round(coef, 4)}  clipped share {frac:.3f}  distance to the clamp's kinks {kink:.2e}")
    if clip:
        assert 0.05 <= frac <= 0.5, frac
    assert kink > 1e-6, kink
    if coefclamp:
        assert abs(coef[0] - 1e3) < 1e-6 and abs(coef[1] - 1e-3) < 1e-9, coef
    finish(name, dict(inp, **m), r64, r32, dict(depth_offset=np.float64(1.0), clipped_share=np.float64(frac)))


def nyu_case(N, name, B, H, Wd, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.random(s).astype(np.float32)
    inp = dict(normal=unit(rng.standard_normal((B, 3, H, Wd))).astype(np.float32), depth=0.5 + 4.0 * f(B, 1, H, Wd),
               normalPred=unit(rng.standard_normal((B, 3, H, Wd)) + 0.0).astype(np.float32), depthPred=q20(0.05 + 0.9 * f(B, 1, H, Wd)),
               segNormal=(rng.random((B, 1, H, Wd)) < 0.8).astype(np.float32), segDepth=(rng.random((B, 1, H, Wd)) < 0.6).astype(np.float32))
    inp["normalPred"][:, :, : H // 2] = unit(inp["normal"][:, :, : H // 2] + 0.3 * rng.standard_normal((B, 3, H // 2, Wd))).astype(np.float32)      # small angles too
    r64, r32 = run_nyu(N, inp, torch.float64), run_nyu(N, inp, torch.float32)
    finish(name, dict(inp, segAll=inp["segNormal"]), r64, r32, dict(depth_offset=np.float64(0.1)))


def run_ranking(M, inp, dtype):
    """wrapperIIW.py:88-109 with np.int64 where it says np.long: per image the slices of :90-100, models.BatchRankingLoss, then :108-109"""
    albedo = torch.from_numpy(inp["albedoPred"]).to(dtype).requires_grad_(True)
    eq_loss, darker_loss = 0, 0
    for m in range(albedo.size(0)):
        ne, nd = int(inp["eqNum"][m]), int(inp["darkerNum"][m])
        e, d = M.BatchRankingLoss(albedo[m, :], inp["eqPoint"][m, :].astype(np.int64)[0:ne, :], inp["eqWeight"][m, :].astype(np.float32)[0:ne],
                                  inp["darkerPoint"][m, :].astype(np.int64)[0:nd, :], inp["darkerWeight"][m, :].astype(np.float32)[0:nd])
        eq_loss += e
        darker_loss += d
    eq_loss = eq_loss / max(albedo.size(0), 1e-5)
    darker_loss = darker_loss / max(albedo.size(0), 1e-5)
    ge, = torch.autograd.grad(eq_loss, [albedo], retain_graph=True)
    gd, = torch.autograd.grad(darker_loss, [albedo])
    return dict(eqLoss=eq_loss.item(), darkerLoss=darker_loss.item()), dict(albedoPred=albedo), dict(g_eq=ge, g_darker=gd)


def ranking_case(M, name, B, H, Wd, N, seed):
    rng = np.random.default_rng(seed)
    inp = dict(albedoPred=(0.02 + 0.96 * rng.random((B, 3, H, Wd))).astype(np.float32))
    hot = np.stack([rng.integers(0, H, 24), rng.integers(0, Wd, 24)], 1)      # judgements drawn from 24 pixels: many repeats
    for kind, nums in (("eq", (25, N, 7)), ("darker", (30, 12, N))):
        pick = lambda: hot[rng.integers(0, len(hot), (B, N))]
        point = np.concatenate([pick(), pick()], -1).astype(np.int32)                 # (r1, c1, r2, c2)
        weight = (0.1 + rng.random((B, N))).astype(np.float32)
        num = np.array(nums[:B], np.int32)
        for m in range(B):      # garbage in the padding: out-of-range coordinates and absurd weights
            point[m, num[m]:] = rng.integers(-10 ** 6, 10 ** 6, (N - num[m], 4))
            weight[m, num[m]:] = 1e30
        inp.update({kind + "Point": point, kind + "Weight": weight, kind + "Num": num})
    # reference-only condition: no darker judgement within 1e-4 of the hinge (fp64, own arithmetic on the stored inputs)
    rho = np.log(inp["albedoPred"].astype(np.float64).mean(1) + 0.001)
    gap = min(np.abs(rho[m, p[:, 2], p[:, 3]] - rho[m, p[:, 0], p[:, 1]] + 0.5).min() for m in range(B) for p in [inp["darkerPoint"][m, :inp["darkerNum"][m]]])
    assert gap > 1e-4, gap
    live = sum(int((rho[m, p[:, 2], p[:, 3]] - rho[m, p[:, 0], p[:, 1]] + 0.5 > 0).sum()) for m in range(B) for p in [inp["darkerPoint"][m, :inp["darkerNum"][m]]])
    print(f"  {name}: distance to the hinge {gap:.2e}, {live} darker judgements active of {int(inp['darkerNum'].sum())}")
    r64, r32 = run_ranking(M, inp, torch.float64), run_ranking(M, inp, torch.float32)
    finish(name, inp, r64, r32, dict(tau=np.float64(0.5)))


def main():
    M, W, N = reference()
    synthetic_case(W, "syn_small", 2, 24, 32, 1401)
    synthetic_case(W, "syn_clip", 2, 24, 32, 1402, clip=True)
    synthetic_case(W, "syn_softmask", 2, 24, 32, 1403, soft=True)
    synthetic_case(W, "syn_coefclamp", 3, 24, 32, 1404, coefclamp=True)
    synthetic_case(W, "syn_odd", 3, 30, 41, 1405)
    nyu_case(N, "nyu_small", 2, 24, 32, 1406)
    ranking_case(M, "rank_small", 3, 24, 32, 40, 1407)


if __name__ == "__main__":
    main()
