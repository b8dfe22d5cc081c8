"""The wrappers of the package as autocast test cases, shared by tests/test_gpu_autocast_ops.py (values and gradients on a GPU) and
tests/test_autocast_wrappers.py (dtypes on fake device tensors): per case a callable, its arguments drawn on the CPU in fp32, which of
them require grad and which are parameters that stay fp32.  Shapes: the smallest the operators' own test files use."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN_DIR
from oracle import sg_oracle as O


class Case:
    """``fn(**args)`` -> tensor or (nested) tuple of tensors / None.  ``args``: name -> fp32 / integer CPU tensor (anything else is passed
    as it is); ``grads``: the names that require grad; ``params``: floating arguments that stay fp32 in every variant (weights, biases);
    ``make_module``: builds the ``nn.Module`` that is the callable (on first use, through :meth:`bind`, so that the caller chooses the
    device); its parameters are fp32 leaves too, and their gradients are compared"""

    def __init__(self, fn, args, grads=(), params=(), make_module=None):
        self.fn, self.args, self.grads, self.params, self.make_module, self.module = fn, args, tuple(grads), tuple(params), make_module, None

    def bind(self, place):
        """``place(constructor) -> module on the device``; once per case"""
        if self.make_module is not None and self.module is None:
            self.module = self.fn = place(self.make_module)
        return self


def is_float(t):
    return isinstance(t, torch.Tensor) and t.is_floating_point()


def flatten(out):
    if out is None or isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out for t in flatten(o)]


def rnd(*shape, seed, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def uni(*shape, seed, lo=0.0, hi=1.0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def conv_cases(sgr):
    c = {}
    for pad in ("replicate", "zeros"):
        c[f"encoder_conv-{pad}"] = Case(lambda x, w, b, pad=pad: sgr.encoder_conv(x, w, b, pad), dict(x=rnd(2, 5, 7, 9, seed=1), w=rnd(16, 5, 4, 4, seed=2, scale=0.2), b=rnd(16, seed=3)),
                                        grads=("x", "w", "b"), params=("w", "b"))
    c["light_final_conv"] = Case(sgr.light_final_conv, dict(y=rnd(2, 16, 5, 7, seed=4), weight=rnd(17, 16, 3, 3, seed=5, scale=0.2), bias=rnd(17, seed=6)),
                                 grads=("y", "weight", "bias"), params=("weight", "bias"))
    c["final_conv"] = Case(sgr.final_conv, dict(y=rnd(2, 8, 5, 7, seed=7), weight=rnd(3, 8, 3, 3, seed=8, scale=0.2), bias=rnd(3, seed=9)),
                           grads=("y", "weight", "bias"), params=("weight", "bias"))
    c["group_norm_relu_final_conv"] = Case(lambda x, gw, gb, w, b: sgr.group_norm_relu_final_conv(x, gw, gb, 2, w, b),
                                           dict(x=rnd(2, 8, 5, 7, seed=10), gw=rnd(8, seed=11), gb=rnd(8, seed=12, scale=0.3), w=rnd(3, 8, 3, 3, seed=13, scale=0.2), b=rnd(3, seed=14)),
                                           grads=("x", "gw", "gb", "w", "b"), params=("gw", "gb", "w", "b"))
    return c


def gn_cases(sgr):
    c = {}
    x, w, b, skip = rnd(2, 64, 5, 8, seed=20), rnd(64, seed=21), rnd(64, seed=22, scale=0.3), rnd(2, 7, 6, 8, seed=23)
    c["group_norm_relu_resize"] = Case(lambda x, w, b: sgr.group_norm_relu_resize(x, w, b, 4, (6, 8)), dict(x=x, w=w, b=b), grads=("x", "w", "b"), params=("w", "b"))
    c["group_norm_relu_resize_upcat"] = Case(lambda x, w, b, skip: sgr.group_norm_relu_resize_upcat(x, w, b, 4, skip), dict(x=x, w=w, b=b, skip=skip),
                                             grads=("x", "w", "b", "skip"), params=("w", "b"))
    args = {f"x{d}": rnd(2, 64, 5, 8, seed=24 + d) for d in range(3)}
    args.update({f"w{d}": rnd(64, seed=27 + d) for d in range(3)})
    args.update({f"b{d}": rnd(64, seed=30 + d, scale=0.3) for d in range(3)})
    args["skip"] = skip

    def siblings(x0, x1, x2, w0, w1, w2, b0, b1, b2, skip):      # the TensorList path of the rule
        return sgr.group_norm_relu_resize_upcat_siblings([x0, x1, x2], [w0, w1, w2], [b0, b1, b2], 4, skip)
    c["group_norm_relu_resize_upcat_siblings"] = Case(siblings, args, grads=tuple(args), params=tuple(k for k in args if k[0] in "wb"))
    # fp16 under an fp16 autocast: the same-size stage runs in fp32 there (bf16 stays bf16 and has its own file, tests/test_gpu_gn_stage_bf16.py)
    c["group_norm_relu-fp16"] = Case(lambda x, w, b: sgr.group_norm_relu(x, w, b, 4), dict(x=x, w=w, b=b), grads=("x", "w", "b"), params=("w", "b"))
    c["group_norm_relu_upcat-fp16"] = Case(lambda x, w, b, skip: sgr.group_norm_relu_upcat(x, w, b, 4, skip), dict(x=x, w=w, b=b, skip=rnd(2, 7, 5, 8, seed=33)),
                                           grads=("x", "w", "b", "skip"), params=("w", "b"))
    return c


def brdf_cases(sgr):
    c = {}
    xs = dict(xA=rnd(2, 3, 5, 7, seed=40), xN=rnd(2, 3, 5, 7, seed=41), xR=rnd(2, 3, 5, 7, seed=42), xD=rnd(2, 3, 5, 7, seed=43))
    for unit in (True, False):
        c[f"brdf_heads-unit{int(unit)}"] = Case(lambda xA, xN, xR, xD, unit=unit: sgr.brdf_heads(xA, xN, xR, xD, unit), xs, grads=tuple(xs))
    c["brdf_heads-optional"] = Case(lambda xN, xD: sgr.brdf_heads(None, xN, None, xD), dict(xN=xs["xN"], xD=xs["xD"]), grads=("xN", "xD"))
    for mode in (0, 1, 2, 4):
        c[f"brdf_head-mode{mode}"] = Case(lambda x, mode=mode: sgr.brdf_head(x, mode), dict(x=xs["xA"]), grads=("x",))
    import brdf_input_checker as BI
    z = np.load(os.path.join(GOLDEN_DIR, "g15_brdfin_small.npz"))
    inp = BI.load_inputs(z)
    ein = {k: torch.from_numpy(inp[k]) for k in BI.INPUTS}
    c["brdf_encoder_input"] = Case(lambda **kw: sgr.brdf_encoder_input(*[kw[k] for k in BI.INPUTS]), ein)
    c["brdf_encoder_input-noregress"] = Case(lambda **kw: sgr.brdf_encoder_input(*[kw[k] for k in BI.INPUTS], regress=False), ein)
    # the objectives: 2 images of 6 x 10
    n = rnd(2, 3, 6, 10, seed=51)
    obj = dict(albedoPred=uni(2, 3, 6, 10, seed=50), normalPred=n / n.norm(dim=1, keepdim=True), roughPred=uni(2, 1, 6, 10, seed=52, lo=-1), depthPred=uni(2, 1, 6, 10, seed=53),
               albedoBatch=uni(2, 3, 6, 10, seed=54), normalBatch=F.normalize(rnd(2, 3, 6, 10, seed=55), dim=1), roughBatch=uni(2, 1, 6, 10, seed=56, lo=-1),
               depthBatch=uni(2, 1, 6, 10, seed=57, hi=3.0), segBRDFBatch=(uni(2, 1, 6, 10, seed=58) < 0.8).float(), segAllBatch=uni(2, 1, 6, 10, seed=59))
    preds = ("albedoPred", "normalPred", "roughPred", "depthPred")
    c["brdf_objective"] = Case(lambda **kw: tuple(sgr.brdf_objective(**kw, return_scaled=True)), obj, grads=preds)
    c["brdf_objective-optional"] = Case(lambda normalPred, depthPred, normalBatch, depthBatch, segAllBatch, segDepthBatch: tuple(sgr.brdf_objective(
        None, normalPred, None, depthPred, None, normalBatch, None, depthBatch, None, segAllBatch, depth_offset=0.1, segDepthBatch=segDepthBatch)),
        dict(normalPred=obj["normalPred"], depthPred=obj["depthPred"], normalBatch=obj["normalBatch"], depthBatch=obj["depthBatch"], segAllBatch=obj["segAllBatch"],
             segDepthBatch=(uni(2, 1, 6, 10, seed=60) < 0.7).float()), grads=("normalPred", "depthPred"))
    g = torch.Generator().manual_seed(61)
    pts = lambda: torch.stack([torch.randint(0, 6, (2, 9), generator=g), torch.randint(0, 10, (2, 9), generator=g), torch.randint(0, 6, (2, 9), generator=g),
                               torch.randint(0, 10, (2, 9), generator=g)], dim=2).to(torch.int32)
    c["batch_ranking_loss"] = Case(sgr.batch_ranking_loss, dict(albedoPred=uni(2, 3, 6, 10, seed=62, lo=0.05), eqPoint=pts(), eqWeight=uni(2, 9, seed=63), eqNum=torch.tensor([9, 4], dtype=torch.int32),
                                                                darkerPoint=pts(), darkerWeight=uni(2, 9, seed=64), darkerNum=torch.tensor([7, 0], dtype=torch.int32)), grads=("albedoPred",))
    return c


def bilateral_cases(sgr):
    from test_gpu_bilateral_edges import maps
    c = {}
    for mode, C, (H, W) in ((0, 3, (7, 1)), (2, 1, (2, 2))):      # the tiny maps of tests/test_gpu_bilateral_edges.py, a 3-channel and a 1-channel mode
        image, pred, conf, _ = [torch.from_numpy(a) for a in maps(2, C, H, W, seed=100 * H + W)]
        kw = dict(sgr.BILATERAL_MODES[mode]["grid"], **sgr.BILATERAL_MODES[mode]["bs"])
        c[f"bilateral_solve-mode{mode}"] = Case(lambda image, pred, confidence, kw=kw: sgr.bilateral_solve(image, pred, confidence, **kw), dict(image=image, pred=pred, confidence=conf),
                                                grads=("pred", "confidence"))

        def make_layer(mode=mode):
            torch.manual_seed(70 + mode)
            return sgr.BilateralLayer(mode=mode)
        image, pred, _, _ = [torch.from_numpy(a) for a in maps(2, C, 8, 12, seed=71)]
        feature = torch.from_numpy(maps(2, 3, 8, 12, seed=72)[0])
        c[f"BilateralLayer-mode{mode}"] = Case(None, dict(image=image, feature=feature, pred=pred), grads=("pred",), make_module=make_layer)
    return c


def sg_inputs(K, eh, ew, ratio, R=5, C=7, bn=2, seed=300):
    inp = O.synthetic_inputs(bn, ratio * R, ratio * C, R, C, K, eh, ew, seed=seed + K + ratio)
    inp["seg"][0, :, : max(1, ratio * R // 2)] = 0.0
    ind = torch.ones(bn, 1, 1, 1)
    ind[-1] = 0.0
    inp["ind"] = ind
    return inp


GRIDS = {"k12_8x16": (12, 8, 16), "k24_16x32": (24, 16, 32)}      # at R x C = 5 x 7, which is ragged


def glue_cases(sgr):
    c = {}
    K, R, C = 12, 5, 7
    heads = dict(xAxis=rnd(2, 3 * K, R, C, seed=80), xLamb=rnd(2, K, R, C, seed=81), xWeight=rnd(2, 3 * K, R, C, seed=82))
    c["light_heads"] = Case(lambda **kw: sgr.light_heads(**kw, need_packed=True), heads, grads=tuple(heads))
    n = rnd(2, 3, R, C, seed=84)
    c["light_encoder_input"] = Case(lambda im, albedo, normal, rough, depth: sgr.light_encoder_input(im, albedo, normal, rough, depth, size=(10, 14)),
                                    dict(im=uni(2, 3, R, C, seed=83), albedo=uni(2, 3, R, C, seed=85, lo=0.05), normal=n / n.norm(dim=1, keepdim=True), rough=uni(2, 1, R, C, seed=86, lo=-1),
                                         depth=uni(2, 1, R, C, seed=87, lo=0.1, hi=3.0)))
    c["light_albedo_scale"] = Case(sgr.light_albedo_scale, dict(diffuseScaled=uni(2, 3, R, C, seed=88, hi=2.0), diffuse=uni(2, 3, R, C, seed=89, lo=0.1), specScaled=uni(2, 3, R, C, seed=90, hi=2.0),
                                                                spec=uni(2, 3, R, C, seed=91, lo=0.1), albedoPred=uni(2, 3, R, C, seed=92)))
    a = rnd(2, K, 3, R, C, seed=93)
    packed = torch.cat([(a / a.norm(dim=2, keepdim=True)).reshape(2, 3 * K, R, C), uni(2, K, R, C, seed=94, hi=0.9), uni(2, 3 * K, R, C, seed=95, hi=0.9)], 1)
    c["predToShading"] = Case(lambda pred: sgr.predToShading(pred, envWidth=16, envHeight=8, SGNum=K), dict(pred=packed))
    c["LSregress"] = Case(sgr.LSregress, dict(pred=uni(2, 3, R, C, seed=96), gt=uni(2, 3, R, C, seed=97), origin=uni(2, 3, R, C, seed=98)), grads=("origin",))
    ds = dict(diff=uni(2, 3, R, C, seed=99), spec=uni(2, 3, R, C, seed=100), imOrig=uni(2, 3, R, C, seed=101), diffOrig=uni(2, 3, R, C, seed=102), specOrig=uni(2, 3, R, C, seed=103))
    c["LSregressDiffSpec"] = Case(sgr.LSregressDiffSpec, ds, grads=("diffOrig", "specOrig"))
    return c


def render_cases(sgr):
    c = {}
    for gid, (K, eh, ew) in GRIDS.items():
        sg = ("axis", "lamb", "weight")
        x = sg_inputs(K, eh, ew, 1)
        o2e = sgr.output2env(K, envWidth=ew, envHeight=eh)
        c[f"output2env-{gid}"] = Case(lambda axis, lamb, weight, o2e=o2e: o2e.output2env(axis, lamb, weight), {k: x[k] for k in sg}, grads=sg)
        c[f"fromSGtoIm-{gid}"] = Case(lambda axis, lamb, weight, o2e=o2e: o2e.fromSGtoIm(axis, lamb, weight), dict(axis=x["axis"], lamb=x["lamb"] * 20.0, weight=x["weight"] * 3.0), grads=sg)
        layer = sgr.renderingLayer(imWidth=7, imHeight=5, envWidth=ew, envHeight=eh)
        mod = sgr.renderLayer(imWidth=7, imHeight=5, envWidth=ew, envHeight=eh)
        maps = ("albedo", "normal", "rough")
        for ratio in (1, 2, 3):      # 3x: torch's pooling in the wrapper, before the operator
            x = sg_inputs(K, eh, ew, ratio)
            six = {k: x[k] for k in maps + sg}
            c[f"forwardSG-{gid}-{ratio}x"] = Case(lambda layer=layer, **kw: layer.forwardSG(*[kw[k] for k in maps + sg], need_env=True), six, grads=maps + sg)
            env = uni(2, 3, 5, 7, eh, ew, seed=110 + ratio, hi=2.0)
            c[f"renderLayer.forward-{gid}-{ratio}x"] = Case(lambda mod=mod, **kw: mod(*[kw[k] for k in maps + ("envmap",)]), dict({k: x[k] for k in maps}, envmap=env), grads=maps + ("envmap",))
            d, s = uni(2, 3, 5, 7, seed=120, hi=0.8), uni(2, 3, 5, 7, seed=121, hi=0.5)
            c[f"render_loss-{gid}-{ratio}x"] = Case(lambda diffuse, spec, im, seg: sgr.render_loss(diffuse, spec, im, seg, 5, 7), dict(diffuse=d, spec=s, im=x["im"], seg=x["seg"]), grads=("diffuse", "spec"))
            c[f"recon_loss-{gid}-{ratio}x"] = Case(lambda env, env_gt, seg, ind: sgr.recon_loss(env, env_gt, seg, ind, 5, 7, return_scaled=True),
                                                   dict(env=env, env_gt=x["env_gt"], seg=x["seg"], ind=x["ind"]), grads=("env",))
        x = sg_inputs(K, eh, ew, 2)
        c[f"render_from_sg-{gid}"] = Case(lambda **kw: sgr.render_from_sg(*[kw[k] for k in maps + sg], envWidth=ew, envHeight=eh), {k: x[k] for k in maps + sg}, grads=maps + sg)
    return c


OBJ_ARGS = ("albedo", "normal", "rough", "axis", "lamb", "weight", "im", "seg", "env_gt", "ind")


def objective_case(sgr, K, eh, ew, ratio, **flags):
    x = sg_inputs(K, eh, ew, ratio)
    if flags.get("decoder_outputs"):
        x["axis"], x["lamb"], x["weight"] = rnd(2, 3 * K, 5, 7, seed=130), rnd(2, K, 5, 7, seed=131), rnd(2, 3 * K, 5, 7, seed=132)
    layer = sgr.renderingLayer(imWidth=7, imHeight=5, envWidth=ew, envHeight=eh)
    grads = ("axis", "lamb", "weight") + (("albedo", "normal", "rough") if flags.get("brdf_grads") else ())
    return Case(lambda **kw: sgr.light_objective(layer, *[kw[k] for k in OBJ_ARGS], 1.0, 10.0, **flags), {k: x[k] for k in OBJ_ARGS}, grads=grads)


def objective_cases(sgr):
    c = {}
    for ratio in (1, 2, 3):
        c[f"light_objective-{ratio}x"] = objective_case(sgr, 12, 8, 16, ratio)
        c[f"light_objective-brdf_grads-{ratio}x"] = objective_case(sgr, 12, 8, 16, ratio, brdf_grads=True)
    c["light_objective-decoder_outputs"] = objective_case(sgr, 12, 8, 16, 2, decoder_outputs=True)
    c["light_objective-decoder_outputs-brdf_grads"] = objective_case(sgr, 12, 8, 16, 2, decoder_outputs=True, brdf_grads=True)
    c["light_objective-k24_16x32"] = objective_case(sgr, 24, 16, 32, 2)
    c["light_objective-unfused-k30"] = objective_case(sgr, 30, 8, 16, 3)
    return c


FAMILIES = dict(conv=conv_cases, gn=gn_cases, brdf=brdf_cases, bilateral=bilateral_cases, glue=glue_cases, render=render_cases, objective=objective_cases)
CASE_IDS = {
    "conv": ["encoder_conv-replicate", "encoder_conv-zeros", "light_final_conv", "final_conv", "group_norm_relu_final_conv"],
    "gn": ["group_norm_relu_resize", "group_norm_relu_resize_upcat", "group_norm_relu_resize_upcat_siblings", "group_norm_relu-fp16", "group_norm_relu_upcat-fp16"],
    "brdf": ["brdf_heads-unit1", "brdf_heads-unit0", "brdf_heads-optional", "brdf_head-mode0", "brdf_head-mode1", "brdf_head-mode2", "brdf_head-mode4", "brdf_encoder_input",
             "brdf_encoder_input-noregress", "brdf_objective", "brdf_objective-optional", "batch_ranking_loss"],
    "bilateral": ["bilateral_solve-mode0", "bilateral_solve-mode2", "BilateralLayer-mode0", "BilateralLayer-mode2"],
    "glue": ["light_heads", "light_encoder_input", "light_albedo_scale", "predToShading", "LSregress", "LSregressDiffSpec"],
    "render": [f"{n}-{g}" for g in GRIDS for n in ("output2env", "fromSGtoIm", "render_from_sg")]
    + [f"{n}-{g}-{r}x" for g in GRIDS for r in (1, 2, 3) for n in ("forwardSG", "renderLayer.forward", "render_loss", "recon_loss")],
    "objective": [f"light_objective-{r}x" for r in (1, 2, 3)] + [f"light_objective-brdf_grads-{r}x" for r in (1, 2, 3)]
    + ["light_objective-decoder_outputs", "light_objective-decoder_outputs-brdf_grads", "light_objective-k24_16x32", "light_objective-unfused-k30"],
}
_BUILT = {}


def get_case(sgr, family, name):
    if family not in _BUILT:
        _BUILT[family] = FAMILIES[family](sgr)
        assert sorted(_BUILT[family]) == sorted(CASE_IDS[family]), sorted(set(_BUILT[family]) ^ set(CASE_IDS[family]))
    return _BUILT[family][name]


