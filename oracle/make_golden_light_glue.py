"""Golden vectors for the light-side glue, in fp32 AND fp64, produced by the UNMODIFIED reference.  TEST INFRASTRUCTURE ONLY --
authoring container (needs the reference mounted, see oracle/ref_import.py):

    python -m oracle.make_golden_light_glue        # writes tests/golden/g18_lightglue_{shading,scale,regress,encoder}.npz

A sibling of make_golden_shading.py / make_golden_wrapper.py (whose g5_* / g6_* files stay as they are):

  shading   ``utils.predToShading`` (utils.py:156-195) at SGNum 13 and 24 (the kernels' second lobe-count instantiation), SGNum 1, the
            8x16 and 16x32 direction grids, a 5x13 and a 1x1 cell grid.
  scale     the ``cLight / cAlbedo`` expressions of testReal.py:421-432, verbatim, on fp32 tensors and on the same tensors cast to
            fp64, once per branch (cSpec < 1e-3, the clip at 1e-3, the clip at 1 / max, no clip) at n = 576 and once at
            n = 3 x 74 x 74 = 16 428 (values on a short dyadic grid there, so that the file stays small).
  regress   ``models.LSregressDiffSpec`` (models.py:23-84) and ``models.LSregress`` (models.py:7-21) in both precisions on the branch
            cases of tests/light_glue_checker.py: the scaled outputs with ``origin`` = the inputs (the testReal.py:413-417 call), and
            for ``LSregress`` the coefficient itself as well (``origin`` = ones).
  encoder   the reference ``wrapperBRDFLight`` with every network ``.double()``, bn = 2 at 32x48, the light encoder's input captured
            by a forward pre-hook (wrapperBRDFLight.py:138-156) on an index lattice, and the same with fp32 networks.  Forward hooks on
            the four BRDF decoders put their outputs on the dyadic grid k / 2048 - 1 (exact in both precisions, so that both runs
            normalise and resize IDENTICAL maps and the stored fp32 inputs are exact) and make image 1's raw albedo all zero, so that
            the 1e-10 floor of :141 is live.  The wrapper itself runs as written; the run is abandoned once the pre-hook has fired."""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

from oracle import ref_import as RI
from oracle.make_golden_shading import reference_utils
from oracle import make_golden_wrapper as MW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import light_glue_checker as LG  # noqa: E402  (the shared, seeded test inputs live there)

SHADING_CASES = (("k13", 13, 5, 13, 8, 16, 51), ("k24w", 24, 5, 13, 16, 32, 52), ("k24", 24, 5, 13, 8, 16, 53), ("k24one", 24, 1, 1, 8, 16, 54),
                 ("k1", 1, 5, 13, 8, 16, 55), ("k1one", 1, 1, 1, 16, 32, 56))
#              tag      cd      cs     albedo gain   n-shape
SCALE_CASES = (("nospec", 0.75, 2.5e-4, 1.0, (3, 12, 16)), ("clip_lo", 1e-3, 4.0, 1.0, (3, 12, 16)), ("clip_hi", 2.0, 0.5, 1.0, (3, 12, 16)),
               ("noclip", 0.3, 1.5, 1.0, (3, 12, 16)), ("clip_hi_dark", 2.0, 0.125, 0.125, (3, 12, 16)), ("big", 0.375, 1.5, 1.0, (3, 74, 74)))
DIFFSPEC_FIXTURE = [(k, 12, 16, 300 + i) for i, k in enumerate(LG.DIFFSPEC_BRANCH_CASES + ("cd_0001",))] + [("regular", 1, 1, 350)]
LSREGRESS_FIXTURE = [(k, 3 * 12 * 16, 400 + i) for i, k in enumerate(("regular", "clamp_lo", "clamp_hi", "floor"))]

LATTICE_ROWS = sorted(set(range(0, 480, 17)) | {0, 1, 478, 479})
LATTICE_COLS = sorted(set(range(0, 640, 13)) | {0, 1, 638, 639})


def shading_blob(U):
    blob = {}
    for tag, K, R, C, eh, ew, seed in SHADING_CASES:
        g = torch.Generator().manual_seed(seed)
        a = torch.randn(1, K, 3, R, C, generator=g)
        a = a / a.norm(dim=2, keepdim=True)
        pred = torch.cat([a.reshape(1, 3 * K, R, C), torch.rand(1, K, R, C, generator=g), torch.rand(1, 3 * K, R, C, generator=g)], 1).numpy()
        blob[f"{tag}_cfg"] = np.array([K, R, C, eh, ew])
        blob[f"{tag}_pred"] = pred
        blob[f"{tag}_ref32"] = U.predToShading(pred.copy(), envWidth=ew, envHeight=eh, SGNum=K).astype(np.float32)
        blob[f"{tag}_ref64"] = U.predToShading(pred.astype(np.float64), envWidth=ew, envHeight=eh, SGNum=K)
    blob["tags"] = np.array([c[0] for c in SHADING_CASES])
    return blob


def scale_expressions(diffusePredNew, diffusePred, specularPredNew, specularPred, albedoPreds):
    """testReal.py:421-429, verbatim"""
    cDiff, cSpec = (torch.sum(diffusePredNew) / torch.sum(diffusePred)).data.item(), ((torch.sum(specularPredNew)) / (torch.sum(specularPred))).data.item()
    if cSpec < 1e-3:
        cAlbedo = 1 / albedoPreds[-1].max().data.item()
        cLight = cDiff / cAlbedo
    else:
        cLight = cSpec
        cAlbedo = cDiff / cLight
        cAlbedo = np.clip(cAlbedo, 1e-3, 1 / albedoPreds[-1].max().data.item())
        cLight = cDiff / cAlbedo
    return np.array([cLight, cAlbedo, cDiff, cSpec], dtype=np.float64)


def scale_blob():
    blob = {}
    for j, (tag, cd, cs, gain, shape) in enumerate(SCALE_CASES):
        g = torch.Generator().manual_seed(500 + j)
        if tag == "big":      # k / 256: the products with the dyadic cd, cs are exact, and the arrays deflate to about a byte per value
            q = lambda *s: (torch.randint(1, 256, s, generator=g).float() / 256.0)
        else:
            q = lambda *s: torch.rand(*s, generator=g)
        d, s = q(1, *shape), q(1, *shape)
        albedo = q(1, shape[0], 2 * shape[1], 2 * shape[2]) * gain
        dNew, sNew = d * cd, s * cs
        for k, v in (("diffuse", d), ("spec", s), ("diffuseNew", dNew), ("specNew", sNew), ("albedo", albedo)):
            blob[f"{tag}_{k}"] = v.numpy()
        blob[f"{tag}_ref32"] = scale_expressions(dNew, d, sNew, s, [albedo])
        blob[f"{tag}_ref64"] = scale_expressions(dNew.double(), d.double(), sNew.double(), s.double(), [albedo.double()])
        print(tag, "fp32", blob[f"{tag}_ref32"], "fp64", blob[f"{tag}_ref64"])
    blob["tags"] = np.array([c[0] for c in SCALE_CASES])
    return blob


def regress_blob(M):
    blob = {}
    tags = []
    for kind, R, C, seed in DIFFSPEC_FIXTURE:
        tag = f"ds_{kind}_{R}x{C}"
        tags.append(tag)
        diff, spec, im = LG.diffspec_batch((kind,), R, C, seed)
        blob[f"{tag}_diff"], blob[f"{tag}_spec"], blob[f"{tag}_im"] = diff.numpy(), spec.numpy(), im.numpy()
        for name, dt in (("32", torch.float32), ("64", torch.float64)):
            d, s, i = diff.to(dt), spec.to(dt), im.to(dt)
            dS, sS = M.LSregressDiffSpec(d, s, i, d, s)
            blob[f"{tag}_diffScaled{name}"], blob[f"{tag}_specScaled{name}"] = dS.numpy(), sS.numpy()
        print(tag, [float(blob[f"{tag}_{k}Scaled64"].sum() / blob[f"{tag}_{k}"].astype(np.float64).sum()) for k in ("diff", "spec")])
    blob["ds_tags"] = np.array(tags)
    tags = []
    for kind, n, seed in LSREGRESS_FIXTURE:
        tag = f"ls_{kind}"
        tags.append(tag)
        pred, gt = [t.reshape(1, 3, 12, 16) for t in LG.lsregress_case(kind, n, seed)]
        blob[f"{tag}_pred"], blob[f"{tag}_gt"] = pred.numpy(), gt.numpy()
        for name, dt in (("32", torch.float32), ("64", torch.float64)):
            p, t = pred.to(dt), gt.to(dt)
            blob[f"{tag}_scaled{name}"] = M.LSregress(p, t, p).numpy()
            blob[f"{tag}_coef{name}"] = np.array([M.LSregress(p, t, torch.ones_like(p))[0, 0, 0, 0].item()], dtype=np.float64)
        print(tag, blob[f"{tag}_coef32"], blob[f"{tag}_coef64"])
    blob["ls_tags"] = np.array(tags)
    return blob


class _Captured(Exception):
    pass


def encoder_run(dtype, replay=None):
    """-> (light encoder input, dict of the four decoder outputs as the wrapper saw them)"""
    M = RI.models()
    W = RI.wrapper_brdf_light()
    cfg = dict(bn=2, imH=32, imW=48, R=16, C=24, seed=61, block=1, stride=1)
    nets = MW.build_nets(M, cfg["seed"])
    for n in nets.values():
        n.to(dtype)
    batch, _ = MW.synthetic_batch(cfg)
    batch = {k: v.to(dtype) for k, v in batch.items()}
    opt = types.SimpleNamespace(cascadeLevel=0, imHeight=cfg["imH"], imWidth=cfg["imW"], envRow=cfg["R"], envCol=cfg["C"],
                                envHeight=MW.EH, envWidth=MW.EW, SGNum=MW.K)
    o2e, rl = RI.make_layers(MW.K, cfg["R"], cfg["C"], MW.EH, MW.EW, dtype=dtype)
    seen, cap = {}, {}

    def on_grid(name):
        def hook(_m, _i, out):
            if replay is not None:
                new = replay[name].to(dtype)
            else:
                new = torch.round((out.detach() + 1) * 2048) / 2048 - 1
                if name == "albedo":
                    new[1] = -1.0                              # 0.5 (x + 1) = 0 over the whole image: the mean floor of :141
            seen[name] = new
            return new
        return hook
    hooks = [nets[n + "Decoder"].register_forward_hook(on_grid(n)) for n in ("albedo", "normal", "rough", "depth")]

    def pre(_m, args):
        cap["light_in"] = args[0].detach().clone()
        raise _Captured()
    hooks.append(nets["lightEncoder"].register_forward_pre_hook(pre))
    try:
        W.wrapperBRDFLight(batch, opt, nets["encoder"], nets["albedoDecoder"], nets["normalDecoder"], nets["roughDecoder"], nets["depthDecoder"],
                           nets["lightEncoder"], nets["axisDecoder"], nets["lambDecoder"], nets["weightDecoder"], o2e, rl, offset=1.0, isLightOut=True)
    except _Captured:
        pass
    for h in hooks:
        h.remove()
    return cap["light_in"], seen, batch["im"]


def encoder_blob():
    in64, seen, im = encoder_run(torch.float64)
    in32, seen32, _ = encoder_run(torch.float32, replay=seen)
    for k in seen:
        assert torch.equal(seen[k].float().double(), seen[k]) and torch.equal(seen32[k].double(), seen[k]), k
    assert tuple(in64.shape) == (2, 11, 480, 640) and in64.dtype == torch.float64 and in32.dtype == torch.float32
    rows, cols = torch.tensor(LATTICE_ROWS), torch.tensor(LATTICE_COLS)
    pick = lambda t: t[:, :, rows][:, :, :, cols].numpy()
    f = lambda t: t.float().numpy()
    return dict(im=f(im), albedo_raw=f(0.5 * (seen["albedo"] + 1)), depth_raw=f(0.5 * (seen["depth"] + 1)), normalPred=f(seen["normal"]),
                roughPred=f(seen["rough"]), rows=rows.numpy(), cols=cols.numpy(), ref64_light_in=pick(in64), ref32_light_in=pick(in32),
                ref64_sum=np.stack([in64.sum(dim=(2, 3)).numpy(), (in64 ** 2).sum(dim=(2, 3)).numpy()]))


def main():
    if not RI.available():
        raise SystemExit("reference not mounted; fixtures can only be generated in the authoring container")
    for name, blob in (("shading", shading_blob(reference_utils())), ("scale", scale_blob()), ("regress", regress_blob(RI.models())),
                       ("encoder", encoder_blob())):
        path = os.path.join(OUT, f"g18_lightglue_{name}.npz")
        np.savez_compressed(path, **blob)
        print("wrote", path, f"{os.path.getsize(path) / 1e3:.0f} KB")


if __name__ == "__main__":
    main()
