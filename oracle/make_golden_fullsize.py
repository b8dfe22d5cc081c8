"""One image of BASELINE config 2 (240x320 BRDF maps -> 120x160 env grid, SGNum 12, 8x16 directions) through the
UNMODIFIED reference, fp32 and fp64, forward and backward.  TEST INFRASTRUCTURE ONLY (authoring container):

    python -m oracle.make_golden_fullsize           # writes tests/golden/g7_cfg2_one_image.npz, g9_ratio1_unit_normals.npz and g12_cfg2_objective.npz
    python -m oracle.make_golden_fullsize g12       # writes g12 alone (the others are left untouched); any subset of g7 g9 g12

The inputs and cotangents are the seeded synthetic ones of SURVEY.md section 8d drawn from NumPy's frozen legacy stream
(``oracle.sg_oracle.synthetic_inputs_np`` -- round 5: torch's CPU generator is an implementation detail of the installed torch, and
rounds 3-4 had to SKIP these comparisons when its stream differed; now the tests regenerate the inputs from the seed and FAIL on a
checksum mismatch), so only results are stored -- sub-sampled over
the pixel grid where they are env- or SG-sized (stride recorded), with full-tensor norms.  This is what lets the
full-size GPU tests bound the error against the fp64 oracle by the REFERENCE's own fp32 error instead of a bare constant."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from oracle import make_golden as MG
from oracle import ref_import as RI
from oracle import sg_oracle as O

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
CFG = dict(bn=1, imH=240, imW=320, R=120, C=160, K=12, eh=8, ew=16, fov=57.0, F0=0.05, seed=20207, flavour="stress", rng="numpy")
S_ENV, S_SG = 6, 3


def checksums(inp):
    return np.array([inp[k].double().sum().item() for k in ("albedo", "normal", "rough", "axis", "lamb", "weight")])


# g9 (round 5): the |N|^2 == 1 clamp kink at size.  BRDF maps AT the env-grid resolution (ratio 1: no pooling, trainFineTune*_cascade1.py /
# testReal.py call the layer that way) with unit input normals: clamp(sum N^2, 1e-6, 1) (models.py:467-468) passes the gradient on one side
# of 1 and blocks it on the other, and a unit fp32 vector squares to 1 - eps, 1 or 1 + eps -- so the normal / roughness gradients of the
# reference's fp32 and fp64 runs differ by O(1) pixel by pixel, fp64 is no arbiter there, and the reference's fp32 VALUES are the
# semantics to match.  Stored: values and all six gradients (fp32 and fp64 runs), plus `agree`: the pixels where the fp32 and the fp64
# evaluation of the clamp take the same branch -- there fp64 IS an arbiter, and the reference's own fp32 error e_ref is measured there.
CFG9 = dict(bn=1, imH=120, imW=160, R=120, C=160, K=12, eh=8, ew=16, fov=57.0, F0=0.05, seed=20209, flavour="stress", rng="numpy")


def clamp_branch_agreement(normal):
    """[1,1,H,W] bool: torch's fp32 sum of squares of the (unpooled) normal and the fp64 one land on the same side of the two-sided
    clamp's upper kink (<= 1: gradient passes; > 1: blocked)."""
    n32 = normal.float()
    nn32 = torch.sum(n32 * n32, dim=1, keepdim=True)                 # models.py:467: torch.sum(normal * normal, dim=1)
    n64 = normal.double()
    nn64 = torch.sum(n64 * n64, dim=1, keepdim=True)
    return (nn32 <= 1.0) == (nn64 <= 1.0)


def kink_fixture():
    inp = MG.make_inputs(CFG9)
    r32, cts = MG.run_reference(CFG9, inp, torch.float32)
    r64, _ = MG.run_reference(CFG9, inp, torch.float64)
    agree = clamp_branch_agreement(inp["normal"])
    keys = sorted(k for k in CFG9 if k not in ("flavour", "rng"))
    blob = dict(cfg_keys=np.array(keys), cfg_vals=np.array([float(CFG9[k]) for k in keys]), strides=np.array([S_ENV, S_SG]), in_checksums=checksums(inp),
                ct_checksums=np.array([cts[k].double().sum().item() for k in ("ct_env", "ct_d", "ct_s")]), agree=agree.numpy())
    for tag, r in (("ref32", r32), ("ref64", r64)):
        blob[f"{tag}_env"] = r["env"].detach()[:, :, ::S_ENV, ::S_ENV].numpy().astype(np.float32)
        blob[f"{tag}_diffuse"] = r["diffuse"].detach().numpy().astype(np.float32)
        blob[f"{tag}_spec"] = r["spec"].detach().numpy().astype(np.float32)
        for k in ("axis", "lamb", "weight"):
            g = r[f"glin_{k}"].detach()
            blob[f"{tag}_glin_{k}"] = g[..., ::S_SG, ::S_SG].numpy().astype(np.float32)
        for k in ("albedo", "normal", "rough"):                     # image-sized (ratio 1): kept whole
            blob[f"{tag}_glin_{k}"] = r[f"glin_{k}"].detach().numpy().astype(np.float32)
    path = os.path.join(OUT, "g9_ratio1_unit_normals.npz")
    np.savez_compressed(path, **blob)
    frac = agree.float().mean().item()
    print("wrote", path, f"{os.path.getsize(path) / 1e6:.2f} MB; clamp branches agree on {100 * frac:.1f} % of the pixels")
    for k in ("normal", "rough", "albedo"):
        a, b = torch.from_numpy(blob[f"ref32_glin_{k}"]).double(), torch.from_numpy(blob[f"ref64_glin_{k}"]).double()
        m = agree.expand_as(a)
        print(f"  reference fp32 vs fp64 glin_{k:7s} rel-L2 all pixels {((a - b).norm() / b.norm()).item():.2e}   where the branches agree {((a[m] - b[m]).norm() / b[m].norm()).item():.2e}")


# g12 (round 7): the training OBJECTIVE of config 2 at size -- renderErr + 10 reconstErr (wrapperBRDFLight.py:167-207, trainLight.py:237) of the
# image of g7 (same CFG, same seed: the tests regenerate the inputs with synthetic_inputs_np), with env_ind = 1, evaluated by the reference in
# fp32 and fp64 (oracle.make_golden.run_reference).  Stored: the loss values and the render loss's numerator / denominator (float64 scalars),
# the rendered image whole, and the gradients of the total w.r.t. the SG parameters sub-sampled at S12 with their full-tensor norms.  The
# stride is 5, not g7's 3: a committed file stays within 1 MiB, and 768 of the 19 200 env cells (all K lobes of each) still sample every
# region of the grid.
S12 = 5
LOSS_KEYS = ("im", "seg", "env_gt")


def checksums_loss(inp):
    return np.array([inp[k].double().sum().item() for k in LOSS_KEYS])


def objective_blob(r32, r64, inp):
    keys = sorted(k for k in CFG if k not in ("flavour", "rng"))
    blob = dict(cfg_keys=np.array(keys), cfg_vals=np.array([float(CFG[k]) for k in keys]), stride_sg=np.array([S12]),
                in_checksums=checksums(inp), in_checksums_loss=checksums_loss(inp))
    for tag, r in (("ref32", r32), ("ref64", r64)):
        for k in ("render_err", "recon_err", "render_num", "render_den"):
            blob[f"{tag}_{k}"] = r[k].detach().double().numpy()
        blob[f"{tag}_rendered"] = r["rendered"].detach().numpy().astype(np.float32)
        for k in ("axis", "lamb", "weight"):
            g = r[f"gtot_{k}"].detach()
            blob[f"{tag}_gtot_{k}"] = g[..., ::S12, ::S12].numpy().astype(np.float32)
            blob[f"{tag}_gtot_{k}_norm"] = np.array([g.double().norm().item()])
    return blob


def objective_fixture():
    inp = MG.make_inputs(CFG)
    r32, _ = MG.run_reference(CFG, inp, torch.float32)
    r64, _ = MG.run_reference(CFG, inp, torch.float64)
    blob = objective_blob(r32, r64, inp)
    path = os.path.join(OUT, "g12_cfg2_objective.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, f"{os.path.getsize(path) / 1e6:.2f} MB")
    for k in ("render_err", "recon_err", "render_num", "render_den"):
        print(f"  reference fp32 vs fp64 {k:12s} {blob['ref32_' + k][0]:.9g} {blob['ref64_' + k][0]:.9g}")
    for k in ("rendered", "gtot_axis", "gtot_lamb", "gtot_weight"):
        a, b = torch.from_numpy(blob["ref32_" + k]).double(), torch.from_numpy(blob["ref64_" + k]).double()
        print(f"  reference fp32 vs fp64 {k:12s} rel-L2 {((a - b).norm() / b.norm()).item():.2e}")
    return blob


def main():
    if not RI.available():
        raise SystemExit("reference not mounted")
    torch.set_num_threads(8)
    only = set(sys.argv[1:])     # e.g. `python -m oracle.make_golden_fullsize g12`: leave g7 / g9 untouched
    unknown = only - {"g7", "g9", "g12"}
    if unknown:
        raise SystemExit(f"unknown fixture(s) {sorted(unknown)}; choose from g7 g9 g12")
    if not only or "g9" in only:
        kink_fixture()
    if not only or "g12" in only:
        objective_fixture()
    if only and "g7" not in only:
        return
    inp = MG.make_inputs(CFG)
    r32, cts = MG.run_reference(CFG, inp, torch.float32)
    r64, _ = MG.run_reference(CFG, inp, torch.float64)
    blob = dict(cfg_keys=np.array(sorted(k for k in CFG if k not in ("flavour", "rng"))),
                cfg_vals=np.array([float(CFG[k]) for k in sorted(k for k in CFG if k not in ("flavour", "rng"))]),
                strides=np.array([S_ENV, S_SG]), in_checksums=checksums(inp),
                ct_checksums=np.array([cts[k].double().sum().item() for k in ("ct_env", "ct_d", "ct_s")]))
    for tag, r in (("ref32", r32), ("ref64", r64)):
        blob[f"{tag}_env"] = r["env"].detach()[:, :, ::S_ENV, ::S_ENV].numpy().astype(np.float32)
        blob[f"{tag}_diffuse"] = r["diffuse"].detach().numpy().astype(np.float32)
        blob[f"{tag}_spec"] = r["spec"].detach().numpy().astype(np.float32)
        for k in ("axis", "lamb", "weight", "albedo", "normal", "rough"):      # the BRDF-map gradients too (round 3): a10 at size
            g = r[f"glin_{k}"].detach()
            blob[f"{tag}_glin_{k}"] = g[..., ::S_SG, ::S_SG].numpy().astype(np.float32)
            blob[f"{tag}_glin_{k}_norm"] = np.array([g.double().norm().item()])
        blob[f"{tag}_env_norm"] = np.array([r["env"].detach().double().norm().item()])
    path = os.path.join(OUT, "g7_cfg2_one_image.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, f"{os.path.getsize(path) / 1e6:.2f} MB")
    for k in ("env", "diffuse", "spec", "glin_axis", "glin_lamb", "glin_weight", "glin_albedo", "glin_normal", "glin_rough"):
        a, b = torch.from_numpy(blob["ref32_" + k]).double(), torch.from_numpy(blob["ref64_" + k]).double()
        print(f"  reference fp32 vs fp64 {k:12s} rel-L2 {((a - b).norm() / b.norm()).item():.2e}")


if __name__ == "__main__":
    main()
