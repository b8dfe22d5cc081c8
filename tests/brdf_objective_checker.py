"""Checker for ``sgr.brdf_objective`` and ``sgr.batch_ranking_loss``: the contract of DESIGN.md section 8b written out in torch, in
whatever dtype and on whatever device its inputs have (fp64 = the arbiter, fp32 = the yardstick ``e_ref`` of the full-size GPU tests).
TEST INFRASTRUCTURE ONLY; own code -- the formulas and the gradients are spelled out, nothing is differentiated automatically, so
that it is an independent statement of what the kernels compute.  tests/test_brdf_objective_checker.py pins it to the fixtures the
unmodified reference produced (tests/golden/g14_brdfobj_*.npz).

Two stated deviations from the reference, reproduced here: denominators go through ``max(., 1e-5)`` (an empty mask gives 0, the
reference NaN), and in the ranking loss an image with ``num == 0`` contributes 0 and a judgement outside the image counts as weight 0."""
import math

import torch


def _coef(pred, gt, mask_pred, mask_gt):
    """models.py:13-14 per image: clamp(<p, g> / max(<p, p>, 1e-5), 1e-3, 1e3) of the masked tensors"""
    p, g = (pred.detach() * mask_pred).flatten(1), (gt * mask_gt).flatten(1)      # a constant in backward: models.py:13 detaches it
    return torch.clamp((p * g).sum(1) / torch.clamp((p * p).sum(1), min=1e-5), 1e-3, 1e3)


def brdf_objective(albedoPred, normalPred, roughPred, depthPred, albedo, normal, rough, depth, segBRDF, segAll, weights=(6.0, 1.0, 0.5, 0.5),
                   depth_offset=1.0, segDepth=None, upstream=(1.0, 0.0, 0.0, 0.0, 0.0)):
    """-> dict(total, albedoErr, normalErr, roughErr, depthErr, angleMean, coef [B,2], g_albedo, g_normal, g_rough, g_depth): the values and
    the gradient of ``sum_k upstream[k] * (total, albedoErr, normalErr, roughErr, depthErr)[k]`` with respect to each prediction present
    (``None`` otherwise).  Any prediction may be ``None`` with its ground truth."""
    ref = next(t for t in (albedoPred, normalPred, roughPred, depthPred) if t is not None)
    B, kw = ref.shape[0], dict(dtype=ref.dtype, device=ref.device)
    zero = torch.zeros((), **kw)
    sB, sA = segBRDF, segAll
    sD = segDepth if segDepth is not None else segAll
    floor = lambda n: torch.clamp(n, min=1e-5)
    nObj = floor(sB.sum()) if sB is not None else None
    nAll = floor(sA.sum()) if sA is not None else None
    nDep = floor(sD.sum()) if sD is not None else None
    wA, wN, wR, wD = [float(x) for x in weights]
    gT, uA, uN, uR, uD = [float(x) for x in upstream]
    out = dict(albedoErr=zero, normalErr=zero, roughErr=zero, depthErr=zero, angleMean=zero, g_albedo=None, g_normal=None, g_rough=None, g_depth=None)
    coef = torch.zeros(B, 2, **kw)
    if albedoPred is not None:
        A = sB * albedo                                             # wrapperBRDF.py:109
        cA = _coef(albedoPred, A, sB, sB)                           # :110-111 -- the mask enters the ground-truth side twice
        raw = albedoPred * cA.reshape(B, 1, 1, 1)
        a1 = torch.clamp(raw, 0, 1)                                 # :112
        out["albedoErr"] = ((a1 - A) ** 2 * sB).sum() / nObj / 3.0
        inside = ((raw >= 0) & (raw <= 1)).to(ref.dtype)          # the clamp passes gradient on the closed interval
        out["g_albedo"] = (gT * wA + uA) * 2.0 * (a1 - A) * sB * cA.reshape(B, 1, 1, 1) * inside / (3.0 * nObj)
        coef[:, 0] = cA
    if normalPred is not None:
        out["normalErr"] = ((normalPred - normal) ** 2 * sA).sum() / nAll / 3.0
        out["g_normal"] = (gT * wN + uN) * 2.0 * (normalPred - normal) * sA / (3.0 * nAll)
        dot = torch.clamp((normalPred * normal).sum(1, keepdim=True), -1, 1)
        out["angleMean"] = (torch.acos(dot) / math.pi * 180.0 * sA).sum() / nAll      # wrapperNYU.py:111
    if roughPred is not None:
        out["roughErr"] = ((roughPred - rough) ** 2 * sB).sum() / nObj
        out["g_rough"] = (gT * wR + uR) * 2.0 * (roughPred - rough) * sB / nObj
    if depthPred is not None:
        cD = _coef(depthPred, depth, sD, sD)                        # wrapperBRDF.py:114-115, wrapperNYU.py:97-98
        d1 = depthPred * cD.reshape(B, 1, 1, 1)
        e = torch.log(d1 + depth_offset) - torch.log(depth + depth_offset)
        out["depthErr"] = (e * e * sD).sum() / nDep
        out["g_depth"] = (gT * wD + uD) * 2.0 * e * cD.reshape(B, 1, 1, 1) / (d1 + depth_offset) * sD / nDep
        coef[:, 1] = cD
    out["total"] = wA * out["albedoErr"] + wN * out["normalErr"] + wR * out["roughErr"] + wD * out["depthErr"]
    out["coef"] = coef
    return out


def batch_ranking_loss(albedoPred, eqPoint, eqWeight, eqNum, darkerPoint, darkerWeight, darkerNum, tau=0.5, upstream=(1.0, 1.0)):
    """-> dict(eqLoss, darkerLoss, g_albedo): models.py:526-563 per image, wrapperIIW.py:105-109 over the batch, and the dense gradient
    of ``upstream[0] * eqLoss + upstream[1] * darkerLoss``."""
    B, _, H, W = albedoPred.shape
    kw = dict(dtype=albedoPred.dtype, device=albedoPred.device)
    mean = albedoPred.mean(1).reshape(B, H * W)
    rho = torch.log(mean + 0.001)
    g_rho = torch.zeros(B, H * W, **kw)
    losses = []
    for kind, (point, weight, num, up) in enumerate(((eqPoint, eqWeight, eqNum, upstream[0]), (darkerPoint, darkerWeight, darkerNum, upstream[1]))):
        N = point.shape[1]
        total = torch.zeros((), **kw)
        for m in range(B):
            n = min(max(int(num[m]), 0), N)
            if n == 0:
                continue                                                  # stated deviation: 0, not the mean of nothing
            pt = point[m, :n].long()
            r1, c1, r2, c2 = pt[:, 0], pt[:, 1], pt[:, 2], pt[:, 3]
            ok = (r1 >= 0) & (r1 < H) & (r2 >= 0) & (r2 < H) & (c1 >= 0) & (c1 < W) & (c2 >= 0) & (c2 < W)
            w = weight[m, :n].to(albedoPred.dtype) * ok.to(albedoPred.dtype)      # stated deviation: outside the image = weight 0
            p1, p2 = torch.where(ok, r1 * W + c1, torch.zeros_like(r1)), torch.where(ok, r2 * W + c2, torch.zeros_like(r1))
            f1, f2 = rho[m, p1], rho[m, p2]
            if kind == 0:
                d = f1 - f2
                total = total + (w * d * d).sum() / n
                g1 = float(up) / B / n * w * 2.0 * d
            else:
                h = torch.relu(f2 - f1 + tau)
                total = total + (w * h * h).sum() / n
                g1 = -float(up) / B / n * w * 2.0 * h
            g_rho[m].index_add_(0, p1, g1)
            g_rho[m].index_add_(0, p2, -g1)
        losses.append(total / B)
    g = (g_rho / (3.0 * (mean + 0.001))).reshape(B, 1, H, W).expand(B, 3, H, W).contiguous()
    return dict(eqLoss=losses[0], darkerLoss=losses[1], g_albedo=g)
