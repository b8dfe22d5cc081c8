"""The BRDF-stage training objectives, backed by libsgrender.so (csrc/sgr_brdf_loss.hip).

  ``brdf_objective(...)``        wrapperBRDF.py:109-134 (= trainBRDF.py:248-286) and wrapperNYU.py:94-111: the four masked errors, the
                                 mean normal angle and their weighted sum, with the LSregress coefficients of albedo and depth
  ``batch_ranking_loss(...)``    wrapperIIW.py:88-109 with models.BatchRankingLoss (models.py:526-563), the whole batch in one call

The reference evaluates these with about a hundred eager launches and two ``.item()`` synchronisations per step (the IIW one with a
Python loop over the images); here the objective is three streaming launches forward and one backward, the ranking loss two and two,
nothing visits the host and two runs are bit-identical.  DESIGN.md section 8b states the arithmetic."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)
from .losses import _allreduce_sum_, _sharded

__all__ = ["brdf_objective", "batch_ranking_loss", "BRDFObjective"]

_sg = torch.ops.sgrender


class BRDFObjective(NamedTuple):
    total: torch.Tensor                      # sum_i w_i Err_i over the terms present
    albedoErr: torch.Tensor                  # 0-d device tensors; the first five carry gradient, an absent term is 0
    normalErr: torch.Tensor
    roughErr: torch.Tensor
    depthErr: torch.Tensor
    angleMean: torch.Tensor                  # degrees, no gradient (wrapperNYU.py:111)
    coef: torch.Tensor                       # [B,2] = (albedo, depth) LSregress coefficients, no gradient
    albedoScaled: Optional[torch.Tensor] = None      # only with return_scaled=True: clamp(albedoPred * coef, 0, 1), detached
    depthScaled: Optional[torch.Tensor] = None       # depthPred * coef, detached


def brdf_objective(albedoPred, normalPred, roughPred, depthPred, albedoBatch, normalBatch, roughBatch, depthBatch, segBRDFBatch, segAllBatch,
                   weights=(6.0, 1.0, 0.5, 0.5), depth_offset: float = 1.0, segDepthBatch=None, return_scaled: bool = False, group=None) -> BRDFObjective:
    """The synthetic (wrapperBRDF.py) and NYU (wrapperNYU.py) objective of the BRDF stage.

    Predictions ``[B,3,H,W] [B,3,H,W] [B,1,H,W] [B,1,H,W]`` with ground truth of the same shapes; any prediction may be ``None``
    together with its ground truth (that term costs nothing and reads 0).  ``albedoPred`` / ``depthPred`` are the wrappers' tensors of
    those names, i.e. after ``0.5 * (decoder + 1)``.  ``segBRDFBatch`` masks albedo and roughness, ``segAllBatch`` the normal and --
    unless ``segDepthBatch`` is given -- the depth; masks are fp32 ``[B,1,H,W]`` with values in [0, 1], not assumed binary.
    ``weights = (4 * albeW, normW, rougW, deptW)`` of trainBRDF.py:285 (the 4x is the caller's); ``depth_offset`` is 1.0 in
    wrapperBRDF.py:129 and 0.1 in wrapperNYU.py:108.  NYU passes ``None`` for albedo and roughness, its ``segNormalBatch`` as
    ``segAllBatch`` and its ``segDepthBatch`` as ``segDepthBatch``, after interpolating its predictions to the ground truth's size.

    Gradients flow to the four predictions only (the coefficients are constants, models.py:13); a ground-truth tensor or mask that
    requires grad raises.  The mask sums stay on the device; a denominator goes through ``max(., 1e-5)``, so an empty mask gives 0
    where the reference gives NaN.  ``group``: the batch is sharded over the ranks of that process group -- the eight batch totals are
    all-reduced (one collective) and every rank receives the gradient of the GLOBAL objective with respect to its shard, the
    convention of :func:`combine_loss_parts`."""
    w = [float(x) for x in weights]
    if len(w) != 4:
        raise RuntimeError("sgrender: brdf_objective: weights must be (albedo, normal, rough, depth)")
    planes = (albedoPred, albedoBatch, normalPred, normalBatch, roughPred, roughBatch, depthPred, depthBatch, segBRDFBatch, segAllBatch, segDepthBatch)
    if torch.is_grad_enabled():      # before any launch or collective, on both routes
        for name, t in zip(("albedoBatch", "normalBatch", "roughBatch", "depthBatch", "segBRDFBatch", "segAllBatch", "segDepthBatch"), planes[1:8:2] + planes[8:]):
            if t is not None and t.requires_grad:
                raise RuntimeError(f"sgrender: brdf_objective differentiates with respect to the four predictions only; {name} requires grad -- detach it")
    if _sharded(group):
        with torch.no_grad():
            _, parts, coef = _sg.brdf_objective_fwd(*planes, w, float(depth_offset), False)
            _allreduce_sum_(parts, group)
        out = _sg.brdf_objective(*planes, parts, coef, w, float(depth_offset))
    else:
        out = _sg.brdf_objective(*planes, None, None, w, float(depth_offset))
    total, a_err, n_err, r_err, d_err, angle, coef, _ = out
    a_s = d_s = None
    if return_scaled:
        with torch.no_grad():
            if albedoPred is not None:
                a_s = torch.clamp(albedoPred * coef[:, 0].reshape(-1, 1, 1, 1), 0, 1)
            if depthPred is not None:
                d_s = depthPred * coef[:, 1].reshape(-1, 1, 1, 1)
    return BRDFObjective(total, a_err, n_err, r_err, d_err, angle, coef, a_s, d_s)


def batch_ranking_loss(albedoPred, eqPoint, eqWeight, eqNum, darkerPoint, darkerWeight, darkerNum, tau: float = 0.5):
    """``(eqLoss, darkerLoss)`` of wrapperIIW.py:88-109 for the whole batch.

    ``albedoPred [B,3,H,W]``; ``eqPoint / darkerPoint`` int32 or int64 ``[B,N,4] = (r1, c1, r2, c2)``, ``eqWeight / darkerWeight`` fp32
    ``[B,N]``, ``eqNum / darkerNum`` int ``[B]`` -- device tensors, padded as iiwDataLoader.py:70-95 pads them (N = 800 there; at most
    2048 equal + darker slots per image).  Entries at or beyond ``num`` are ignored whatever they hold.  Two stated deviations from the
    reference: an image with ``num == 0`` contributes 0 (the reference: NaN), and a judgement with a row or column outside the image
    counts as weight 0 and is never dereferenced (the reference would raise).  Differentiable with respect to ``albedoPred``: a dense
    gradient, zero off the judged pixels, bit-reproducible although judgements share pixels."""
    return tuple(_sg.batch_ranking_loss(albedoPred, eqPoint, eqWeight, eqNum, darkerPoint, darkerWeight, darkerNum, float(tau)))
