"""The reference's three evaluation metrics on the device, backed by libsgrender.so (csrc/sgr_eval_metrics.hip).

  ``whdr(reflectance, point, weight, label, num, delta)``            CompareWHDR.compute_whdr (:8-66)
  ``whdr_from_ranking(reflectance, eqPoint, ..., darkerNum, delta)``  the same on what iiwDataLoader hands to the ranking loss
  ``iiw_judgements(judgements, rows, cols, max_num)``                 the decoded JSON dict -> point / weight / label / num (host, plain Python)
  ``normal_angle_error(normalPred, normalGt, mask, return_map)``      the loop body of CompareNormal.py (:18-42)
  ``depth_log_rmse(depthPred, depthGt)``                              the loop body of CompareDepth.py (:16-32)

They take the predictions where the network leaves them and the ground truth as the file readers decode it, and return one number per image:
the validation pass of ``trainFineTune{IIW,NYU}*.py`` without writing a file or visiting the host.  Sums are formed in double in a fixed
order and there are no float atomics, so two runs are bit-identical and an image does not depend on its batch; the calls capture in a HIP
graph.  Metrics: no autograd.  Dataset-level averages are one torch line on the returned tensors.  DESIGN.md section 8o states the
arithmetic, INTEGRATION.md section 18 the validation loops."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["whdr", "whdr_from_ranking", "iiw_judgements", "normal_angle_error", "depth_log_rmse", "WHDR", "NormalAngleError", "DepthLogRMSE", "WHDR_LABELS"]

_sg = torch.ops.sgrender

WHDR = namedtuple("WHDR", ["whdr", "equal", "inequal", "sums"])
NormalAngleError = namedtuple("NormalAngleError", ["mean", "median", "count"])
NormalAngleErrorMap = namedtuple("NormalAngleErrorMap", ["mean", "median", "count", "theta"])
DepthLogRMSE = namedtuple("DepthLogRMSE", ["rmse", "count"])
WHDR_LABELS = {"E": 0, "1": 1, "2": 2}


def _need(t, name, who):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"sgrender: {who}: {name} must be a tensor, got {type(t).__name__}")
    return t.detach()


def whdr(reflectance, point, weight, label, num, delta: float = 0.1):
    """``WHDR(whdr, equal, inequal, sums)`` of ``CompareWHDR.compute_whdr`` per image.

    ``reflectance``: fp32 ``[B,3,H,W]``, or uint8 ``[B,H,W,3]`` -- what ``export_image(albedo, 'albedo')`` returns; the bytes are divided by
    255 in the kernel, the route of the reference, which reads the saved PNG.  ``point`` int32 or int64 ``[B,N,4] = (r1, c1, r2, c2)``,
    ``weight`` fp32 ``[B,N]``, ``label`` integer ``[B,N]`` with 0 / 1 / 2 for ``'E'`` / ``'1'`` / ``'2'``, ``num`` int ``[B]``: entries at or
    beyond it are ignored whatever they hold.  Per judgement ``l = max(1e-10, mean of the three channels)`` in fp32; the algorithm says
    ``'1'`` if ``l2 / l1 > 1 + delta``, else ``'2'`` if ``l1 / l2 > 1 + delta``, else ``'E'``.

    ``whdr``, ``equal``, ``inequal`` fp32 ``[B]`` are ``error / weight``, ``error_equal / (weight_equal + 1e-10)`` and
    ``error_inequal / (weight_inequal + 1e-10)``; ``sums`` fp64 ``[B,6]`` holds error, error_equal, error_inequal, weight, weight_equal,
    weight_inequal, accumulated in double in a fixed order.  Stated deviations: an image whose weight sum is 0 gives NaN for ``whdr`` (the
    reference returns ``None``); a judgement with a row or column outside the image, or a label outside 0..2, counts as weight 0 and is never
    dereferenced; a weight ``<= 0`` is skipped, as in the reference."""
    who = "whdr"
    args = [_need(t, n, who) for t, n in ((reflectance, "reflectance"), (point, "point"), (weight, "weight"), (label, "label"), (num, "num"))]
    return WHDR(*_sg.eval_whdr(*args, float(delta)))


def whdr_from_ranking(reflectance, eqPoint, eqWeight, eqNum, darkerPoint, darkerWeight, darkerNum, delta: float = 0.1):
    """:func:`whdr` on the arrays ``iiwDataLoader`` hands to ``batch_ranking_loss``: the equal rows map to label 0; in a darker row the second
    point is the darker one, so it maps to label 2.  The two lists are joined; a padded row (at or beyond its list's ``num``) gets weight 0, so
    nothing visits the host and the call captures in a HIP graph.  The same bits as :func:`whdr` on the arrays of :func:`ranking_to_whdr`."""
    return whdr(reflectance, *ranking_to_whdr(eqPoint, eqWeight, eqNum, darkerPoint, darkerWeight, darkerNum), delta)


def ranking_to_whdr(eqPoint, eqWeight, eqNum, darkerPoint, darkerWeight, darkerNum):
    """``(point [B,Ne+Nd,4], weight, label, num)`` of :func:`whdr_from_ranking`; plain torch on the inputs' device."""
    who = "whdr_from_ranking"
    ep, ew, en, dp, dw, dn = (_need(t, n, who) for t, n in ((eqPoint, "eqPoint"), (eqWeight, "eqWeight"), (eqNum, "eqNum"), (darkerPoint, "darkerPoint"),
                                                            (darkerWeight, "darkerWeight"), (darkerNum, "darkerNum")))
    for p, w, n, what in ((ep, ew, en, "eq"), (dp, dw, dn, "darker")):
        if p.dim() != 3 or p.shape[2] != 4 or w.dim() != 2 or tuple(w.shape) != tuple(p.shape[:2]) or n.dim() != 1 or n.shape[0] != p.shape[0]:
            raise RuntimeError(f"sgrender: {who}: {what}Point must be [B,N,4] with {what}Weight [B,N] and {what}Num [B], got {tuple(p.shape)}, {tuple(w.shape)}, {tuple(n.shape)}")
    if ep.shape[0] != dp.shape[0]:
        raise RuntimeError(f"sgrender: {who}: eqPoint {tuple(ep.shape)} and darkerPoint {tuple(dp.shape)} must share B (mismatched batch sizes?)")
    live = lambda w, n: torch.where(torch.arange(w.shape[1], device=w.device)[None, :] < n[:, None], w, torch.zeros_like(w))
    point = torch.cat([ep.to(torch.int32), dp.to(torch.int32)], dim=1)
    weight = torch.cat([live(ew, en), live(dw, dn)], dim=1)
    label = torch.cat([torch.zeros_like(ew, dtype=torch.int32), torch.full_like(dw, 2, dtype=torch.int32)], dim=1)
    num = torch.full_like(en, point.shape[1], dtype=torch.int32)
    return point, weight, label, num


def iiw_judgements(judgements, rows: int, cols: int, max_num=None):
    """``(point [N,4] int32, weight [N] fp32, label [N] int32, num)`` of ONE image from its decoded IIW JSON dict, as host tensors; stack the
    images of a batch.  The reference's filters in its order: ``darker`` in ``'1' '2' 'E'``, ``darker_score`` present and ``> 0``, both points
    opaque; a point is ``(int(y * rows), int(x * cols))``.  ``max_num``: pad to that many rows (zeros: ignored, being beyond ``num``);
    more judgements than ``max_num`` raise.  The weights become fp32, the type the device operators take."""
    pts = {p["id"]: p for p in judgements["intrinsic_points"]}
    point, weight, label = [], [], []
    for c in judgements["intrinsic_comparisons"]:
        darker = c["darker"]
        if darker not in WHDR_LABELS:
            continue
        w = c["darker_score"]
        if w is None or w <= 0.0:
            continue
        p1, p2 = pts[c["point1"]], pts[c["point2"]]
        if not p1["opaque"] or not p2["opaque"]:
            continue
        point.append([int(p1["y"] * rows), int(p1["x"] * cols), int(p2["y"] * rows), int(p2["x"] * cols)])
        weight.append(float(w))
        label.append(WHDR_LABELS[darker])
    n = len(point)
    N = n if max_num is None else int(max_num)
    if n > N:
        raise RuntimeError(f"sgrender: iiw_judgements: {n} judgements pass the filters, more than max_num = {N}")
    pad = N - n
    return (torch.tensor(point + [[0, 0, 0, 0]] * pad, dtype=torch.int32).reshape(N, 4), torch.tensor(weight + [0.0] * pad, dtype=torch.float32),
            torch.tensor(label + [0] * pad, dtype=torch.int32), n)


def normal_angle_error(normalPred, normalGt, mask, return_map: bool = False):
    """``NormalAngleError(mean, median, count)`` of the loop body of ``CompareNormal.py`` per image, in degrees.

    ``normalPred`` fp32 ``[B,3,h,w]`` is resized to the ground truth's ``H x W`` by OpenCV's ``INTER_LINEAR`` rule and NOT renormalised, as the
    reference does not; ``normalGt`` uint8 ``[B,H,W,3]`` in RGB order becomes ``(byte - 127.5) / 127.5`` divided by its norm; ``mask`` uint8
    ``[B,H,W,3]`` or ``[B,H,W]``: a pixel counts when the minimum of its channels ``== 255``.  ``theta = acos(clip(dot, -1, 1)) / pi * 180``.
    ``mean`` fp32 ``[B]`` is the double-accumulated sum over the counted pixels divided by ``count`` (int32 ``[B]``); ``median`` is numpy's: the
    middle element, or ``(a + b) * 0.5`` in fp32 of the two middle ones.  ``count == 0`` or a NaN among the counted angles gives NaN for both.
    ``return_map=True`` adds ``theta`` fp32 ``[B,H,W]``, the angle at EVERY pixel (the kernel's workspace: an error image)."""
    who = "normal_angle_error"
    mean, median, count, theta = _sg.eval_normal_angle(_need(normalPred, "normalPred", who), _need(normalGt, "normalGt", who), _need(mask, "mask", who))
    return NormalAngleErrorMap(mean, median, count, theta) if return_map else NormalAngleError(mean, median, count)


def depth_log_rmse(depthPred, depthGt):
    """``DepthLogRMSE(rmse, count)`` of the loop body of ``CompareDepth.py`` per image.

    ``depthPred`` fp32 ``[B,1,h,w]`` or ``[B,h,w]`` is resized to the ground truth's size by OpenCV's ``INTER_LINEAR`` rule; ``depthGt`` fp32
    ``[B,H,W]`` or ``[B,1,H,W]``.  The mask is ``1 < gt < 10``, strict; both maps become ``log(x + 1e-20)`` and lose their mean over ALL pixels,
    masked or not, as in the reference (a zero in the ground truth contributes ``log(1e-20)``); ``rmse = sqrt(sum((d - g)^2 mask) / sum(mask))``
    fp32 ``[B]``, ``count = sum(mask)`` int32 ``[B]``.  An empty mask gives NaN."""
    who = "depth_log_rmse"
    return DepthLogRMSE(*_sg.eval_depth_log_rmse(_need(depthPred, "depthPred", who), _need(depthGt, "depthGt", who)))
