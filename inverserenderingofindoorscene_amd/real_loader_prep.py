"""The real-image loaders' batch preparation, backed by libsgrender.so (csrc/sgr_real_loader.hip).

  ``nyu_prepare_batch(raw, phase, crop, flip, colour, imHeight, imWidth)``   nyuDataLoader.py:75-131, 143-173
  ``nyu_augmentation(u, imHeight, imWidth, ...)``                            :76-82, 121-129 (plain torch, float64)
  ``iiw_image(im_u8)``                                                       iiwDataLoader.py:136-137, 205-214

They take what the loaders have DECODED -- ``cv2.imread``'s uint8 HWC arrays and the fp32 depth for NYU; for IIW the resized and cropped bytes
(``iiw_resize_crop`` of pil_resize.py, or PIL and a slice on the host) -- and do the per-sample arithmetic the reference runs in numpy inside its loader workers: for NYU a random crop, the
byte maps, two normalisations of the normal, four ``cv2.resize(INTER_LINEAR)`` calls, two thresholds, a mirror and a colour scale, in ONE
launch for the whole batch with one crop rectangle per image.  The results are inputs of the training step, so there is no autograd.  Nothing
visits the host when the augmentation arguments are device tensors, two runs are bit-identical, an image does not depend on its batch, and the
calls capture in a HIP graph.  DESIGN.md section 8n states the arithmetic, INTEGRATION.md section 17 the ``Dataset`` side."""
from __future__ import annotations

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["nyu_prepare_batch", "nyu_augmentation", "iiw_image"]

_sg = torch.ops.sgrender


def _need(t, name, who):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"sgrender: {who}: {name} must be a tensor, got {type(t).__name__}")
    return t.detach()


def nyu_augmentation(u, imHeight: int, imWidth: int, imWidthMax: int = 600, imWidthMin: int = 560, srcHeight: int = 480, srcWidth: int = 640):
    """``(crop [bn,4] int32, flip [bn] bool, colour [bn,3] float64)`` from ``u [bn,7]``: a sample's ``np.random.random()`` draws in the
    reference's order -- scale, row, column, flip, three colour values -- turned into what ``NYULoader.__getitem__`` forms from them, in
    float64 as Python does: ``cropW = int(round((imWidthMax - imWidthMin) * u0 + imWidthMin))`` (round-half-to-even, numpy's and torch's rule),
    ``cropH = int(imHeight / imWidth * cropW)`` (truncation), ``rs = int(round((srcHeight - cropH) * u1))``, ``cs`` alike with ``u2``;
    ``flip = u3 > 0.5``; ``colour = 1 + (u[4:7] * 0.4 - 0.2)``.  ``crop`` is ``(rs, cs, cropH, cropW)``.  Plain torch on the device ``u`` lives
    on (host or GPU), without a synchronisation."""
    u = _need(u, "u", "nyu_augmentation")
    if u.dim() != 2 or u.shape[1] != 7:
        raise RuntimeError(f"sgrender: nyu_augmentation: u must be [bn,7] (scale, row, column, flip, three colour values), got {tuple(u.shape)}")
    u = u.to(torch.float64)
    cw = torch.round((imWidthMax - imWidthMin) * u[:, 0] + imWidthMin)
    ch = torch.trunc((float(imHeight) / float(imWidth)) * cw)
    rs = torch.round((srcHeight - ch) * u[:, 1])
    cs = torch.round((srcWidth - cw) * u[:, 2])
    crop = torch.stack([rs, cs, ch, cw], dim=1).to(torch.int32)
    return crop, u[:, 3] > 0.5, 1 + (u[:, 4:7] * 0.4 - 0.2)


def _host_values(x):
    """the values of an argument that lives on the host (a sequence, a numpy array, a CPU tensor); None for a device tensor"""
    if isinstance(x, torch.Tensor):
        return None if x.is_cuda or x.device.type == "meta" else x.tolist()
    return x.tolist() if hasattr(x, "tolist") else [v for v in x]


def _crop(crop, bn, Hs, Ws, device):
    vals = _host_values(crop)
    if vals is None:      # a device tensor: the kernel clamps, nothing is checked here
        return crop.detach()
    try:
        rows = [[int(v) for v in row] for row in vals]
    except (TypeError, ValueError):
        raise RuntimeError(f"sgrender: nyu_prepare_batch: crop must be [bn,4] integers (rs, cs, cropH, cropW), got {crop!r}") from None
    if len(rows) != bn or any(len(r) != 4 for r in rows):
        raise RuntimeError(f"sgrender: nyu_prepare_batch: crop must be [bn,4] = [{bn},4] (mismatched batch sizes?), got {len(rows)} rows")
    for b, (rs, cs, ch, cw) in enumerate(rows):
        if ch < 1 or cw < 1:
            raise RuntimeError(f"sgrender: nyu_prepare_batch: crop[{b}] has cropH = {ch}, cropW = {cw}: both must be at least 1")
        if rs < 0 or cs < 0 or rs + ch > Hs or cs + cw > Ws:
            raise RuntimeError(f"sgrender: nyu_prepare_batch: crop[{b}] = rows {rs}:{rs + ch}, columns {cs}:{cs + cw} leaves the source {Hs} x {Ws}")
    return torch.tensor(rows, dtype=torch.int32).to(device)


def _flags(flip, bn, device):
    vals = _host_values(flip)
    if vals is None:
        return flip.detach()
    vals = [bool(v) for v in vals]
    if len(vals) != bn:
        raise RuntimeError(f"sgrender: nyu_prepare_batch: flip must hold one flag per image ({bn}; mismatched batch sizes?), got {len(vals)}")
    return torch.tensor(vals, dtype=torch.bool).to(device)


def _colour(colour, bn, device):
    vals = _host_values(colour)
    if vals is None:
        return colour.detach()
    try:
        rows = [[float(v) for v in row] for row in vals]
    except (TypeError, ValueError):
        raise RuntimeError(f"sgrender: nyu_prepare_batch: colour must be [bn,3] numbers, got {colour!r}") from None
    if len(rows) != bn or any(len(r) != 3 for r in rows):
        raise RuntimeError(f"sgrender: nyu_prepare_batch: colour must be [bn,3] = [{bn},3] (mismatched batch sizes?), got {len(rows)} rows")
    return torch.tensor(rows, dtype=torch.float64).to(device)


def nyu_prepare_batch(raw, phase: str = "TRAIN", crop=None, flip=None, colour=None, imHeight: int = 480, imWidth: int = 640):
    """The ``batchDict`` of ``nyuDataLoader.NYULoader.__getitem__`` for a collated batch of raw arrays on the device.

    ``raw``: ``im`` ``normal`` ``seg`` uint8 ``[bn,Hs,Ws,3]`` in ``cv2.imread``'s channel order (BGR: the operator reverses it, as ``loadImage``
    does); ``depth`` fp32 ``[bn,Hs,Ws]`` or ``[bn,1,Hs,Ws]``; ``name`` is passed through when present.  ``phase='TRAIN'`` needs ``crop [bn,4]``
    ``= (rs, cs, cropH, cropW)`` int32, ``flip [bn]`` bool and ``colour [bn,3]`` float64 (:func:`nyu_augmentation` forms them from the random
    draws); ``'TEST'`` takes none: the crop is the whole source, no mirror, no colour scale.

    Returns the reference's keys, fp32: ``normal [bn,3,H,W]``, ``depth``, ``segNormal``, ``segDepth`` ``[bn,1,H,W]`` and ``im [bn,3,H,W]`` with
    ``(H, W) = (imHeight, imWidth)``.  Per source pixel ``im = 0.5 ((2 (u8 / 255) ** 2.2 - 1) + 1)``, ``normal = n / sqrt(max(|n|^2, 1e-5))`` with
    ``n = (u8 - 127.5) / 127.5``, ``segNormal = 0.5 (n + 1)`` of the reversed image's channel 0; the crop is resized to ``(H, W)`` by OpenCV's
    ``INTER_LINEAR`` rule for float data (the border clamp against the crop; equal sizes pass the values through); then
    ``segDepth = (depth > 1) & (depth < 10)``, ``normal / max(|normal|, 1e-5)``, the mirror (``normal[0]`` negated) and ``im * colour`` in double.

    The augmentation arguments may be host values (sequences, numpy arrays, CPU tensors) -- then a rectangle that leaves the source, or with
    ``cropH < 1`` or ``cropW < 1``, raises -- or device tensors: no host work, so the call captures in a HIP graph, BUT THE KERNEL CANNOT
    RAISE.  It then clamps the rectangle into the source (``rs`` to ``[0, Hs - 1]``, ``cropH`` to ``[1, Hs - rs]``, columns alike), so a bad
    value gives a well-defined result from another rectangle and never reads out of bounds."""
    who = "nyu_prepare_batch"
    ph = str(phase).upper()
    if ph not in ("TRAIN", "TEST"):
        raise RuntimeError(f"sgrender: {who}: unrecognized phase {phase!r} (TRAIN or TEST)")
    given = [k for k, v in (("crop", crop), ("flip", flip), ("colour", colour)) if v is not None]
    if ph == "TRAIN" and len(given) != 3:
        raise RuntimeError(f"sgrender: {who}: phase 'TRAIN' needs crop, flip and colour (nyu_augmentation forms them); got {given or 'none'}")
    if ph == "TEST" and given:
        raise RuntimeError(f"sgrender: {who}: phase 'TEST' takes no {', '.join(given)} (the whole source, no mirror, no colour scale)")
    missing = [k for k in ("im", "normal", "seg", "depth") if k not in raw]
    if missing:
        raise RuntimeError(f"sgrender: {who}: raw lacks {missing}")
    im, normal, seg, depth = (_need(raw[k], k, who) for k in ("im", "normal", "seg", "depth"))
    if im.dim() != 4:
        raise RuntimeError(f"sgrender: {who}: im must be a non-empty [bn,H,W,3], got {tuple(im.shape)}")
    bn, Hs, Ws = im.shape[0], im.shape[1], im.shape[2]
    if depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if depth.dim() != 3:
        raise RuntimeError(f"sgrender: {who}: depth must be [bn,Hs,Ws] or [bn,1,Hs,Ws], got {tuple(depth.shape)}")
    args = (None, None, None)
    if ph == "TRAIN":
        args = (_crop(crop, bn, Hs, Ws, im.device), _flags(flip, bn, im.device), _colour(colour, bn, im.device))
    n, d, sn, sd, i = _sg.nyu_prepare(im, normal, seg, depth, *args, int(imHeight), int(imWidth))
    batch = dict(normal=n, depth=d, segNormal=sn, segDepth=sd, im=i)
    if "name" in raw:
        batch["name"] = raw["name"]
    return batch


def iiw_image(im_u8):
    """fp32 ``[bn,3,H,W]`` from ``im_u8 [bn,H,W,3]`` uint8 in PIL's channel order, already resized and cropped (``iiw_resize_crop``, or PIL and a slice on the host; the crop is a
    slice and commutes with the point-wise maps): ``(u8 / 255) ** 2.2``, transposed to CHW and divided by its maximum over the image -- the
    ``im`` of ``iiwDataLoader.loadImage`` with ``isGama``.  The map is monotone, so the maximum is the value of the image's largest byte and a
    non-black image's maximum element is exactly 1.  AN ALL-BLACK IMAGE GIVES 0 / 0 = NaN THROUGHOUT, as numpy does in the reference."""
    return _sg.iiw_image(_need(im_u8, "im_u8", "iiw_image"))
