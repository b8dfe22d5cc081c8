"""testReal's output stage and the image writers, backed by libsgrender.so (csrc/sgr_export.hip).

  ``export_image(x, kind, size, scale, bgr)``        testReal.py:542-657, utils.writeImageToFile (utils.py:65-76)
  ``export_env_mosaic(env, nrows, ncols, gap, bgr)`` utils.writeEnvToFile / writeNumpyEnvToFile (utils.py:102-154)
  ``export_env_hwc(env, flip)``                      the env ``.npz`` layout (testReal.py:626-631)
  ``export_predictions(preds, size, cAlbedos, bgr)`` the whole ``Output Results`` block, named after the reference's files

They take fp32 device tensors in the layouts the operators produce and return device tensors that are ready to write -- ``uint8`` HWC for
the images, fp32 for the env copy -- so that what crosses to the host is a quarter (images) or a hundredth (mosaics) of the fp32 source.
The file encoders (``cv2.imwrite``, ``np.savez_compressed``) stay on the host.  No autograd.  Two runs are bit-identical, an image does not
depend on its batch, strided inputs are read in place, and the calls capture in a HIP graph.  DESIGN.md section 8m states the arithmetic,
INTEGRATION.md section 16 the lines that remain on the host."""
from __future__ import annotations

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["EXPORT_KINDS", "export_image", "export_env_mosaic", "export_env_hwc", "export_predictions"]

_sg = torch.ops.sgrender

# the `kind` codes of include/sgrender.h (SGR_EXPORT_*)
EXPORT_KINDS = {"albedo": 0, "normal": 1, "rough": 2, "depth": 3, "rendered": 4, "shading": 5, "image": 6, "image_gamma": 7}


def _need(t, name, who):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"sgrender: {who}: {name} must be a tensor, got {type(t).__name__}")
    return t.detach()


def _size(size, who):
    if size is None:
        return None
    try:
        nh, nw = (int(v) for v in size)
    except (TypeError, ValueError):
        raise RuntimeError(f"sgrender: {who}: size must be two positive integers (nh, nw), got {size!r}") from None
    if nh <= 0 or nw <= 0:
        raise RuntimeError(f"sgrender: {who}: size must be two positive integers (nh, nw), got {size!r}")
    return [nh, nw]


def _per_image(scale, B, like, who):
    """``scale`` [B] fp32 on ``like``'s device from a tensor, a sequence or one number (formed in double, used as fp32, as numpy's are)"""
    if scale is None:
        return None
    if isinstance(scale, torch.Tensor):
        s = scale.detach()
        if s.numel() != B:
            raise RuntimeError(f"sgrender: {who}: scale must hold one value per image ({B}), got {tuple(s.shape)}")
        return s.reshape(B) if s.dtype == torch.float32 else s.to(torch.float64).to(torch.float32).reshape(B)
    vals = [float(scale)] * B if isinstance(scale, (int, float)) else [float(v) for v in (scale.tolist() if hasattr(scale, "tolist") else scale)]
    if len(vals) != B:
        raise RuntimeError(f"sgrender: {who}: scale must hold one value per image ({B}), got {len(vals)}")
    return torch.tensor(vals, dtype=torch.float64).to(torch.float32).to(like.device)


def export_image(x, kind: str, size=None, scale=None, bgr: bool = False):
    """``uint8 [B,nh,nw,C_out]`` from ``x [B,C,h,w]`` fp32 (any strides): the bytes ``testReal.py`` hands to ``cv2.imwrite``.

    ``kind`` names the lines of the reference: ``albedo`` ``255 (x scale[b]) ** (1/2.2)``; ``normal`` and ``rough`` ``255 * 0.5 * (v + 1)``;
    ``depth`` ``255 / clip(x / max(mean(x[b]), 1e-10) * 3 + 1, 1e-6, 10)``; ``rendered`` ``255 clip((x / max(x[b])) ** (1/2.2), 0, 1)``; ``shading``
    ``255 clip(x / mean(x[b]) / 3, 0, 1) ** (1/2.2)``; ``image`` / ``image_gamma`` ``255 clip(x, 0, 1)`` (``** (1/2.2)``), one channel written
    three times.  The first five are resized to ``size = (nh, nw)`` by OpenCV's ``INTER_LINEAR`` rule for float data (the coordinate formed in
    double; not torch's rule) between the power and the scaling by 255, as the reference does; ``size=None`` keeps ``(h, w)``.  The byte is
    ``(uint8) min(max(t, 0), 255)`` by truncation: values the reference leaves to numpy's undefined cast saturate, a NaN gives 0.  ``scale``:
    the reference's ``cAlbedo`` per image (albedo only).  ``bgr`` reverses the channels, as ``cv2.imwrite(..., im[:, :, ::-1])`` expects."""
    x = _need(x, "x", "export_image")
    if kind not in EXPORT_KINDS:
        raise RuntimeError(f"sgrender: export_image: unknown kind {kind!r} (one of {', '.join(EXPORT_KINDS)})")
    if scale is not None and kind != "albedo":
        raise RuntimeError(f"sgrender: export_image({kind}): scale (cAlbedo) belongs to the albedo kind")
    s = _per_image(scale, x.shape[0] if x.dim() else 0, x, "export_image")
    return _sg.export_image(x, EXPORT_KINDS[kind], _size(size, "export_image"), s, bool(bgr))


def export_env_mosaic(env, nrows: int = 12, ncols: int = 8, gap: int = 1, bgr: bool = False):
    """``uint8 [B,Hm,Wm,3]`` from ``env [B,3,R,C,eh,ew]``: ``utils.writeEnvToFile`` for every image of the batch.  Cells ``r = 0, interY, ..``
    and ``c = 0, interX, ..`` (``interY = int(R / nrows)``) are laid out ``gap`` apart on a background of 255 -- ``ceil(R / interY)`` rows of
    tiles, which can be more than ``nrows`` -- with ``255 clip(v, 0, 1) ** (1/2.2)``.  Cells that are not sampled are never read.
    ``nrows > R`` or ``ncols > C`` raises (the reference divides by zero there)."""
    return _sg.export_env_mosaic(_need(env, "env", "export_env_mosaic"), int(nrows), int(ncols), int(gap), bool(bgr))


def export_env_hwc(env, flip: bool = True):
    """fp32 ``[B,R,C,eh,ew,3]`` from ``env [B,3,R,C,eh,ew]``, the channels reversed with ``flip``: exact copies, the layout of the reference's
    ``np.savez_compressed(..., env=np.ascontiguousarray(env.transpose(1, 2, 3, 4, 0)[..., ::-1]))``."""
    return _sg.export_env_hwc(_need(env, "env", "export_env_hwc"), bool(flip))


# key of `preds` -> (kind, file stem of the reference, takes cAlbedos, is resized)
_PRED_IMAGES = (("albedo", "albedo", "albedo", True), ("normal", "normal", "normal", False), ("rough", "rough", "rough", False), ("depth", "depth", "depth", False),
                ("albedoBS", "albedo", "albedoBS", True), ("roughBS", "rough", "roughBS", False), ("depthBS", "depth", "depthBS", False),
                ("rendered", "rendered", "rendered", False), ("shading", "shading", "shading", False))


def export_predictions(preds, size, cAlbedos=None, bgr: bool = True):
    """The ``Output Results`` block of ``testReal.py`` (lines 542-657) for the lists it holds, one entry per cascade level.

    ``preds``: a dict of lists of device tensors under the keys ``albedo normal rough depth`` (the ``*Preds`` lists), ``albedoBS roughBS depthBS``
    (``opt.isBS``), ``rendered`` (``renderedPreds``), ``shading`` (``predToShading`` of each ``envmapsPreds[n]``, ``[B,3,h,w]``) and ``envmaps``
    (``envmapsPredImages``); keys that are absent are skipped.  ``size = (nh, nw)``: the photograph's size.  ``cAlbedos[n]``: the scale of level
    ``n``'s albedo (a number, a sequence or a tensor per image); levels beyond the list have none, as in the reference.

    Returns a dict of device tensors named after the reference's output files: ``'albedo0.png'`` .. (``uint8 [B,nh,nw,C]``), ``'shading0.png'``
    (``[B,h,w,3]``), ``'envmap0.png'`` (the mosaic, ``nrows=24, ncols=16``) and ``'envmap0.npz'`` (fp32 ``[B,R,C,eh,ew,3]``, the channels
    reversed as the reference stores them).  ``bgr=True`` orders the three-channel images for ``cv2.imwrite`` as they are."""
    cAlbedos = [] if cAlbedos is None else list(cAlbedos)
    out = {}
    for key, kind, stem, scaled in _PRED_IMAGES:
        for n, x in enumerate(preds.get(key, ())):
            scale = cAlbedos[n] if scaled and n < len(cAlbedos) else None
            out[f"{stem}{n}.png"] = export_image(x, kind, None if kind == "shading" else size, scale, bgr)
    for n, env in enumerate(preds.get("envmaps", ())):
        out[f"envmap{n}.npz"] = export_env_hwc(env, flip=True)
        out[f"envmap{n}.png"] = export_env_mosaic(env, nrows=24, ncols=16, bgr=bgr)
    return out
