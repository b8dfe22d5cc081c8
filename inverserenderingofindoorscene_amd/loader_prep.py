"""The synthetic loader's batch preparation, backed by libsgrender.so (csrc/sgr_loader_prep.hip).

  ``loader_masks(seg_u8)``                      dataLoader.py:120-131
  ``loader_scale_hdr(hdr, seg_u8, u)``          :134-136, 246-259
  ``loader_brdf_maps(albedo_u8, normal_u8, rough_u8)``   :139-147
  ``loader_envmaps(env_raw, scale, env_ind)``   :153-154, 286-310
  ``prepare_batch(raw, phase, isLight, u)``     the ``dataBatch`` dict of ``BatchLoader.__getitem__`` for a whole batch

They take what the loader has DECODED AND RESIZED -- the file readers and ``cv2.resize(INTER_AREA)`` stay on the host; PIL's resize is ``loader_resize`` of pil_resize.py -- in the
layout the readers hand it over (HWC), and do the per-sample arithmetic that the reference runs in numpy inside its loader workers: a masked
order statistic, a 7 x 7 erosion, three point-wise maps and a transposing 2 x 2 block mean.  The results are inputs of the training step, so
there is no autograd.  Nothing visits the host (``u`` given as a device tensor), two runs are bit-identical, an image does not depend on its
batch, and the calls capture in a HIP graph.  DESIGN.md section 8l states the arithmetic, INTEGRATION.md section 15 the ``Dataset`` side."""
from __future__ import annotations

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["loader_masks", "loader_scale_hdr", "loader_brdf_maps", "loader_envmaps", "prepare_batch"]

_sg = torch.ops.sgrender


def _need(t, name, who):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"sgrender: {who}: {name} must be a tensor, got {type(t).__name__}")
    return t.detach()


def loader_masks(seg_u8, erode: bool = True):
    """``(segArea, segEnv, segObj)``, each ``[bn,1,H,W]`` fp32 of exact 0 / 1, from ``seg_u8 [bn,H,W,Cin]`` uint8 (channel 0 is used).
    ``seg = 0.5 * ((u8 - 127.5) / 127.5 + 1)`` in fp32; ``segArea = (seg > 0.49) & (seg < 0.51)``, ``segEnv = seg < 0.1``, ``segObj = seg > 0.9``,
    and with ``erode`` (the reference's ``isLight``) ``segObj`` is eroded by a 7 x 7 box, what lies outside the image counting as set."""
    return tuple(_sg.loader_masks(_need(seg_u8, "seg_u8", "loader_masks"), bool(erode)))


def _numerator(u, bn, device):
    """fp32(0.95 - 0.1 u) per image, formed in double as the reference's Python floats are; ``None`` stays ``None`` (the TEST rule)"""
    if u is None:
        return None
    if isinstance(u, torch.Tensor):
        if u.numel() != bn:
            raise RuntimeError(f"sgrender: loader_scale_hdr: u must hold one value per image ({bn}), got {tuple(u.shape)}")
        return (0.95 - 0.1 * u.detach().to(device=device, dtype=torch.float64)).to(torch.float32).reshape(bn)
    vals = [float(x) for x in (u.tolist() if hasattr(u, "tolist") else u)] if not isinstance(u, (int, float)) else [float(u)] * bn
    if len(vals) != bn:
        raise RuntimeError(f"sgrender: loader_scale_hdr: u must hold one value per image ({bn}), got {len(vals)}")
    return torch.tensor([0.95 - 0.1 * x for x in vals], dtype=torch.float64).to(torch.float32).to(device)


def loader_scale_hdr(hdr, seg_u8, u=None, return_v: bool = False):
    """``(im [bn,3,H,W], scale [bn])`` from ``hdr [bn,H,W,3]`` fp32 in the reader's channel order and ``seg_u8 [bn,H,W,Cin]``.

    Per image ``v`` is element ``k = int(0.95 * W * H * 3)`` of the ascending sort of ``hdr * seg`` (``seg`` the continuous fp32 value of
    :func:`loader_masks`), ``scale = fp32(0.95 - 0.1 u) / max(v, 0.1)`` and ``im = clip(scale * hdr, 0, 1)[::-1]``.  ``u``: the TRAIN rule's
    ``np.random.random()`` per image, as host values (a sequence, or one number for all) or as a tensor (a device tensor keeps the call free of
    host work: it captures in a HIP graph); ``None`` is the TEST rule, ``0.95 - 0.05``.  ``return_v`` appends ``v [bn]``.

    NaN or inf in ``hdr`` are outside the domain (``v`` is then some element of the data; nothing faults); ``-0.0`` and ``0.0`` compare equal,
    so ``v`` may be either where both occur at the rank."""
    hdr, seg_u8 = _need(hdr, "hdr", "loader_scale_hdr"), _need(seg_u8, "seg_u8", "loader_scale_hdr")
    if hdr.dim() != 4:
        raise RuntimeError(f"sgrender: loader_scale_hdr: hdr must be [bn,H,W,3], got {tuple(hdr.shape)}")
    bn, H, W = hdr.shape[0], hdr.shape[1], hdr.shape[2]
    k = int(0.95 * W * H * 3)      # dataLoader.py:255, the very expression
    im, scale, v = _sg.loader_scale_hdr(hdr, seg_u8, _numerator(u, bn, hdr.device), k)
    return (im, scale, v) if return_v else (im, scale)


def loader_brdf_maps(albedo_u8=None, normal_u8=None, rough_u8=None):
    """``(albedo [bn,3,H,W], normal [bn,3,H,W], rough [bn,1,H,W])`` fp32 from HWC uint8; ``None`` in, ``None`` out.
    ``albedo = (0.5 * ((u8 - 127.5) / 127.5 + 1)) ** 2.2``; ``normal = n / sqrt(max(sum_c n^2, 1e-5))`` with ``n = (u8 - 127.5) / 127.5``;
    ``rough`` is channel 0 of ``(u8 - 127.5) / 127.5``."""
    given = [None if t is None else _need(t, name, "loader_brdf_maps") for t, name in ((albedo_u8, "albedo_u8"), (normal_u8, "normal_u8"), (rough_u8, "rough_u8"))]
    if all(t is None for t in given):
        raise RuntimeError("sgrender: loader_brdf_maps: at least one of albedo_u8, normal_u8, rough_u8 is needed")
    out = _sg.loader_brdf_maps(*given)
    return tuple(None if t is None else o for t, o in zip(given, out))


def loader_envmaps(env_raw, scale, env_ind=None, envHeight: int = 8, envWidth: int = 16):
    """``envmaps [bn,3,R,C,envHeight,envWidth]`` from ``env_raw [bn, R*16, C*32, 3]`` fp32 in the file's layout: the reference's reshape /
    ``transpose([4,0,2,1,3])`` / 2 x 2 block mean (8 x 16; 16 x 32 is the transpose alone), times ``scale [bn]``.  Output channel ``k`` is file
    channel ``k``.  ``env_ind [bn]`` (or ``[bn,1,1,1]``): an image whose entry is 0 has no env map -- it gives exact zeros and its raw block is
    never read.  Any other ratio or shape raises, naming the numpy composition that does the work on the host."""
    env_raw, scale = _need(env_raw, "env_raw", "loader_envmaps"), _need(scale, "scale", "loader_envmaps")
    ind = None if env_ind is None else _need(env_ind, "env_ind", "loader_envmaps")
    return _sg.loader_envmaps(env_raw, scale, ind, int(envHeight), int(envWidth))


def prepare_batch(raw, phase: str = "TRAIN", isLight: bool = True, u=None, envHeight: int = 8, envWidth: int = 16):
    """The ``dataBatch`` dict of ``dataLoader.BatchLoader.__getitem__`` (cascade 0) for a collated batch of raw arrays on the device.

    ``raw``: ``seg`` ``albedo`` ``normal`` ``rough`` uint8 ``[bn,H,W,c]``; ``im`` fp32 ``[bn,H,W,3]`` (the HDR reader's output after the resize);
    ``depth`` fp32 ``[bn,H,W]`` or ``[bn,1,H,W]``; with ``isLight`` ``envmaps`` fp32 ``[bn,R*16,C*32,3]`` and ``envmapsInd`` (one value per
    image); ``name`` is passed through when present.  ``phase='TRAIN'`` needs ``u`` (see :func:`loader_scale_hdr`), ``'TEST'`` takes none.
    Returns the reference's keys: ``albedo normal rough depth segArea segEnv segObj im`` and, with ``isLight``, ``envmaps envmapsInd``
    (``[bn,1,1,1]``).  ``segObj`` is eroded only with ``isLight``, as in the reference."""
    ph = str(phase).upper()
    if ph not in ("TRAIN", "TEST"):
        raise RuntimeError(f"sgrender: prepare_batch: unrecognized phase {phase!r} (TRAIN or TEST)")
    if ph == "TRAIN" and u is None:
        raise RuntimeError("sgrender: prepare_batch: phase 'TRAIN' needs u, the np.random.random() of scaleHdr per image")
    if ph == "TEST" and u is not None:
        raise RuntimeError("sgrender: prepare_batch: phase 'TEST' takes no u (its scale is 0.95 - 0.05)")
    need = ("seg", "im", "albedo", "normal", "rough", "depth") + (("envmaps", "envmapsInd") if isLight else ())
    missing = [k for k in need if k not in raw]
    if missing:
        raise RuntimeError(f"sgrender: prepare_batch: raw lacks {missing}")
    segArea, segEnv, segObj = loader_masks(raw["seg"], erode=bool(isLight))
    im, scale = loader_scale_hdr(raw["im"], raw["seg"], u)
    albedo, normal, rough = loader_brdf_maps(raw["albedo"], raw["normal"], raw["rough"])
    depth = _need(raw["depth"], "depth", "prepare_batch")
    bn, H, W = im.shape[0], im.shape[2], im.shape[3]
    if depth.numel() != bn * H * W:
        raise RuntimeError(f"sgrender: prepare_batch: depth must be [bn,H,W] = {(bn, H, W)}, got {tuple(depth.shape)}")
    batch = dict(albedo=albedo, normal=normal, rough=rough, depth=depth.reshape(bn, 1, H, W), segArea=segArea, segEnv=segEnv, segObj=segObj, im=im)
    if "name" in raw:
        batch["name"] = raw["name"]
    if isLight:
        ind = _need(raw["envmapsInd"], "envmapsInd", "prepare_batch").to(torch.float32).reshape(bn)
        batch["envmaps"] = loader_envmaps(raw["envmaps"], scale, ind, envHeight, envWidth)
        batch["envmapsInd"] = ind.reshape(bn, 1, 1, 1)
    return batch
