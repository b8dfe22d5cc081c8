"""The output activations of the four BRDF decoders, backed by libsgrender.so (csrc/sgr_brdf_heads.hip).

  ``brdf_heads(xAlbedo, xNormal, xRough, xDepth, unit=True)``   the tail of ``models.decoder0.forward`` (models.py:189-203) for the four
                                                                decoders at once, with the ``0.5 * (x + 1)`` the wrappers put on the
                                                                albedo and depth decoders (wrapperBRDF.py, wrapperBRDFLight.py:112-115,
                                                                wrapperNYU.py:89-92, wrapperIIW.py:83-86, testReal.py:360-363,452-455)
  ``brdf_head(x_orig, mode)``                                   one decoder, ``decoder0``'s own return value

The reference spends about 22 eager launches forward and as many backward on this, over twelve full-resolution planes; here it is one
launch each way, and the backward recomputes ``tanh`` from the saved decoder outputs.  DESIGN.md section 8d states the arithmetic."""
from __future__ import annotations

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["brdf_heads", "brdf_head"]

_sg = torch.ops.sgrender

_MODE_SLOT = {0: 0, 1: 1, 2: 2, 4: 3}      # decoder0's mode -> position among (albedo, normal, rough, depth)


def brdf_heads(xAlbedo, xNormal, xRough, xDepth, unit: bool = True):
    """``(albedoPred [B,3,H,W], normalPred [B,3,H,W], roughPred [B,1,H,W], depthPred [B,1,H,W])`` from the ``dconvFinal`` outputs of the
    four decoders (modes 0, 1, 2, 4), fp32 ``[B,3,H,W]`` each on a HIP device, sharing ``B, H, W``.

    With ``s(x) = clamp(1.01 tanh(x), -1, 1)``: albedo ``s(x_c)``; normal ``t / max(|t|, 1e-6)`` with ``t_c = s(x_c)``; roughness the
    channel mean of ``s(x_c)``; depth ``s`` of the channel mean of ``x``.  ``unit=True`` returns albedo and depth as the wrappers use them,
    ``0.5 * (decoder + 1)``; ``unit=False`` returns the decoders' own values.

    Any ``x*`` may be ``None``: its result is ``None`` and nothing is read or written for it (``wrapperNYU.py`` uses normal and depth
    only); all four ``None`` raises.  Differentiable with respect to the ``x*`` that require grad, and a gradient plane is allocated only
    for those.  A CPU tensor raises; non-contiguous inputs (channels-last convolution outputs) are accepted."""
    xs = (xAlbedo, xNormal, xRough, xDepth)
    if all(x is None for x in xs):
        raise RuntimeError("sgrender: brdf_heads: every decoder output is None")
    out = _sg.brdf_heads(xAlbedo, xNormal, xRough, xDepth, bool(unit))
    return tuple(y if x is not None else None for x, y in zip(xs, out))


def brdf_head(x_orig, mode: int):
    """``models.decoder0``'s return value for its ``dconvFinal`` output ``x_orig`` and its ``mode``: 0 albedo, 1 normal, 2 roughness,
    4 depth -- :func:`brdf_heads` with one term and ``unit=False``.  Mode 3 (``softmax``, ``isSeg``) is refused: no script of the
    reference constructs it."""
    mode = int(mode)
    if mode == 3:
        raise RuntimeError("sgrender: brdf_head: mode 3 (softmax, the segmentation head) is not supported; modes are 0 albedo, 1 normal, 2 roughness, 4 depth")
    if mode not in _MODE_SLOT:
        raise RuntimeError(f"sgrender: brdf_head: unknown decoder0 mode {mode}; modes are 0 albedo, 1 normal, 2 roughness, 4 depth")
    if x_orig is None:
        raise RuntimeError("sgrender: brdf_head: the decoder output is None")
    xs = [None] * 4
    xs[_MODE_SLOT[mode]] = x_orig
    return brdf_heads(*xs, unit=False)[_MODE_SLOT[mode]]
