"""The cascade-1 BRDF encoder's input, backed by libsgrender.so (csrc/sgr_brdf_input.hip).

  ``brdf_encoder_input(...)``    wrapperBRDF.py:56-100 (= wrapperBRDFLight.py:58-92,106-108), the in-memory form of
                                 trainFineTune{NYU,IIW}_cascade1.py:368-374 and the inference form of testReal.py:439-449

The reference assembles this tensor with about 30 eager launches (six conditional bilinear resizes, an adaptive pooling,
``LSregressDiffSpec``, two mean-normalisations, a 17-channel concat); here it is at most three, nothing visits the host and two runs are
bit-identical.  DESIGN.md section 8c states the arithmetic."""
from __future__ import annotations

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["brdf_encoder_input"]

_sg = torch.ops.sgrender


def brdf_encoder_input(imBatch, albedoPre, normalPre, roughPre, depthPre, diffusePre, specularPre, size=None, regress: bool = True, normalize: bool = True,
                       remap: bool = False):
    """``(inputBatch [bn,17,H,W], coef [bn,2])``: the tensor the cascade-1 BRDF encoder reads, in the channel order of wrapperBRDF.py:98-100
    (im 3, albedo 3, normal 3, rough 1, depth 1, diffuse 3, specular 3), and the ``LSregressDiffSpec`` coefficients ``(c_im c_d, c_im c_s)``
    that scaled the last six channels (all ones with ``regress=False``).

    ``imBatch [bn,3,H,W]``; ``size`` plays the part of ``(opt.imHeight, opt.imWidth)`` and must be the image's ``(H, W)`` (its default): the
    reference concatenates the image unresized.  ``albedoPre, normalPre [bn,3,h,w]`` and ``roughPre, depthPre [bn,1,h,w]`` share one
    ``(h, w)`` -- a narrowing of the reference, which resizes each on its own but is never called otherwise -- and ``diffusePre,
    specularPre`` are ``[bn,3,R,C]``.  A map of the image's size is taken as it is, one smaller along an axis is resized with torch's
    bilinear rule (``align_corners=False``); any other size raises, as the reference's ``torch.cat`` would.

    The three call sites: the wrappers use the defaults; the fine-tuning scripts pass raw cascade-0 predictions with ``remap=True``
    (``0.5 (x + 1)`` on normal and rough, before the resize); testReal.py:439-449 is ``regress=False, normalize=False, remap=True``.

    Forward only: every input is data in the reference, so the inputs are detached, as :func:`light_encoder_input` does.  fp32 tensors on
    a HIP device; a CPU tensor raises; non-contiguous inputs are accepted."""
    if imBatch.dim() != 4:
        raise RuntimeError(f"sgrender: brdf_encoder_input: imBatch must be [bn,3,H,W], got {tuple(imBatch.shape)}")
    if size is not None and (int(size[0]), int(size[1])) != (imBatch.shape[2], imBatch.shape[3]):
        raise RuntimeError(f"sgrender: brdf_encoder_input: size {tuple(size)} must be the image's {tuple(imBatch.shape[2:])}: the image is concatenated unresized")
    maps = (albedoPre, normalPre, roughPre, depthPre)
    if any(t.dim() != 4 or tuple(t.shape[2:]) != tuple(albedoPre.shape[2:]) for t in maps):
        raise RuntimeError("sgrender: brdf_encoder_input: albedoPre, normalPre, roughPre and depthPre must share one size, got "
                           + ", ".join(str(tuple(t.shape)) for t in maps))
    return tuple(_sg.brdf_encoder_input(imBatch.detach(), albedoPre.detach(), normalPre.detach(), roughPre.detach(), depthPre.detach(), diffusePre.detach(),
                                        specularPre.detach(), bool(regress), bool(normalize), bool(remap)))
