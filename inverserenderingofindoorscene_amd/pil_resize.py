"""PIL's antialiased resize of 8-bit images on the device, backed by libsgrender.so (csrc/sgr_pil_resize.hip).

  ``pil_resize(im_u8, size, filter, window, path)``          ``Image.resize(size, Image.ANTIALIAS)``: dataLoader.py:223-224
  ``iiw_resize_crop(im_u8, imHeight, imWidth, offset)``      iiwDataLoader.py:113-134, 208 for one decoded photograph
  ``iiw_geometry(nh, nw, imHeight, imWidth)``                :115-133: the resized size, the gap and the axis the crop moves on
  ``loader_resize(raw, size)``                               the uint8 entries of a ``prepare_batch`` raw dict

For 8-bit images PIL's resampler is integer arithmetic on a table of fixed-point coefficients that is formed in double, so the operator gives
PIL's BYTES, not an approximation of them: the tests compare with ``==``.  The ``Dataset`` hands over the decoded full-size arrays; nothing
visits the host after the first call of a geometry (which builds its two tables and copies them to the device), two runs are bit-identical,
an image does not depend on its batch, there is no autograd, and a repeated geometry captures in a HIP graph.  DESIGN.md section 8p states the
arithmetic, INTEGRATION.md section 19 the ``Dataset`` side."""
from __future__ import annotations

import numpy as np
import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["pil_resize", "iiw_resize_crop", "iiw_geometry", "loader_resize", "PIL_FILTERS", "PIL_RESIZE_PATHS"]

_sg = torch.ops.sgrender

PIL_FILTERS = ("lanczos", "bilinear", "bicubic", "box", "hamming")
PIL_RESIZE_PATHS = ("auto", "two_pass", "tiled")
_PIL_CODES = {1: "lanczos", 2: "bilinear", 3: "bicubic", 4: "box", 5: "hamming", 0: "nearest"}      # Image.Resampling's values


def _need(t, name, who):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"sgrender: {who}: {name} must be a tensor, got {type(t).__name__}")
    return t.detach()


def pil_resize(im_u8, size, filter="lanczos", window=None, path: str = "auto", box=None, reducing_gap=None):
    """uint8 ``[H,W,C]`` or ``[bn,H,W,C]`` (``C`` 1 or 3: PIL's ``L`` and ``RGB``) -> uint8 ``[h,w,C]`` / ``[bn,h,w,C]``: the bytes of
    ``Image.resize(size, filter)`` with ``size = (width, height)`` as PIL takes it.

    ``filter``: ``'lanczos'`` (the reference's ``Image.ANTIALIAS``), ``'bilinear'``, ``'bicubic'``, ``'box'``, ``'hamming'``, or PIL's integer
    code for one of them; ``'nearest'`` is another code path of PIL's and is refused.  ``window = (r0, c0, h, w)`` computes only that rectangle
    of the resized image (the horizontal pass visits only the source rows those output rows read); the bytes equal resize-then-slice.
    ``path``: ``'auto'``, or ``'two_pass'`` / ``'tiled'`` to force a route (the same bytes; ``'tiled'`` raises where the geometry does not fit
    its tiles).  ``C`` of 2 or 4 raises: PIL resizes ``LA`` / ``RGBA`` on its premultiplied-alpha route.  A source ``box`` and
    ``reducing_gap`` are not offered."""
    who = "pil_resize"
    if box is not None:
        raise RuntimeError(f"sgrender: {who}: a source box is not offered (the whole image is resized; slice the tensor first, which changes the border as PIL's box does not)")
    if reducing_gap is not None:
        raise RuntimeError(f"sgrender: {who}: reducing_gap is not offered (PIL then shrinks by Image.reduce first and gives other bytes)")
    im = _need(im_u8, "im_u8", who)
    try:
        width, height = (int(v) for v in size)
    except (TypeError, ValueError):
        raise RuntimeError(f"sgrender: {who}: size must be (width, height), got {size!r}") from None
    if isinstance(filter, (int, np.integer)) and not isinstance(filter, bool):
        if int(filter) not in _PIL_CODES:
            raise RuntimeError(f"sgrender: {who}: unknown filter code {int(filter)} (PIL's: 1 lanczos, 2 bilinear, 3 bicubic, 4 box, 5 hamming)")
        filter = _PIL_CODES[int(filter)]
    if window is not None:
        try:
            window = [int(v) for v in window]
        except (TypeError, ValueError):
            raise RuntimeError(f"sgrender: {who}: window must be (r0, c0, h, w), got {window!r}") from None
    return _sg.pil_resize(im, width, height, str(filter).lower(), window, str(path))


def iiw_geometry(nh: int, nw: int, imHeight: int, imWidth: int):
    """``(newH, newW, gap, along)`` of ``IIWLoader.loadImage`` for a photograph of ``nh`` rows and ``nw`` columns, by the reference's own float
    expressions (``np.ceil`` included): the image is resized so that one side equals the target and the other is at least it; ``gap`` is the
    excess along ``along`` (``'rows'`` | ``'columns'``), the axis the random crop moves on."""
    scaleW = float(imWidth) / float(nw)
    scaleH = float(imHeight) / float(nh)
    if scaleW > scaleH:
        newW = imWidth
        newH = int(np.ceil(scaleW * nh))
        return newH, newW, newH - imHeight, "rows"
    newH = imHeight
    newW = int(np.ceil(scaleH * nw))
    return newH, newW, newW - imWidth, "columns"


def iiw_resize_crop(im_u8, imHeight: int, imWidth: int, offset: int):
    """iiwDataLoader.py:113-134, 208 for ONE decoded photograph ``im_u8 [H,W,C]`` uint8: ``(crop_u8 [imHeight,imWidth,C], newH, newW, rs, cs)``.
    ``offset`` is the draw ``np.random.randint(gap + 1)`` -- ``rs`` where the rows exceed the target, ``cs`` where the columns do -- and must
    lie in ``0 .. gap``.  The crop is the operator's output window, so only its rectangle is computed.  ``iiw_image`` of ``crop_u8[None]`` is
    the reference's ``im``; ``newH`` and ``newW`` are what the judgements' coordinates are scaled by."""
    who = "iiw_resize_crop"
    im = _need(im_u8, "im_u8", who)
    if im.dim() != 3:
        raise RuntimeError(f"sgrender: {who}: im_u8 must be one photograph [H,W,C], got {tuple(im.shape)}")
    if im.shape[0] < 1 or im.shape[1] < 1:
        raise RuntimeError(f"sgrender: {who}: zero-sized photograph {tuple(im.shape)}")
    imHeight, imWidth, offset = int(imHeight), int(imWidth), int(offset)
    if imHeight < 1 or imWidth < 1:
        raise RuntimeError(f"sgrender: {who}: imHeight and imWidth must be positive, got {imHeight} x {imWidth}")
    newH, newW, gap, along = iiw_geometry(im.shape[0], im.shape[1], imHeight, imWidth)
    if not (newW >= imWidth and newH >= imHeight):      # the reference's assert
        raise RuntimeError(f"sgrender: {who}: the resized size {newH} x {newW} is below the target {imHeight} x {imWidth}")
    if not 0 <= offset <= gap:
        raise RuntimeError(f"sgrender: {who}: offset {offset} is outside 0 .. gap = {gap} (np.random.randint(gap + 1) along the {along})")
    rs, cs = (offset, 0) if along == "rows" else (0, offset)
    crop = pil_resize(im, (newW, newH), "lanczos", window=(rs, cs, imHeight, imWidth))
    return crop, newH, newW, rs, cs


_RESIZED_KEYS = ("seg", "albedo", "normal", "rough")


def loader_resize(raw, size):
    """A ``prepare_batch`` raw dict with its uint8 entries ``seg albedo normal rough`` (``[bn,H,W,c]``, the decoded full-size PNGs) resized to
    ``size = (width, height)`` as ``dataLoader.py:223-224`` does; every other entry passes through.  ``prepare_batch(loader_resize(raw, (320,
    240)), ...)`` is then the reference's batch built from the full-size files (``im`` and ``depth``, which the reference resizes with
    ``cv2.resize(INTER_AREA)``, come at the target size from the ``Dataset``)."""
    out = dict(raw)
    for key in _RESIZED_KEYS:
        if key in raw and raw[key] is not None:
            t = _need(raw[key], key, "loader_resize")
            if t.dtype != torch.uint8:
                raise RuntimeError(f"sgrender: loader_resize: {key} must be uint8 (the decoded PNG), got {t.dtype}")
            out[key] = pil_resize(t, size)
    return out
