"""The repeated stage of the reference's network classes around its convolution, backed by libsgrender.so (csrc/sgr_gn_stage.hip).

  ``group_norm_relu(x, weight, bias, num_groups, eps)``               ``F.relu(gn(x))`` of ``models.encoder0`` / ``encoderLight``
                                                                      (models.py:122-127, 262-267 and the two ``preProcess`` pairs)
  ``group_norm_relu_upcat(x, weight, bias, num_groups, skip, eps)``   ``F.interpolate(torch.cat([F.relu(dgnK(x)), skip], 1), scale_factor=2,
                                                                      mode='bilinear')`` of ``models.decoder0`` / ``decoderLight``
                                                                      (models.py:160-183, 307-330): what ``dconv{K+1}`` reads
  ``group_norm_relu_resize_upcat(x, weight, bias, num_groups, skip, eps)``   the same stage with a ``skip`` of another size: the normalised
                                                                      map is resized to it first (models.py:165-166 and its siblings)
  ``group_norm_relu_resize(x, weight, bias, num_groups, size, eps)``  ``F.interpolate(F.relu(dgn6(x)), size, mode='bilinear')``: the final
                                                                      stage's resize to the image (models.py:183-186, 330-333)
  ``GroupNormReLU(num_groups, num_channels, eps, resize=False)``      the module form; ``weight`` / ``bias`` load a checkpoint's ``gnK.*``
  ``group_norm_relu_upcat_siblings(xs, weights, biases, num_groups, skip, eps)``   the upcat stage of ``D`` sibling decoders on one ``skip``
  ``group_norm_relu_resize_upcat_siblings(...)``                      in one call (the reference runs four ``decoder0`` and three
  ``SiblingGroupNormReLU(stages, resize=False)``                      ``decoderLight`` instances on the same encoder features)

Eager PyTorch spends four launches forward on a decoder stage (GroupNorm, ReLU, ``cat``, ``upsample_bilinear2d``) and keeps three maps for
the backward; here it is two launches forward and three backward, and ``x`` with the per-group statistics is all that is kept.  The resize
forms are two launches forward and four (without a skip: three) backward and keep the same.  DESIGN.md section 8e states the arithmetic.

Mixed precision: the two same-size forms also take ``x`` and ``skip`` in ``torch.bfloat16`` (together; ``weight`` and
``bias`` stay fp32) and return bf16 -- the fp32 result on the upcast input, rounded once, bit for bit, with ``dx`` / ``dskip`` in bf16 and
``dweight`` / ``dbias`` in fp32; the node keeps the bf16 ``x``.  Under ``torch.autocast('cuda', dtype=torch.bfloat16)`` a bf16 ``x`` stays bf16
and ``skip`` and the parameters are cast as needed; the resize forms proper run in fp32 there.  fp16 is refused as before.

Siblings: at stage ``k`` the four BRDF decoders (three light decoders) do the same thing on the same shapes with the
same skip; only ``x`` and the ``dgnK`` parameters differ.  The sibling forms run that stage for all of them with the launches of one
(two forward, three -- resize: four -- backward), read a skip channel once, and return ONE ``dskip``, the cotangents' contributions added
in sibling order in fp32.  Every other result is the single form's, bit for bit."""
from __future__ import annotations

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["group_norm_relu", "group_norm_relu_upcat", "group_norm_relu_resize", "group_norm_relu_resize_upcat", "GroupNormReLU",
           "group_norm_relu_upcat_siblings", "group_norm_relu_resize_upcat_siblings", "SiblingGroupNormReLU"]

MAX_SIBLINGS = 8

_sg = torch.ops.sgrender


def group_norm_relu(x, weight, bias, num_groups: int, eps: float = 1e-5):
    """``relu(F.group_norm(x, num_groups, weight, bias, eps))`` for fp32 or bf16 ``x [B,C,H,W]`` on a HIP device, fp32 ``weight`` / ``bias [C]``,
    ``C % num_groups == 0``.  ``x`` may be non-contiguous (a channels-last convolution output is read in place); the result is contiguous.
    Differentiable with respect to ``x``, ``weight`` and ``bias``; a gradient is computed only for those that require it.  A CPU tensor
    raises: there is no fallback."""
    return _sg.gn_stage(x, weight, bias, None, int(num_groups), float(eps))[0]


def group_norm_relu_upcat(x, weight, bias, num_groups: int, skip, eps: float = 1e-5):
    """``F.interpolate(torch.cat([group_norm_relu(x, ...), skip], 1), scale_factor=2, mode='bilinear')``: ``[B, C + Cs, 2H, 2W]`` from
    ``x [B,C,H,W]`` and ``skip [B,Cs,H,W]``, ``Cs >= 1``, both fp32 or both bf16 on a HIP device and possibly non-contiguous.  Differentiable with respect
    to ``x``, ``weight``, ``bias`` and ``skip``.

    A ``skip`` of another ``H, W`` raises: the reference resizes the normalised map first in that case (models.py:165-166 and its
    siblings), and that branch stays the caller's -- ``group_norm_relu``, then torch's ``interpolate`` / ``cat``."""
    if skip is None:
        raise RuntimeError("sgrender: group_norm_relu_upcat: skip is None; group_norm_relu is the form without a skip")
    return _sg.gn_stage(x, weight, bias, skip, int(num_groups), float(eps))[0]


def group_norm_relu_resize_upcat(x, weight, bias, num_groups: int, skip, eps: float = 1e-5):
    """``F.interpolate(torch.cat([F.interpolate(group_norm_relu(x, ...), [Hs, Ws], mode='bilinear'), skip], 1), scale_factor=2,
    mode='bilinear')``: ``[B, C + Cs, 2Hs, 2Ws]`` from ``x [B,C,H,W]`` and ``skip [B,Cs,Hs,Ws]`` -- a decoder stage with the reference's
    ``if`` taken (models.py:165-166, 312-313 and their siblings).  Per axis ``H <= Hs <= 2H`` and ``W <= Ws <= 2W``; anything else raises and
    stays the caller's composition.  With ``(Hs, Ws) == (H, W)`` the reference skips the resize and this is :func:`group_norm_relu_upcat`,
    bit for bit.  Differentiable with respect to ``x``, ``weight``, ``bias`` and ``skip``; the node keeps ``x``, the parameters and the
    per-group statistics, no resized or concatenated map and no ``skip``."""
    if skip is None:
        raise RuntimeError("sgrender: group_norm_relu_resize_upcat: skip is None; group_norm_relu_resize is the form without a skip")
    if skip.dim() == 4 and x.dim() == 4 and tuple(skip.shape[2:]) == tuple(x.shape[2:]):
        return _sg.gn_stage(x, weight, bias, skip, int(num_groups), float(eps))[0]
    h, w = (int(skip.shape[2]), int(skip.shape[3])) if skip.dim() == 4 else (0, 0)
    return _sg.gn_resize(x, weight, bias, skip, int(num_groups), h, w, float(eps))[0]


def group_norm_relu_resize(x, weight, bias, num_groups: int, size, eps: float = 1e-5):
    """``F.interpolate(group_norm_relu(x, ...), size, mode='bilinear')``: ``[B, C, Hs, Ws]`` for ``size = (Hs, Ws)`` in the same domain -- the
    final stage's resize to the image (models.py:185-186, 332-333).  ``size == (H, W)`` is :func:`group_norm_relu`, bit for bit."""
    h, w = (int(v) for v in size)
    if x.dim() == 4 and (h, w) == tuple(x.shape[2:]):
        return _sg.gn_stage(x, weight, bias, None, int(num_groups), float(eps))[0]
    return _sg.gn_resize(x, weight, bias, None, int(num_groups), h, w, float(eps))[0]


class GroupNormReLU(torch.nn.Module):
    """``nn.GroupNorm(num_groups, num_channels, eps)`` followed by ReLU as one operator.  The parameters are named as ``nn.GroupNorm``'s, so
    ``load_state_dict`` takes a reference checkpoint's ``gnK.weight`` / ``gnK.bias`` (``dgnK.*``) under the same prefix.
    ``forward(x)`` is :func:`group_norm_relu`; ``forward(x, skip)`` is :func:`group_norm_relu_upcat`.  With ``resize=True`` a ``skip`` of
    another size is accepted (:func:`group_norm_relu_resize_upcat`) and ``forward(x, size=(h, w))`` is :func:`group_norm_relu_resize`."""

    def __init__(self, num_groups: int, num_channels: int, eps: float = 1e-5, resize: bool = False):
        super().__init__()
        if num_channels % num_groups != 0:
            raise ValueError(f"sgrender: GroupNormReLU: num_channels {num_channels} is not a multiple of num_groups {num_groups}")
        self.num_groups, self.num_channels, self.eps = int(num_groups), int(num_channels), float(eps)
        self.resize = bool(resize)
        self.weight = torch.nn.Parameter(torch.ones(num_channels))
        self.bias = torch.nn.Parameter(torch.zeros(num_channels))

    def forward(self, x, skip=None, size=None):
        if size is not None:
            if not self.resize or skip is not None:
                raise RuntimeError("sgrender: GroupNormReLU: size= is the final-stage form of resize=True and takes no skip")
            return group_norm_relu_resize(x, self.weight, self.bias, self.num_groups, size, self.eps)
        if skip is None:
            return group_norm_relu(x, self.weight, self.bias, self.num_groups, self.eps)
        if self.resize:
            return group_norm_relu_resize_upcat(x, self.weight, self.bias, self.num_groups, skip, self.eps)
        return group_norm_relu_upcat(x, self.weight, self.bias, self.num_groups, skip, self.eps)

    def extra_repr(self):
        return f"{self.num_groups}, {self.num_channels}, eps={self.eps}" + (", resize=True" if self.resize else "")


def _check_siblings(who, xs, weights, biases, num_groups, skip):
    """the refusals of the sibling forms, before any launch (the operators repeat them for callers of ``torch.ops``).  Inside an autocast
    region siblings of different floating dtypes are let through: the operators' autocast rules cast the lists to one dtype first."""
    xs, weights, biases = list(xs), list(weights), list(biases)
    if not 1 <= len(xs) <= MAX_SIBLINGS:
        raise RuntimeError(f"sgrender: {who}: the number of siblings must be 1 .. {MAX_SIBLINGS}, got {len(xs)}")
    if len(weights) != len(xs) or len(biases) != len(xs):
        raise RuntimeError(f"sgrender: {who}: {len(xs)} xs but {len(weights)} weights and {len(biases)} biases")
    if skip is None:
        raise RuntimeError(f"sgrender: {who}: skip is None; the sibling forms share one skip (group_norm_relu is the form without a skip)")
    for d, x in enumerate(xs):
        if tuple(x.shape) != tuple(xs[0].shape):
            raise RuntimeError(f"sgrender: {who}: the siblings must have one shape, got xs[0] {tuple(xs[0].shape)} and xs[{d}] {tuple(x.shape)}")
        if x.dtype != xs[0].dtype and not (torch.is_autocast_enabled("cuda") and x.is_cuda):      # autocast gives the siblings one dtype; the operator checks after it
            raise RuntimeError(f"sgrender: {who}: the siblings must have one dtype, got xs[0] {xs[0].dtype} and xs[{d}] {x.dtype}")
        if x.device != xs[0].device:
            raise RuntimeError(f"sgrender: {who}: tensors on different devices (xs[0] {xs[0].device}, xs[{d}] {x.device})")
    if xs[0].dim() == 4 and (int(num_groups) <= 0 or xs[0].shape[1] % int(num_groups) != 0):
        raise RuntimeError(f"sgrender: {who}: the channel count {xs[0].shape[1]} is not a multiple of num_groups {num_groups}")
    return xs, weights, biases


def group_norm_relu_upcat_siblings(xs, weights, biases, num_groups: int, skip, eps: float = 1e-5):
    """:func:`group_norm_relu_upcat` for ``D`` sibling decoders at once: a tuple of ``D`` tensors ``[B, C + Cs, 2H, 2W]`` from ``xs[d] [B,C,H,W]``
    (one shape, dtype and device; fp32, or bf16 with a bf16 ``skip``), fp32 ``weights[d]`` / ``biases[d] [C]`` and ONE ``skip [B,Cs,H,W]``,
    ``1 <= D <= 8``.  ``outs[d]`` is ``group_norm_relu_upcat(xs[d], weights[d], biases[d], num_groups, skip, eps)`` bit for bit, and so are the
    gradients of ``xs[d]``, ``weights[d]`` and ``biases[d]``; the gradient of ``skip`` is ``((s_0 + s_1) + s_2) + ...`` in fp32, ``s_d`` the
    single form's contribution for the cotangent of ``outs[d]`` -- what autograd's ``D - 1`` adds would give in that order, without the
    ``D`` maps.  A result left out of the loss is left out of the sum.  One autograd node keeps the ``xs``, the parameters and the
    ``[D,B,G,4]`` statistics; ``skip`` is not kept."""
    xs, weights, biases = _check_siblings("group_norm_relu_upcat_siblings", xs, weights, biases, num_groups, skip)
    return tuple(_sg.gn_stage_siblings(xs, weights, biases, skip, int(num_groups), float(eps))[0])


def group_norm_relu_resize_upcat_siblings(xs, weights, biases, num_groups: int, skip, eps: float = 1e-5):
    """:func:`group_norm_relu_resize_upcat` for ``D`` siblings: ``skip [B,Cs,Hs,Ws]`` with ``H <= Hs <= 2H`` and ``W <= Ws <= 2W`` per axis (fp32
    only); anything else raises.  With ``(Hs, Ws) == (H, W)`` it is :func:`group_norm_relu_upcat_siblings`, bit for bit."""
    who = "group_norm_relu_resize_upcat_siblings"
    xs, weights, biases = _check_siblings(who, xs, weights, biases, num_groups, skip)
    if skip.dim() == 4 and xs[0].dim() == 4:
        (h, w), (hs, ws) = xs[0].shape[2:], skip.shape[2:]
        if (hs, ws) == (h, w):
            return tuple(_sg.gn_stage_siblings(xs, weights, biases, skip, int(num_groups), float(eps))[0])
        if not (h <= hs <= 2 * h and w <= ws <= 2 * w):
            raise RuntimeError(f"sgrender: {who}: the skip {hs}x{ws} is outside the resize domain of x {h}x{w} (H <= Hs <= 2H and W <= Ws <= 2W per axis); "
                               "any other size stays the caller's composition")
    return tuple(_sg.gn_resize_siblings(xs, weights, biases, skip, int(num_groups), float(eps))[0])


class SiblingGroupNormReLU(torch.nn.Module):
    """``D`` :class:`GroupNormReLU` modules -- the ``dgnK`` of ``D`` sibling decoders -- behind one fused call.  ``stages`` are kept as an
    ``nn.ModuleList`` and their parameters are used as they are: ``stages[d]`` may stay a member of its decoder too, and a reference
    checkpoint's ``dgnK.*`` keys load per sibling exactly as before (here under ``stages.<d>.``).  ``forward(xs, skip)`` returns the tuple of
    :func:`group_norm_relu_upcat_siblings`; with ``resize=True`` a ``skip`` of another size is accepted
    (:func:`group_norm_relu_resize_upcat_siblings`)."""

    def __init__(self, stages, resize: bool = False):
        super().__init__()
        stages = list(stages)
        if not 1 <= len(stages) <= MAX_SIBLINGS:
            raise ValueError(f"sgrender: SiblingGroupNormReLU: the number of siblings must be 1 .. {MAX_SIBLINGS}, got {len(stages)}")
        for m in stages:
            if not isinstance(m, GroupNormReLU):
                raise TypeError(f"sgrender: SiblingGroupNormReLU: stages must be GroupNormReLU modules, got {type(m).__name__}")
            if (m.num_groups, m.num_channels, m.eps) != (stages[0].num_groups, stages[0].num_channels, stages[0].eps):
                raise ValueError("sgrender: SiblingGroupNormReLU: the siblings must share num_groups, num_channels and eps")
        self.stages = torch.nn.ModuleList(stages)
        self.resize = bool(resize)

    def forward(self, xs, skip):
        s0 = self.stages[0]
        f = group_norm_relu_resize_upcat_siblings if self.resize else group_norm_relu_upcat_siblings
        return f(xs, [m.weight for m in self.stages], [m.bias for m in self.stages], s0.num_groups, skip, s0.eps)

    def extra_repr(self):
        return f"siblings={len(self.stages)}" + (", resize=True" if self.resize else "")
