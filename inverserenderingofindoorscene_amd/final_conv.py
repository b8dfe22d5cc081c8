"""The BRDF decoders' last step, ``x_orig = dconvFinal(dpadFinal(dx6))`` (models.py:155-156, 187), backed by libsgrender.so
(csrc/sgr_final_conv.hip).

  ``final_conv(y, weight, bias)``                                  ``Conv2d(C -> 3, k=3)(ReplicationPad2d(1)(y))``: the padded copy is never
                                                                   written, and the pad's backward is a gather, not an atomic scatter
  ``group_norm_relu_final_conv(x, gn_weight, gn_bias, num_groups,  the same from ``dconv6``'s output: ``relu(dgn6(x))`` is formed on load and
                               weight, bias, eps)``                never written either (models.py:183, 187)
  ``FinalConv(in_channels)``                                       the module form; ``weight`` / ``bias`` load a checkpoint's ``dconvFinal.*``

When the reference's final resize to the image fires (``dx6``'s size differs from the image's, models.py:185-186), the resized map has to
exist: compose ``group_norm_relu_resize(x, ..., size=im.shape[2:])`` and ``final_conv``.  ``decoderLight``'s final convolution (128 -> 12 /
36 channels) is outside the domain: it is ``light_final_conv``.  The heads stay ``brdf_heads``.  DESIGN.md section 8g states the arithmetic."""
from __future__ import annotations

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)
from .gn_stage import GroupNormReLU

__all__ = ["final_conv", "group_norm_relu_final_conv", "FinalConv"]

_sg = torch.ops.sgrender

MAX_CHANNELS = 256      # the weight tile [C,3,3,3] stays in LDS (csrc/sgr_final_conv.h)


def final_conv(y, weight, bias):
    """``F.conv2d(F.pad(y, (1, 1, 1, 1), mode='replicate'), weight, bias)`` for fp32 ``y [B,C,H,W]`` on a HIP device, ``weight [3,C,3,3]``,
    ``bias [3]``, ``C <= 256``, ``H, W >= 1``: ``[B,3,H,W]``.  ``y`` may be non-contiguous (a channels-last map is read in place); the result
    is contiguous.  Differentiable with respect to all three; a gradient is computed only for those that require it, without atomics: two
    runs give the same bits.  Any other convolution raises and names the composition to use; a CPU tensor raises: there is no fallback."""
    return _sg.final_conv(y, weight, bias, None, None, 1, 1e-5)[0]


def group_norm_relu_final_conv(x, gn_weight, gn_bias, num_groups: int, weight, bias, eps: float = 1e-5):
    """``final_conv(group_norm_relu(x, gn_weight, gn_bias, num_groups, eps), weight, bias)``, bit for bit in the value and in all five
    gradients, without the normalised map: the forward reads ``x`` twice (moments, convolution) and writes three planes; the node keeps
    ``x``, the GroupNorm parameters, the per-group statistics and ``weight``.  The backward is ``sgrender::final_conv_bwd`` with the same
    prologue followed by ``sgrender::gn_stage_bwd``."""
    return _sg.final_conv(x, weight, bias, gn_weight, gn_bias, int(num_groups), float(eps))[0]


class FinalConv(torch.nn.Module):
    """``nn.ReplicationPad2d(1)`` + ``nn.Conv2d(in_channels, 3, 3)`` as one operator.  The parameters are named and shaped as ``nn.Conv2d``'s,
    so ``load_state_dict`` takes a reference checkpoint's ``dconvFinal.weight`` / ``dconvFinal.bias`` under the same prefix, and they are
    initialised as ``nn.Conv2d`` initialises them.  ``forward(y)`` is :func:`final_conv`; ``forward(x, gn=stage)`` with an
    ``sgr.GroupNormReLU`` is :func:`group_norm_relu_final_conv` with that stage's parameters."""

    def __init__(self, in_channels: int = 64):
        super().__init__()
        if not 1 <= int(in_channels) <= MAX_CHANNELS:
            raise ValueError(f"sgrender: FinalConv: in_channels {in_channels} is outside 1..{MAX_CHANNELS}; use nn.ReplicationPad2d + nn.Conv2d")
        self.in_channels = int(in_channels)
        ref = torch.nn.Conv2d(self.in_channels, 3, 3)
        self.weight = torch.nn.Parameter(ref.weight.detach().clone())
        self.bias = torch.nn.Parameter(ref.bias.detach().clone())

    def forward(self, x, gn=None):
        if gn is None:
            return final_conv(x, self.weight, self.bias)
        if not isinstance(gn, GroupNormReLU):
            raise RuntimeError("sgrender: FinalConv: gn= takes an sgr.GroupNormReLU (the stage whose output this convolution reads)")
        return group_norm_relu_final_conv(x, gn.weight, gn.bias, gn.num_groups, self.weight, self.bias, gn.eps)

    def extra_repr(self):
        return f"{self.in_channels}, 3, kernel_size=(3, 3), padding=replicate"
