"""The light decoders' last step, ``x_orig = dconvFinal(dpadFinal(dx6))`` of ``models.decoderLight`` (models.py:297-302, 334), backed by
libsgrender.so (csrc/sgr_light_final_conv.hip): the forward and the data gradient on the fp32-input matrix instruction, in exact fp32.

  ``light_final_conv(y, weight, bias)``         ``Conv2d(C -> O, k=3)(ReplicationPad2d(1)(y))`` for ``1 <= O <= 48``: the padded copy is never
                                                written, and the pad's backward is a gather, not an atomic scatter
  ``LightFinalConv(in_channels, out_channels)`` the module form; ``weight`` / ``bias`` load a checkpoint's ``dconvFinal.*``

Not in this operator, on purpose: no GroupNorm prologue (at 128 -> 36 channels the step is compute-bound about nine times over, so writing
``dx6`` costs a tenth of it: compose ``group_norm_relu`` / ``group_norm_relu_upcat``), no fused head (``light_heads`` already does all three
decoders in one launch) and no resize (when ``dx6``'s size differs from ``env``'s, models.py:332-333, compose
``group_norm_relu_resize(x, ..., size=env.shape[2:])`` first).  The BRDF decoders' three-output convolution is ``final_conv``.  DESIGN.md
section 8h states the arithmetic."""
from __future__ import annotations

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["light_final_conv", "LightFinalConv"]

_sg = torch.ops.sgrender

MAX_OUT_CHANNELS = 48      # three 16-wide tiles of the matrix instruction (csrc/sgr_light_final_conv.h)
MIN_CHANNELS, MAX_CHANNELS = 16, 256


def light_final_conv(y, weight, bias):
    """``F.conv2d(F.pad(y, (1, 1, 1, 1), mode='replicate'), weight, bias)`` for fp32 ``y [B,C,H,W]`` on a HIP device, ``weight [O,C,3,3]``,
    ``bias [O]``, ``1 <= O <= 48``, ``C`` a multiple of 16 in 16..256, ``H, W >= 1``: ``[B,O,H,W]``.  ``y`` may be non-contiguous (a
    channels-last map is read in place); the result is contiguous.  Differentiable with respect to all three; a gradient is computed only
    for those that require it, without atomics: two runs give the same bits, also under ``torch.use_deterministic_algorithms(True)``.  Any
    other convolution raises and names the composition to use; a CPU tensor raises: there is no fallback."""
    return _sg.light_final_conv(y, weight, bias)


class LightFinalConv(torch.nn.Module):
    """``nn.ReplicationPad2d(1)`` + ``nn.Conv2d(in_channels, out_channels, 3)`` as one operator.  The parameters are named and shaped as
    ``nn.Conv2d``'s, so ``load_state_dict`` takes a reference checkpoint's ``dconvFinal.weight`` / ``dconvFinal.bias`` under the same prefix,
    and they are initialised as ``nn.Conv2d`` initialises them.  ``out_channels`` is ``3 * SGNum`` for the axis decoder and ``SGNum`` for
    the other two."""

    def __init__(self, in_channels: int = 128, out_channels: int = 36):
        super().__init__()
        if not (MIN_CHANNELS <= int(in_channels) <= MAX_CHANNELS and int(in_channels) % 16 == 0):
            raise ValueError(f"sgrender: LightFinalConv: in_channels {in_channels} is not a multiple of 16 in {MIN_CHANNELS}..{MAX_CHANNELS}; "
                             "use nn.ReplicationPad2d + nn.Conv2d")
        if not 1 <= int(out_channels) <= MAX_OUT_CHANNELS:
            raise ValueError(f"sgrender: LightFinalConv: out_channels {out_channels} is outside 1..{MAX_OUT_CHANNELS}; use nn.ReplicationPad2d + nn.Conv2d")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        ref = torch.nn.Conv2d(self.in_channels, self.out_channels, 3)
        self.weight = torch.nn.Parameter(ref.weight.detach().clone())
        self.bias = torch.nn.Parameter(ref.bias.detach().clone())

    def forward(self, y):
        return light_final_conv(y, self.weight, self.bias)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, kernel_size=(3, 3), padding=replicate"
