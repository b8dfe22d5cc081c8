"""The encoders' down-sampling layers -- ``Conv2d(C -> O, 4, stride=2)`` behind ``ReplicationPad2d(1)`` or ``ZeroPad2d(1)``: ``encoder0.conv1`` /
``conv2`` and ``encoderLight.preProcess[1]`` / ``[5]`` / ``conv1`` of models.py:93-115, 122-126, 213-246, 254-266 -- backed by libsgrender.so
(csrc/sgr_encoder_conv.hip): the forward and both large gradients on the fp32-input matrix instruction, in exact fp32.

  ``encoder_conv(x, weight, bias, padding='replicate')``   ``F.conv2d(F.pad(x, (1, 1, 1, 1), mode=padding), weight, bias, stride=2)``: the padded
                                                           copy is never written, and the pad's backward is a gather, not an atomic scatter
  ``EncoderConv(in_channels, out_channels, padding)``      the module form; ``weight`` / ``bias`` load a checkpoint's ``conv1.*`` / ``conv2.*`` /
                                                           ``preProcess.1.*`` / ``preProcess.5.*``

Not in this operator, on purpose: the deeper layers (``C >= 128 -> O >= 256`` on planes of 60 x 80 and smaller).  Their pads are zero pads,
whose backward is a slice and deterministic, their padded copies are small, and with at most 4800 output pixels an image they are plain
GEMMs: they stay ``F.pad`` + ``F.conv2d``.  DESIGN.md section 8i states the arithmetic."""
from __future__ import annotations

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["encoder_conv", "EncoderConv"]

_sg = torch.ops.sgrender

MAX_CHANNELS = 160                             # csrc/sgr_encoder_conv.h
MIN_OUT_CHANNELS, MAX_OUT_CHANNELS = 16, 128   # a multiple of 16: whole tiles of the matrix instruction
PAD_MODES = {"replicate": 0, "zeros": 1}
_COMPOSE = "compose F.pad(x, (1, 1, 1, 1), mode=...) and F.conv2d(., stride=2) instead"


def _pad_mode(padding, who):
    if padding not in PAD_MODES:
        raise ValueError(f"sgrender: {who}: padding {padding!r} is not one of {sorted(PAD_MODES)}; {_COMPOSE}")
    return PAD_MODES[padding]


def encoder_conv(x, weight, bias, padding="replicate"):
    """``F.conv2d(F.pad(x, (1, 1, 1, 1), mode=padding), weight, bias, stride=2)`` (``'zeros'`` is ``F.pad``'s ``'constant'``) for fp32
    ``x [B,C,H,W]`` on a HIP device, ``weight [O,C,4,4]``, ``bias [O]``, ``1 <= C <= 160``, ``O`` a multiple of 16 in 16..128, ``H, W >= 2``:
    ``[B,O,H//2,W//2]``.  ``x`` may be non-contiguous (a channels-last map or a slice is read in place); the result is contiguous.
    Differentiable with respect to all three; a gradient is computed only for those that require it, without atomics: two runs give the
    same bits, also under ``torch.use_deterministic_algorithms(True)``.  Any other convolution raises and names the composition to use; a
    CPU tensor raises: there is no fallback."""
    return _sg.encoder_conv(x, weight, bias, _pad_mode(padding, "encoder_conv"))


class EncoderConv(torch.nn.Module):
    """``nn.ReplicationPad2d(1)`` (or ``nn.ZeroPad2d(1)``) + ``nn.Conv2d(in_channels, out_channels, 4, stride=2)`` as one operator.  The
    parameters are named and shaped as ``nn.Conv2d``'s, so ``load_state_dict`` takes a reference checkpoint's ``conv1.*`` / ``conv2.*`` /
    ``preProcess.1.*`` / ``preProcess.5.*`` under the same prefix, and they are initialised as ``nn.Conv2d`` initialises them."""

    def __init__(self, in_channels: int, out_channels: int, padding: str = "replicate"):
        super().__init__()
        _pad_mode(padding, "EncoderConv")
        if not 1 <= int(in_channels) <= MAX_CHANNELS:
            raise ValueError(f"sgrender: EncoderConv: in_channels {in_channels} is outside 1..{MAX_CHANNELS} (the deeper encoder layers are plain "
                             f"GEMMs with small zero-padded copies); {_COMPOSE}")
        if not (MIN_OUT_CHANNELS <= int(out_channels) <= MAX_OUT_CHANNELS and int(out_channels) % 16 == 0):
            raise ValueError(f"sgrender: EncoderConv: out_channels {out_channels} is not a multiple of 16 in {MIN_OUT_CHANNELS}..{MAX_OUT_CHANNELS}; "
                             f"{_COMPOSE}")
        self.in_channels, self.out_channels, self.padding = int(in_channels), int(out_channels), padding
        ref = torch.nn.Conv2d(self.in_channels, self.out_channels, 4, stride=2)
        self.weight = torch.nn.Parameter(ref.weight.detach().clone())
        self.bias = torch.nn.Parameter(ref.bias.detach().clone())

    def forward(self, x):
        return encoder_conv(x, self.weight, self.bias, self.padding)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, kernel_size=(4, 4), stride=(2, 2), padding={self.padding}"
