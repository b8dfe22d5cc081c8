"""The encoders' down-sampling layers -- ``Conv2d(C -> O, 4, stride=2)`` behind ``ReplicationPad2d(1)`` or ``ZeroPad2d(1)``: ``encoder0.conv1`` /
``conv2`` and ``encoderLight.preProcess[1]`` / ``[5]`` / ``conv1`` of models.py:93-115, 122-126, 213-246, 254-266 -- backed by libsgrender.so
(csrc/sgr_encoder_conv.hip): the forward and both large gradients on the fp32-input matrix instruction, in exact fp32.

  ``encoder_conv(x, weight, bias, padding='replicate')``   ``F.conv2d(F.pad(x, (1, 1, 1, 1), mode=padding), weight, bias, stride=2)``: the padded
                                                           copy is never written, and the pad's backward is a gather, not an atomic scatter
  ``encoder_conv_cat(xs, weight, bias, padding)``          ``encoder_conv(torch.cat(xs, 1), ...)`` bit for bit, for up to four sources: the concatenated
                                                           copy is never written, and a source that does not require grad costs no data gradient
  ``EncoderConv(in_channels, out_channels, padding)``      the module form; ``weight`` / ``bias`` load a checkpoint's ``conv1.*`` / ``conv2.*`` /
                                                           ``preProcess.1.*`` / ``preProcess.5.*``.  ``in_channels=(64, 84)`` is ``encoderLight.conv1``
                                                           at cascade 1, called as ``conv1(input1, envs)``

Not in this operator, on purpose: the deeper layers (``C >= 128 -> O >= 256`` on planes of 60 x 80 and smaller).  Their pads are zero pads,
whose backward is a slice and deterministic, their padded copies are small, and with at most 4800 output pixels an image they are plain
GEMMs: they stay ``F.pad`` + ``F.conv2d``.  DESIGN.md section 8i states the arithmetic."""
from __future__ import annotations

import torch

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["encoder_conv", "encoder_conv_cat", "EncoderConv"]

_sg = torch.ops.sgrender

MAX_CHANNELS = 160                             # csrc/sgr_encoder_conv.h
MAX_SOURCES = 4                                # SGR_ENCODER_CONV_MAX_SOURCES: the source table travels in the kernel arguments
MIN_OUT_CHANNELS, MAX_OUT_CHANNELS = 16, 128   # a multiple of 16: whole tiles of the matrix instruction
PAD_MODES = {"replicate": 0, "zeros": 1}
_COMPOSE = "compose F.pad(x, (1, 1, 1, 1), mode=...) and F.conv2d(., stride=2) instead"
_COMPOSE_CAT = "compose torch.cat(xs, 1), F.pad(x, (1, 1, 1, 1), mode=...) and F.conv2d(., stride=2) instead"


def _pad_mode(padding, who, compose=_COMPOSE):
    if padding not in PAD_MODES:
        raise ValueError(f"sgrender: {who}: padding {padding!r} is not one of {sorted(PAD_MODES)}; {compose}")
    return PAD_MODES[padding]


def encoder_conv(x, weight, bias, padding="replicate"):
    """``F.conv2d(F.pad(x, (1, 1, 1, 1), mode=padding), weight, bias, stride=2)`` (``'zeros'`` is ``F.pad``'s ``'constant'``) for fp32
    ``x [B,C,H,W]`` on a HIP device, ``weight [O,C,4,4]``, ``bias [O]``, ``1 <= C <= 160``, ``O`` a multiple of 16 in 16..128, ``H, W >= 2``:
    ``[B,O,H//2,W//2]``.  ``x`` may be non-contiguous (a channels-last map or a slice is read in place); the result is contiguous.
    Differentiable with respect to all three; a gradient is computed only for those that require it, without atomics: two runs give the
    same bits, also under ``torch.use_deterministic_algorithms(True)``.  Any other convolution raises and names the composition to use; a
    CPU tensor raises: there is no fallback."""
    return _sg.encoder_conv(x, weight, bias, _pad_mode(padding, "encoder_conv"))


def encoder_conv_cat(xs, weight, bias, padding="replicate"):
    """``encoder_conv(torch.cat(xs, 1), weight, bias, padding)`` for a list of ``1 <= S <= 4`` fp32 sources ``[B,C_i,H,W]`` on one HIP device,
    ``C_i >= 1``, ``sum C_i <= 160``, ``weight [O,sum C_i,4,4]``: the same bits, value and gradients, without the concatenated copy.  Each
    source is read through its own strides (channels-last, a slice, a different layout per source).  ``dxs[i]`` is the matching channel slice
    of the concatenation's ``dx`` as a fresh contiguous tensor; a source that does not require grad gets none and costs no data-gradient
    launch.  One forward launch; no atomics.  ``S == 1`` is ``encoder_conv``.  Anything else raises and names the composition to use."""
    if isinstance(xs, torch.Tensor):
        raise TypeError(f"sgrender: encoder_conv_cat: xs must be a list of tensors, got a tensor; {_COMPOSE_CAT}")
    return _sg.encoder_conv_cat(list(xs), weight, bias, _pad_mode(padding, "encoder_conv_cat", _COMPOSE_CAT))


class EncoderConv(torch.nn.Module):
    """``nn.ReplicationPad2d(1)`` (or ``nn.ZeroPad2d(1)``) + ``nn.Conv2d(in_channels, out_channels, 4, stride=2)`` as one operator.  The
    parameters are named and shaped as ``nn.Conv2d``'s, so ``load_state_dict`` takes a reference checkpoint's ``conv1.*`` / ``conv2.*`` /
    ``preProcess.1.*`` / ``preProcess.5.*`` under the same prefix, and they are initialised as ``nn.Conv2d`` initialises them.

    ``in_channels`` may be a tuple, one count per source: ``EncoderConv((64, 84), 128)`` is ``nn.Conv2d(148, 128, 4, stride=2)`` -- the same
    ``weight`` / ``bias`` -- whose ``forward(input1, envs)`` takes the sources that the reference concatenates first (``encoderLight.conv1``,
    models.py:254-262), through ``encoder_conv_cat``."""

    def __init__(self, in_channels, out_channels: int, padding: str = "replicate"):
        super().__init__()
        _pad_mode(padding, "EncoderConv")
        self.sources = None      # an integer in_channels: one source, forward(x)
        if not isinstance(in_channels, int):
            self.sources = tuple(int(c) for c in in_channels)
            if not 1 <= len(self.sources) <= MAX_SOURCES or min(self.sources, default=0) < 1:
                raise ValueError(f"sgrender: EncoderConv: in_channels {in_channels!r} is not 1..{MAX_SOURCES} positive channel counts; {_COMPOSE_CAT}")
            in_channels = sum(self.sources)
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

    def forward(self, x, *more):
        if self.sources is None:
            if more:
                raise ValueError(f"sgrender: EncoderConv: {1 + len(more)} sources given to a module built with an integer in_channels; build it with "
                                 f"in_channels=(C_1, C_2, ..) to pass the sources of a concatenation; {_COMPOSE_CAT}")
            return encoder_conv(x, self.weight, self.bias, self.padding)
        xs = (x,) + more
        if len(xs) != len(self.sources) or any(t.dim() != 4 or t.size(1) != c for t, c in zip(xs, self.sources)):
            raise ValueError(f"sgrender: EncoderConv: the sources must be [B,C_i,H,W] with C_i = {self.sources}, got "
                             f"{[tuple(t.shape) for t in xs]}; {_COMPOSE_CAT}")
        return encoder_conv_cat(xs, self.weight, self.bias, self.padding)

    def extra_repr(self):
        cin = self.in_channels if self.sources is None else "+".join(map(str, self.sources))
        return f"{cin}, {self.out_channels}, kernel_size=(4, 4), stride=(2, 2), padding={self.padding}"
