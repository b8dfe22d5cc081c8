"""The bilateral solver layer, backed by libsgrender.so (csrc/sgr_bilateral.hip).

Drop-in for the reference's ``BilateralLayer.BilateralLayer`` (BilateralLayer.py:126-274: same constructor, parameter tables,
sub-module names and ``forward(image, feature, pred) -> (output, confidence)``), which ``testReal.py:186-188,531-540`` and
``trainBRDFBilateral.py:98-101`` use to refine albedo, roughness and depth.  The reference's ``BilateralFunction`` copies the batch
to the host and, per image, in forward and again in backward, builds the 5-D bilateral grid with numpy and solves it with scipy's
sparse CG; here the whole batch stays on the device (``torch.ops.sgrender.bilateral_solve``: grid build, bistochastisation, a
fixed-length PCG, no host synchronisation) and the grid built in forward is reused in backward.

The confidence CNN is the reference's, in plain PyTorch.  The contract of the solver is ``BilateralGrid.solve`` / ``solveForGrad``
with the mode table's own ``cg_maxiter`` (INTEGRATION.md explains why, DESIGN.md section 8 states the arithmetic)."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops as _ops      # noqa: F401  (loads libsgrender_torch.so)

__all__ = ["BilateralLayer", "bilateral_solve", "BILATERAL_MODES"]

_sg = torch.ops.sgrender

# BilateralLayer.py:137-190 -- bilateral solver for albedo (0), normal (1), roughness (2), depth (4)
BILATERAL_MODES = {
    0: dict(grid=dict(sigma_luma=8, sigma_chroma=2, sigma_spatial=7), bs=dict(lam=200, A_diag_min=1e-5, cg_tol=1e-5, cg_maxiter=12)),
    1: dict(grid=dict(sigma_luma=0.5, sigma_chroma=0.5, sigma_spatial=0.5), bs=dict(lam=5, A_diag_min=1e-5, cg_tol=1e-5, cg_maxiter=10)),
    2: dict(grid=dict(sigma_luma=8, sigma_chroma=2, sigma_spatial=8), bs=dict(lam=300, A_diag_min=1e-5, cg_tol=1e-5, cg_maxiter=10)),
    4: dict(grid=dict(sigma_luma=4, sigma_chroma=2, sigma_spatial=4), bs=dict(lam=100, A_diag_min=1e-5, cg_tol=1e-5, cg_maxiter=10)),
}


def bilateral_solve(image, pred, confidence, sigma_luma, sigma_chroma, sigma_spatial, lam, A_diag_min=1e-5, cg_tol=1e-5, cg_maxiter=10):
    """Refine ``pred`` [B,C,H,W] (C = 1..3) with the bilateral solver guided by ``image`` [B,3,H,W] in [0,1] and weighted by
    ``confidence`` [B,1,H,W]: ``BilateralGrid.solve`` per image, on the device.  Differentiable w.r.t. ``pred`` and ``confidence``
    (``BilateralGrid.solveForGrad``); no gradient to the guide image."""
    return _sg.bilateral_solve(image, pred, confidence, float(sigma_luma), float(sigma_chroma), float(sigma_spatial), float(lam), float(A_diag_min),
                               float(cg_tol), int(cg_maxiter))


def _unit_scale(x):
    """x / clamp(max over (C,H,W) per image, 1e-5, 1)        BilateralLayer.py:235-245"""
    scale = torch.clamp(x.amax(dim=(1, 2, 3), keepdim=True), 1e-5, 1)
    return x / scale.expand_as(x)


class BilateralLayer(nn.Module):
    """Mirror of BilateralLayer.py:126-274; a reference checkpoint's ``state_dict`` loads unchanged."""

    def __init__(self, mode=0, isCuda=True, gpuId=0):
        super().__init__()
        if mode not in BILATERAL_MODES:
            raise ValueError(f"sgrender: BilateralLayer mode must be one of {sorted(BILATERAL_MODES)}, got {mode}")
        self.mode = mode
        self.grid_params = dict(BILATERAL_MODES[mode]["grid"])
        self.bs_params = dict(BILATERAL_MODES[mode]["bs"])
        self.pad1 = nn.ReplicationPad2d(1)
        self.conv1 = nn.Conv2d(in_channels=4 if mode in (2, 4) else 6, out_channels=16, kernel_size=4, stride=2, bias=True)
        self.gn1 = nn.GroupNorm(num_groups=2, num_channels=16)
        self.pad2 = nn.ReplicationPad2d(1)
        self.conv2 = nn.Conv2d(in_channels=16, out_channels=16, kernel_size=4, stride=2, bias=True)
        self.gn2 = nn.GroupNorm(num_groups=2, num_channels=16)
        self.dconv1 = nn.Conv2d(in_channels=16, out_channels=16, kernel_size=3, stride=1, padding=1, bias=True)
        self.dgn1 = nn.GroupNorm(num_groups=2, num_channels=16)
        self.dconv2 = nn.Conv2d(in_channels=32, out_channels=16, kernel_size=3, stride=1, padding=1, bias=True)
        self.dgn2 = nn.GroupNorm(num_groups=2, num_channels=16)
        self.dpad3 = nn.ReplicationPad2d(1)
        self.dconvFinal = nn.Conv2d(in_channels=16, out_channels=1, kernel_size=3, stride=1, bias=True)

    def _scaled(self, image, feature):
        return _unit_scale(image), _unit_scale(feature)

    def confidence(self, image, feature, pred):
        """The confidence CNN alone (BilateralLayer.py:235-266): plain PyTorch, runs on any device.  Inside an autocast region it runs in
        fp32 like the solver it feeds: the inputs are cast to fp32 and its convolutions are kept out of autocast."""
        image, feature, pred = _ops.autocast_fp32(image, feature, pred)
        with _ops.autocast_off(image, pred):
            return self._confidence(image, feature, pred)

    def _confidence(self, image, feature, pred):
        image, _ = self._scaled(image, feature)
        x = torch.cat([image, pred], dim=1).detach()
        x1 = F.relu(self.gn1(self.conv1(self.pad1(x))), True)
        x2 = F.relu(self.gn2(self.conv2(self.pad2(x1))), True)
        dx1 = F.relu(self.dgn1(self.dconv1(x2)), True)
        dx1 = F.interpolate(dx1, [x1.size(2), x1.size(3)], mode="bilinear")
        dx2 = F.relu(self.dgn2(self.dconv2(torch.cat([dx1, x1], dim=1))), True)
        dx2 = F.interpolate(dx2, [x.size(2), x.size(3)], mode="bilinear")
        conf = 0.5 * (torch.tanh(self.dconvFinal(self.dpad3(dx2))) + 1)
        return conf / torch.clamp(conf.max(), min=1e-5)

    def forward(self, image, feature, pred):
        """-> (refined pred, confidence).  The solver's guide is the scaled, detached ``feature`` (the albedo prediction at every
        call site of the reference), ``image`` only feeds the confidence CNN (BilateralLayer.py:268)."""
        image, feature, pred = _ops.autocast_fp32(image, feature, pred)
        conf = self.confidence(image, feature, pred)
        _, guide = self._scaled(image, feature)
        out = bilateral_solve(guide.detach(), pred, conf, **self.grid_params, **self.bs_params)
        return out, conf.detach()      # passed through; carries no gradient of its own (grad_not_used, BilateralLayer.py:76)
