"""The contract of sgr.group_norm_relu_resize / sgr.group_norm_relu_resize_upcat in torch, own code: GroupNorm + ReLU,
the bilinear resize to a given size (models.py:165-166 and its siblings, 185-186), the skip concatenation and the 2x bilinear upsample, with
hand-written gradients, device- and dtype-generic (fp64 is the arbiter; fp32 gives the algorithm's own rounding noise).  TEST INFRASTRUCTURE
ONLY.

Both resamplings are dense matrices built from the index rule, ``R_h @ Y @ R_w^T`` and ``U_h @ . @ U_w^T``, and their adjoints the transposes:
nothing here shares a line with the kernels' gathers.  The resize's rule is torch's for a given output size: ``scale = n / ns`` FORMED IN THE
RUN'S DTYPE (in fp32 that is the rounding the kernel and torch's fp32 run carry), ``s = max(scale (o + 0.5) - 0.5, 0)``.

tests/test_gn_resize.py pins this file at 1e-12 to the fixtures the unmodified reference produced (tests/golden/g19_gnresize_*.npz)."""
import torch

import gn_stage_checker as S


def resize_matrix(n, ns, dtype, device="cpu"):
    """[ns, n]: row o holds the weights 1 - (s - i0) at i0 = floor(s) and s - i0 at i1 = min(i0 + 1, n - 1)"""
    scale = (torch.tensor(float(n), dtype=dtype) / torch.tensor(float(ns), dtype=dtype))
    o = torch.arange(ns, dtype=dtype)
    s = (scale * (o + 0.5) - 0.5).clamp(min=0)
    i0 = s.floor().long().clamp(max=n - 1)
    i1 = (i0 + 1).clamp(max=n - 1)
    l1 = s - i0.to(dtype)
    R = torch.zeros(ns, n, dtype=dtype)
    R.scatter_add_(1, i0[:, None], (1 - l1)[:, None])
    R.scatter_add_(1, i1[:, None], l1[:, None])
    return R.to(device)


def resize(t, size):
    H, W = t.shape[-2:]
    return resize_matrix(H, size[0], t.dtype, t.device) @ t @ resize_matrix(W, size[1], t.dtype, t.device).T


def resize_adjoint(g, size):
    """the cotangent of a map resized from `size`"""
    return resize_matrix(size[0], g.shape[-2], g.dtype, g.device).T @ g @ resize_matrix(size[1], g.shape[-1], g.dtype, g.device)


def gn_resize(x, weight, bias, G, size, skip=None, eps=1e-5, cotangent=None):
    """-> (out, (dx, dweight, dbias, dskip)); ``size = (Hs, Ws)``; with a skip [B,Cs,Hs,Ws] the result is upsampled 2x.  The gradients are
    None without a cotangent, dskip without a skip."""
    B, C, H, W = x.shape
    pre, xhat, rstd = S.pre_relu(x, weight, bias, G, eps)
    r = resize(pre.clamp(min=0), size)
    out = r if skip is None else S.upsample2(torch.cat([r, skip], 1))
    if cotangent is None:
        return out, (None, None, None, None)
    ga = cotangent if skip is None else S.upsample2_adjoint(cotangent)
    dskip = None if skip is None else ga[:, C:]
    dy = torch.where(pre > 0, resize_adjoint(ga[:, :C], (H, W)), torch.zeros_like(pre))
    dbias = dy.sum((0, 2, 3))
    dweight = (dy * xhat).sum((0, 2, 3))
    dyw = (dy * weight.reshape(1, C, 1, 1)).reshape(B, G, -1)
    xg = xhat.reshape(B, G, -1)
    dx = rstd * (dyw - dyw.mean(2, keepdim=True) - xg * (dyw * xg).mean(2, keepdim=True))
    return out, (dx.reshape(B, C, H, W), dweight, dbias, dskip)


def reference_lines(x, weight, bias, G, size, skip=None, eps=1e-5):
    """the same stage composed of torch's own operators, as the reference composes it"""
    F = torch.nn.functional
    y = F.interpolate(torch.relu(F.group_norm(x, G, weight, bias, eps)), list(size), mode="bilinear")
    if skip is None:
        return y
    return F.interpolate(torch.cat([y, skip], 1), scale_factor=2, mode="bilinear")


def max_fan_in(n, ns):
    """the largest number of resized indices that reference one source index with a non-zero weight"""
    return int((resize_matrix(n, ns, torch.float64) != 0).sum(0).max())
