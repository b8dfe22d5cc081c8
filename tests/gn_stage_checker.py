"""The contract of sgr.group_norm_relu / sgr.group_norm_relu_upcat in torch, own code: GroupNorm + ReLU, the skip
concatenation and the 2x bilinear upsample of models.py:160-183, with hand-written gradients, device- and dtype-generic (fp64 is the
arbiter; fp32 gives the algorithm's own rounding noise).  TEST INFRASTRUCTURE ONLY.

The upsample is written as two dense matrices built from the index rule (``s = max(0.5 (o + 0.5) - 0.5, 0)``), ``U_h @ X @ U_w^T``, and its
adjoint as their transposes: nothing here shares a line with the kernels' gather.

tests/test_gn_stage.py pins this file at 1e-12 to the fixtures the unmodified reference produced (tests/golden/g17_gnstage_*.npz)."""
import torch


def up_matrix(n, dtype, device="cpu"):
    """[2n, n]: row o holds the weights 1 - (s - i0) at i0 = floor(s) and s - i0 at i1 = min(i0 + 1, n - 1)"""
    o = torch.arange(2 * n, dtype=torch.float64)
    s = (0.5 * (o + 0.5) - 0.5).clamp(min=0)
    i0 = s.floor().long().clamp(max=n - 1)
    i1 = (i0 + 1).clamp(max=n - 1)
    l1 = s - i0
    U = torch.zeros(2 * n, n, dtype=torch.float64)
    U.scatter_add_(1, i0[:, None], (1 - l1)[:, None])
    U.scatter_add_(1, i1[:, None], l1[:, None])
    return U.to(dtype=dtype, device=device)


def upsample2(t):
    H, W = t.shape[-2:]
    return up_matrix(H, t.dtype, t.device) @ t @ up_matrix(W, t.dtype, t.device).T


def upsample2_adjoint(g):
    H, W = g.shape[-2] // 2, g.shape[-1] // 2
    return up_matrix(H, g.dtype, g.device).T @ g @ up_matrix(W, g.dtype, g.device)


def moments(x, G, eps):
    B, C, H, W = x.shape
    xg = x.reshape(B, G, -1)
    mean = xg.mean(2, keepdim=True)
    var = ((xg - mean) ** 2).mean(2, keepdim=True)
    return mean, 1 / torch.sqrt(var + eps)


def pre_relu(x, weight, bias, G, eps=1e-5):
    """the ReLU's argument, [B,C,H,W], and xhat"""
    B, C, H, W = x.shape
    mean, rstd = moments(x, G, eps)
    xhat = ((x.reshape(B, G, -1) - mean) * rstd).reshape(B, C, H, W)
    return xhat * weight.reshape(1, C, 1, 1) + bias.reshape(1, C, 1, 1), xhat, rstd


def gn_stage(x, weight, bias, G, skip=None, eps=1e-5, cotangent=None):
    """-> (out, (dx, dweight, dbias, dskip)); the gradients are None without a cotangent, dskip without a skip"""
    B, C, H, W = x.shape
    pre, xhat, rstd = pre_relu(x, weight, bias, G, eps)
    y = pre.clamp(min=0)
    out = y if skip is None else upsample2(torch.cat([y, skip], 1))
    if cotangent is None:
        return out, (None, None, None, None)
    ga = cotangent if skip is None else upsample2_adjoint(cotangent)
    dskip = None if skip is None else ga[:, C:]
    dy = torch.where(pre > 0, ga[:, :C], torch.zeros_like(pre))
    dbias = dy.sum((0, 2, 3))
    dweight = (dy * xhat).sum((0, 2, 3))
    dyw = (dy * weight.reshape(1, C, 1, 1)).reshape(B, G, -1)
    xg = xhat.reshape(B, G, -1)
    dx = rstd * (dyw - dyw.mean(2, keepdim=True) - xg * (dyw * xg).mean(2, keepdim=True))
    return out, (dx.reshape(B, C, H, W), dweight, dbias, dskip)


def reference_lines(x, weight, bias, G, skip=None, eps=1e-5):
    """the same stage composed of torch's own operators (what the eager reference executes)"""
    y = torch.relu(torch.nn.functional.group_norm(x, G, weight, bias, eps))
    if skip is None:
        return y
    return torch.nn.functional.interpolate(torch.cat([y, skip], 1), scale_factor=2, mode="bilinear")
