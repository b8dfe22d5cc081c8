"""The contract of sgr.final_conv / sgr.group_norm_relu_final_conv in torch, own code: ReplicationPad2d(1) followed by a
3x3 convolution to three channels (models.py:155-156, 187), optionally behind GroupNorm + ReLU (models.py:183), with hand-written gradients,
device- and dtype-generic (fp64 is the arbiter; fp32 gives the algorithm's own rounding noise).  TEST INFRASTRUCTURE ONLY.

Two parts that share nothing:
  * ``final_conv`` states the contract with explicit index arithmetic -- ``cl(t, n) = min(max(t, 0), n - 1)`` gathers for the forward and
    the weight gradient, the set ``R_n(h)`` for the data gradient -- without ``F.pad`` or ``F.conv2d``;
  * ``composition`` is ``F.pad(mode='replicate')`` + ``F.conv2d`` + ``F.group_norm`` under autograd: what the eager reference executes.

tests/test_final_conv.py pins both at 1e-12 to the fixtures the unmodified reference produced (tests/golden/g20_finalconv_*.npz) and to
each other."""
import torch

import gn_stage_checker as GN


def cl(t, n):
    return min(max(t, 0), n - 1)


def pairs(h, n):
    """R_n(h) = {(i, k): 0 <= i < n, k in {0, 1, 2}, cl(i + k - 1, n) == h}, by its definition: the outputs i that read input h, with the tap"""
    return [(i, k) for k in range(3) for i in range(n) if cl(i + k - 1, n) == h]


def _shifted(y, kh, kw):
    """y[b, c, cl(i + kh - 1, H), cl(j + kw - 1, W)] for every (i, j)"""
    H, W = y.shape[-2:]
    ri = torch.tensor([cl(i + kh - 1, H) for i in range(H)], device=y.device)
    ci = torch.tensor([cl(j + kw - 1, W) for j in range(W)], device=y.device)
    return y.index_select(-2, ri).index_select(-1, ci)


def conv_forward(y, Wt, bias):
    out = bias.reshape(1, 3, 1, 1).expand(y.shape[0], 3, *y.shape[-2:]).clone()
    for kh in range(3):
        for kw in range(3):
            out = out + torch.einsum("oc,bchw->bohw", Wt[:, :, kh, kw], _shifted(y, kh, kw))
    return out


def conv_backward(g, y, Wt):
    """-> (dy, dWt, dbias) of conv_forward for the cotangent g: dy by the gather over R_H(h) x R_W(w), nothing scattered"""
    B, C, H, W = y.shape
    dbias = g.sum((0, 2, 3))
    dWt = torch.stack([torch.stack([torch.einsum("bohw,bchw->oc", g, _shifted(y, kh, kw)) for kw in range(3)], -1) for kh in range(3)], -2)
    rows, cols = [pairs(h, H) for h in range(H)], [pairs(w, W) for w in range(W)]
    dy = torch.zeros_like(y)
    for p in range(3):
        ri = torch.tensor([rows[h][p][0] for h in range(H)], device=y.device)
        rk = [rows[h][p][1] for h in range(H)]
        for q in range(3):
            ci = torch.tensor([cols[w][q][0] for w in range(W)], device=y.device)
            ck = [cols[w][q][1] for w in range(W)]
            gg = g.index_select(-2, ri).index_select(-1, ci)                                   # g[b, o, i_p(h), j_q(w)]
            wsel = Wt[:, :, rk, :][:, :, :, ck]                                                # Wt[o, c, kh_p(h), kw_q(w)]  [3,C,H,W]
            dy = dy + torch.einsum("ochw,bohw->bchw", wsel, gg)
    return dy, dWt, dbias


def final_conv(x, Wt, bias, gn=None, cotangent=None):
    """``gn = None``: x is y.  ``gn = (weight, bias, G, eps)``: y = relu(group_norm(x)).
    -> (out, (dx, dgn_weight, dgn_bias, dWt, dbias)); the gradients are None without a cotangent, the GroupNorm's without one"""
    if gn is None:
        y = x
    else:
        gw, gb, G, eps = gn
        pre, _, _ = GN.pre_relu(x, gw, gb, G, eps)
        y = pre.clamp(min=0)
    out = conv_forward(y, Wt, bias)
    if cotangent is None:
        return out, (None,) * 5
    dy, dWt, dbias = conv_backward(cotangent, y, Wt)
    if gn is None:
        return out, (dy, None, None, dWt, dbias)
    _, (dx, dgw, dgb, _) = GN.gn_stage(x, gw, gb, G, None, eps, cotangent=dy)      # masks dy with pre > 0 itself
    return out, (dx, dgw, dgb, dWt, dbias)


def composition(x, Wt, bias, gn=None, cotangent=None):
    """the same from torch's own operators under autograd: what the eager reference executes"""
    F = torch.nn.functional
    leaves = [t.detach().clone().requires_grad_(True) for t in ((x, Wt, bias) if gn is None else (x, gn[0], gn[1], Wt, bias))]
    if gn is None:
        xl, wl, bl = leaves
        y = xl
    else:
        xl, gwl, gbl, wl, bl = leaves
        y = torch.relu(F.group_norm(xl, gn[2], gwl, gbl, gn[3]))
    out = F.conv2d(F.pad(y, (1, 1, 1, 1), mode="replicate"), wl, bl)
    if cotangent is None:
        return out.detach(), (None,) * 5
    gs = torch.autograd.grad(out, leaves, grad_outputs=cotangent)
    if gn is None:
        return out.detach(), (gs[0], None, None, gs[1], gs[2])
    return out.detach(), tuple(gs)
