"""The contract of sgr.light_final_conv in torch, own code: ReplicationPad2d(1) followed by a 3x3 convolution to ``O``
channels (models.py:297-302, 334), with hand-written gradients, device- and dtype-generic (fp64 is the arbiter; fp32 gives the algorithm's own
rounding noise).  TEST INFRASTRUCTURE ONLY.

Two parts that share nothing:
  * ``light_final_conv`` states the contract with explicit index arithmetic -- ``cl(t, n) = min(max(t, 0), n - 1)`` gathers for the forward
    and the weight gradient, the set ``R_n(h)`` for the data gradient (``cl``, ``pairs`` and the shifted gather are
    tests/final_conv_checker.py's) -- without ``F.pad`` or ``F.conv2d``, for any ``O``;
  * ``composition`` is ``F.pad(mode='replicate')`` + ``F.conv2d`` under autograd: what the eager reference executes.

tests/test_light_final_conv.py pins both at 1e-12 to the fixtures the unmodified reference produced (tests/golden/g21_lightconv_*.npz) and to
each other."""
import torch

from final_conv_checker import _shifted, cl, pairs      # noqa: F401


def conv_forward(y, Wt, bias):
    O = Wt.shape[0]
    out = bias.reshape(1, O, 1, 1).expand(y.shape[0], O, *y.shape[-2:]).clone()
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
            wsel = Wt[:, :, rk, :][:, :, :, ck]                                                # Wt[o, c, kh_p(h), kw_q(w)]  [O,C,H,W]
            dy = dy + torch.einsum("ochw,bohw->bchw", wsel, gg)
    return dy, dWt, dbias


def light_final_conv(y, Wt, bias, cotangent=None):
    """-> (out, (dy, dWt, dbias)); the gradients are None without a cotangent"""
    out = conv_forward(y, Wt, bias)
    if cotangent is None:
        return out, (None,) * 3
    return out, conv_backward(cotangent, y, Wt)


def composition(y, Wt, bias, cotangent=None):
    """the same from torch's own operators under autograd: what the eager reference executes"""
    F = torch.nn.functional
    leaves = [t.detach().clone().requires_grad_(True) for t in (y, Wt, bias)]
    out = F.conv2d(F.pad(leaves[0], (1, 1, 1, 1), mode="replicate"), leaves[1], leaves[2])
    if cotangent is None:
        return out.detach(), (None,) * 3
    return out.detach(), tuple(torch.autograd.grad(out, leaves, grad_outputs=cotangent))
