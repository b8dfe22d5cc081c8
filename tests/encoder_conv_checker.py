"""The contract of sgr.encoder_conv in torch, own code: a pad of one (replicate or zeros) followed by a 4x4 stride-2
convolution to ``O`` channels (models.py:93-115, 122-126, 213-246, 254-266), with hand-written gradients, device- and dtype-generic (fp64 is the
arbiter; fp32 gives the algorithm's own rounding noise).  TEST INFRASTRUCTURE ONLY.

Two parts that share nothing:
  * ``encoder_conv`` states the contract with explicit index arithmetic -- ``src(t, n)`` gathers for the forward and the weight gradient, the
    set ``R_n(h)`` for the data gradient -- without ``F.pad`` or ``F.conv2d``;
  * ``composition`` is ``F.pad`` + ``F.conv2d(stride=2)`` under autograd: what the eager reference executes.

tests/test_encoder_conv.py pins both at 1e-12 to the fixtures the unmodified reference produced (tests/golden/g22_encconv_*.npz) and to each
other."""
import torch

MODES = ("replicate", "zeros")


def src(t, n, mode):
    """the source index of padded position t (the map starts at 0), or None where the pad is an exact zero"""
    if mode == "replicate":
        return min(max(t, 0), n - 1)
    return t if 0 <= t < n else None


def pairs(h, n, mode):
    """R_n(h): the (i, k) with 0 <= i < n // 2, 0 <= k < 4 and src(2 i + k - 1, n) == h, found by enumeration"""
    return [(i, k) for i in range(n // 2) for k in range(4) if src(2 * i + k - 1, n, mode) == h]


def _gathered(x, k, n_out, axis, mode):
    """x's rows (axis -2) or columns (-1) src(2 i + k - 1) for i = 0 .. n_out - 1; an absent one is a zero"""
    n = x.shape[axis]
    idx = [src(2 * i + k - 1, n, mode) for i in range(n_out)]
    sel = x.index_select(axis, torch.tensor([0 if t is None else t for t in idx], device=x.device))
    keep = torch.tensor([0.0 if t is None else 1.0 for t in idx], dtype=x.dtype, device=x.device)
    return sel * (keep.view(-1, 1) if axis == -2 else keep)


def _shifted(x, kh, kw, mode):
    """x[b, c, src(2 i + kh - 1), src(2 j + kw - 1)] as [B,C,Ho,Wo]"""
    H, W = x.shape[-2:]
    return _gathered(_gathered(x, kh, H // 2, -2, mode), kw, W // 2, -1, mode)


def conv_forward(x, Wt, bias, mode):
    B, _, H, W = x.shape
    O = Wt.shape[0]
    out = bias.reshape(1, O, 1, 1).expand(B, O, H // 2, W // 2).clone()
    for kh in range(4):
        for kw in range(4):
            out = out + torch.einsum("oc,bchw->bohw", Wt[:, :, kh, kw], _shifted(x, kh, kw, mode))
    return out


def conv_backward(g, x, Wt, mode):
    """-> (dx, dWt, dbias) of conv_forward for the cotangent g: dx by the gather over R_H(h) x R_W(w), nothing scattered"""
    B, C, H, W = x.shape
    dbias = g.sum((0, 2, 3))
    dWt = torch.stack([torch.stack([torch.einsum("bohw,bchw->oc", g, _shifted(x, kh, kw, mode)) for kw in range(4)], -1) for kh in range(4)], -2)
    rows, cols = [pairs(h, H, mode) for h in range(H)], [pairs(w, W, mode) for w in range(W)]
    assert max(len(r) for r in rows + cols) <= 2
    dx = torch.zeros_like(x)
    t = lambda v, dt=x.dtype: torch.tensor(v, dtype=dt, device=x.device)
    for p in range(2):      # the p-th member of R_H(h), where there is one
        ri = t([r[p][0] if len(r) > p else 0 for r in rows], torch.long)
        for q in range(2):
            ci = t([c[q][0] if len(c) > q else 0 for c in cols], torch.long)
            gg = g.index_select(-2, ri).index_select(-1, ci)                                   # g[b, o, i_p(h), j_q(w)]
            for kh in range(4):
                mh = t([1.0 if len(r) > p and r[p][1] == kh else 0.0 for r in rows])           # the rows whose p-th member reads through kh
                for kw in range(4):
                    mw = t([1.0 if len(c) > q and c[q][1] == kw else 0.0 for c in cols])
                    if float(mh.sum()) * float(mw.sum()) > 0:
                        dx = dx + torch.einsum("oc,bohw->bchw", Wt[:, :, kh, kw], gg * mh.view(-1, 1) * mw)
    return dx, dWt, dbias


def encoder_conv(x, Wt, bias, mode="replicate", cotangent=None):
    """-> (out, (dx, dWt, dbias)); the gradients are None without a cotangent"""
    assert mode in MODES
    out = conv_forward(x, Wt, bias, mode)
    if cotangent is None:
        return out, (None,) * 3
    return out, conv_backward(cotangent, x, Wt, mode)


def composition(x, Wt, bias, mode="replicate", cotangent=None):
    """the same from torch's own operators under autograd: what the eager reference executes"""
    F = torch.nn.functional
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, Wt, bias)]
    out = F.conv2d(F.pad(leaves[0], (1, 1, 1, 1), mode="replicate" if mode == "replicate" else "constant"), leaves[1], leaves[2], stride=2)
    if cotangent is None:
        return out.detach(), (None,) * 3
    return out.detach(), tuple(torch.autograd.grad(out, leaves, grad_outputs=cotangent))
