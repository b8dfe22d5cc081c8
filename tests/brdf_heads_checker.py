"""The contract of sgr.brdf_heads in torch, own code: the output activations of models.decoder0 (models.py:189-203,
modes 0 / 1 / 2 / 4) with hand-written gradients, device- and dtype-generic (fp64 is the arbiter; fp32 gives the algorithm's own rounding
noise).  TEST INFRASTRUCTURE ONLY.

One stated deviation from the reference: a normal triplet with ``|t| < 1e-6`` has the gradient ``g / 1e-6 * s'(x)`` here -- the norm path
is blocked by the min-clamp -- where the reference's ``sqrt`` backward gives ``0 / 0 = NaN``.

tests/test_brdf_heads.py pins this file at 1e-12 to the fixtures the unmodified reference produced (tests/golden/g16_brdfheads_*.npz)."""
import torch

TERMS = ("albedo", "normal", "rough", "depth")
MODES = {"albedo": 0, "normal": 1, "rough": 2, "depth": 4}


def act(x):
    """s(x) = clamp(1.01 tanh(x), -1, 1) and s'(x) = 1.01 (1 - tanh^2 x) on the closed interval -1 <= 1.01 tanh x <= 1, 0 outside"""
    t = torch.tanh(x)
    a = 1.01 * t
    d = torch.where((a >= -1) & (a <= 1), 1.01 * (1 - t * t), torch.zeros_like(t))
    return a.clamp(-1, 1), d


def head(x, term, g=None, unit=False):
    """-> (y, gx): one decoder's output for its dconvFinal output ``x [B,3,H,W]`` and, for the cotangent ``g`` (shaped like y), the gradient
    at x (None without g).  ``unit``: albedo and depth as 0.5 (y + 1)."""
    u = 0.5 if unit and term in ("albedo", "depth") else 1.0
    gx = None
    if term == "albedo":
        y, d = act(x)
        if g is not None:
            gx = u * g * d
    elif term == "normal":
        t, d = act(x)
        nr = torch.sqrt((t[:, 0:1] * t[:, 0:1] + t[:, 1:2] * t[:, 1:2]) + t[:, 2:3] * t[:, 2:3])
        n = nr.clamp(min=1e-6)
        y = t / n
        if g is not None:
            dot = torch.where(nr >= 1e-6, (y * g).sum(1, keepdim=True), torch.zeros_like(nr))      # blocked below 1e-6: the stated deviation
            gx = (g - y * dot) / n * d
    elif term == "rough":
        s, d = act(x)
        y = ((s[:, 0:1] + s[:, 1:2]) + s[:, 2:3]) / 3
        if g is not None:
            gx = g / 3 * d
    elif term == "depth":
        m = ((x[:, 0:1] + x[:, 1:2]) + x[:, 2:3]) / 3
        y, d = act(m)
        if g is not None:
            gx = (u * g * d / 3).expand_as(x).clone()
    else:
        raise ValueError(term)
    if u != 1.0:
        y = 0.5 * (y + 1)
    return y, gx


def brdf_heads(xAlbedo, xNormal, xRough, xDepth, unit=True, cotangents=(None, None, None, None)):
    """-> (four outputs, four gradients), None for an absent term / without a cotangent"""
    ys, gs = [], []
    for term, x, g in zip(TERMS, (xAlbedo, xNormal, xRough, xDepth), cotangents):
        y, gx = (None, None) if x is None else head(x, term, g, unit)
        ys.append(y)
        gs.append(gx)
    return tuple(ys), tuple(gs)


def saturated(x, term):
    """the elements whose activation sits on the clamp (for depth: of the channel mean)"""
    x = x.double()
    if term == "depth":
        x = ((x[:, 0:1] + x[:, 1:2]) + x[:, 2:3]) / 3
    return (1.01 * torch.tanh(x)).abs() > 1


def kink_distance(x, term):
    """min | |1.01 tanh| - 1 | in fp64 (for depth: of the channel mean)"""
    x = x.double()
    if term == "depth":
        x = ((x[:, 0:1] + x[:, 1:2]) + x[:, 2:3]) / 3
    return float(((1.01 * torch.tanh(x)).abs() - 1).abs().min())
