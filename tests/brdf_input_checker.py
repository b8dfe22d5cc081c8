"""Checker for ``sgr.brdf_encoder_input``: the contract of DESIGN.md section 8c written out in torch, in whatever dtype and on whatever
device its inputs have (fp64 = the arbiter, fp32 = the yardstick ``e_ref`` where no fixture supplies the reference's own).
TEST INFRASTRUCTURE ONLY; own code, written from the contract: the bilinear resize and the adaptive pooling are spelled out as
interpolation / averaging matrices built from their index rules, nothing calls ``F.interpolate`` or ``F.adaptive_avg_pool2d`` -- so that
it is an independent statement of what the kernels compute.  tests/test_brdf_input.py pins it to the fixtures the unmodified reference
produced (tests/golden/g15_brdfin_*.npz)."""
import numpy as np
import torch

INPUTS = ("im", "albedoPre", "normalPre", "roughPre", "depthPre", "diffusePre", "specularPre")
GROUPS = dict(im=(0, 3), albedo=(3, 6), normal=(6, 9), rough=(9, 10), depth=(10, 11), diffuse=(11, 14), specular=(14, 17))      # wrapperBRDF.py:98-100


def load_inputs(z):
    """the seven fp32 input arrays of a fixture.  An array too large to store as fp32 (case ``full``) is stored as ``<name>_q`` uint8 with
    ``<name>_scale`` (a power of two) and ``<name>_offset``: ``x = q * scale + offset``, exact in fp32."""
    out = {}
    for k in INPUTS:
        if k in z.files:
            out[k] = z[k].astype(np.float32)
        else:
            out[k] = z[k + "_q"].astype(np.float32) * np.float32(z[k + "_scale"]) + np.float32(z[k + "_offset"])
    return out


def _bilinear_matrix(n_out, n_in, like):
    """[n_out, n_in]: torch's bilinear rule, align_corners=False, no antialiasing: source = max(scale (dst + 0.5) - 0.5, 0)"""
    kw = dict(dtype=like.dtype, device=like.device)
    scale = torch.tensor(float(n_in), **kw) / torch.tensor(float(n_out), **kw)
    r = torch.clamp(scale * (torch.arange(n_out, **kw) + 0.5) - 0.5, min=0)
    i0 = torch.clamp(r.floor().long(), max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = r - i0.to(like.dtype)
    m = torch.zeros(n_out, n_in, **kw)
    rows = torch.arange(n_out, device=like.device)
    m.index_put_((rows, i0), 1 - l1, accumulate=True)
    m.index_put_((rows, i1), l1, accumulate=True)
    return m


def _pool_matrix(n_out, n_in, like):
    """[n_out, n_in]: adaptive average pooling, window [floor(i n_in / n_out), ceil((i + 1) n_in / n_out))"""
    m = torch.zeros(n_out, n_in, dtype=like.dtype, device=like.device)
    for i in range(n_out):
        a, b = (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)
        m[i, a:b] = 1.0 / (b - a)
    return m


def resize(x, H, W):
    h, w = x.shape[2], x.shape[3]
    if (h, w) == (H, W):
        return x
    if not (h < H or w < W):
        raise ValueError(f"a {h}x{w} map cannot enter a {H}x{W} input tensor")
    return _bilinear_matrix(H, h, x) @ x @ _bilinear_matrix(W, w, x).T


def pooled(im, R, C):
    return _pool_matrix(R, im.shape[2], im) @ im @ _pool_matrix(C, im.shape[3], im).T


def diffspec_sums(diffuse, spec, im_small):
    """the five masked sums of the first regression per image, and det = a11 a22 - a12^2"""
    m = (im_small < 0.9).to(im_small.dtype)
    d, s, i = (diffuse * m).flatten(1), (spec * m).flatten(1), (im_small * m).flatten(1)
    a11, a22, a12, b1, b2 = (d * d).sum(1), (s * s).sum(1), (d * s).sum(1), (d * i).sum(1), (s * i).sum(1)
    return a11, a22, a12, b1, b2, a11 * a22 - a12 * a12


def diffspec_coefs(diffuse, spec, im_small):
    """-> (c_d, c_s, c_im) per image, [bn] each"""
    a11, a22, a12, b1, b2, det = diffspec_sums(diffuse, spec, im_small)
    floor = torch.clamp(det, min=1e-2)
    c1, c2 = (b1 * a22 - b2 * a12) / floor, (a11 * b2 - b1 * a12) / floor
    c3 = torch.clamp(b1 / torch.clamp(a11, min=1e-5), 1e-3, 1e3)
    two = det / diffuse[0].numel() > 1e-2
    cd = torch.clamp(torch.where(two, c1, c3), 0, 1000)
    cs = torch.clamp(torch.where(two, c2, torch.zeros_like(c2)), 0, 1000)
    v = lambda c: c.reshape(-1, 1, 1, 1)
    rendered = torch.clamp(v(cd) * diffuse + v(cs) * spec, 0, 1).flatten(1)
    flat = im_small.flatten(1)
    cim = torch.clamp((rendered * flat).sum(1) / torch.clamp((rendered * rendered).sum(1), min=1e-5), 1e-3, 1e3)
    return cd, cs, cim


def brdf_encoder_input(im, albedo, normal, rough, depth, diffuse, spec, size=None, regress=True, normalize=True, remap=False):
    """-> (inputBatch [bn,17,H,W], coef [bn,2])"""
    H, W = (im.shape[2], im.shape[3]) if size is None else size
    if remap:
        normal, rough = 0.5 * (normal + 1), 0.5 * (rough + 1)
    albedo, normal, rough, depth = [resize(t, H, W) for t in (albedo, normal, rough, depth)]
    coef = torch.ones(im.shape[0], 2, dtype=im.dtype, device=im.device)
    if regress:
        cd, cs, cim = diffspec_coefs(diffuse, spec, pooled(im, diffuse.shape[2], diffuse.shape[3]))
        v = lambda c: c.reshape(-1, 1, 1, 1)
        diffuse, spec = v(cim) * (v(cd) * diffuse), v(cim) * (v(cs) * spec)
        coef = torch.stack([cim * cd, cim * cs], 1)
    diffuse, spec = resize(diffuse, H, W), resize(spec, H, W)
    if normalize:
        mean = lambda t: torch.clamp(t.flatten(1).mean(1), min=1e-10).reshape(-1, 1, 1, 1)
        albedo, depth = albedo / mean(albedo) / 3.0, depth / mean(depth) / 3.0
    return torch.cat([im, albedo, normal, rough, depth, diffuse, spec], 1), coef
