"""Golden vectors for the cascade-1 BRDF encoder input, produced by the UNMODIFIED reference (wrapperBRDF.py, models.py).
TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout); never runs on the GPU machine:

    python tools/make_golden_brdf_input.py        # writes tests/golden/g15_brdfin_<case>.npz

``wrapperBRDF.wrapperBRDF`` runs as it is with ``opt.cascadeLevel = 1``, in the manner of tools/make_golden_brdf_objective.py: stub
decoders, a stub encoder that records the ``inputBatch`` it is handed (wrapperBRDF.py:103), ``torch.Tensor.cuda`` rebound to the identity
on a GPU-less machine.  Each case runs twice, in fp64 (the arbiter) and in fp32; per channel group of the 17-channel tensor the file holds
``ref64_*``, ``ref32_*`` and ``e_ref_*`` = the rel-L2 distance between them.  The wrapper does not return the ``LSregressDiffSpec``
coefficients, so the tool calls ``models.LSregressDiffSpec`` on the wrapper's own arguments (wrapperBRDF.py:66-71) and reads them off one
element per image that the inputs hold at a power of two (``diffusePre[b,0,0,0]``, ``specularPre[b,0,0,0]``): there the scaled render is
the coefficient times a power of two, exactly.  ``e_ref_coef`` is the absolute fp32-vs-fp64 distance per coefficient.

The result is discontinuous at ``imSmall == 0.9`` and at ``det / (3 R C) == 1e-2``; no fixture may decide these by rounding.  For every
case the tool asserts ``min |imSmall - 0.9| >= 1e-4``, ``|det / (3 R C) - 1e-2| >= 1e-5`` per image and that the fp32 and the fp64 run
took the same branch; it darkens the windows of offending cells before the reference runs.

The case ``full`` (240 x 320) stores its inputs as uint8 codes with a power-of-two scale (``x = q * scale + offset``, exact in fp32) and
its outputs as ``out[:, :, ::8, ::8]`` plus per-channel fp64 sums, to stay under the size limit; its ``e_ref_*`` are those of the whole
tensor."""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("SGR_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
MAX_BYTES = 1 << 20
INPUTS = ("im", "albedoPre", "normalPre", "roughPre", "depthPre", "diffusePre", "specularPre")
GROUPS = dict(im=(0, 3), albedo=(3, 6), normal=(6, 9), rough=(9, 10), depth=(10, 11), diffuse=(11, 14), specular=(14, 17))
STRIDE = 8


def reference():
    if not os.path.isfile(os.path.join(REF, "wrapperBRDF.py")):
        raise SystemExit("reference not mounted")
    if REF not in sys.path:
        sys.path.insert(0, REF)
    if not torch.cuda.is_available():
        torch.Tensor.cuda = lambda self, *a, **k: self      # the wrapper calls .cuda() unconditionally
    import models
    import wrapperBRDF
    return models, wrapperBRDF


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.abs(a).max())


class Recorder:
    """the stub encoder: keeps what it is handed, returns six placeholders"""

    def __init__(self):
        self.seen = None

    def __call__(self, x):
        self.seen = x.detach().clone()
        return (None,) * 6


class Stub:
    def __init__(self, out):
        self.out = out

    def __call__(self, *args):
        return self.out


def run_wrapper(W, inp, dtype):
    """wrapperBRDF.wrapperBRDF, cascadeLevel 1 -> the inputBatch its encoder received"""
    t = lambda k: torch.from_numpy(inp[k]).to(dtype)
    bn, _, H, Wd = inp["im"].shape
    z = lambda c: torch.zeros(bn, c, H, Wd, dtype=dtype)
    data = dict(albedo=z(3), normal=z(3), rough=z(1), depth=z(1), segArea=z(1), segEnv=z(1), segObj=z(1) + 1, im=t("im"), albedoPre=t("albedoPre"),
                normalPre=t("normalPre"), roughPre=t("roughPre"), depthPre=t("depthPre"), diffusePre=t("diffusePre"), specularPre=t("specularPre"),
                envmapsPre=torch.zeros(bn, 1, dtype=dtype))
    opt = types.SimpleNamespace(cascadeLevel=1, imHeight=H, imWidth=Wd)
    enc = Recorder()
    W.wrapperBRDF(data, opt, enc, Stub(z(3)), Stub(z(3)), Stub(z(1)), Stub(z(1)))
    assert enc.seen is not None and enc.seen.dtype == dtype and tuple(enc.seen.shape) == (bn, 17, H, Wd)
    return enc.seen.numpy()


def run_coef(M, inp, dtype):
    """models.LSregressDiffSpec on the wrapper's arguments (wrapperBRDF.py:66-71) -> [bn,2], read off the power-of-two elements"""
    t = lambda k: torch.from_numpy(inp[k]).to(dtype)
    d, s = t("diffusePre"), t("specularPre")
    small = F.adaptive_avg_pool2d(t("im"), (d.size(2), d.size(3)))
    ds, ss = M.LSregressDiffSpec(d.detach(), s.detach(), small, d, s)
    out = np.zeros((d.size(0), 2), np.float64)
    for b in range(d.size(0)):
        for k, (orig, scaled) in enumerate(((d, ds), (s, ss))):
            p = float(orig[b, 0, 0, 0])
            if p == 0.0:      # an all-zero plane: the reference's coefficient is 0 there (the diffuse-only branch) or irrelevant
                assert float(orig[b].abs().max()) == 0.0 and float(scaled[b].abs().max()) == 0.0
                continue
            assert np.frexp(p)[0] == 0.5, p      # a power of two
            out[b, k] = float(scaled[b, 0, 0, 0]) / p
    return out


def conditions(inp, dtype):
    """(min |imSmall - 0.9|, det / (3 R C) per image, bright share per image) of the reference's regression in `dtype`, own arithmetic on
    torch's own pooling"""
    t = lambda k: torch.from_numpy(inp[k]).to(dtype)
    d, s = t("diffusePre"), t("specularPre")
    small = F.adaptive_avg_pool2d(t("im"), (d.size(2), d.size(3)))
    m = (small < 0.9).to(dtype)
    dm, sm = (d * m).flatten(1), (s * m).flatten(1)
    det = (dm * dm).sum(1) * (sm * sm).sum(1) - (dm * sm).sum(1) ** 2
    return float((small - 0.9).abs().min()), (det / d[0].numel()).double().numpy(), (1 - m).flatten(1).mean(1).double().numpy(), small


def settle(inp):
    """darken the pooling windows of cells within 2e-4 of the 0.9 threshold until none is left"""
    R, C = inp["diffusePre"].shape[2:]
    H, W = inp["im"].shape[2:]
    for _ in range(50):
        small = F.adaptive_avg_pool2d(torch.from_numpy(inp["im"]).double(), (R, C)).numpy()
        bad = np.argwhere(np.abs(small - 0.9) < 2e-4)
        if len(bad) == 0:
            return
        for b, ch, r, c in bad:
            y0, y1, x0, x1 = (r * H) // R, -((-(r + 1) * H) // R), (c * W) // C, -((-(c + 1) * W) // C)
            inp["im"][b, ch, y0:y1, x0:x1] *= np.float32(0.97)
    raise AssertionError("cells stay at the 0.9 threshold")


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def inputs(rng, bn, H, W, h, w, R, C):
    f = lambda *s: rng.random(s).astype(np.float32)
    # the image: blocks of differing brightness, so that between a third and a half of the pooled cells lie above 0.9
    bright = np.kron(0.4 + 1.2 * f(bn, 1, (H + 5) // 6, (W + 5) // 6), np.ones((6, 6), np.float32))[:, :, :H, :W]
    inp = dict(im=(bright * (0.7 + 0.3 * f(bn, 3, H, W))).astype(np.float32), albedoPre=f(bn, 3, h, w),
               normalPre=unit(rng.standard_normal((bn, 3, h, w))).astype(np.float32), roughPre=f(bn, 1, h, w), depthPre=0.5 + 4.0 * f(bn, 1, h, w),
               diffusePre=0.8 * f(bn, 3, R, C), specularPre=0.3 * f(bn, 3, R, C))
    inp["diffusePre"][:, 0, 0, 0] = 1.0      # where the coefficients are read off (run_coef)
    inp["specularPre"][:, 0, 0, 0] = 0.25
    return inp


def finish(name, inp, M, W, stored_inputs=None, strided=False, expect=None):
    settle(inp)
    gap64, det64, bright, _ = conditions(inp, torch.float64)
    gap32, det32, _, _ = conditions(inp, torch.float32)
    assert min(gap64, gap32) >= 1e-4, (name, gap64, gap32)
    assert (np.abs(det64 - 1e-2) >= 1e-5).all() and (np.abs(det32 - 1e-2) >= 1e-5).all(), (name, det64, det32)
    assert ((det64 > 1e-2) == (det32 > 1e-2)).all(), (name, det64, det32)
    r64, r32 = run_wrapper(W, inp, torch.float64), run_wrapper(W, inp, torch.float32)
    c64, c32 = run_coef(M, inp, torch.float64), run_coef(M, inp, torch.float32)
    if expect:
        expect(c64, det64, bright, r64)
    blob = dict(stored_inputs if stored_inputs is not None else inp)
    for g, (a, b) in GROUPS.items():
        x64, x32 = r64[:, a:b], r32[:, a:b]
        blob["e_ref_" + g] = np.float64(rel(x32, x64))
        if strided:
            blob["sum64_" + g], blob["sum32_" + g] = x64.sum((2, 3)), x32.astype(np.float64).sum((2, 3))
            x64, x32 = x64[:, :, ::STRIDE, ::STRIDE], x32[:, :, ::STRIDE, ::STRIDE]
        blob["ref64_" + g], blob["ref32_" + g] = np.ascontiguousarray(x64), np.ascontiguousarray(x32)
    blob["ref64_coef"], blob["ref32_coef"], blob["e_ref_coef"] = c64, c32.astype(np.float32), np.abs(c32 - c64)
    blob["det_over_n"], blob["bright_share"], blob["stride"] = det64, bright, np.int64(STRIDE if strided else 1)
    path = os.path.join(OUT, f"g15_brdfin_{name}.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    e = {k[6:]: f"{float(np.max(v)):.1e}" for k, v in blob.items() if k.startswith("e_ref_")}
    print(f"{name:10s} {size / 1024:7.1f} KiB  gap {min(gap64, gap32):.1e}  det/n {np.round(det64, 4)}  bright {np.round(bright, 2)}  coef {np.round(c64, 4).tolist()}\n"
          f"           e_ref {e}")


def main():
    M, W = reference()
    rng = lambda s: np.random.default_rng(s)

    # odd planes (the unaligned path), non-integer pooling windows along W, a resize in both directions
    finish("small", inputs(rng(1501), 3, 30, 41, 15, 21, 15, 21), M, W)
    # the identity branch for the BRDF maps, an integer pooling ratio, the vector path
    finish("same", inputs(rng(1502), 2, 24, 32, 24, 32, 12, 16), M, W)

    inp = inputs(rng(1503), 3, 24, 32, 12, 16, 12, 16)
    inp["specularPre"][0] = 0.0                                  # image 0: no specular render, det = 0 -> the diffuse-only branch
    inp["diffusePre"][1] *= np.float32(2.0 ** -17)               # image 1: renders so dark that c_d sits at its 1e3 clamp (diffuse-only branch again:
    inp["specularPre"][1] *= np.float32(2.0 ** -17)              #          det / n is far below 1e-2)
    inp["im"][2] = (0.75 + 0.4 * rng(15031).random(inp["im"][2].shape)).astype(np.float32)      # image 2: most pooled cells at or above 0.9

    def expect_fallback(c64, det, bright, r64):
        assert det[0] == 0.0 and c64[0, 1] == 0.0 and c64[0, 0] > 0.0, (det, c64)
        assert det[1] < 1e-3, det
        assert 0.5 < bright[2] < 0.95, bright
    finish("fallback", inp, M, W, expect=expect_fallback)

    inp = inputs(rng(1504), 2, 24, 32, 12, 16, 12, 16)
    inp["albedoPre"][0] = 0.0                                    # mean 0 -> the 1e-10 floor, output 0
    inp["depthPre"][0] *= np.float32(1e-12)                      # tiny depth: its mean is below the floor

    def expect_floor(c64, det, bright, r64):
        assert np.abs(r64[0, 3:6]).max() == 0.0 and 0.0 < r64[0, 10].max() < 1.0, (r64[0, 3:6].max(), r64[0, 10].max())
    finish("meanfloor", inp, M, W, expect=expect_floor)

    # an env grid with fewer cells than workgroups
    inp = inputs(rng(1505), 1, 12, 16, 6, 8, 3, 4)
    inp["im"] *= np.float32(0.6)                                 # 36 cells: keep most of them below the 0.9 mask

    def expect_tiny(c64, det, bright, r64):
        assert bright[0] < 0.5 and det[0] > 1e-2, (bright, det)
    finish("tiny", inp, M, W, expect=expect_tiny)

    # full size; inputs as uint8 codes (a 2 x 2 pooling window of multiples of 2^-8 is a multiple of 2^-10: at least 3.9e-4 from 0.9)
    r = rng(1506)
    H, Wd, h, w = 240, 320, 120, 160
    q = lambda *s: r.integers(0, 256, s, dtype=np.uint8)
    bright = np.kron(0.4 + 1.2 * r.random((1, 1, H // 8, Wd // 8)), np.ones((8, 8)))
    codes = dict(im=(np.clip(bright * (0.7 + 0.3 * r.random((1, 3, H, Wd))), 0, 1.99) * 128).astype(np.uint8), albedoPre=q(1, 3, h, w), normalPre=q(1, 3, h, w),
                 roughPre=q(1, 1, h, w), depthPre=q(1, 1, h, w), diffusePre=q(1, 3, h, w), specularPre=q(1, 3, h, w))
    codes["diffusePre"][:, 0, 0, 0] = 128
    codes["specularPre"][:, 0, 0, 0] = 128
    affine = dict(im=(2.0 ** -7, 0.0), albedoPre=(2.0 ** -8, 0.0), normalPre=(2.0 ** -7, -1.0), roughPre=(2.0 ** -8, 0.0), depthPre=(2.0 ** -6, 0.5),
                  diffusePre=(2.0 ** -8, 0.0), specularPre=(2.0 ** -10, 0.0))
    inp, stored = {}, {}
    for k in INPUTS:
        sc, off = affine[k]
        inp[k] = codes[k].astype(np.float32) * np.float32(sc) + np.float32(off)
        stored[k + "_q"], stored[k + "_scale"], stored[k + "_offset"] = codes[k], np.float32(sc), np.float32(off)
    before = inp["im"].copy()
    finish("full", inp, M, W, stored_inputs=stored, strided=True)
    assert np.array_equal(before, inp["im"]), "the stored codes no longer describe the image"


if __name__ == "__main__":
    main()
