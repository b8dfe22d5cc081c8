"""Seeded inputs for ``sgr.brdf_encoder_input`` at shapes no reference-made fixture holds, and the list of those shapes.
TEST INFRASTRUCTURE ONLY; needs nothing but numpy, torch and tests/brdf_input_checker.py.

The recipe is the one of tools/make_golden_brdf_input.py: an image of 6 x 6 blocks of differing brightness, U(0,1) albedo and roughness,
unit normals, depth in 0.5..4.5, ``diffusePre[:, 0, 0, 0] = 1`` and ``specularPre[:, 0, 0, 0] = 0.25``, and that tool's settle step (the
pooling windows of cells within 2e-4 of the 0.9 mask threshold are darkened until none is left), here with the checker's ``pooled``.

The operator is discontinuous at ``imSmall == 0.9`` and at ``det / (3 R C) == 1e-2``.  ``conditions`` evaluates the distances to both in
fp32 and in fp64 with the checker, ``assert_settled`` asserts what the tool asserts of a fixture: every pooled cell at least 1e-4 from 0.9,
``|det / n - 1e-2| >= 1e-5`` and the same side in both precisions.  These are conditions on the INPUTS, not tolerances: with them the fp32
and the fp64 evaluation take the same branches, so a GPU result off its bound means the kernel.  tests/test_brdf_input.py asserts them on
the CPU for every case below; the GPU tests build the same arrays from the same seeds."""
import functools

import numpy as np
import torch

import brdf_input_checker as C

# (H, W, h, w, R, C): the image, the four BRDF maps, the env grid
GEOMETRIES = {
    "maps_equal_along_H": (12, 20, 12, 10, 6, 10),
    "maps_equal_along_W_env_at_image_size": (12, 20, 5, 20, 12, 20),
    "nothing_resized": (12, 20, 12, 20, 12, 20),
    "maps_larger_along_H": (12, 20, 16, 10, 6, 10),            # a bilinear down-sample along H
    "env_taller_than_image": (12, 20, 6, 10, 15, 8),           # pooling with R > H
    "non_integer_ratios": (11, 13, 4, 5, 3, 7),
    "single_pixel_maps": (2, 3, 1, 1, 1, 1),
}
HALF = (24, 32, 12, 16, 12, 16)              # W % 4 == 0, maps and env half size
SAME = (24, 32, 24, 32, 12, 16)              # the maps at image size
SAME_ENV = (24, 32, 24, 32, 24, 32)          # and the env grid too
HALF_ENV_SAME = (24, 32, 12, 16, 24, 32)     # half-size maps, env grid at image size
TINY = (12, 16, 6, 8, 3, 4)                  # fewer env cells per channel than workgroups per image

# (bn, H, W, h, w, R, C): more workgroups wanted per image than the cap allows, so pass C strides
STRIDING = {
    "32x129x131": (32, 129, 131, 64, 65, 64, 65),      # V = 1, cap floor 64, two rounds, the second ragged
    "32x200x201": (32, 200, 201, 100, 100, 100, 100),  # V = 1, three rounds
    "32x260x256": (32, 260, 256, 130, 128, 130, 128),  # V = 4, two rounds
    "8x257x259": (8, 257, 259, 128, 129, 128, 129),    # V = 1, the 2048 / bn branch of the cap, two rounds
    "32x260x256_same": (32, 260, 256, 260, 256, 130, 128),  # the identity branch under V = 4: pass C two rounds, pass A's albedo stream
}                                                          # (3 x 66560 elements, 65536 per round) four rounds, its depth stream two
# the identity branch at batch 32 in ONE round: 16896 / 4 / 256 = 17 workgroups against a cap of 64, and pass A's streams (50688 and 16896
# elements) stay below the 65536 of a round -- the batch-32 partner of the fixture `same`, not a striding case
SAME_BATCH32 = (32, 132, 128, 132, 128, 66, 64)


def pass_c_grid(bn, H, W, V):
    """the host's own formula (sgr_brdf_input_fwd): workgroups per image wanted for one round of V pixels per thread, and the cap"""
    return -(-(H * W // V) // 256), max(2048 // bn, 64)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _settle(inp):
    R, Cc = inp["diffusePre"].shape[2:]
    H, W = inp["im"].shape[2:]
    for _ in range(50):
        small = C.pooled(torch.from_numpy(inp["im"]).double(), R, Cc).numpy()
        bad = np.argwhere(np.abs(small - 0.9) < 2e-4)
        if len(bad) == 0:
            return
        for b, ch, r, c in bad:
            y0, y1, x0, x1 = (r * H) // R, -((-(r + 1) * H) // R), (c * W) // Cc, -((-(c + 1) * W) // Cc)
            inp["im"][b, ch, y0:y1, x0:x1] *= np.float32(0.97)
    raise AssertionError("cells stay at the 0.9 threshold")


@functools.lru_cache(maxsize=None)
def _build(seed, bn, H, W, h, w, R, Cc, im_scale):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.random(s).astype(np.float32)
    bright = np.kron(0.4 + 1.2 * f(bn, 1, (H + 5) // 6, (W + 5) // 6), np.ones((6, 6), np.float32))[:, :, :H, :W]
    inp = dict(im=(bright * (0.7 + 0.3 * f(bn, 3, H, W)) * np.float32(im_scale)).astype(np.float32), albedoPre=f(bn, 3, h, w),
               normalPre=_unit(rng.standard_normal((bn, 3, h, w))).astype(np.float32), roughPre=f(bn, 1, h, w), depthPre=0.5 + 4.0 * f(bn, 1, h, w),
               diffusePre=0.8 * f(bn, 3, R, Cc), specularPre=0.3 * f(bn, 3, R, Cc))
    inp["diffusePre"][:, 0, 0, 0] = 1.0
    inp["specularPre"][:, 0, 0, 0] = 0.25
    _settle(inp)
    return inp


def build(seed, bn, H, W, h, w, R, Cc, im_scale=1.0):
    """-> the seven fp32 arrays by name; built once per argument set, never written to afterwards"""
    return _build(int(seed), bn, H, W, h, w, R, Cc, float(im_scale))


def tensors(inp, device="cpu", dtype=torch.float32):
    """the seven inputs in the operator's order, as copies"""
    return [torch.tensor(inp[k], device=device).to(dtype) for k in C.INPUTS]


def conditions(inp, dtype):
    """(min |imSmall - 0.9|, det / (3 R C) per image) of the checker's regression evaluated in `dtype`"""
    d, s = torch.from_numpy(inp["diffusePre"]).to(dtype), torch.from_numpy(inp["specularPre"]).to(dtype)
    small = C.pooled(torch.from_numpy(inp["im"]).to(dtype), d.shape[2], d.shape[3])
    det = C.diffspec_sums(d, s, small)[5]
    return float((small - 0.9).abs().min()), (det / d[0].numel()).double().numpy()


def assert_settled(tag, inp):
    gap64, det64 = conditions(inp, torch.float64)
    gap32, det32 = conditions(inp, torch.float32)
    assert min(gap64, gap32) >= 1e-4, (tag, gap64, gap32)
    assert (np.abs(det64 - 1e-2) >= 1e-5).all() and (np.abs(det32 - 1e-2) >= 1e-5).all(), (tag, det64, det32)
    assert ((det64 > 1e-2) == (det32 > 1e-2)).all(), (tag, det64, det32)
    return min(gap64, gap32), det64


# every input set tests/test_gpu_brdf_input_edges.py draws: tag -> arguments of build()
def _gpu_cases():
    cases = {}
    for k, (name, g) in enumerate(GEOMETRIES.items()):
        cases["geometry " + name] = (1700 + k, 2) + g
    for k, (name, s) in enumerate(STRIDING.items()):
        cases["striding " + name] = (1720 + k,) + s
    cases["same 32x132x128"] = (1730,) + SAME_BATCH32
    for k, (name, g) in enumerate((("half", HALF), ("same", SAME), ("same_env", SAME_ENV), ("half_env_same", HALF_ENV_SAME))):
        cases["aligned " + name] = (1740 + k, 2) + g
    cases["tiny"] = (1750, 1) + TINY + (0.6,)      # most of the 36 cells below the 0.9 mask, as the fixture `tiny`
    return cases


GPU_CASES = _gpu_cases()
