"""The contracts of the loader-preparation operators (inverserenderingofindoorscene_amd/loader_prep.py), stated in numpy from the reference's
lines (dataLoader.py:118-154, 231, 246-259, 286-310).  TEST INFRASTRUCTURE: the arbiter of tests/test_loader_prep.py and
tests/test_gpu_loader_prep.py, in fp64 (``dtype=np.float64``) and as the fp32 statement whose bits the kernels aim at (``np.float32``).

Inputs are what the operators take: uint8 / fp32 arrays in the readers' HWC layout, batched.  The masks are decided in fp32 in either mode
(the contract: for each byte value the bits of numpy's fp32 evaluation); everything else follows ``dtype``."""
from __future__ import annotations

import numpy as np

ENV_H0, ENV_W0 = 16, 32      # dataLoader.py:294


def unit(u8, dtype=np.float32):
    """loadImage, :231"""
    return (np.asarray(u8).astype(dtype) - dtype(127.5)) / dtype(127.5)


def seg_value(u8, dtype=np.float32):
    """:120"""
    return dtype(0.5) * (unit(u8, dtype) + dtype(1))


def erode7(obj):
    """binary_erosion(obj, ones((7, 7)), border_value=1) of a [H,W] bool array, written out: the AND over the window, outside = set"""
    H, W = obj.shape
    p = np.ones((H + 6, W + 6), bool)
    p[3:3 + H, 3:3 + W] = obj
    out = np.ones((H, W), bool)
    for dy in range(7):
        for dx in range(7):
            out &= p[dy:dy + H, dx:dx + W]
    return out


def scipy_erosion(obj):
    """the reference's own call (:127-128), for the tests that hold erode7 and the kernels against it.  scipy is imported here, at the call,
    so that no test module loads it while pytest collects: the process in which the earlier GPU tests run stays as it was"""
    import scipy.ndimage as ndimage
    return ndimage.binary_erosion(obj, structure=np.ones((7, 7)), border_value=1)


def masks(seg_u8, erode=True):
    """-> segArea, segEnv, segObj [bn,1,H,W] fp32; :120-131"""
    seg = seg_value(np.asarray(seg_u8)[..., 0], np.float32)
    area = np.logical_and(seg > np.float32(0.49), seg < np.float32(0.51))
    env = seg < np.float32(0.1)
    obj = seg > np.float32(0.9)
    if erode:
        obj = np.stack([erode7(o) for o in obj])
    return tuple(x.astype(np.float32)[:, None] for x in (area, env, obj))


def rank_k(H, W):
    return int(0.95 * W * H * 3)      # :255


def numerator(u, bn, dtype=np.float32):
    """0.95 - 0.1 u formed in double, rounded to fp32 (the reference divides a Python float by an fp32 element); None: the TEST rule"""
    if u is None:
        vals = [0.95 - 0.05] * bn      # :257
    else:
        vals = [0.95 - 0.1 * float(x) for x in np.broadcast_to(np.asarray(u, np.float64).reshape(-1), (bn,))]
    return np.asarray(vals, np.float64).astype(np.float32).astype(dtype)


def scale_hdr(hdr, seg_u8, u=None, dtype=np.float32):
    """-> im [bn,3,H,W], scale [bn], v [bn]; :246-259.  fp32: v is an element of the fp32 products; fp64: of the fp64 products."""
    hdr = np.asarray(hdr, np.float32)
    bn, H, W, _ = hdr.shape
    seg = seg_value(np.asarray(seg_u8)[..., 0], dtype)
    prod = hdr.astype(dtype) * seg[..., None]
    k = rank_k(H, W)
    v = np.stack([np.sort(prod[b].reshape(-1))[k] for b in range(bn)]).astype(dtype)
    scale = (numerator(u, bn, dtype) / np.maximum(v, dtype(0.1))).astype(dtype)
    im = np.clip(scale[:, None, None, None] * hdr.astype(dtype), 0, 1)
    return np.ascontiguousarray(im.transpose(0, 3, 1, 2)[:, ::-1]), scale, v


def brdf_maps(albedo_u8=None, normal_u8=None, rough_u8=None, dtype=np.float32):
    """-> albedo, normal [bn,3,H,W], rough [bn,1,H,W] (None for None); :139-147"""
    chw = lambda x: np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    albedo = normal = rough = None
    if albedo_u8 is not None:
        albedo = chw(seg_value(albedo_u8, dtype) ** dtype(2.2))
    if normal_u8 is not None:
        n = chw(unit(normal_u8, dtype))
        ss = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
        normal = n / np.sqrt(np.maximum(ss, dtype(1e-5)))[:, None]
    if rough_u8 is not None:
        rough = chw(unit(rough_u8, dtype))[:, 0:1]
    return albedo, normal, rough


def envmaps(env_raw, scale, env_ind=None, envHeight=8, envWidth=16, dtype=np.float32):
    """-> [bn,3,R,C,envHeight,envWidth]; :153-154, 298-307.  The 2 x 2 mean is ((a00 + a01) + (a10 + a11)) * 0.25, a00 and a01 horizontal
    neighbours; images with env_ind == 0 are exact zeros whatever their raw block holds."""
    env_raw = np.asarray(env_raw, np.float32)
    bn, rawH, rawW, ch = env_raw.shape
    if ch != 3 or rawH % ENV_H0 or rawW % ENV_W0 or (envHeight, envWidth) not in ((8, 16), (16, 32)):
        raise ValueError("env_raw must be [bn, R*16, C*32, 3] and envHeight x envWidth 8 x 16 or 16 x 32")
    R, C = rawH // ENV_H0, rawW // ENV_W0
    e = env_raw.astype(dtype).reshape(bn, R, ENV_H0, C, ENV_W0, 3).transpose(0, 5, 1, 3, 2, 4)      # [bn,3,R,C,16,32]
    if envHeight == 8:
        e = ((e[..., 0::2, 0::2] + e[..., 0::2, 1::2]) + (e[..., 1::2, 0::2] + e[..., 1::2, 1::2])) * dtype(0.25)
    out = np.ascontiguousarray(e * np.asarray(scale).astype(dtype).reshape(bn, 1, 1, 1, 1, 1))
    if env_ind is not None:
        out[np.asarray(env_ind).reshape(bn) == 0] = 0
    return out


def prepare_batch(raw, phase="TRAIN", isLight=True, u=None, envHeight=8, envWidth=16, dtype=np.float32):
    """the dataBatch dict (cascade 0) for a batch of raw arrays"""
    assert (phase.upper() == "TRAIN") == (u is not None)
    area, env, obj = masks(raw["seg"], erode=isLight)
    im, scale, _ = scale_hdr(raw["im"], raw["seg"], u, dtype)
    albedo, normal, rough = brdf_maps(raw["albedo"], raw["normal"], raw["rough"], dtype)
    bn, _, H, W = im.shape
    out = dict(albedo=albedo, normal=normal, rough=rough, depth=np.asarray(raw["depth"], np.float32).reshape(bn, 1, H, W).astype(dtype), segArea=area, segEnv=env,
               segObj=obj, im=im)
    if isLight:
        ind = np.asarray(raw["envmapsInd"], np.float32).reshape(bn)
        out["envmaps"] = envmaps(raw["envmaps"], scale, ind, envHeight, envWidth, dtype)
        out["envmapsInd"] = ind.reshape(bn, 1, 1, 1)
    return out


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.abs(a).max())
