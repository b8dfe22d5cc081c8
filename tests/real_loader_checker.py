"""The contracts of the real-image loader operators (inverserenderingofindoorscene_amd/real_loader_prep.py) in numpy:
nyuDataLoader.py:75-131, 143-173 and iiwDataLoader.py:136-137, 205-214.  tests/test_real_loader_prep.py pins this module to the fixtures the
unmodified reference produced (tests/golden/g27_*.npz, tools/make_golden_real_loader.py); the GPU tests use it at shapes no fixture holds.

``dtype`` is the type the ARITHMETIC runs in: np.float32 follows the reference's own order of operations, np.float64 is the yardstick.  The
resize coordinates are the same in both: OpenCV's INTER_LINEAR rule rounds them to fp32 (export_checker.resize_linear)."""
import numpy as np

from export_checker import resize_linear

NYU_KEYS = ("normal", "depth", "segNormal", "segDepth", "im")
DEPTH_THRESHOLDS = (1.0, 10.0)
SEG_DEPTH_MARGIN, SEG_DEPTH_EXEMPT_SHARE = 1e-5, 0.01


def load_image(u8, rs, re, cs, ce, dtype, gamma=False):
    """nyuDataLoader.NYULoader.loadImage on a decoded BGR array"""
    im = u8[:, :, ::-1]
    im = np.ascontiguousarray(im[rs:re, cs:ce, :].astype(dtype))
    if gamma:
        im = (im / 255.0) ** 2.2
        im = 2 * im - 1
    else:
        im = (im - 127.5) / 127.5
    return np.transpose(im, [2, 0, 1])


def nyu_sample(im_u8, normal_u8, seg_u8, depth, crop, flip, colour, H, W, dtype=np.float32):
    """one sample -> dict of CHW arrays in ``dtype``.  ``crop`` (rs, cs, cropH, cropW) or None (TEST: the whole source); ``flip`` / ``colour``
    None in TEST."""
    Hs, Ws = depth.shape
    rs, cs, ch, cw = (0, 0, Hs, Ws) if crop is None else (int(v) for v in crop)
    assert ch >= 1 and cw >= 1 and 0 <= rs and rs + ch <= Hs and 0 <= cs and cs + cw <= Ws, (crop, Hs, Ws)
    re, ce = rs + ch, cs + cw
    segNormal = 0.5 * (load_image(seg_u8, rs, re, cs, ce, dtype) + 1)[0:1]
    im = 0.5 * (load_image(im_u8, rs, re, cs, ce, dtype, gamma=True) + 1)
    normal = load_image(normal_u8, rs, re, cs, ce, dtype)
    normal = normal / np.sqrt(np.maximum(np.sum(normal * normal, axis=0), 1e-5))[np.newaxis, :]
    d = np.asarray(depth).astype(dtype)[rs:re, cs:ce][np.newaxis]
    if (ch, cw) != (H, W):
        d, normal, segNormal, im = (resize_linear(np.ascontiguousarray(v), H, W) for v in (d, normal, segNormal, im))
    segDepth = np.logical_and(d > 1, d < 10).astype(dtype)
    normal = normal / np.maximum(np.sqrt(np.sum(normal * normal, axis=0)[np.newaxis]), 1e-5)
    if flip is not None and bool(flip):
        normal = np.ascontiguousarray(normal[:, :, ::-1])
        normal[0] = -normal[0]
        d, segNormal, segDepth, im = (np.ascontiguousarray(v[:, :, ::-1]) for v in (d, segNormal, segDepth, im))
    if colour is not None:
        im = im * np.asarray(colour, np.float64).reshape(3, 1, 1)      # float64 whatever im is, as in the reference
    out = dict(normal=normal, depth=d, segNormal=segNormal, segDepth=segDepth, im=im.astype(dtype))
    assert all(v.dtype == np.dtype(dtype) for v in out.values()), {k: v.dtype for k, v in out.items()}
    return out


def nyu_prepare(raw, crop=None, flip=None, colour=None, H=480, W=640, dtype=np.float32):
    """the batch: ``raw`` holds im / normal / seg uint8 [bn,Hs,Ws,3] and depth [bn,Hs,Ws]; the three augmentation arguments all or none"""
    assert (crop is None) == (flip is None) == (colour is None)
    bn = raw["im"].shape[0]
    rows = [nyu_sample(raw["im"][b], raw["normal"][b], raw["seg"][b], raw["depth"][b], None if crop is None else crop[b], None if flip is None else flip[b],
                       None if colour is None else colour[b], H, W, dtype) for b in range(bn)]
    return {k: np.stack([r[k] for r in rows]) for k in NYU_KEYS}


def nyu_augmentation(u, imHeight, imWidth, imWidthMax=600, imWidthMin=560):
    """nyuDataLoader.py:76-82, 121-129 from the seven draws of one sample, in Python's own arithmetic -> (crop, flip, colour)"""
    scale = float(u[0])
    cw = int(np.round((imWidthMax - imWidthMin) * scale + imWidthMin))
    ch = int(float(imHeight) / float(imWidth) * cw)
    rs = int(np.round((480 - ch) * float(u[1])))
    cs = int(np.round((640 - cw) * float(u[2])))
    return (rs, cs, ch, cw), bool(u[3] > 0.5), 1 + (np.asarray(u[4:7], np.float64) * 0.4 - 0.2)


def iiw_image(im_u8, dtype=np.float32):
    """iiwDataLoader.py:136-137, 205-214 per image: [bn,H,W,3] uint8 -> [bn,3,H,W]; an all-black image is NaN throughout"""
    out = []
    for a in im_u8:
        im = np.asarray(a, dtype=dtype)
        im = im / 255.0
        im = im ** (2.2)
        im = np.transpose(im, [2, 0, 1])
        with np.errstate(invalid="ignore"):
            out.append(im / im.max())
    return np.stack(out)


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------

def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def bound_of(e_ref):
    """the project's standing bound on a rel-L2 distance from the fp64 evaluation"""
    return max(2.0 * float(e_ref), 1e-6)


def ulp_distance(a, b):
    """the largest distance in units of the last place between two fp32 arrays of equal shape (equal signs or zeros assumed near zero)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    key = lambda v: np.where(v.view(np.int32) < 0, np.int64(-2147483648) - v.view(np.int32).astype(np.int64), v.view(np.int32).astype(np.int64))
    return int(np.abs(key(a) - key(b)).max()) if a.size else 0


def seg_depth_mask(depth64):
    """where segDepth is compared with ==: the fp64 resized depth farther than 1e-5 t from both thresholds t"""
    d = np.asarray(depth64, np.float64)
    return np.all([np.abs(d - t) > SEG_DEPTH_MARGIN * t for t in DEPTH_THRESHOLDS], axis=0)


def check_seg_depth(got, want64, depth64, tag=""):
    m = seg_depth_mask(depth64)
    left_out = 1.0 - float(m.mean())
    print(f"{tag}: segDepth {m.size} pixels, left out {left_out * 100:.3f} %, mismatches {int(np.count_nonzero(np.asarray(got)[m] != np.asarray(want64)[m]))}")
    assert left_out <= SEG_DEPTH_EXEMPT_SHARE, (tag, left_out)
    assert np.array_equal(np.asarray(got)[m], np.asarray(want64, np.float32)[m]), tag
    assert np.isin(np.asarray(got), (0.0, 1.0)).all(), tag


def check_nyu(got, want64, e_ref, tag="", seg_depth_everywhere=False):
    """the GPU tests' value check: rel-L2 from the fp64 evaluation within max(2 e_ref, 1e-6) per output; segDepth with == under its cap, or
    (depths that are exact in fp32 and no resize) everywhere.  ``e_ref``: {key: the reference's own fp32 distance from fp64}"""
    for k in ("normal", "depth", "segNormal", "im"):
        g = np.asarray(got[k])
        assert g.dtype == np.float32 and g.shape == want64[k].shape, (tag, k, g.dtype, g.shape, want64[k].shape)
        e = rel_l2(g, want64[k])
        print(f"{tag} {k}: rel-L2 {e:.2e}, bound {bound_of(e_ref[k]):.2e}")
        assert e <= bound_of(e_ref[k]), (tag, k, e, bound_of(e_ref[k]))
    if seg_depth_everywhere:
        assert np.array_equal(np.asarray(got["segDepth"]), np.asarray(want64["segDepth"], np.float32)), tag
    else:
        check_seg_depth(got["segDepth"], want64["segDepth"], want64["depth"], tag)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------

def draw_raw(bn, Hs, Ws, seed):
    """a raw batch: bytes over the whole range (a few normals at the centre value 127/128: the 1e-5 floor's neighbourhood), depths in [0.5, 12]"""
    rng = np.random.default_rng(seed)
    raw = dict(im=rng.integers(0, 256, (bn, Hs, Ws, 3), dtype=np.uint8), normal=rng.integers(0, 256, (bn, Hs, Ws, 3), dtype=np.uint8),
               seg=rng.integers(0, 256, (bn, Hs, Ws, 3), dtype=np.uint8), depth=(0.5 + 11.5 * rng.random((bn, Hs, Ws))).astype(np.float32))
    raw["normal"].reshape(-1, 3)[:: 17] = (128, 127, 128)
    return raw


def draw_aug(bn, Hs, Ws, seed, min_side=1):
    """crop rectangles inside the source, flips and colour scales"""
    rng = np.random.default_rng(seed)
    crop = np.zeros((bn, 4), np.int32)
    for b in range(bn):
        ch, cw = int(rng.integers(min(min_side, Hs), Hs + 1)), int(rng.integers(min(min_side, Ws), Ws + 1))
        crop[b] = (int(rng.integers(0, Hs - ch + 1)), int(rng.integers(0, Ws - cw + 1)), ch, cw)
    return crop, rng.random(bn) > 0.5, 1 + (rng.random((bn, 3)) * 0.4 - 0.2)


# (tag, bn, Hs, Ws, H, W, least crop side): shapes no fixture holds.  The output tile is 16 x 64, four pixels per thread; its source pixels
# are staged in LDS when they fit 24 x 72, and a workgroup whose tile needs more maps each pixel's own 2 x 2.
GPU_SHAPES = (
    ("two tiles and a bit each way", 2, 40, 150, 33, 130, 20),
    ("W = 5: one full group and a tail", 1, 9, 9, 7, 5, 3),
    ("W = 4", 1, 9, 9, 7, 4, 3),
    ("W = 3", 2, 9, 9, 7, 3, 3),
    ("steep reduction", 2, 90, 120, 5, 6, 80),
    ("up by 3", 1, 12, 16, 36, 48, 8),
    ("the training ratio: 120x160 crops near 107x143 to 60x80", 3, 120, 160, 60, 80, 100),
    ("24 source rows: the tile's limit", 1, 24, 9, 16, 7, 24),              # the whole source is the crop
    ("25 source rows: past it", 1, 25, 9, 16, 7, 25),
    ("72 source columns: the limit", 1, 9, 72, 5, 64, 72),
    ("73 source columns: past it", 2, 9, 73, 5, 64, 73),
)
