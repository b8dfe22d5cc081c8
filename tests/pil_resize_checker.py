"""numpy restatement of PIL's 8-bit ``ImagingResample``, the arbiter of the ``pil_resize`` tests next to the bytes the
installed Pillow wrote into tests/golden/g31_pil_resize_*.npz.  Everything here is integer arithmetic on a table of fixed-point coefficients
that is formed in double, so every comparison against it is ``==``."""
import math

import numpy as np

PRECISION_BITS = 22
FILTERS = {"lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4, "hamming": 5}      # PIL's own codes (Image.Resampling)
SUPPORT = {"lanczos": 3.0, "bilinear": 1.0, "bicubic": 2.0, "box": 0.5, "hamming": 1.0}


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


_F = {"lanczos": _lanczos, "bilinear": _bilinear, "bicubic": _bicubic, "box": _box, "hamming": _hamming}


def ksize_of(in_size, out_size, filt):
    filterscale = max(in_size / out_size, 1.0)
    return int(math.ceil(SUPPORT[filt] * filterscale)) * 2 + 1


def table(in_size, out_size, filt):
    """-> (bounds [out,2] int32 = (xmin, xmax), kk [out,ksize] int32, ksize); the source box is the whole axis"""
    f = _F[filt]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[filt] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale      # PIL multiplies by the reciprocal
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def table_stats(kk):
    """(max |k|, max over the rows of sum |k|): the figures the 24-bit multiply and the int32 sum depend on"""
    a = np.abs(kk.astype(np.int64))
    return int(a.max()), int(a.sum(axis=1).max())


def one_pass(src, bounds, kk, axis):
    """src uint8 [H,W,C]; the pass along `axis` (0 rows, 1 columns) for the table's output indices"""
    s = np.moveaxis(src.astype(np.int64), axis, 0)
    out = np.empty((len(bounds),) + s.shape[1:], np.int64)
    for xx, (xmin, xmax) in enumerate(bounds):
        acc = np.full(s.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for x in range(xmax):
            acc = acc + s[xmin + x] * int(kk[xx, x])
        assert np.abs(acc).max() < 2 ** 31      # the sum stays an int32
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def needed_rows(H, out_h, filt, r0, h):
    """source rows [ya, yb) the output rows r0 .. r0 + h - 1 read"""
    b, _, _ = table(H, out_h, filt)
    return int(b[r0, 0]), int(b[r0 + h - 1, 0] + b[r0 + h - 1, 1])


def resize(im, size, filt="lanczos", window=None):
    """im uint8 [H,W,C] -> uint8 [h,w,C] of ``Image.resize(size, filt)``, size = (width, height); window = (r0, c0, h, w) of the result"""
    H, W, _ = im.shape
    out_w, out_h = size
    r0, c0, h, w = window if window is not None else (0, 0, out_h, out_w)
    out = im
    if out_w != W:
        bh, kh, _ = table(W, out_w, filt)
        rows = slice(None)
        if out_h != H:
            ya, yb = needed_rows(H, out_h, filt, r0, h)
            rows = slice(ya, yb)
        else:
            rows = slice(r0, r0 + h)
        out = one_pass(im[rows], bh[c0:c0 + w], kh[c0:c0 + w], 1)
    else:
        out = im[:, c0:c0 + w]
    if out_h != H:
        bv, kv, _ = table(H, out_h, filt)
        bv = bv[r0:r0 + h].copy()
        if out_w != W:
            bv[:, 0] -= needed_rows(H, out_h, filt, r0, h)[0]
        out = one_pass(out, bv, kv[r0:r0 + h], 0)
    elif out_w == W:
        out = out[r0:r0 + h]
    return np.ascontiguousarray(out)


def iiw_geometry(nh, nw, imHeight, imWidth):
    """iiwDataLoader.py:115-133 without the draw: (newH, newW, gap, along) with along = 'rows' | 'columns' the axis the crop moves on"""
    scaleW = float(imWidth) / float(nw)
    scaleH = float(imHeight) / float(nh)
    if scaleW > scaleH:
        newW = imWidth
        newH = int(np.ceil(scaleW * nh))
        return newH, newW, newH - imHeight, "rows"
    newH = imHeight
    newW = int(np.ceil(scaleH * nw))
    return newH, newW, newW - imWidth, "columns"


# ---- the fixtures' cases (tools/make_golden_pil_resize.py writes them, the tests read them) ------------------------------------------------
# number: (source H, source W, target W, target H, filters)
ALL_FILTERS = ("lanczos", "bilinear", "bicubic", "box", "hamming")
CASES = {
    1: (48, 64, 32, 24, ALL_FILTERS),
    2: (37, 53, 20, 17, ALL_FILTERS),
    3: (30, 40, 57, 41, ALL_FILTERS),
    4: (33, 47, 47, 20, ALL_FILTERS),
    5: (33, 47, 30, 33, ALL_FILTERS),
    6: (5, 7, 3, 2, ALL_FILTERS),
    7: (2, 3, 1, 1, ALL_FILTERS),
    8: (341, 512, 320, 214, ("lanczos",)),
    9: (500, 375, 240, 320, ("lanczos",)),
    10: (33, 47, 47, 33, ALL_FILTERS),
    11: (97, 131, 9, 7, ("lanczos",)),
    12: (480, 640, 320, 240, ("lanczos",)),
    13: (341, 512, 361, 240, ("lanczos",)),      # the IIW geometry: imHeight 240, imWidth 320, gap 41 along the columns
}
TILED, TWO_PASS = 2, 1
# where the tiled route takes a case: both passes run, ksize <= 32 and the tiles' extents fit; `auto` goes there from
# 256 tiles in a launch on
ROUTE = {1: TILED, 2: TILED, 3: TILED, 4: TWO_PASS, 5: TWO_PASS, 6: TILED, 7: TILED, 8: TILED, 9: TILED, 10: TWO_PASS, 11: TWO_PASS, 12: TILED, 13: TILED}
# (r0, c0, h, w): interior and edge-touching windows of cases 2 and 8; the crop offsets of the IIW geometry (case 13, gap 41)
WINDOWS = {2: [(3, 4, 9, 11), (0, 0, 5, 20), (12, 13, 5, 7), (16, 0, 1, 1), (0, 19, 17, 1)],
           8: [(50, 70, 40, 100), (0, 0, 214, 1), (213, 0, 1, 320), (100, 256, 33, 64), (7, 1, 200, 318)]}
IIW_CS = (0, 20, 41)
KINDS = ("noise", "smooth", "binary")
SMALL = (1, 2, 3, 4, 5, 6, 7, 10)      # one file per case: every C, kind and filter
LARGE = (8, 9, 11)                     # one file per (case, C, kind)
SINGLE = {12: (3, "binary"), 13: (3, "noise")}      # one image each


def fixture_names():
    names = [f"c{n}" for n in SMALL]
    names += [f"c{n}_C{C}_{kind}" for n in LARGE for C in (1, 3) for kind in KINDS]
    names += [f"c{n}_C{C}_{kind}" for n, (C, kind) in SINGLE.items()]
    return names


def entries(z):
    """the (C, kind, filter) triples a fixture file holds, with its arrays: yields (tag, im, filter, want)"""
    for key in z.files:
        if key.startswith("out_"):
            _, C, kind, filt = key.split("_")
            yield key[4:], z[f"im_{C}_{kind}"], filt, z[key]
