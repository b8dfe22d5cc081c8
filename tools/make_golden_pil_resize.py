"""Writes tests/golden/g31_pil_resize_*.npz: inputs and the bytes the INSTALLED Pillow's ``Image.resize`` gives for them, with the integer
coefficient tables and bounds of each geometry from the numpy checker (tests/pil_resize_checker.py).  Data only.

    python tools/make_golden_pil_resize.py

Per file: ``geom`` = (H, W, outW, outH); ``im_<C>_<kind>`` uint8 [H,W,C]; ``out_<C>_<kind>_<filter>`` uint8 [outH,outW,C]; per filter ``hb_ hk_``
(the horizontal table's bounds [outW,2] and coefficients [outW,ksize]) and ``vb_ vk_`` (vertical); ``pillow`` the version that wrote the bytes.
The cases are tests/pil_resize_checker.CASES; images are noise, a smooth pattern and random 0 / 255 (which reaches both clamps)."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pil_resize_checker as K      # noqa: E402

PIL_FILTER = {"lanczos": Image.Resampling.LANCZOS, "bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC,
              "box": Image.Resampling.BOX, "hamming": Image.Resampling.HAMMING}


def image(kind, H, W, C, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (H, W, C), dtype=np.uint8) * 255).astype(np.uint8)
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    v = 127.5 + 90.0 * np.sin(0.11 * x + 0.5 * c) * np.cos(0.07 * y - 0.3 * c) + 37.0 * np.sin(0.9 * x + 1.3 * y)
    return np.clip(np.round(v), 0, 255).astype(np.uint8)


def pil_resize(im, size, filt):
    """the installed Pillow on an 'L' or 'RGB' image"""
    pim = Image.fromarray(im[:, :, 0], "L") if im.shape[2] == 1 else Image.fromarray(im, "RGB")
    out = np.asarray(pim.resize(size, PIL_FILTER[filt]))
    return np.ascontiguousarray(out.reshape(size[1], size[0], im.shape[2]))


def build(n, combos):
    H, W, out_w, out_h, filters = K.CASES[n]
    d = dict(geom=np.array([H, W, out_w, out_h], np.int32), pillow=np.array(PIL.__version__))
    for filt in filters:
        hb, hk, _ = K.table(W, out_w, filt)
        vb, vk, _ = K.table(H, out_h, filt)
        d.update({f"hb_{filt}": hb, f"hk_{filt}": hk, f"vb_{filt}": vb, f"vk_{filt}": vk})
    for C, kind in combos:
        im = image(kind, H, W, C, 3100 + 10 * n + C + K.KINDS.index(kind) * 3)
        d[f"im_{C}_{kind}"] = im
        for filt in filters:
            d[f"out_{C}_{kind}_{filt}"] = pil_resize(im, (out_w, out_h), filt)
    return d


def main():
    out_dir = os.path.join(ROOT, "tests", "golden")
    jobs = {f"c{n}": (n, [(C, kind) for C in (1, 3) for kind in K.KINDS]) for n in K.SMALL}
    jobs.update({f"c{n}_C{C}_{kind}": (n, [(C, kind)]) for n in K.LARGE for C in (1, 3) for kind in K.KINDS})
    jobs.update({f"c{n}_C{C}_{kind}": (n, [(C, kind)]) for n, (C, kind) in K.SINGLE.items()})
    assert sorted(jobs) == sorted(K.fixture_names())
    for name, (n, combos) in jobs.items():
        path = os.path.join(out_dir, f"g31_pil_resize_{name}.npz")
        np.savez_compressed(path, **build(n, combos))
        size = os.path.getsize(path)
        assert size < (1 << 20), (path, size)
        print(f"{os.path.basename(path)}: {size} bytes")


if __name__ == "__main__":
    main()
