"""Golden vectors for the loader-preparation operators, produced by the UNMODIFIED reference (dataLoader.py).
TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout); never runs on the GPU machine:

    python tools/make_golden_loader_prep.py        # writes tests/golden/g25_loader_<case>.npz

``BatchLoader.__getitem__`` (and through it ``loadImage``, ``loadHdr``, ``scaleHdr``, ``loadBinary``, ``loadEnvmap``) runs as it is on small
samples.  The instance is created without ``__init__`` (its directory walk needs the dataset) and given the attributes ``__init__`` would set.
The PNG maps and the depth file are real files in a temporary directory, read by the reference's own PIL / struct code.  Three imports of
dataLoader.py are absent where this tool runs and get stand-ins:

  cv2       ``imread`` hands back the array prepared under that name (None for a missing one), ``resize`` to the same size is the identity
  h5py      never called at cascade 0
  skimage   ``block_reduce`` is its documented meaning, ``func`` over non-overlapping blocks, applied as skimage applies it (to the
            ``view_as_blocks`` view, over the trailing block axes)

and ``Image.ANTIALIAS`` is aliased to ``Image.LANCZOS`` for the installed PIL (a resize to the same size is a copy there).  ``block_reduce`` is
therefore THE ONE PIECE OF ARITHMETIC NOT EXECUTED FROM THE REFERENCE'S OWN DEPENDENCY; every file says so in ``notes``.  ``scipy.ndimage`` is
the real one.  numpy is seeded per image and the ``u`` that ``scaleHdr`` draws is recorded.

Each file holds the raw inputs as the operators take them (HWC, batched; ``env_raw`` as float16, whose values the fp32 file holds exactly),
every array the reference returned (stacked over the batch), ``v`` (element k of the reference's own sort expression; checked against the
returned scale), ``u``, and ``e_ref_<key>``: the rel-L2 distance of the returned fp32 array from tests/loader_prep_checker.py's fp64
evaluation of the same inputs."""
from __future__ import annotations

import os
import struct
import sys
import tempfile
import types

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SGR_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20
NOTES = ("dataLoader.BatchLoader.__getitem__ run unmodified (numpy %s); stand-ins: cv2.imread hands back the prepared array, cv2.resize to the same size is the "
         "identity, Image.ANTIALIAS = Image.LANCZOS, skimage.measure.block_reduce = the mean over non-overlapping blocks -- the one piece of arithmetic not "
         "executed from the reference's own dependency" % np.__version__)
KEYS = ("albedo", "normal", "rough", "depth", "segArea", "segEnv", "segObj", "im", "envmaps", "envmapsInd")

sys.path.insert(0, os.path.join(ROOT, "tests"))
import loader_prep_checker as K      # noqa: E402

_ARRAYS = {}      # what the stand-in imread hands back, by file name


def block_reduce(image, block_size, func=np.sum, cval=0):
    assert image.ndim == len(block_size) and all(s % b == 0 for s, b in zip(image.shape, block_size))
    nd = image.ndim
    inter = image.reshape([x for s, b in zip(image.shape, block_size) for x in (s // b, b)])
    blocked = inter.transpose(list(range(0, 2 * nd, 2)) + list(range(1, 2 * nd, 2)))      # view_as_blocks: the block axes last
    return func(blocked, axis=tuple(range(nd, 2 * nd)))


def reference():
    if not os.path.isfile(os.path.join(REF, "dataLoader.py")):
        raise SystemExit("reference not mounted")
    cv2 = types.ModuleType("cv2")
    cv2.INTER_AREA = 3

    def imread(name, flag=None):
        a = _ARRAYS.get(name)
        return None if a is None else a.copy()

    def resize(im, size, interpolation=None):
        assert tuple(size) == (im.shape[1], im.shape[0]), (size, im.shape)
        return im
    cv2.imread, cv2.resize = imread, resize
    sk, skm = types.ModuleType("skimage"), types.ModuleType("skimage.measure")
    skm.block_reduce = block_reduce
    sk.measure = skm
    for name, mod in (("cv2", cv2), ("h5py", types.ModuleType("h5py")), ("skimage", sk), ("skimage.measure", skm)):
        assert name not in sys.modules, name + " is installed: use it"
        sys.modules[name] = mod
    if not hasattr(Image, "ANTIALIAS"):
        Image.ANTIALIAS = Image.LANCZOS
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import dataLoader
    return dataLoader


def run_image(D, tmp, tag, s, phase, isLight, eh, ew, R, C, seed):
    """one sample through BatchLoader.__getitem__ -> (batchDict, u)"""
    H, W = s["seg"].shape[:2]
    p = lambda kind, ext: os.path.join(tmp, f"{kind}_{tag}.{ext}")
    for kind in ("seg", "albedo", "normal", "rough"):
        Image.fromarray(s[kind]).save(p(kind, "png"))
        assert np.array_equal(np.asarray(Image.open(p(kind, "png"))), s[kind])
    open(p("im", "hdr"), "wb").close()      # loadHdr asks that the file exists; its pixels come from the stand-in imread
    _ARRAYS[p("im", "hdr")] = s["im"]
    with open(p("depth", "dat"), "wb") as f:
        f.write(struct.pack("i", H) + struct.pack("i", W) + s["depth"].astype(np.float32).tobytes())
    if s["envmapsInd"]:
        open(p("imenv", "hdr"), "wb").close()
        _ARRAYS[p("imenv", "hdr")] = s["envmaps"]
    L = D.BatchLoader.__new__(D.BatchLoader)
    L.imHeight, L.imWidth, L.phase, L.cascadeLevel, L.isLight, L.isAllLight = H, W, phase, 0, isLight, False
    L.envWidth, L.envHeight, L.envRow, L.envCol, L.SGNum = ew, eh, R, C, 12
    L.imList, L.segList, L.albedoList, L.normalList = [p("im", "hdr")], [p("seg", "png")], [p("albedo", "png")], [p("normal", "png")]
    L.roughList, L.depthList, L.envList = [p("rough", "png")], [p("depth", "dat")], [p("imenv", "hdr")]
    L.count, L.perm = 1, [0]
    np.random.seed(seed)
    u = np.random.random()
    np.random.seed(seed)
    out = L[0]
    return out, (u if phase == "TRAIN" else np.nan)


def sample(rng, H, W, R, C, ind=1):
    q = lambda *sh: rng.integers(0, 256, sh, dtype=np.uint8)
    # the mask: blobs of object (255), environment (0) and the area-light code (127 / 128), a few in-between codes
    coarse = rng.choice(np.array([255, 255, 255, 0, 127, 128, 60, 230], np.uint8), ((H + 3) // 4, (W + 3) // 4))
    seg1 = np.kron(coarse, np.ones((4, 4), np.uint8))[:H, :W]
    holes = rng.random((H, W)) < 0.03
    seg1 = np.where(holes, q(H, W), seg1).astype(np.uint8)
    seg = np.stack([seg1, q(H, W), q(H, W)], -1)      # channels 1 and 2 must not matter
    im = (rng.random((H, W, 3)) ** 3 * 6.0).astype(np.float16).astype(np.float32)
    env = (rng.random((R * 16, C * 32, 3)) ** 2 * 8.0).astype(np.float16).astype(np.float32)
    return dict(seg=seg, im=im, albedo=q(H, W, 3), normal=q(H, W, 3), rough=q(H, W, 3), depth=(0.5 + 4 * rng.random((H, W))).astype(np.float32), envmaps=env,
                envmapsInd=ind)


def finish(D, name, samples, phase, eh, ew, R, C, seed, expect=None, isLight=True):
    keys = KEYS if isLight else KEYS[:-2]
    with tempfile.TemporaryDirectory() as tmp:
        runs = [run_image(D, tmp, f"{name}{i}", s, phase, isLight, eh, ew, R, C, seed + i) for i, s in enumerate(samples)]
    outs, us = [r[0] for r in runs], np.array([r[1] for r in runs], np.float64)
    H, W = samples[0]["seg"].shape[:2]
    raw = {k: np.stack([s[k] for s in samples]) for k in ("seg", "im", "albedo", "normal", "rough", "depth", "envmaps")}
    raw["envmapsInd"] = np.array([s["envmapsInd"] for s in samples], np.float32)
    blob = {"raw_" + k: v for k, v in raw.items()}
    blob["raw_envmaps"] = raw["envmaps"].astype(np.float16)
    assert np.array_equal(blob["raw_envmaps"].astype(np.float32), raw["envmaps"])
    for k in keys:
        blob["ref_" + k] = np.stack([np.asarray(o[k], np.float32) for o in outs])
        assert all(np.asarray(o[k]).dtype == np.float32 for o in outs), (k, [np.asarray(o[k]).dtype for o in outs])
    # v: the reference's own expression (scaleHdr :252-255) on the reference's own loadHdr layout and seg
    kk = int(0.95 * W * H * 3)
    v = []
    for s in samples:
        hdr = np.transpose(s["im"], [2, 0, 1])[::-1]
        seg = 0.5 * ((np.transpose(s["seg"].astype(np.float32), [2, 0, 1]) - 127.5) / 127.5 + 1)[0:1]
        arr = (hdr * seg).flatten()
        arr.sort()
        v.append(arr[kk])
    v = np.array(v, np.float32)
    u_arg = None if phase == "TEST" else us
    scale = K.numerator(u_arg, len(samples)) / np.maximum(v, np.float32(0.1))
    blob["v"], blob["u"], blob["scale"] = v, us, scale.astype(np.float32)
    im_again = np.clip(scale[:, None, None, None] * np.transpose(raw["im"], [0, 3, 1, 2])[:, ::-1], 0, 1)
    assert np.array_equal(im_again, blob["ref_im"]), name + ": v / u do not reproduce the reference's im"
    c64 = K.prepare_batch(raw, phase, isLight, u_arg, eh, ew, np.float64)
    for k in keys:
        blob["e_ref_" + k] = np.float64(K.rel(blob["ref_" + k], c64[k]))
    blob["cfg"] = np.array([len(samples), H, W, R, C, eh, ew, kk, int(isLight)], np.int64)
    blob["phase"], blob["notes"] = np.array(phase), np.array(NOTES)
    if expect:
        expect(blob)
    path = os.path.join(OUT, f"g25_loader_{name}.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name:8s} {size / 1024:7.1f} KiB  v {v}  scale {np.round(scale, 4)}  e_ref " + " ".join(f"{k}={float(blob['e_ref_' + k]):.1e}" for k in keys))


def main():
    D = reference()
    rng = lambda s: np.random.default_rng(s)

    # a single pixel.  isLight=False: with isLight the reference's `segObj.squeeze()` (:126) leaves no 2-D array for the erosion of a plane that
    # is one pixel high or wide and raises, so such planes have no reference result for the eroded mask or the env maps
    finish(D, "tiny", [sample(rng(2501), 1, 1, 1, 1)], "TRAIN", 8, 16, 1, 1, 100, isLight=False)
    # a single cell
    finish(D, "cell", [sample(rng(2505), 6, 10, 1, 1)], "TRAIN", 8, 16, 1, 1, 150)

    # a batch of three with distinct scales: an ordinary image; one whose 95 % point is a masked zero (the 0.1 floor is live); one without env map
    r = rng(2502)
    a, b, c = sample(r, 5, 7, 3, 5), sample(r, 5, 7, 3, 5), sample(r, 5, 7, 3, 5, ind=0)
    a["seg"][..., 0] = np.where(a["seg"][..., 0] < 100, 255, a["seg"][..., 0])      # mostly object: v is a bright sample
    b["seg"][..., 0] = 0
    b["seg"][0, 0, 0] = 255      # 3 of 105 products are not zero; k = 99

    def expect_odd(z):
        assert z["v"][0] > 0.1 and z["v"][1] == 0.0 and len(set(np.round(z["scale"], 5))) == 3, (z["v"], z["scale"])
        assert np.abs(z["ref_envmaps"][2]).max() == 0.0 and z["ref_envmapsInd"].reshape(-1).tolist() == [1.0, 1.0, 0.0]
    finish(D, "odd", [a, b, c], "TRAIN", 8, 16, 3, 5, 200, expect_odd)

    # a wide grid (more cells in a row than a workgroup takes, not a multiple of it): an image of one repeated value, one with negative samples
    r = rng(2503)
    a, b = sample(r, 6, 10, 2, 40), sample(r, 6, 10, 2, 40)
    a["im"][:] = np.float32(0.75)
    a["seg"][..., 0] = 255
    b["im"] -= np.float32(1.5)
    b["seg"][..., 0] = np.where(b["seg"][..., 0] < 100, 255, b["seg"][..., 0])

    def expect_wide(z):
        assert z["v"][0] == np.float32(0.75) and (z["raw_im"][1] < 0).mean() > 0.3 and z["v"][1] > 0.1, z["v"]
        assert z["ref_im"][1].min() == 0.0
    finish(D, "wide", [a, b], "TRAIN", 8, 16, 2, 40, 300, expect_wide)

    # the TEST rule, ratio 1 (BASELINE config 5 keeps 16 x 32), a plane that is odd both ways and spans several rows of mask tiles
    finish(D, "ratio1", [sample(rng(2504), 30, 41, 3, 5)], "TEST", 16, 32, 3, 5, 400, lambda z: None)


if __name__ == "__main__":
    main()
