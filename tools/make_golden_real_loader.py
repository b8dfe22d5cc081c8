"""Golden vectors for the real-image loader operators, produced by the unmodified reference loaders (nyuDataLoader.py, iiwDataLoader.py).
TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout); never runs on the GPU machine:

    python tools/make_golden_real_loader.py        # writes tests/golden/g27_nyu_<case>.npz and g27_iiw_<case>.npz

Nothing of the reference is copied: its text is imported or parsed and executed where it lies.

  nyuDataLoader.py   imported with stand-in ``cv2`` and ``skimage`` modules.  ``NYULoader.__getitem__`` runs as it is, on an instance built without
                     its file lists (``object.__new__`` and the attributes ``__getitem__`` reads); the three image files and the depth file of a
                     sample are empty files in a temporary directory (``loadImage`` asks ``osp.isfile``) and ``cv2.imread`` serves the case's
                     arrays from memory by file name.  ``np.random.random`` is replaced by a recorded stream, stored as ``u`` ([bn,7]: scale, row,
                     column, flip, three colour values), chosen so that the reference's own arithmetic lands on the case's rectangle.
  the fp64 run       the same module text with every ``np.float32`` rewritten to ``np.float64`` on the syntax tree, at run time, and the depth
                     served as float64: the same statements in double.
  iiwDataLoader.py   cannot be imported on current numpy and PIL (``np.long``, ``Image.ANTIALIAS``): the statements of ``loadImage`` at lines 136-137
                     and 205-214 are taken from the syntax tree and executed as they lie, on an array standing for the resized image.
  cv2                is not installed here.  ``resize`` IS A STAND-IN WRITTEN FROM OpenCV's INTER_LINEAR RULE FOR FLOAT DATA
                     (tests/export_checker.py: resize_linear), in the array's own dtype: THE ONE PIECE OF ARITHMETIC NOT EXECUTED FROM THE
                     REFERENCE'S OWN DEPENDENCY.  Every file says so in ``notes``.

The reference ties the crop's height to its width, ``cropH = int(imHeight / imWidth * cropW)``, so a case names the width and gets the height.

Each NYU file holds the raw inputs (``im`` ``normal`` ``seg`` uint8 [bn,Hs,Ws,3] in cv2.imread's order, ``depth`` fp32), ``u``, ``cfg`` = (imHeight,
imWidth, imWidthMax, imWidthMin, TRAIN?), ``crop`` / ``flip`` / ``colour`` as the reference formed them, ``ref_<key>`` (the fp32 run), ``ref64_<key>``
(the fp64 run) and ``e_ref_<key>`` (the rel-L2 distance between the two).  Depths are drawn in [0.5, 12] and the fp32 run's segDepth must
equal the fp64 run's outside 1 % of the pixels at most (those within 1e-5 t of a threshold t)."""
from __future__ import annotations

import ast
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SGR_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20
NOTES = ("nyuDataLoader.NYULoader.__getitem__ run unmodified on an instance built without its file lists (numpy %s), np.random.random replaced by the "
         "recorded stream u; the fp64 run is the same text with np.float32 rewritten to np.float64; iiwDataLoader.loadImage lines 136-137 and 205-214 "
         "executed from the reference's text; stand-ins: cv2.imread serves the arrays from memory, skimage is empty, cv2.resize = INTER_LINEAR for "
         "float data written from the rule (f = (float)((d + 0.5) * ((double)in / out) - 0.5), columns then rows, in the array's dtype) -- the one "
         "piece of arithmetic not executed from the reference's own dependency" % np.__version__)

sys.path.insert(0, os.path.join(ROOT, "tests"))
import export_checker as E      # noqa: E402
import real_loader_checker as K      # noqa: E402

FILES = {}      # file name -> array, what cv2.imread serves


def cv2_module():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1

    def resize(img, size, interpolation=None):
        assert interpolation == cv2.INTER_LINEAR and img.dtype in (np.float32, np.float64)
        nw, nh = size
        a = img[None] if img.ndim == 2 else img.transpose(2, 0, 1)
        r = E.resize_linear(np.ascontiguousarray(a), nh, nw)
        assert r.dtype == img.dtype
        return r[0] if img.ndim == 2 else np.ascontiguousarray(r.transpose(1, 2, 0))

    def imread(name, flags=None):
        return FILES[name].copy()
    cv2.resize, cv2.imread = resize, imread
    return cv2


class _Double(ast.NodeTransformer):
    def visit_Attribute(self, node):
        self.generic_visit(node)
        if node.attr == "float32" and isinstance(node.value, ast.Name) and node.value.id == "np":
            node.attr = "float64"
        return node


def reference():
    """(the NYULoader class as it is, the same class in double, the statements of iiwDataLoader.loadImage in fp32 and in double)"""
    path = os.path.join(REF, "nyuDataLoader.py")
    if not os.path.isfile(path):
        raise SystemExit("reference not mounted")
    skimage, measure = types.ModuleType("skimage"), types.ModuleType("skimage.measure")
    measure.block_reduce = None
    skimage.measure = measure
    for name, mod in (("cv2", cv2_module()), ("skimage", skimage), ("skimage.measure", measure)):
        assert name not in sys.modules, name + " is installed: use it"
        sys.modules[name] = mod
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import nyuDataLoader
    ns = {"__name__": "nyuDataLoader_double"}
    exec(compile(ast.fix_missing_locations(_Double().visit(ast.parse(open(path).read()))), path, "exec"), ns)
    ipath = os.path.join(REF, "iiwDataLoader.py")
    fn = [n for n in ast.walk(ast.parse(open(ipath).read())) if isinstance(n, ast.FunctionDef) and n.name == "loadImage"]
    assert len(fn) == 1
    stmts = [s for s in fn[0].body if (136 <= s.lineno and s.end_lineno <= 137) or (205 <= s.lineno and s.end_lineno <= 214)]
    assert [s.lineno for s in stmts] == [136, 137, 205, 208, 209, 211, 213, 214], [s.lineno for s in stmts]
    comp = lambda body: compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), ipath, "exec")
    iiw32 = comp(stmts)
    iiw64 = comp([_Double().visit(s) for s in stmts])
    return nyuDataLoader.NYULoader, ns["NYULoader"], nyuDataLoader, ns, iiw32, iiw64


class Stream:
    """np.random.random from a recorded list"""
    def __init__(self, values):
        self.values, self.at = [float(v) for v in values], 0

    def __call__(self, size=None):
        n = 1 if size is None else int(size)
        got = self.values[self.at:self.at + n]
        assert len(got) == n, "the stream ran out"
        self.at += n
        return got[0] if size is None else np.array(got, np.float64)


def run_sample(cls, tmp, raw, b, cfg, u, depth_dtype):
    """NYULoader.__getitem__ for image b of the case -> the batchDict"""
    imH, imW, wmax, wmin, train = cfg
    names = {k: os.path.join(tmp, k, "s.png") for k in ("im", "normal", "seg")}
    names["depth"] = os.path.join(tmp, "depth", "s.tiff")
    for k, n in names.items():
        os.makedirs(os.path.dirname(n), exist_ok=True)
        open(n, "wb").close()
        FILES[n] = raw[k][b].astype(depth_dtype) if k == "depth" else raw[k][b]
    ld = object.__new__(cls)
    ld.imHeight, ld.imWidth, ld.imWidthMax, ld.imWidthMin, ld.phase = imH, imW, wmax, wmin, "TRAIN" if train else "TEST"
    ld.perm, ld.imList, ld.normalList, ld.segList, ld.depthList = [0, 0], [names["im"]] * 2, [names["normal"]] * 2, [names["seg"]] * 2, [names["depth"]] * 2
    stream = Stream(u)
    keep = np.random.random
    np.random.random = stream
    try:
        out = ld[1]      # index 1: index 0 reshuffles the (constant) permutation
    finally:
        np.random.random = keep
    assert stream.at == (7 if train else 0)
    return out


def u_for(rs, cs, cw, cfg, flip, colour_u):
    """the seven draws that make the reference's arithmetic land on (rs, cs) with a crop cw wide"""
    imH, imW, wmax, wmin, _ = cfg
    ch = int(float(imH) / float(imW) * cw)
    u0 = 0.0 if wmax == wmin else (cw - wmin) / (wmax - wmin)
    return [u0, (rs + 0.1) / (480 - ch) if rs else 0.0, (cs + 0.1) / (640 - cw) if cs else 0.0, 0.9 if flip else 0.1] + list(colour_u)


def nyu_case(classes, tmp, name, Hs, Ws, cfg, rects, seed, quarter_depth=False):
    """rects: per image (rs, cs, cropW, flip) in TRAIN, None in TEST"""
    cls32, cls64 = classes
    imH, imW, wmax, wmin, train = cfg
    bn = len(rects)
    raw = K.draw_raw(bn, Hs, Ws, seed)
    rng = np.random.default_rng(seed + 500)
    if quarter_depth:      # multiples of 0.25 with exactly 1.0 and 10.0 among them: segDepth must be equal everywhere
        raw["depth"] = (0.25 * rng.integers(2, 49, raw["depth"].shape)).astype(np.float32)
        raw["depth"].reshape(-1)[:4] = (1.0, 10.0, 0.75, 10.25)
    us = np.zeros((bn, 7))
    fix = dict(notes=np.array(NOTES), cfg=np.array([imH, imW, wmax, wmin, int(train)]), **raw)
    rows32, rows64 = [], []
    for b, rect in enumerate(rects):
        if train:
            us[b] = u_for(rect[0], rect[1], rect[2], cfg, rect[3], rng.random(3))
        rows32.append(run_sample(cls32, tmp, raw, b, cfg, us[b], np.float32))
        rows64.append(run_sample(cls64, tmp, raw, b, cfg, us[b], np.float64))
    if train:
        aug = [K.nyu_augmentation(us[b], imH, imW, wmax, wmin) for b in range(bn)]
        fix["u"], fix["crop"] = us, np.array([a[0] for a in aug], np.int32)
        fix["flip"], fix["colour"] = np.array([a[1] for a in aug]), np.stack([a[2] for a in aug])
        for b, rect in enumerate(rects):
            assert tuple(fix["crop"][b][[0, 1, 3]]) == rect[:3] and bool(fix["flip"][b]) == rect[3], (name, b, fix["crop"][b], rect)
            assert fix["crop"][b][0] + fix["crop"][b][2] <= Hs and fix["crop"][b][1] + fix["crop"][b][3] <= Ws, (name, b, fix["crop"][b])
    for k in K.NYU_KEYS:
        r32, r64 = np.stack([r[k] for r in rows32]), np.stack([r[k] for r in rows64])
        assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == (bn, 3 if k in ("normal", "im") else 1, imH, imW), (name, k, r32.dtype, r64.dtype, r32.shape)
        fix["ref_" + k], fix["ref64_" + k], fix["e_ref_" + k] = r32, r64, np.array(K.rel_l2(r32, r64))
    if quarter_depth:      # values that sit ON the thresholds, and no resize: nothing is left out
        assert np.array_equal(fix["ref_segDepth"], fix["ref64_segDepth"])
    else:
        K.check_seg_depth(fix["ref_segDepth"], fix["ref64_segDepth"], fix["ref64_depth"], name + ": the reference's fp32 run")
    return "nyu_" + name, fix


def iiw_case(codes, name, im_full, rs, cs, H, W):
    """im_full [bn,h,w,3] uint8 stands for the resized image; the crop (rs, cs, H, W) is the loader's"""
    outs = {}
    for tag, code, dt in (("ref", codes[0], np.float32), ("ref64", codes[1], np.float64)):
        rows = []
        for a in im_full:
            ns = dict(np=np, im=a, isGama=True, rs=rs, re=rs + H, cs=cs, ce=cs + W, self=types.SimpleNamespace(imHeight=H, imWidth=W))
            with np.errstate(invalid="ignore"):
                exec(code, ns)
            assert ns["im"].dtype == dt and ns["im"].shape == (3, H, W)
            rows.append(ns["im"])
        outs[tag] = np.stack(rows)
    fix = dict(notes=np.array(NOTES), im_full=im_full, crop=np.array([rs, cs, H, W]), im_u8=np.ascontiguousarray(im_full[:, rs:rs + H, cs:cs + W]), ref_im=outs["ref"],
               ref64_im=outs["ref64"])
    fix["e_ref_im"] = np.array(0.0 if np.isnan(outs["ref"]).all() else K.rel_l2(outs["ref"], outs["ref64"]))
    return "iiw_" + name, fix


def main():
    cls32, cls64, _, _, iiw32, iiw64 = reference()
    classes = (cls32, cls64)
    cases = []
    T, F = True, False
    with tempfile.TemporaryDirectory() as tmp:
        # (name, Hs, Ws, (imHeight, imWidth, imWidthMax, imWidthMin, TRAIN), [(rs, cs, cropW, flip)], seed)
        cases.append(nyu_case(classes, tmp, "tiny", 1, 1, (1, 1, 1, 1, T), [(0, 0, 1, F)], 2700))
        cases.append(nyu_case(classes, tmp, "up", 5, 7, (6, 8, 4, 4, T), [(1, 2, 4, T)], 2701))                      # crop 3 x 4 at (1, 2) -> 6 x 8
        cases.append(nyu_case(classes, tmp, "down", 11, 16, (5, 6, 13, 13, T), [(1, 2, 13, F)], 2702))                # crop 10 x 13 -> 5 x 6
        cases.append(nyu_case(classes, tmp, "corner", 9, 12, (6, 8, 8, 8, T), [(3, 4, 8, T)], 2703))                  # crop 6 x 8 ends at (9, 12): no resize
        cases.append(nyu_case(classes, tmp, "corner2", 9, 13, (4, 6, 10, 10, T), [(3, 3, 10, F)], 2704))              # crop 6 x 10 ends at (9, 13) -> 4 x 6
        cases.append(nyu_case(classes, tmp, "mixed", 12, 16, (6, 8, 14, 10, T), [(2, 3, 10, F), (0, 1, 12, T), (1, 0, 14, F)], 2705))
        cases.append(nyu_case(classes, tmp, "test", 6, 10, (6, 10, 600, 560, F), [None, None], 2706))
        cases.append(nyu_case(classes, tmp, "w1", 7, 3, (3, 1, 2, 2, T), [(1, 1, 2, T)], 2707))                       # crop 6 x 2 -> 3 x 1
        cases.append(nyu_case(classes, tmp, "w7", 8, 11, (5, 7, 9, 9, T), [(2, 1, 9, F), (0, 2, 9, T)], 2708))        # crop 6 x 9 -> 5 x 7: one group and a tail
        cases.append(nyu_case(classes, tmp, "ratio", 48, 64, (24, 32, 43, 43, T), [(9, 14, 43, F), (16, 21, 43, T)], 2709))      # crop 32 x 43 -> 24 x 32
        cases.append(nyu_case(classes, tmp, "quarter", 6, 8, (6, 8, 8, 8, T), [(0, 0, 8, F), (0, 0, 8, T)], 2710, quarter_depth=True))
    rng = np.random.default_rng(2720)
    cases.append(iiw_case((iiw32, iiw64), "tiny", rng.integers(1, 256, (1, 1, 1, 3), dtype=np.uint8), 0, 0, 1, 1))
    cases.append(iiw_case((iiw32, iiw64), "odd", rng.integers(0, 250, (2, 8, 9, 3), dtype=np.uint8), 2, 1, 5, 7))
    cases.append(iiw_case((iiw32, iiw64), "black", np.zeros((1, 4, 6, 3), np.uint8), 0, 1, 3, 4))
    os.makedirs(OUT, exist_ok=True)
    for name, fix in cases:
        path = os.path.join(OUT, f"g27_{name}.npz")
        np.savez_compressed(path, **fix)
        size = os.path.getsize(path)
        assert size < MAX_BYTES, (path, size)
        e = {k[6:]: float(v) for k, v in fix.items() if k.startswith("e_ref_")}
        print(f"{path}: {size} bytes; e_ref " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))


if __name__ == "__main__":
    main()
