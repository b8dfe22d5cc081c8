"""Golden vectors for the export operators, produced by the reference's own statements (testReal.py, utils.py).
TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout); never runs on the GPU machine:

    python tools/make_golden_export.py        # writes tests/golden/g26_export_<case>.npz

Nothing of the reference is copied: its text is parsed and executed where it lies.

  testReal.py   the ``Output Results`` block is a stretch of a long script, so it is taken at run time with ``ast``: the statements between
                lines 542 and 657 of the body that holds them, executed in a namespace with the prediction lists, ``opt``, ``nw``, ``nh`` and
                file names in a temporary directory -- once per image (the script handles one photograph), once with fp32 tensors and once
                with the same values as fp64 tensors.  The env ``.npz`` lines (626-631) run the same way on their own: line 633 asks for
                ``nrows=24``, which the small env grids here do not have.
  utils.py      imported with stand-in ``cv2`` / ``h5py`` modules.  ``writeImageToFile`` and ``writeEnvToFile`` run as they are; the former saves
                through PIL (installed) and the file is read back.
  instrumented  in both, every ``X.astype(np.uint8)`` is rewritten (on the syntax tree, at run time) to ``_rec(X).astype(np.uint8)``, where
                ``_rec`` notes ``X`` -- the value ``t`` the cast truncates -- and hands it back unchanged.
  cv2           is not installed here.  ``imwrite`` notes the array it is given.  ``resize`` IS A STAND-IN WRITTEN FROM OpenCV's INTER_LINEAR
                RULE FOR FLOAT DATA (tests/export_checker.py: resize_linear), in the array's own dtype: THE ONE PIECE OF ARITHMETIC NOT
                EXECUTED FROM THE REFERENCE'S OWN DEPENDENCY.  Every file says so in ``notes``.
  predToShading is outside these operators: the stand-in hands back the shading image prepared for the case.

  .squeeze()    drops every axis of size one, so a plane one pixel high or wide does not survive the block; for the ``tiny`` and ``row`` cases
                only, ``X.squeeze()`` is rewritten to drop the batch (and a single channel) axis alone, which is what it does otherwise.

``writeEnvToFile`` builds its mosaic in an fp32 array whatever it is given, so its fp64 ``t`` comes from tests/export_checker.py instead
(said in the env file's notes).

The inputs are drawn until at most 1 % of every kind's bytes lie within 1e-3 of an integer (few_near_an_integer: the input condition of the
byte bound; small cases end up with none).

Each file holds the inputs, ``ref_<kind>`` (the bytes of the fp32 run, in RGB order: where the reference hands ``[:, :, ::-1]`` to ``imwrite`` the
noted array is turned back), ``t64_<kind>`` (the fp64 run's ``t``; for the albedo the value the reference casts is ``np.clip(255 a, 0, 255)``) and ``e_t_<kind>`` (the largest ``|t_fp32 - t_fp64|`` of the reference's own runs)."""
from __future__ import annotations

import ast
import copy
import inspect
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SGR_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20
NOTES = ("testReal.py:542-657 and utils.writeImageToFile / writeEnvToFile executed from the reference's text (numpy %s, torch %s), X.astype(np.uint8) "
         "instrumented to note X; stand-ins: cv2.imwrite notes its array, predToShading hands back the prepared image, cv2.resize = INTER_LINEAR for "
         "float data written from the rule (f = (float)((d + 0.5) * ((double)in / out) - 0.5), columns then rows, in the array's dtype) -- the one "
         "piece of arithmetic not executed from the reference's own dependency" % (np.__version__, torch.__version__))
FLIPPED = ("albedo", "normal", "shading", "rendered")      # handed to imwrite as [:, :, ::-1]

sys.path.insert(0, os.path.join(ROOT, "tests"))
import export_checker as K      # noqa: E402

REC, WRITTEN = [], {}


def _rec(x):
    REC.append(np.array(x, copy=True))
    return x


class _Instrument(ast.NodeTransformer):
    def visit_Call(self, node):
        self.generic_visit(node)
        f = node.func
        if (isinstance(f, ast.Attribute) and f.attr == "astype" and len(node.args) == 1 and isinstance(node.args[0], ast.Attribute)
                and node.args[0].attr == "uint8"):
            f.value = ast.Call(func=ast.Name(id="_rec", ctx=ast.Load()), args=[f.value], keywords=[])
        return node


class _Squeeze(ast.NodeTransformer):
    """``X.squeeze()`` -> ``_squeeze(X)``: for the cases one pixel high or wide only (see _squeeze)"""
    def visit_Call(self, node):
        self.generic_visit(node)
        f = node.func
        if isinstance(f, ast.Attribute) and f.attr == "squeeze" and not node.args and not node.keywords:
            return ast.Call(func=ast.Name(id="_squeeze", ctx=ast.Load()), args=[f.value], keywords=[])
        return node


def _squeeze(a):
    """what ``a.squeeze()`` gives for a [1,C,h,w] prediction with h, w > 1 -- [C,h,w], or [h,w] for C == 1 -- also when h or w is 1"""
    assert a.ndim == 4 and a.shape[0] == 1
    return a.reshape(a.shape[1:] if a.shape[1] > 1 else a.shape[2:])


def cv2_module():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1

    def resize(img, size, interpolation=None):
        assert interpolation == cv2.INTER_LINEAR and img.dtype in (np.float32, np.float64)
        nw, nh = size
        a = img[None] if img.ndim == 2 else img.transpose(2, 0, 1)
        r = K.resize_linear(np.ascontiguousarray(a), nh, nw)
        assert r.dtype == img.dtype
        return r[0] if img.ndim == 2 else np.ascontiguousarray(r.transpose(1, 2, 0))

    def imwrite(name, arr):
        WRITTEN[name] = np.array(arr, copy=True)
        return True
    cv2.resize, cv2.imwrite = resize, imwrite
    return cv2


def reference():
    """(statements of the Output Results block, statements of the .npz lines, the instrumented utils namespace)"""
    if not os.path.isfile(os.path.join(REF, "testReal.py")):
        raise SystemExit("reference not mounted")
    cv2 = cv2_module()
    for name, mod in (("cv2", cv2), ("h5py", types.ModuleType("h5py"))):
        assert name not in sys.modules, name + " is installed: use it"
        sys.modules[name] = mod
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import utils
    uns = dict(vars(utils), _rec=_rec)
    for fn in ("writeImageToFile", "writeEnvToFile"):
        tree = _Instrument().visit(ast.parse(inspect.getsource(getattr(utils, fn))))
        exec(compile(ast.fix_missing_locations(tree), os.path.join(REF, "utils.py"), "exec"), uns)
    path = os.path.join(REF, "testReal.py")
    tree = ast.parse(open(path).read())
    body = None
    for node in ast.walk(tree):
        for field in ("body", "orelse"):
            stmts = getattr(node, field, None)
            if isinstance(stmts, list) and any(isinstance(s, ast.For) and s.lineno == 544 for s in stmts):
                body = stmts
    assert body is not None, "the Output Results block has moved"
    block = [s for s in body if s.lineno >= 542 and s.end_lineno <= 657]
    light = [s for s in block if isinstance(s, ast.If) and s.lineno == 623]
    assert len(light) == 1 and isinstance(light[0].body[0], ast.For) and light[0].body[0].lineno == 625
    env_for = light[0].body[0]
    npz = ast.For(target=env_for.target, iter=env_for.iter, body=[s for s in env_for.body if s.end_lineno <= 631], orelse=[])
    assert len(npz.body) == 3
    thin = [_Squeeze().visit(copy.deepcopy(s)) for s in block]      # before the block itself is instrumented in place
    compile_ = lambda stmts: compile(ast.fix_missing_locations(_Instrument().visit(ast.Module(body=stmts, type_ignores=[]))), path, "exec")
    return compile_(block), compile_(thin), compile_([npz]), uns, cv2


def run_block(code, cv2, tmp, x, scale, size, ttype):
    """the Output Results block for ONE image -> {kind: (t, bytes in RGB order)}"""
    nh, nw = size
    ten = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ttype)[None]
    p = lambda s: os.path.join(tmp, s)
    shading = x["shading"].astype(np.float64 if ttype == torch.float64 else np.float32)
    ns = dict(np=np, cv2=cv2, torch=torch, nw=nw, nh=nh, io=types.SimpleNamespace(), _rec=_rec, _squeeze=_squeeze,
              opt=types.SimpleNamespace(isBS=False, isLight=True, SGNum=12, level=1),
              utils=types.SimpleNamespace(predToShading=lambda pred, SGNum: shading),
              albedoPreds=[ten(x["albedo"])], cAlbedos=[] if scale is None else [np.float64(scale)], normalPreds=[ten(x["normal"])], roughPreds=[ten(x["rough"])],
              depthPreds=[ten(x["depth"])], renderedPreds=[ten(x["rendered"])], envmapsPreds=[torch.zeros(1, 1)], envmapsPredImages=[], cLights=[],
              albedoImNames=[p("albedo0.png")], normalNames=[p("normal0.npy")], normalImNames=[p("normal0.png")], roughImNames=[p("rough0.png")],
              depthNames=[p("depth0.npy")], depthImNames=[p("depth0.png")], envmapsPredSGNames=[p("envmapSG0.npy")], shadingNames=[p("shading0.png")],
              renderedImNames=[p("rendered0.png")], envmapPredImNames=[], cLightNames=[])
    del REC[:]
    WRITTEN.clear()
    exec(code, ns)
    order = ("albedo", "normal", "rough", "depth", "shading", "rendered")      # the order of the block's casts
    assert len(REC) == len(order) and len(WRITTEN) == len(order)
    out = {}
    for kind, t in zip(order, REC):
        b = WRITTEN[p(kind + "0.png")]
        t = t[..., None] if t.ndim == 2 else t
        b = b[..., None] if b.ndim == 2 else b
        b = b[..., ::-1] if kind in FLIPPED else b
        assert b.dtype == np.uint8 and b.shape == t.shape, (kind, b.shape, t.shape)
        out[kind] = (np.asarray(t, np.float64), np.ascontiguousarray(b))
    return out


def few_near_an_integer(t64_unclipped):
    """the input condition of the byte bound (tests/export_checker.py): at most 1 % of a case's bytes within delta of an integer"""
    return K.exempt_mask(t64_unclipped, K.DELTA_FLOOR).mean() <= K.EXEMPT_SHARE


def image_case(code, cv2, tmp, name, B, h, w, size, seed, with_scale):
    """the seed advances by 1000 until every kind of the case meets the input condition"""
    while True:
        name, fix, ok = image_case_once(code, cv2, tmp, name, B, h, w, size, seed, with_scale)
        if ok:
            fix["seed"] = np.array(seed)
            return name, fix
        seed += 1000


def image_case_once(code, cv2, tmp, name, B, h, w, size, seed, with_scale):
    rng = np.random.default_rng(seed)
    x = dict(albedo=(1.15 * rng.random((B, 3, h, w))).astype(np.float32), normal=(2 * rng.random((B, 3, h, w)) - 1).astype(np.float32),
             rough=(2 * rng.random((B, 1, h, w)) - 1).astype(np.float32), depth=K.draw("depth", B, 1, h, w, seed + 1),
             rendered=K.draw("rendered", B, 3, h, w, seed + 2), shading=K.draw("shading", B, 3, h, w, seed + 3))
    scale = (0.6 + 0.8 * rng.random(B)).astype(np.float32) if with_scale else None
    nh, nw = size if size is not None else (h, w)
    thin = h == 1 or w == 1
    code = code[1] if thin else code[0]
    fix = dict(notes=np.array(NOTES + ("; a plane one pixel high or wide loses that axis in the block's .squeeze(), so for this case .squeeze() is "
                                       "rewritten to drop the batch (and a single channel) axis alone" if thin else "")), size=np.array([nh, nw]), resized=np.array(size is not None))
    if scale is not None:
        fix["scale"] = scale
    for kind, v in x.items():
        fix["x_" + kind] = v
    runs = {tt: [run_block(code, cv2, tmp, {k: v[b] for k, v in x.items()}, None if scale is None else scale[b], (nh, nw), tt) for b in range(B)]
            for tt in (torch.float32, torch.float64)}
    for kind in x:
        t32 = np.stack([r[kind][0] for r in runs[torch.float32]])
        t64 = np.stack([r[kind][0] for r in runs[torch.float64]])
        fix["ref_" + kind] = np.stack([r[kind][1] for r in runs[torch.float32]])
        fix["t64_" + kind] = t64
        fix["e_t_" + kind] = np.array(np.abs(t32 - t64).max())
    ok = all(few_near_an_integer(K.image_t(v, kind, size if kind in K.RESIZED else None, scale if kind == "albedo" else None, clip=False)) for kind, v in x.items())
    return name, fix, ok


def image_writer(uns, tmp, x, gamma, dtype):
    """utils.writeImageToFile on a batch -> (t [B,h,w,3], bytes read back from the files)"""
    names = [os.path.join(tmp, f"im_{b}.png") for b in range(x.shape[0])]
    del REC[:]
    uns["writeImageToFile"](torch.from_numpy(x).to(dtype), names, isGama=gamma)
    t = np.stack([np.asarray(r, np.float64) for r in REC])
    t = np.concatenate([t, t, t], axis=3) if t.shape[3] == 1 else t
    got = np.stack([np.asarray(Image.open(n)) for n in names])
    assert got.shape == t.shape and got.dtype == np.uint8
    return t, got


def env_case(npz_code, uns, cv2, tmp):
    rng = np.random.default_rng(2604)
    fix = dict(notes=np.array(NOTES + "; writeEnvToFile builds its mosaic in an fp32 array whatever it is given, so t64_mosaic_* is "
                              "tests/export_checker.py's fp64 evaluation and e_t_mosaic_* the distance of the reference's fp32 t from it"))
    for tag, shape, nrows, ncols in (("a", (2, 3, 7, 9, 8, 16), 3, 4), ("b", (1, 3, 2, 2, 16, 32), 2, 1)):
        env = (1.25 * rng.random(shape) - 0.05).astype(np.float32)
        assert few_near_an_integer(K.env_mosaic_t(env, nrows, ncols, 1, clip=False))
        B, _, R, C, eh, ew = shape
        ts, bs, hwc = [], [], []
        for b in range(B):
            del REC[:]
            WRITTEN.clear()
            uns["writeEnvToFile"](torch.from_numpy(env), b, "mosaic", nrows=nrows, ncols=ncols, envHeight=eh, envWidth=ew, gap=1)
            assert len(REC) == 1
            ts.append(np.asarray(REC[0], np.float64))
            bs.append(np.ascontiguousarray(WRITTEN["mosaic"][..., ::-1]))
            name = os.path.join(tmp, f"env_{tag}{b}.npz")
            exec(npz_code, dict(np=np, _rec=_rec, envmapsPredImages=[torch.from_numpy(env[b:b + 1])], envmapPredImNames=[name]))
            hwc.append(np.load(name)["env"])
        t64 = K.env_mosaic_t(env, nrows, ncols, 1, dtype=np.float64)
        fix.update({f"env_{tag}": env, f"cfg_{tag}": np.array([nrows, ncols, 1]), f"ref_mosaic_{tag}": np.stack(bs), f"t64_mosaic_{tag}": t64,
                    f"e_t_mosaic_{tag}": np.array(np.abs(np.stack(ts) - t64).max()), f"ref_hwc_{tag}": np.stack(hwc)})
    return "env", fix


def main():
    block, thin, npz_code, uns, cv2 = reference()
    block = (block, thin)
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        cases.append(image_case(block, cv2, tmp, "tiny", 1, 1, 1, (3, 2), 2600, True))
        cases.append(image_case(block, cv2, tmp, "row", 1, 1, 7, (2, 11), 2601, False))
        cases.append(image_case(block, cv2, tmp, "odd", 3, 6, 10, (9, 13), 2602, True))
        cases.append(image_case(block, cv2, tmp, "down", 2, 9, 13, (6, 10), 2603, False))
        name, fix = image_case(block, cv2, tmp, "same", 2, 5, 7, None, 2605, False)
        rng = np.random.default_rng(2606)
        for C in (1, 3):
            x = (1.3 * rng.random((2, C, 5, 7)) - 0.15).astype(np.float32)
            while not (few_near_an_integer(K.image_t(x, "image", clip=False)) and few_near_an_integer(K.image_t(x, "image_gamma", clip=False))):
                x = (1.3 * rng.random((2, C, 5, 7)) - 0.15).astype(np.float32)
            fix[f"x_image{C}"] = x
            for gamma, kind in ((False, "image"), (True, "image_gamma")):
                t32, got = image_writer(uns, tmp, x, gamma, torch.float32)
                t64, _ = image_writer(uns, tmp, x, gamma, torch.float64)
                fix[f"ref_{kind}{C}"], fix[f"t64_{kind}{C}"], fix[f"e_t_{kind}{C}"] = got, t64, np.array(np.abs(t32 - t64).max())
        cases.append((name, fix))
        cases.append(env_case(npz_code, uns, cv2, tmp))
    os.makedirs(OUT, exist_ok=True)
    for name, fix in cases:
        path = os.path.join(OUT, f"g26_export_{name}.npz")
        np.savez_compressed(path, **fix)
        size = os.path.getsize(path)
        assert size < MAX_BYTES, (path, size)
        e = {k[4:]: float(v) for k, v in fix.items() if k.startswith("e_t_")}
        print(f"{path}: {size} bytes; e_t " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))


if __name__ == "__main__":
    main()
