"""Makes tests/golden/g28_evalmetrics_*.npz by running the reference's OWN statements (needs the reference checkout; nothing of its text is
copied into the repository):

    [SGR_REFERENCE_ROOT=...] python tools/make_golden_eval_metrics.py

  compute_whdr    the FunctionDef of CompareWHDR.py, taken from the file's syntax tree at run time and compiled alone (the script's body would
                  read files); the reflectance is the image's bytes / 255.0 in fp32, as the script's line 86 forms it from the saved PNG
  CompareNormal   the body of the script's ``for`` loop, taken the same way.  The literal ``(640, 480)`` is replaced by the ground truth's
                  size so that small cases can run; the accumulators the body adds to are set to 0 and its prints are swallowed
  CompareDepth    the body of the script's ``for`` loop, unchanged

  cv2 is not installed here.  ``imread`` returns the arrays prepared for the case (BGR where the body reverses them), ``np.load`` the prediction.
  ``resize`` IS THE STAND-IN WRITTEN FROM OpenCV's INTER_LINEAR RULE FOR FLOAT DATA that tools/make_golden_export.py uses
  (tests/export_checker.py: resize_linear), in the array's own dtype: THE ONE PIECE OF ARITHMETIC NOT EXECUTED FROM THE REFERENCE'S OWN
  DEPENDENCY.  Every file says so in ``notes``.

Each file holds the inputs, the fp32 run as the scripts are (``ref_*``) and an fp64 run (``ref64_*``): the same statements with the inputs in
double and a namespace whose ``np.float32`` is ``np.float64``; ``e_*`` is the distance between the two, the reference's own fp32 error.  For
WHDR the weights are fp32-representable doubles, so the device's fp32 weights are the reference's."""
from __future__ import annotations

import ast
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SGR_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_metrics_checker as K      # noqa: E402
from export_checker import resize_linear      # noqa: E402

NOTES = ("made by tools/make_golden_eval_metrics.py with numpy %s from the reference's own statements: compute_whdr of CompareWHDR.py and the loop bodies of "
         "CompareNormal.py and CompareDepth.py, taken from the syntax trees at run time; (640, 480) in CompareNormal.py replaced by the ground truth's size; "
         "stand-ins: cv2.imread and np.load hand back the prepared arrays, cv2.resize = INTER_LINEAR for float data written from the rule "
         "(f = (float)((d + 0.5) * ((double)in / out) - 0.5), columns then rows, in the array's dtype) -- the one piece of arithmetic not executed from the "
         "reference's own dependency; the fp64 run: the same statements, inputs in double, np.float32 = np.float64" % np.__version__)


class NP:
    """numpy with ``load`` handing back the prepared prediction and, for the fp64 run, float32 = float64"""
    def __init__(self, loaded, double):
        self._loaded, self._double = loaded, double

    def __getattr__(self, name):
        if name == "load":
            return lambda path: self._loaded
        if name == "float32" and self._double:
            return np.float64
        return getattr(np, name)


def cv2_module(files):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1

    def resize(img, size, dst=None, interpolation=1):      # CompareNormal.py passes INTER_LINEAR in dst's place; the default is INTER_LINEAR
        assert interpolation == cv2.INTER_LINEAR and img.dtype in (np.float32, np.float64)
        nw, nh = size
        a = img[None] if img.ndim == 2 else img.transpose(2, 0, 1)
        r = resize_linear(np.ascontiguousarray(a), nh, nw)
        assert r.dtype == img.dtype
        return r[0] if img.ndim == 2 else np.ascontiguousarray(r.transpose(1, 2, 0))

    cv2.resize = resize
    cv2.imread = lambda path, flag=None: files[path]
    return cv2


def tree_of(script):
    path = os.path.join(REF, script)
    if not os.path.isfile(path):
        raise SystemExit("reference not mounted")
    return path, ast.parse(open(path).read())


def loop_body(script, size=None):
    path, tree = tree_of(script)
    loop = [n for n in tree.body if isinstance(n, ast.For)]
    assert len(loop) == 1
    body = loop[0].body
    if size is not None:
        class Size(ast.NodeTransformer):
            hits = 0

            def visit_Tuple(self, node):
                if [getattr(e, "value", None) for e in node.elts] == [640, 480]:
                    Size.hits += 1
                    return ast.copy_location(ast.Tuple(elts=[ast.Constant(size[0]), ast.Constant(size[1])], ctx=ast.Load()), node)
                return node
        body = [Size().visit(n) for n in body]
        assert Size.hits == 1
    return compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), path, "exec")


def run(code, ns):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        exec(code, ns)
    return ns


def save(name, **arrays):
    path = os.path.join(OUT, f"g28_evalmetrics_{name}.npz")
    np.savez_compressed(path, notes=np.array(NOTES), **arrays)
    assert os.path.getsize(path) < 200000, path
    print(name, os.path.getsize(path))


# ---- WHDR -----------------------------------------------------------------------------------------------------------------------------------

def compute_whdr_fn():
    path, tree = tree_of("CompareWHDR.py")
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "compute_whdr"]
    ns = dict(np=np)
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["compute_whdr"]


def whdr_case(name, im, point, weight, label, num):
    fn = compute_whdr_fn()
    B, H, W, _ = im.shape
    assert np.array_equal(weight[~np.isnan(weight)].astype(np.float64).astype(np.float32), weight[~np.isnan(weight)])
    out = {}
    for tag, dtype in (("ref", np.float32), ("ref64", np.float64)):
        res = np.full((B, 3), np.nan)
        for b in range(B):
            n = int(num[b])
            r = fn(K.reflectance_of(im[b], dtype), K.judgement_dict(point[b, :n], weight[b, :n], label[b, :n], H, W))
            if r is not None:
                res[b] = [float(v) for v in r]
        out[tag] = res
    chk = K.whdr(K.reflectance_of(im, np.float64), point, weight, label, num)
    with np.errstate(invalid="ignore"):
        e = np.abs(out["ref"] - out["ref64"])
    save("whdr_" + name, im_u8=im, point=point, weight=weight, label=label, num=num, ref_ratios=out["ref"], ref64_ratios=out["ref64"], e_ratios=e, sums64=chk["sums"])


def whdr_cases():
    im, point, weight, label, num = K.draw_whdr(3, 5, 7, 300, 2801, nums=[11, 0, 300])
    point[0, 1], point[0, 2] = point[0, 0], point[0, 0][[2, 3, 0, 1]]      # repeated pixels
    label[0, :3] = [0, 1, 2]
    assert K.whdr_margin_violations(im, point, weight, label, num) == 0
    whdr_case("mix", im, point, weight, label, num)
    im = np.random.default_rng(2802).integers(40, 256, (1, 4, 6, 3), dtype=np.uint8)
    im[0, 0, 0] = im[0, 0, 1] = 0      # two black pixels
    pairs = [(0, 0, 0, 1), (0, 0, 2, 3), (2, 3, 0, 1), (1, 1, 3, 5), (0, 1, 0, 0)]      # both black; first black; second black; neither; both black
    point = np.array([[p for p in pairs for _ in range(3)]], np.int32)
    label = np.array([[0, 1, 2] * len(pairs)], np.int32)
    weight = (np.arange(1, 16, dtype=np.float32) / 8)[None]
    num = np.array([15], np.int32)
    assert K.whdr_margin_violations(im, point, weight, label, num) == 0
    whdr_case("floor", im, point, weight, label, num)


# ---- normal angle ---------------------------------------------------------------------------------------------------------------------------

def normal_case(name, pred, gt, mask):
    B, H, W, _ = gt.shape
    code = loop_body("CompareNormal.py", (W, H))
    out = {k: [] for k in ("ref_theta", "ref64_theta", "ref_mean", "ref64_mean", "ref_median", "ref64_median", "count")}
    for b in range(B):
        for tag, dtype in (("ref", np.float32), ("ref64", np.float64)):
            files = {"gt/x.png": gt[b][:, :, ::-1], "mask/x.png": mask[b][:, :, ::-1]}
            ns = run(code, dict(np=NP(np.ascontiguousarray(pred[b].transpose(1, 2, 0)).astype(dtype), dtype == np.float64), cv2=cv2_module(files), normalName="pred/x_normal1.npy",
                                suffix="_normal1.npy", predRoot="pred/", gtRoot="gt/", maskRoot="mask/", thetaTotalMean=0, thetaTotalMedian=0, cnt=0))
            assert ns["theta"].dtype == dtype, ns["theta"].dtype
            out[tag + "_theta"].append(ns["theta"])
            out[tag + "_mean"].append(float(ns["thetaMean"]))
            out[tag + "_median"].append(float(ns["thetaMedian"]))
        out["count"].append(int(ns["mask"].sum()))
    arr = {k: np.asarray(v) for k, v in out.items()}
    with np.errstate(invalid="ignore"):
        save("normal_" + name, pred=pred, gt_u8=gt, mask_u8=mask, e_theta=np.array(K.rel_l2(arr["ref_theta"], arr["ref64_theta"])), e_mean=np.abs(arr["ref_mean"] - arr["ref64_mean"]),
             e_median=np.abs(arr["ref_median"] - arr["ref64_median"]), **arr)


def normal_cases():
    normal_case("id", *K.draw_normal(2, 6, 10, 6, 10, 2811))
    normal_case("up", *K.draw_normal(2, 3, 5, 6, 10, 2812))
    pred, gt, mask = K.draw_normal(2, 5, 7, 9, 12, 2813)
    m = (mask.min(axis=3) == 255)
    if m[0].sum() % 2 == m[1].sum() % 2:      # an even and an odd count
        y, x = np.argwhere(m[1])[0]
        mask[1, y, x] = 0
    normal_case("odd", pred, gt, mask)
    pred, gt, mask = K.draw_normal(1, 1, 1, 1, 1, 2814)
    mask[:] = 255
    normal_case("one", pred, gt, mask)
    # ties: four distinct ground-truth colours, the prediction constant -> four distinct angles, many times each; image 1: the prediction IS the
    # unit ground truth, so the dot product reaches 1 and beyond and the clip is live
    rng = np.random.default_rng(2815)
    colours = np.array([[255, 128, 128], [128, 255, 128], [128, 128, 255], [200, 200, 30]], np.uint8)
    gt = colours[rng.integers(0, 4, (2, 6, 10))]
    pred = np.zeros((2, 3, 6, 10), np.float32)
    pred[0, 2] = 1.0
    g = (gt[1].astype(np.float32) - np.float32(127.5)) / np.float32(127.5)
    pred[1] = (g / np.sqrt(np.sum(g * g, axis=2))[:, :, None]).transpose(2, 0, 1) * np.float32(1.0000005)
    mask = np.full((2, 6, 10, 3), 255, np.uint8)
    mask[0, 0, :3] = 254
    normal_case("ties", pred, gt, mask)
    pred, gt, mask = K.draw_normal(1, 3, 5, 6, 10, 2816)
    mask[mask == 255] = 254
    normal_case("none", pred, gt, mask)


# ---- log-depth RMSE -------------------------------------------------------------------------------------------------------------------------

def depth_case(name, pred, gt):
    code = loop_body("CompareDepth.py")
    out = {k: [] for k in ("ref_rmse", "ref64_rmse", "count")}
    for b in range(gt.shape[0]):
        for tag, dtype in (("ref", np.float32), ("ref64", np.float64)):
            ns = run(code, dict(np=NP(pred[b].astype(dtype), dtype == np.float64), cv2=cv2_module({"gt/x.tiff": gt[b].astype(dtype)}), depthName="pred/x_depthBS1.npy",
                                suffix="_depthBS1.npy", predRoot="pred/", gtRoot="gt/", errorAccu=0, cnt=0))
            assert np.asarray(ns["error"]).dtype == dtype
            out[tag + "_rmse"].append(float(np.sqrt(ns["error"])))
        out["count"].append(int(ns["mask"].sum()))
    arr = {k: np.asarray(v) for k, v in out.items()}
    with np.errstate(invalid="ignore"):
        save("depth_" + name, pred=pred, gt=gt, e_rmse=np.abs(arr["ref_rmse"] - arr["ref64_rmse"]), **arr)


def plain_depth(B, h, w, H, W, seed):
    rng = np.random.default_rng(seed)
    gt = (1.2 + 8.0 * rng.random((B, H, W))).astype(np.float32)
    gt[rng.random((B, H, W)) < 0.2] = np.float32(12.5)
    gt[rng.random((B, H, W)) < 0.1] = np.float32(0.6)
    return (0.3 + 11.7 * rng.random((B, h, w))).astype(np.float32), gt


def depth_cases():
    depth_case("id", *plain_depth(2, 6, 10, 6, 10, 2821))
    depth_case("up", *plain_depth(2, 3, 5, 6, 10, 2822))
    pred, gt = plain_depth(2, 6, 10, 6, 10, 2823)
    gt[0, 0, :4] = 0.0
    gt[1, 2, 3] = 0.0
    pred[0, 1, 1] = 0.0
    pred[1, 5, 9] = 0.0
    depth_case("zeros", pred, gt)
    pred, gt = plain_depth(1, 6, 10, 6, 10, 2824)
    gt[0, 0, :5], gt[0, 1, :5] = 1.0, 10.0
    depth_case("edge", pred, gt)
    pred, gt = plain_depth(1, 3, 5, 6, 10, 2825)
    gt[gt < 10] = 0.5
    depth_case("none", pred, gt)
    depth_case("one", np.array([[[2.5]]], np.float32), np.array([[[3.0]]], np.float32))


if __name__ == "__main__":
    whdr_cases()
    normal_cases()
    depth_cases()
