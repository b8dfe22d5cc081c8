"""Golden vectors for the bilateral solver layer, produced by the UNMODIFIED reference (BilateralGrid.py, BilateralLayer.py).
TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout and scipy); never runs on the GPU machine:

    python tools/make_golden_bilateral.py        # writes tests/golden/g13_bilateral_<case>.npz

The reference modules are imported where they lie; at run time only, (a) ``BilateralGrid.cg`` is rebound to a wrapper that maps
the removed ``tol=`` keyword of scipy's cg to ``rtol=`` with ``atol=0`` (and, for the yardstick run, casts the system and the
vectors to fp32), (b) ``BilateralLayer.BilateralFunction`` is rebound to a recorder so that the layer's guide and confidence can
be captured without ``.cuda()``.  ``torchvision`` (imported by BilateralLayer.py, unused) gets an empty stand-in if absent.

The contract pinned is ``BilateralGrid.solve`` / ``solveForGrad`` with the mode table's own parameters.
Per case the file holds the inputs, parameters, pixel->vertex index, nvertices, m, n, yhat, output, grad_pred, grad_conf (fp64 as
the reference produces them), ``e_ref_*`` = rel-L2 distance of the reference's fp32-cast solve from its fp64 one, ``margin`` = the
smallest distance of a scaled colour coordinate to an integer (a case below 1e-9 is refused: truncation must not hang on the
last bit), and the reference's CPU time on the authoring machine."""
from __future__ import annotations

import os
import sys
import time
import types

import numpy as np
import torch

REF = os.environ.get("SGR_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
MAX_BYTES = 1 << 20


def reference():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    for name in ("torchvision", "torchvision.transforms", "torchvision.datasets"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    import matplotlib
    matplotlib.use("Agg")
    import BilateralGrid as BG
    import BilateralLayer as BL
    return BG, BL


def install_cg(BG, fp32):
    from scipy.sparse.linalg import cg

    def wrapper(A, b, x0=None, M=None, maxiter=None, tol=1e-5):
        if fp32:
            x, info = cg(A.astype(np.float32), b.astype(np.float32), x0=x0.astype(np.float32), M=M.astype(np.float32), maxiter=maxiter, rtol=tol, atol=0)
            return x.astype(np.float64), info
        return cg(A, b, x0=x0, M=M, maxiter=maxiter, rtol=tol, atol=0)
    BG.cg = wrapper


def mode_params(BL, mode):
    layer = BL.BilateralLayer(mode=mode, isCuda=False)
    return dict(layer.grid_params), dict(layer.bs_params)


def synth_image(rng, H, W, noise=0.0015):
    """smooth colour field + an edge + a little noise, in [0.05, 0.95]: vertices are shared, unlike white noise"""
    y, x = np.mgrid[:H, :W]
    u, v = x / max(W - 1, 1), y / max(H - 1, 1)
    im = np.stack([0.45 + 0.25 * np.sin(2.1 * u + 0.7 * v + p) + 0.1 * np.cos(3.3 * v + p) for p in (0.3, 1.1, 2.2)], -1)
    im[:, W // 2:, :] *= 0.6 + 0.3 * rng.random(3)
    im += 0.17 * (v[..., None] > 0.6) * np.array([0.3, -0.2, 0.5])
    im += noise * rng.standard_normal(im.shape)
    return np.clip(im, 0.05, 0.95).astype(np.float32)


def rel(a, b):
    d = np.linalg.norm(np.asarray(b, np.float64))
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / d) if d > 0 else float(np.abs(a).max())


def run_reference(BG, image, pred, conf, grad, gp, bp, fp32):
    install_cg(BG, fp32)
    t0 = time.perf_counter()
    grid = BG.BilateralGrid(image * 255.0, **gp)
    t1 = time.perf_counter()
    out, yhat = BG.solve(grid, pred, conf, bp, pred.shape)
    t2 = time.perf_counter()
    grid_b = BG.BilateralGrid(image * 255.0, **gp)           # the reference rebuilds the grid in backward
    g_pred, g_conf = BG.solveForGrad(grid_b, grad, conf, bp, pred.shape, yhat, pred)
    t3 = time.perf_counter()
    return grid, dict(out=out, yhat=yhat, grad_pred=g_pred, grad_conf=g_conf), (t1 - t0, t2 - t1, t3 - t2)


def one_image(BG, image, pred, conf, grad, gp, bp, need_shared=True):
    grid, r64, times = run_reference(BG, image, pred, conf, grad, gp, bp, False)
    _, r32, _ = run_reference(BG, image, pred, conf, grad, gp, bp, True)
    install_cg(BG, False)
    Dn, Dm = BG.bistochastize(grid)
    idx = grid.S.tocsc().indices.astype(np.int32).reshape(image.shape[:2])
    yuv = BG.rgb2yuv(image * 255.0)
    scaled = yuv / np.array([gp["sigma_luma"], gp["sigma_chroma"], gp["sigma_chroma"]])
    margin = float(np.abs(scaled - np.round(scaled)).min())
    if margin < 1e-9:
        raise SystemExit(f"refused: a scaled colour coordinate is {margin:.2e} from an integer")
    if need_shared and grid.nvertices >= 0.9 * image.shape[0] * image.shape[1]:
        raise SystemExit(f"refused: {grid.nvertices} vertices for {image.shape[0] * image.shape[1]} pixels (vertices must be shared)")
    d = dict(idx=idx, nvertices=np.int64(grid.nvertices), m=Dm.diagonal(), n=Dn.diagonal(), margin=margin, ref_cpu_seconds=np.array(times), **r64)
    for k in ("out", "grad_pred", "grad_conf"):
        d["e_ref_" + k] = rel(r32[k], r64[k])
    return d


def save(name, blob):
    path = os.path.join(OUT, f"g13_bilateral_{name}.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    e = {k: (float(np.max(v))) for k, v in blob.items() if k.startswith("e_ref_")}
    print(f"{name:12s} {size / 1024:7.1f} KiB  nvertices {np.ravel(blob['nvertices'])}  pixels {blob['image'].shape[-3] * blob['image'].shape[-2]}  margin {np.min(blob['margin']):.2e}  "
          f"e_ref {e}  ref cpu s (grid, solve, backward) {np.round(np.reshape(blob['ref_cpu_seconds'], (-1, 3)).sum(0), 4)}")


def solver_case(BG, BL, name, mode, C, H, W, seed, B=1, const_channel=False, zero_conf=False, need_shared=True):
    rng = np.random.default_rng(seed)
    gp, bp = mode_params(BL, mode)
    per = []
    ins = dict(image=[], pred=[], conf=[], grad=[])
    for _ in range(B):
        image = synth_image(rng, H, W)
        base = image.mean(-1, keepdims=True) if C == 1 else image
        pred = np.clip(base + 0.05 * rng.standard_normal((H, W, C)), 0, 1).astype(np.float32)
        if const_channel:
            pred[..., 1] = np.float32(0.375)
        conf = (np.zeros((H, W)) if zero_conf else 0.05 + 0.95 * rng.random((H, W))).astype(np.float32)
        grad = rng.standard_normal((H, W, C)).astype(np.float32)
        per.append(one_image(BG, image, pred, conf, grad, gp, bp, need_shared))
        for k, v in zip(("image", "pred", "conf", "grad"), (image, pred, conf, grad)):
            ins[k].append(v)
    blob = {k: np.stack(v) for k, v in ins.items()}                       # [B,H,W,(C)] -- the reference's HWC layout
    for k in per[0]:
        blob[k] = np.stack([np.asarray(p[k]) for p in per]) if k not in ("m", "n", "yhat") else np.concatenate([np.ravel(p[k]) for p in per])
    blob["mode"] = np.int64(mode)
    blob["params"] = np.array([gp["sigma_luma"], gp["sigma_chroma"], gp["sigma_spatial"], bp["lam"], bp["A_diag_min"], bp["cg_tol"], bp["cg_maxiter"]], np.float64)
    save(name, blob)


def layer_case(BG, BL, name, mode, C, B, H, W, seed):
    rec = {}

    class Recorder:
        @staticmethod
        def apply(guide, pred, conf, grid_arr, bs_arr):
            rec.update(guide=guide.detach().numpy().copy(), conf=conf.detach().numpy().copy())
            return pred, conf
    BL.BilateralFunction = Recorder
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    layer = BL.BilateralLayer(mode=mode, isCuda=False)
    image = np.stack([synth_image(rng, H, W, noise=0.004) for _ in range(B)]).transpose(0, 3, 1, 2).copy()
    feature = np.stack([synth_image(rng, H, W) for _ in range(B)]).transpose(0, 3, 1, 2).copy()
    base = feature.mean(1, keepdims=True) if C == 1 else feature
    pred = np.clip(base + 0.05 * rng.standard_normal((B, C, H, W)), 0, 1).astype(np.float32)
    grad = rng.standard_normal((B, C, H, W)).astype(np.float32)
    with torch.no_grad():
        layer(torch.from_numpy(image), torch.from_numpy(feature), torch.from_numpy(pred))
    gp, bp = dict(layer.grid_params), dict(layer.bs_params)
    per = [one_image(BG, rec["guide"][b].transpose(1, 2, 0).copy(), pred[b].transpose(1, 2, 0).copy(), rec["conf"][b, 0], grad[b].transpose(1, 2, 0).copy(), gp, bp)
           for b in range(B)]
    blob = dict(image=image, feature=feature, pred=pred, grad=grad, guide=rec["guide"], conf=rec["conf"], mode=np.int64(mode))
    for k in ("idx", "nvertices", "out", "grad_pred", "grad_conf", "margin", "ref_cpu_seconds", "e_ref_out", "e_ref_grad_pred", "e_ref_grad_conf"):
        blob[k] = np.stack([np.asarray(p[k]) for p in per])
    sd = layer.state_dict()
    blob["state_keys"] = np.array(list(sd.keys()))
    for k, v in sd.items():
        blob["w_" + k] = v.numpy()
    save(name, blob)


def main():
    if not os.path.isfile(os.path.join(REF, "BilateralGrid.py")):
        raise SystemExit("reference not mounted")
    BG, BL = reference()
    for mode, seed in ((0, 1), (2, 2), (4, 3)):
        solver_case(BG, BL, f"m{mode}c3", mode, 3, 48, 64, 100 + seed)
        solver_case(BG, BL, f"m{mode}c1", mode, 1, 48, 64, 200 + seed)
    solver_case(BG, BL, "m1wide", 1, 3, 6, 136, 301, need_shared=False)      # x / 0.5 passes 255: colliding hashes
    solver_case(BG, BL, "batch3", 0, 3, 40, 56, 302, B=3)
    solver_case(BG, BL, "constch", 0, 3, 48, 64, 303, const_channel=True)
    solver_case(BG, BL, "zeroconf", 2, 1, 48, 64, 304, zero_conf=True)
    solver_case(BG, BL, "120x160", 2, 1, 120, 160, 305)
    layer_case(BG, BL, "layer", 0, 3, 2, 32, 48, 306)


if __name__ == "__main__":
    main()
