"""numpy-only fp64 restatement of the bilateral solver's arithmetic contract: the 5-D bilateral grid of
BilateralGrid.py:43-104, its bistochastisation (:106-118), the forward solve (:126-153) and the backward solve (:155-191) with
scipy's preconditioned CG written out (``rtol = cg_tol, atol = 0``).  No scipy, so it runs anywhere; tests/test_bilateral_checker.py
pins it to reference-made fixtures (tests/golden/g13_bilateral*.npz), which is what lets the GPU tests use it on inputs made on
the spot.

Everything here is per image: ``image`` [H,W,3] fp32 in [0,1], ``pred`` [H,W,C], ``conf`` [H,W]."""
from __future__ import annotations

import numpy as np

RGB_TO_YUV = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]])
YUV_OFFSET = np.array([0.0, 128.0, 128.0])
MAX_VAL = 255
NDIM = 5

# BilateralLayer.py:137-190 -- mode: (sigma_luma, sigma_chroma, sigma_spatial, lam, A_diag_min, cg_tol, cg_maxiter)
MODES = {0: (8.0, 2.0, 7.0, 200.0, 1e-5, 1e-5, 12), 1: (0.5, 0.5, 0.5, 5.0, 1e-5, 1e-5, 10),
         2: (8.0, 2.0, 8.0, 300.0, 1e-5, 1e-5, 10), 4: (4.0, 2.0, 4.0, 100.0, 1e-5, 1e-5, 10)}


def scaled_colour(image, sigma_luma, sigma_chroma):
    """[H,W,3] fp64 colour coordinates before truncation (Y / sigma_luma, U / sigma_chroma, V / sigma_chroma)."""
    im255 = np.asarray(image, np.float32) * np.float32(255.0)
    yuv = im255.astype(np.float64) @ RGB_TO_YUV.T + YUV_OFFSET
    return yuv / np.array([sigma_luma, sigma_chroma, sigma_chroma], np.float64)


class Grid:
    def __init__(self, image, sigma_luma, sigma_chroma, sigma_spatial):
        H, W = image.shape[:2]
        col = scaled_colour(image, sigma_luma, sigma_chroma)
        iy, ix = np.mgrid[:H, :W]
        coords = np.stack([(ix / float(sigma_spatial)).astype(np.int64), (iy / float(sigma_spatial)).astype(np.int64),
                           col[..., 0].astype(np.int64), col[..., 1].astype(np.int64), col[..., 2].astype(np.int64)], -1).reshape(-1, NDIM)
        hvec = MAX_VAL ** np.arange(NDIM, dtype=np.int64)
        hashes = coords @ hvec
        uniq, first, inv = np.unique(hashes, return_index=True, return_inverse=True)
        self.npixels, self.nvertices = H * W, len(uniq)
        self.idx = inv.reshape(-1).astype(np.int64)            # pixel -> vertex
        # a vertex takes the coordinates of its lowest-index pixel (np.unique's return_index), and its neighbour along +-d is the
        # vertex whose hash equals the hash of those coordinates +- 1 in d
        vcoords = coords[first]
        self.nbr = np.full((self.nvertices, 2 * NDIM), -1, np.int64)
        for d in range(NDIM):
            for k, off in enumerate((-1, 1)):
                nh = (vcoords @ hvec) + off * hvec[d]
                loc = np.clip(np.searchsorted(uniq, nh), 0, self.nvertices - 1)
                ok = uniq[loc] == nh
                self.nbr[ok, 2 * d + k] = loc[ok]

    def splat(self, x):
        x = np.asarray(x, np.float64)
        out = np.zeros((self.nvertices,) + x.shape[1:], np.float64)
        np.add.at(out, self.idx, x)
        return out

    def slice(self, y):
        return y[self.idx]

    def nbr_sum(self, y):
        out = np.zeros_like(y)
        for k in range(2 * NDIM):
            j = self.nbr[:, k]
            ok = j >= 0
            out[ok] = out[ok] + y[j[ok]]
        return out

    def blur(self, y):
        return 2 * NDIM * y + self.nbr_sum(y)

    def bistochastize(self, sweeps=10):
        m = self.splat(np.ones(self.npixels))
        n = np.ones(self.nvertices)
        for _ in range(sweeps):
            n = np.sqrt(n * m / self.blur(n))
        return n * self.blur(n), n


B_ZERO = -1      # pcg's record: the marker for a right-hand side of norm zero (no stop test is ever made)


def pcg(matvec, b, x0, minv, rtol, maxiter, record=None):
    """scipy.sparse.linalg.cg(A, b, x0, M=diag(minv), rtol=rtol, atol=0, maxiter=maxiter) for one right-hand side.

    ``record``, if a dict, receives ``stop``: the iteration at whose top the solve stopped (0..maxiter-1), ``maxiter`` if it never
    did, ``B_ZERO`` for ``|b| = 0``; and ``ratios``: ``|r| / atol`` at every stop test made, in order.  Recording reads the norm the
    stop test computes anyway and changes no arithmetic."""
    if record is not None:
        record["stop"], record["ratios"] = int(maxiter), []
    bn = np.linalg.norm(b)
    if bn == 0:
        if record is not None:
            record["stop"] = B_ZERO
        return b.copy()
    atol = rtol * bn
    x = x0.copy()
    r = b - matvec(x) if x.any() else b.copy()
    rho_prev, p = None, None
    for it in range(int(maxiter)):
        rn = np.linalg.norm(r)
        if record is not None:
            record["ratios"].append(float(rn / atol))
        if rn < atol:
            if record is not None:
                record["stop"] = it
            return x
        z = minv * r
        rho = np.dot(r, z)
        p = z.copy() if it == 0 else z + (rho / rho_prev) * p
        q = matvec(p)
        alpha = rho / np.dot(p, q)
        x += alpha * p
        r -= alpha * q
        rho_prev = rho
    return x


def stop_margin(records):
    """smallest |ln(|r| / atol)| over all stop tests of the recorded solves: how far the closest test was from going the other way
    (inf if no test was made)"""
    ratios = np.array([q for rec in records for q in rec["ratios"]], np.float64)
    if ratios.size == 0:
        return float("inf")
    with np.errstate(divide="ignore"):
        return float(np.abs(np.log(ratios)).min())


class Solver:
    def __init__(self, grid, lam, A_diag_min, cg_tol, cg_maxiter):
        self.g, self.lam, self.amin, self.tol, self.maxiter = grid, float(lam), float(A_diag_min), float(cg_tol), int(cg_maxiter)
        self.m, self.n = grid.bistochastize()

    def _system(self, w):
        g = self.g
        ws = g.splat(w)
        # A = lam (Dm - Dn blur(Dn)) + diag(ws) as the reference FORMS it (a sparse matrix, BilateralGrid.py:131-136): the diagonal
        # lam (m - 10 n^2) + ws is one number per vertex.  Applying m y - n blur(n y) term by term instead leaves a different
        # rounding residue where m = 10 n^2 (a vertex without neighbours, zero confidence), which the 1 / A_diag_min
        # preconditioner then amplifies -- 7e-3 on the zero-confidence fixture.
        diag = self.lam * (self.m - 2 * NDIM * self.n * self.n) + ws
        matvec = lambda y: diag * y - self.lam * self.n * g.nbr_sum(self.n * y)
        return ws, matvec, 1.0 / np.maximum(diag, self.amin)

    def _pcg_all(self, matvec, b, y0, minv, records):
        cols = []
        for c in range(b.shape[1]):
            rec = None
            if records is not None:
                rec = {}
                records.append(rec)
            cols.append(pcg(matvec, b[:, c], y0[:, c], minv, self.tol, self.maxiter, rec))
        return np.stack(cols, 1)

    def solve(self, pred, conf, records=None):
        t = np.asarray(pred, np.float64).reshape(self.g.npixels, -1)
        w = np.asarray(conf, np.float64).reshape(-1)
        ws, matvec, minv = self._system(w)
        b = self.g.splat(t * w[:, None])
        y0 = b / np.maximum(ws, 1e-10)[:, None]
        yhat = self._pcg_all(matvec, b, y0, minv, records)
        return self.g.slice(yhat), yhat

    def solve_grad(self, grad, conf, yhat, pred, records=None):
        gr = np.asarray(grad, np.float64).reshape(self.g.npixels, -1)
        t = np.asarray(pred, np.float64).reshape(self.g.npixels, -1)
        w = np.asarray(conf, np.float64).reshape(-1)
        ws, matvec, minv = self._system(w)
        b = self.g.splat(gr)
        y0 = b / self.g.splat(np.ones(self.g.npixels))[:, None]
        yb = self._pcg_all(matvec, b, y0, minv, records)
        s = self.g.slice(yb)
        return s * w[:, None], (self.g.slice(-yb * yhat) + s * t).sum(1)


def run_case(image, pred, conf, grad, params, record=True):
    """One image through forward and backward.  ``params`` = (sigma_luma, sigma_chroma, sigma_spatial, lam, A_diag_min, cg_tol, cg_maxiter).

    With ``record`` the result also has ``stops_fwd`` / ``stops_bwd`` (per channel: pcg's ``stop``) and ``margin`` (stop_margin over
    both solves); the other entries have the same bits either way."""
    sl, sc, ss, lam, amin, tol, mi = params
    H, W = image.shape[:2]
    g = Grid(image, sl, sc, ss)
    s = Solver(g, lam, amin, tol, mi)
    rf, rb = ([], []) if record else (None, None)
    out, yhat = s.solve(pred, conf, rf)
    gp, gc = s.solve_grad(grad, conf, yhat, pred, rb)
    C = out.shape[1]
    res = dict(idx=g.idx.reshape(H, W), nvertices=g.nvertices, m=s.m, n=s.n, yhat=yhat, nbr=g.nbr, out=out.reshape(H, W, C),
               grad_pred=gp.reshape(H, W, C), grad_conf=gc.reshape(H, W))
    if record:
        res.update(stops_fwd=np.array([r["stop"] for r in rf]), stops_bwd=np.array([r["stop"] for r in rb]), margin=stop_margin(rf + rb))
    return res


def run_batch(image, pred, conf, grad, params):
    """NCHW batch wrapper: image [B,3,H,W], pred/grad [B,C,H,W], conf [B,1,H,W] -> dict of stacked NCHW fp64 results; ``nbr`` and
    ``yhat`` ([nvertices,10] and [nvertices,C] per image) as lists, ``stops_fwd`` / ``stops_bwd`` [B,C], ``margin`` over the batch."""
    outs = [run_case(np.moveaxis(image[b], 0, -1), np.moveaxis(pred[b], 0, -1), conf[b, 0], np.moveaxis(grad[b], 0, -1), params)
            for b in range(image.shape[0])]
    return dict(idx=np.stack([o["idx"] for o in outs]), nvertices=np.array([o["nvertices"] for o in outs]),
                out=np.stack([np.moveaxis(o["out"], -1, 0) for o in outs]),
                grad_pred=np.stack([np.moveaxis(o["grad_pred"], -1, 0) for o in outs]),
                grad_conf=np.stack([o["grad_conf"] for o in outs])[:, None],
                stops_fwd=np.stack([o["stops_fwd"] for o in outs]), stops_bwd=np.stack([o["stops_bwd"] for o in outs]),
                margin=min(o["margin"] for o in outs), nbr=[o["nbr"] for o in outs], yhat=[o["yhat"] for o in outs])
