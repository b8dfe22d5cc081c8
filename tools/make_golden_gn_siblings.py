"""Golden vectors for the sibling forms of the decoders' upcat stage, produced by the UNMODIFIED reference
(models.decoder0, models.decoderLight).  TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout,
oracle/ref_import.py); never runs on the GPU machine:

    python tools/make_golden_gn_siblings.py        # writes tests/golden/g23_gnsib_{brdf,light}.npz

The reference never runs one decoder alone: wrapperBRDF.py:104-107 calls four ``decoder0`` instances (modes 0, 1, 2, 4) and
wrapperBRDFLight.py:104-115 three ``decoderLight`` instances (modes 0, 1, 2) on the same encoder features.  Here ``D`` such instances are driven
at ONE stage with the hook trick of tools/make_golden_gn_stage.py -- a forward hook on ``dconvK`` RETURNS sibling ``d``'s leaf ``x``,
``dgnK.weight`` / ``bias`` are set to stored values, a forward pre-hook on ``dconv{K+1}`` captures its input -- and every instance receives
the SAME skip leaf, as the wrappers pass the same ``x1..x6``.  One ``backward`` of ``sum_d <y_d, ct_d>`` then leaves in ``skip.grad`` what the
reference's own autograd accumulated over the siblings.  Every run is repeated in fp64.

  brdf    4 x decoder0 (modes 0, 1, 2, 4), stage 5, 2 x 64 x 3 x 5 with the skip [2,64,3,5]: the same-size form
  light   3 x decoderLight (modes 0, 1, 2), stage 5, 2 x 128 x 2 x 2 with the skip [2,128,3,3]: the reference's resize fires on both axes

Per file: ``D, G, skip``, the accumulated ``ds32 / ds64 / e_ref_ds`` and per sibling ``s<d>_x, _weight, _bias, _ct, _y32, _y64, _dx32 .. _db64,
_e_ref_{y,dx,dw,db}`` (``e_ref``: the rel-L2 distance between the reference's two runs).  Sibling 1's input is ``100 + N(0,1)``, so statistics
swapped between siblings cannot pass; every sibling's scales have negative entries and one exact zero; the cotangents differ.  The
conditions of make_golden_gn_stage.py hold per sibling (asserted): no ReLU argument within 1e-5 of zero, 30-70 % positive, one zero pattern
of dx in both runs, nothing NaN.  The plane sizes are what keeps a file with its fp64 arrays under the 1 MiB cap."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_gn_stage as G17      # noqa: E402  (puts ROOT and tests/ on the path; draw, rel, the decoders' channel tables)
from oracle import ref_import as RI     # noqa: E402

MODES = {"decoder0": (0, 1, 2, 4), "decoderLight": (0, 1, 2)}


def run(M, cls, stage, ps, skip_np, dtype):
    """D unmodified decoders at `stage` on one skip leaf -> ([y_d], [(dx_d, dw_d, db_d)], skip.grad)"""
    skip = torch.from_numpy(skip_np).to(dtype).requires_grad_(True)
    ys, leaves, gns = [], [], []
    for d, (mode, p) in enumerate(zip(MODES[cls], ps)):
        torch.manual_seed(2300 + d)
        dec = (M.decoder0(mode=mode) if cls == "decoder0" else M.decoderLight(SGNum=12, mode=mode)).to(dtype)
        gn = getattr(dec, f"dgn{stage}")
        with torch.no_grad():
            gn.weight.copy_(torch.from_numpy(p["weight"]).to(dtype))
            gn.bias.copy_(torch.from_numpy(p["bias"]).to(dtype))
        assert gn.num_groups == p["G"] and gn.num_channels == p["x"].shape[1] and gn.eps == 1e-5
        leaf = torch.from_numpy(p["x"]).to(dtype).requires_grad_(True)
        B = leaf.shape[0]
        feats = [torch.zeros(B, c, 1, 1, dtype=dtype) for c in G17.FEATURE_CH[cls]]
        feats[G17.SKIP_OF[stage] - 1] = skip
        got = []

        def stop(m, i):
            got.append(i[0])
            raise G17.Captured
        h1 = getattr(dec, f"dconv{stage}").register_forward_hook(lambda m, i, o, leaf=leaf: leaf)
        h2 = getattr(dec, f"dconv{stage + 1}").register_forward_pre_hook(stop)
        try:
            dec(torch.zeros(B, 3, 2, 2, dtype=dtype), *feats) if cls == "decoder0" else dec(*feats, env=torch.zeros(B, 1, 2, 2, dtype=dtype))
        except G17.Captured:
            pass
        h1.remove()
        h2.remove()
        y, = got
        assert y.dtype == dtype and tuple(y.shape) == (B, leaf.shape[1] + skip.shape[1], 2 * skip.shape[2], 2 * skip.shape[3]), y.shape
        ys.append(y)
        leaves.append(leaf)
        gns.append(gn)
    total = sum((y * torch.from_numpy(p["ct"]).to(dtype)).sum() for y, p in zip(ys, ps))
    total.backward()      # the reference's autograd adds the siblings' contributions into skip.grad
    return ([y.detach().numpy() for y in ys], [(l.grad.numpy(), g.weight.grad.numpy(), g.bias.grad.numpy()) for l, g in zip(leaves, gns)], skip.grad.numpy())


def case(M, name, cls, stage, B, C, G, H, W, Hs, Ws, Cs, seed):
    rng = np.random.default_rng(seed)
    D = len(MODES[cls])
    ps = []
    for d in range(D):
        p = G17.draw(rng, B, C, G, H, W, Cs=0, offset=100.0 if d == 1 else 0.0)
        p["ct"] = (rng.integers(-8, 9, (B, C + Cs, 2 * Hs, 2 * Ws)) / 4.0).astype(np.float32)
        assert (p["weight"] < 0).any() and (p["weight"] == 0).sum() == 1
        ps.append(p)
    skip = (rng.integers(-32, 33, (B, Cs, Hs, Ws)) / 16.0).astype(np.float32)
    y64, g64, ds64 = run(M, cls, stage, ps, skip, torch.float64)
    y32, g32, ds32 = run(M, cls, stage, ps, skip, torch.float32)
    blob = dict(D=np.int64(D), G=np.int64(G), skip=skip, ds32=ds32, ds64=ds64, e_ref_ds=np.float64(G17.rel(ds32, ds64)))
    for d, p in enumerate(ps):
        pre, _, _ = G17.C_pre(p["x"], p["weight"], p["bias"], G)
        share = float((pre > 0).mean())
        assert np.abs(pre).min() >= G17.MARGIN and 0.30 <= share <= 0.70, (name, d, np.abs(pre).min(), share)
        assert np.array_equal(g32[d][0] == 0, g64[d][0] == 0), (name, d, "zero pattern of dx")
        for k in ("x", "weight", "bias", "ct"):
            blob[f"s{d}_{k}"] = p[k]
        blob[f"s{d}_y32"], blob[f"s{d}_y64"], blob[f"s{d}_e_ref_y"] = y32[d], y64[d], np.float64(G17.rel(y32[d], y64[d]))
        for k, a, b in zip(("dx", "dw", "db"), g32[d], g64[d]):
            blob[f"s{d}_{k}32"], blob[f"s{d}_{k}64"], blob[f"s{d}_e_ref_{k}"] = a, b, np.float64(G17.rel(a, b))
        print(f"  {name} sibling {d}: positive {share:.3f}  e_ref " + " ".join(f"{k} {float(blob[f's{d}_e_ref_{k}']):.1e}" for k in ("y", "dx", "dw", "db")))
    for a in blob.values():
        assert np.isfinite(np.asarray(a, np.float64)).all(), name
    print(f"  {name}: e_ref ds {float(blob['e_ref_ds']):.1e}")
    path = os.path.join(G17.OUT, f"g23_gnsib_{name}.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    assert size <= G17.MAX_BYTES, (name, size)
    print(f"{name}: {size / 1024:.1f} KiB")


def main():
    if not RI.available():
        raise SystemExit("reference not mounted")
    M = RI.models()
    case(M, "brdf", "decoder0", 5, 2, 64, 4, 3, 5, 3, 5, 64, 2301)
    case(M, "light", "decoderLight", 5, 2, 128, 8, 2, 2, 3, 3, 128, 2302)


if __name__ == "__main__":
    main()
