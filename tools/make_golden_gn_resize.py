"""Golden vectors for the decoders' resize-to-skip stage (GroupNorm + ReLU + bilinear resize to the skip + skip concat + 2x upsample, and the
final stage's resize to the image), produced by the UNMODIFIED reference (models.decoder0, models.decoderLight).  TEST INFRASTRUCTURE ONLY --
authoring container (needs the reference checkout, oracle/ref_import.py); never runs on the GPU machine:

    python tools/make_golden_gn_resize.py        # writes tests/golden/g19_gnresize_{h1,hw,dbl,one,fin}.npz

The hook trick of tools/make_golden_gn_stage.py: a forward hook on ``dconvK`` RETURNS a chosen leaf ``x``, ``dgnK.weight`` / ``bias`` are set to
stored values, and a forward pre-hook on ``dconv{K+1}`` captures its input.  Here the skip has another size than ``x``, so the reference's
``if dxK.size(3) != x.size(3) or ...`` fires and its own ``F.interpolate(dxK, [h, w], mode='bilinear')`` runs before the concatenation.  The
final-stage form hooks ``dconv6`` and captures ``dpadFinal``'s input, with ``im`` (decoder0) / ``env`` (decoderLight) of the target size.
Every run is repeated in fp64.

A file holds one or two parts (``parts``); per part ``<part>_x, _weight, _bias, _G, _size, _ct`` (and ``_skip``), the output ``_y32`` / ``_y64``,
the gradients ``_dx / _dw / _db / _ds`` as ``32`` and ``64`` and ``_e_ref_{y,dx,dw,db,ds}`` = the rel-L2 distance between the reference's two
runs.  Skip and cotangent are drawn from short dyadic grids, so the files compress.  The conditions of make_golden_gn_stage.py are asserted
(its ``finish``): no ReLU argument within 1e-5 of zero, 30-70 % positive, one zero pattern of dx in both runs, nothing NaN, negative scales
and one exact zero.  Every file came out under the 1 MiB cap at the batch sizes below; none had to be shrunk."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_gn_stage as G17      # noqa: E402  (puts ROOT and tests/ on the path; draw, finish, the decoders' channel tables)
from oracle import ref_import as RI     # noqa: E402


def make(M, cls, dtype):
    return (M.decoder0(mode=0) if cls == "decoder0" else M.decoderLight(SGNum=12, mode=0)).to(dtype)


def run(M, cls, stage, p, dtype):
    """the unmodified decoder with ``x`` returned from dconv<stage> -> (what the next layer reads, gradients at x, weight, bias[, skip])"""
    torch.manual_seed(1900 + stage)
    dec = make(M, cls, dtype)
    gn = getattr(dec, f"dgn{stage}")
    with torch.no_grad():
        gn.weight.copy_(torch.from_numpy(p["weight"]).to(dtype))
        gn.bias.copy_(torch.from_numpy(p["bias"]).to(dtype))
    assert gn.num_groups == p["G"] and gn.num_channels == p["x"].shape[1] and gn.eps == 1e-5
    leaf = torch.from_numpy(p["x"]).to(dtype).requires_grad_(True)
    B, Hs, Ws = leaf.shape[0], int(p["size"][0]), int(p["size"][1])
    feats = [torch.zeros(B, c, 1, 1, dtype=dtype) for c in G17.FEATURE_CH[cls]]
    skip = None
    if stage < 6:
        skip = torch.from_numpy(p["skip"]).to(dtype).requires_grad_(True)
        feats[G17.SKIP_OF[stage] - 1] = skip
    got = []

    def stop(m, i):
        got.append(i[0])
        raise G17.Captured
    h1 = getattr(dec, f"dconv{stage}").register_forward_hook(lambda m, i, o: leaf)
    h2 = (dec.dpadFinal if stage == 6 else getattr(dec, f"dconv{stage + 1}")).register_forward_pre_hook(stop)
    target = torch.zeros(B, 3, Hs, Ws, dtype=dtype) if stage == 6 else torch.zeros(B, 3, 2, 2, dtype=dtype)
    try:
        dec(target, *feats) if cls == "decoder0" else dec(*feats, env=target)
    except G17.Captured:
        pass
    h1.remove()
    h2.remove()
    y, = got
    want = (B, leaf.shape[1], Hs, Ws) if stage == 6 else (B, leaf.shape[1] + skip.shape[1], 2 * Hs, 2 * Ws)
    assert y.dtype == dtype and tuple(y.shape) == want and (Hs, Ws) != tuple(leaf.shape[2:]), y.shape      # the `if` fired
    wrt = [leaf, gn.weight, gn.bias] + ([skip] if skip is not None else [])
    g = torch.autograd.grad(y, wrt, grad_outputs=torch.from_numpy(p["ct"]).to(dtype))
    return y.detach().numpy(), [t.numpy() for t in g]


def draw(rng, B, C, G, H, W, Hs, Ws, Cs):
    p = G17.draw(rng, B, C, G, H, W, Cs=0)
    p["size"] = np.array([Hs, Ws], np.int64)
    if Cs:
        p["skip"] = (rng.integers(-32, 33, (B, Cs, Hs, Ws)) / 16.0).astype(np.float32)
        p["ct"] = (rng.integers(-8, 9, (B, C + Cs, 2 * Hs, 2 * Ws)) / 4.0).astype(np.float32)
    else:
        p["ct"] = (rng.integers(-8, 9, (B, C, Hs, Ws)) / 4.0).astype(np.float32)
    return p


def case(M, name, specs, seed):
    """specs: (part, cls, stage, B, C, G, H, W, Hs, Ws, Cs)"""
    rng = np.random.default_rng(seed)
    blob, parts = {}, []
    for part, cls, stage, B, C, G, H, W, Hs, Ws, Cs in specs:
        p = draw(rng, B, C, G, H, W, Hs, Ws, Cs)
        y64, g64 = run(M, cls, stage, p, torch.float64)
        y32, g32 = run(M, cls, stage, p, torch.float32)
        blob.update(G17.finish(name, part, p, y32, g32, y64, g64))
        parts.append(part)
    blob["parts"] = np.array(parts)
    path = os.path.join(G17.OUT, f"g19_gnresize_{name}.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    assert size <= G17.MAX_BYTES, (name, size)
    print(f"{name}: {size / 1024:.1f} KiB")


def main():
    if not RI.available():
        raise SystemExit("reference not mounted")
    M = RI.models()
    case(M, "h1", [("s", "decoder0", 5, 2, 64, 4, 5, 8, 6, 8, 64)], 1901)
    case(M, "hw", [("s", "decoder0", 5, 3, 64, 4, 3, 5, 4, 6, 64)], 1902)
    case(M, "dbl", [("s", "decoder0", 5, 1, 64, 4, 2, 3, 4, 6, 64)], 1903)
    case(M, "one", [("w", "decoderLight", 5, 2, 128, 8, 1, 1, 1, 2, 128), ("hw", "decoderLight", 5, 2, 128, 8, 1, 1, 2, 2, 128)], 1904)
    case(M, "fin", [("d0", "decoder0", 6, 2, 64, 4, 6, 9, 7, 10, 0), ("dl", "decoderLight", 6, 2, 128, 8, 2, 4, 3, 4, 0)], 1905)


if __name__ == "__main__":
    main()
