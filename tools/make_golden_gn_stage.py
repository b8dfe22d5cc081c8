"""Golden vectors for the CNN stage glue (GroupNorm + ReLU + skip concat + 2x upsample), produced by the UNMODIFIED reference
(models.decoder0, models.decoderLight, models.encoder0).  TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout,
oracle/ref_import.py); never runs on the GPU machine:

    python tools/make_golden_gn_stage.py        # writes tests/golden/g17_gnstage_{dec,odd,one,row,enc,big}.npz

A decoder runs as it is on hand-sized feature maps.  A forward hook on ``dconvK`` RETURNS a chosen leaf ``x`` (fp32 values cast to the run's
dtype), ``dgnK.weight`` / ``bias`` are set to stored values (negative scales, one exact zero), and a forward pre-hook on ``dconv{K+1}``
captures its input: the reference's own ``F.interpolate(torch.cat([F.relu(dgnK(x)), skip], 1), scale_factor=2, mode='bilinear')``.  For the
plain form ``encoder0`` runs with the hook on ``convK`` and ``xK`` -- the ReLU's output -- is captured where ``pad{K+1}`` receives it (``x6``
is the forward's own return value).  Every run is repeated in fp64.

A file holds one or two parts (``parts``); per part ``<part>_x, _weight, _bias, _G, _ct`` (and ``_skip``), the output ``_y32`` / ``_y64``, the
gradients ``_dx / _dw / _db / _ds`` as ``32`` and ``64`` and ``_e_ref_{y,dx,dw,db,ds}`` = the rel-L2 distance between the reference's two
runs.  The cotangent and the skip are drawn from short dyadic grids (multiples of 1/4 and 1/16): they compress, which keeps the decoder
cases under the 1 MiB cap on a committed file, and the skip half of the result and ``dskip`` / ``dbias`` are exact in both precisions.

Conditions asserted here (tests/test_gn_stage.py re-asserts them from the stored arrays):
  * no pre-ReLU value is within 1e-5 of zero in fp64 -- offending elements of ``x`` are redrawn -- so a 1-ulp difference cannot flip a branch;
  * the zero pattern of ``dx32`` equals that of ``dx64``;
  * between 30 % and 70 % of the pre-ReLU values are positive;
  * nothing is NaN.

``big`` (``x = 100 + N(0,1)``: a one-pass fp32 ``E[x^2] - E[x]^2`` fails there) is the plain form at 1 x 64 x 16 x 23: a plane of 30 x 41
does not fit the cap with its fp64 arrays; tests/test_gpu_gn_stage.py runs that size against the checker instead."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_import as RI      # noqa: E402
import gn_stage_checker as C             # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20
MARGIN = 1e-5
SKIP_OF = {1: 5, 2: 4, 3: 3, 4: 2, 5: 1}      # decoder stage K concatenates x_{6-K}
FEATURE_CH = {"decoder0": (64, 128, 256, 256, 512, 1024), "decoderLight": (128, 256, 256, 512, 512, 1024)}


class Captured(Exception):
    pass


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.abs(a).max())


def run_decoder(M, cls, stage, p, dtype):
    """the unmodified decoder with ``x`` returned from dconv<stage> -> (dconv<stage+1>'s input, gradients at x, weight, bias, skip)"""
    torch.manual_seed(1700 + stage)
    dec = (M.decoder0(mode=0) if cls == "decoder0" else M.decoderLight(SGNum=12, mode=0)).to(dtype)
    gn = getattr(dec, f"dgn{stage}")
    with torch.no_grad():
        gn.weight.copy_(torch.from_numpy(p["weight"]).to(dtype))
        gn.bias.copy_(torch.from_numpy(p["bias"]).to(dtype))
    assert gn.num_groups == p["G"] and gn.num_channels == p["x"].shape[1] and gn.eps == 1e-5
    leaf = torch.from_numpy(p["x"]).to(dtype).requires_grad_(True)
    skip = torch.from_numpy(p["skip"]).to(dtype).requires_grad_(True)
    B = leaf.shape[0]
    feats = [torch.zeros(B, c, 1, 1, dtype=dtype) for c in FEATURE_CH[cls]]
    feats[SKIP_OF[stage] - 1] = skip
    got = []
    h1 = getattr(dec, f"dconv{stage}").register_forward_hook(lambda m, i, o: leaf)
    h2 = getattr(dec, f"dconv{stage + 1}").register_forward_pre_hook(lambda m, i: got.append(i[0]))
    if cls == "decoder0":
        dec(torch.zeros(B, 3, 2, 2, dtype=dtype), *feats)
    else:
        dec(*feats, env=torch.zeros(B, 1, 2, 2, dtype=dtype))
    h1.remove()
    h2.remove()
    y, = got
    assert y.dtype == dtype and tuple(y.shape) == (B, leaf.shape[1] + skip.shape[1], 2 * leaf.shape[2], 2 * leaf.shape[3]), y.shape
    g = torch.autograd.grad(y, [leaf, gn.weight, gn.bias, skip], grad_outputs=torch.from_numpy(p["ct"]).to(dtype))
    return y.detach().numpy(), [t.numpy() for t in g]


def run_encoder(M, k, p, dtype):
    """the unmodified encoder0 with ``x`` returned from conv<k> -> (x<k>, gradients at x, weight, bias)"""
    torch.manual_seed(1750 + k)
    enc = M.encoder0(cascadeLevel=0).to(dtype)
    gn = getattr(enc, f"gn{k}")
    with torch.no_grad():
        gn.weight.copy_(torch.from_numpy(p["weight"]).to(dtype))
        gn.bias.copy_(torch.from_numpy(p["bias"]).to(dtype))
    assert gn.num_groups == p["G"] and gn.num_channels == p["x"].shape[1] and gn.eps == 1e-5
    leaf = torch.from_numpy(p["x"]).to(dtype).requires_grad_(True)
    got = []
    hooks = [getattr(enc, f"conv{k}").register_forward_hook(lambda m, i, o: leaf)]
    if k < 6:
        def stop(m, i):
            got.append(i[0])
            raise Captured
        hooks.append(getattr(enc, f"pad{k + 1}").register_forward_pre_hook(stop))
    try:
        got.append(enc(torch.zeros(leaf.shape[0], 3, 64, 64, dtype=dtype))[5])
    except Captured:
        pass
    for h in hooks:
        h.remove()
    y = got[0]
    assert y.dtype == dtype and y.shape == leaf.shape
    g = torch.autograd.grad(y, [leaf, gn.weight, gn.bias], grad_outputs=torch.from_numpy(p["ct"]).to(dtype))
    return y.detach().numpy(), [t.numpy() for t in g]


def draw(rng, B, C, G, H, W, Cs, offset=0.0):
    """x = offset + N(0,1); scales N(0,1) with negative ones and one exact zero, biases 0.3 N(0,1); x redrawn where the ReLU's argument is
    within MARGIN of zero"""
    x = (offset + rng.standard_normal((B, C, H, W))).astype(np.float32)
    weight = rng.standard_normal(C).astype(np.float32)
    weight[C // 3] = 0.0
    assert (weight < 0).sum() >= 4
    bias = (0.3 * rng.standard_normal(C)).astype(np.float32)
    bias[np.abs(bias) < 1e-3] = 0.05
    for _ in range(200):
        pre, _, _ = C_pre(x, weight, bias, G)
        bad = np.abs(pre) < 10 * MARGIN
        if not bad.any():
            break
        x = np.where(bad, (offset + rng.standard_normal(x.shape)).astype(np.float32), x)
    else:
        raise AssertionError("redrawing did not converge")
    p = dict(x=x, weight=weight, bias=bias, G=G)
    if Cs:
        p["skip"] = (rng.integers(-32, 33, (B, Cs, H, W)) / 16.0).astype(np.float32)
        p["ct"] = (rng.integers(-8, 9, (B, C + Cs, 2 * H, 2 * W)) / 4.0).astype(np.float32)
    else:
        p["ct"] = (rng.integers(-8, 9, (B, C, H, W)) / 4.0).astype(np.float32)
    return p


def C_pre(x, weight, bias, G):
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    pre, xhat, rstd = C.pre_relu(t(x), t(weight), t(bias), G)
    return pre.numpy(), xhat, rstd


def finish(name, part, p, y32, g32, y64, g64):
    pre, _, _ = C_pre(p["x"], p["weight"], p["bias"], p["G"])
    assert np.abs(pre).min() >= MARGIN, (name, part, np.abs(pre).min())
    share = float((pre > 0).mean())
    assert 0.30 <= share <= 0.70, (name, part, share)
    assert np.array_equal(g32[0] == 0, g64[0] == 0), (name, part, "zero pattern of dx")
    for a in [y32, y64] + g32 + g64:
        assert np.isfinite(a).all(), (name, part)
    blob = {f"{part}_{k}": (np.int64(v) if k == "G" else v) for k, v in p.items()}
    blob[f"{part}_y32"], blob[f"{part}_y64"] = y32, y64
    blob[f"{part}_e_ref_y"] = np.float64(rel(y32, y64))
    for k, a, b in zip(("dx", "dw", "db", "ds"), g32, g64):
        blob[f"{part}_{k}32"], blob[f"{part}_{k}64"], blob[f"{part}_e_ref_{k}"] = a, b, np.float64(rel(a, b))
    print(f"  {name:4s} {part:4s} positive {share:.3f}  min |pre| {np.abs(pre).min():.1e}  e_ref " +
          " ".join(f"{k} {float(blob[f'{part}_e_ref_{k}']):.1e}" for k in ("y", "dx", "dw", "db", "ds") if f"{part}_e_ref_{k}" in blob))
    return blob


def save(name, blob, parts):
    blob["parts"] = np.array(parts)
    path = os.path.join(OUT, f"g17_gnstage_{name}.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size / 1024:.1f} KiB")


def decoder_case(M, name, cls, stage, B, C, G, H, W, seed):
    p = draw(np.random.default_rng(seed), B, C, G, H, W, Cs=C)
    y64, g64 = run_decoder(M, cls, stage, p, torch.float64)
    y32, g32 = run_decoder(M, cls, stage, p, torch.float32)
    save(name, finish(name, "s", p, y32, g32, y64, g64), ["s"])


def encoder_case(M, name, specs, seed, offset=0.0):
    rng = np.random.default_rng(seed)
    blob, parts = {}, []
    for k, B, C, G, H, W in specs:
        p = draw(rng, B, C, G, H, W, Cs=0, offset=offset)
        y64, g64 = run_encoder(M, k, p, torch.float64)
        y32, g32 = run_encoder(M, k, p, torch.float32)
        blob.update(finish(name, f"gn{k}", p, y32, g32, y64, g64))
        parts.append(f"gn{k}")
    save(name, blob, parts)


def main():
    if not RI.available():
        raise SystemExit("reference not mounted")
    M = RI.models()
    decoder_case(M, "dec", "decoder0", 5, 2, 64, 4, 6, 10, 1701)
    decoder_case(M, "odd", "decoder0", 2, 3, 256, 16, 3, 5, 1702)
    decoder_case(M, "one", "decoderLight", 2, 1, 512, 32, 1, 1, 1703)
    decoder_case(M, "row", "decoder0", 4, 2, 128, 8, 1, 7, 1704)
    encoder_case(M, "enc", [(1, 2, 64, 4, 5, 7), (6, 2, 1024, 64, 1, 2)], 1705)
    encoder_case(M, "big", [(1, 1, 64, 4, 16, 23)], 1706, offset=100.0)


if __name__ == "__main__":
    main()
