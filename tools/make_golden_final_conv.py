"""Golden vectors for the BRDF decoders' final pad + 3x3 convolution, produced by the UNMODIFIED reference (models.decoder0).  TEST
INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout, oracle/ref_import.py); never runs on the GPU machine:

    python tools/make_golden_final_conv.py        # writes tests/golden/g20_finalconv_{vec,odd,one,row,col,two,plain}.npz

The decoder runs as it is, with the hook trick of tools/make_golden_gn_stage.py: a forward hook on ``dconv6`` RETURNS a chosen leaf ``x`` (fp32
values cast to the run's dtype), ``dgn6.*`` and ``dconvFinal.*`` are set to stored values, the image has the leaf's size (so the reference's
final resize, models.py:185-186, does not fire) and a forward hook on ``dconvFinal`` captures ``x_orig = dconvFinal(dpadFinal(relu(dgn6(x))))``
(models.py:183, 187).  Gradients are taken at the leaf, at ``dgn6.weight`` / ``bias`` and at ``dconvFinal.weight`` / ``bias`` for a stored
cotangent.  ``plain`` is the pair ``dconvFinal(dpadFinal(y))`` of the same module on a signed ``y``.  Every run is repeated in fp64.

A file holds ``x`` (``plain``: ``y``), ``gn_weight, gn_bias, G`` (not in ``plain``), ``Wt, bias, ct``, the output ``out32`` / ``out64``, the
gradients ``dx, dgw, dgb, dW, db`` as ``32`` and ``64`` and ``e_ref_{out,dx,dgw,dgb,dW,db}`` = the rel-L2 distance between the reference's two
runs.

Conditions asserted here (tests/test_final_conv.py re-asserts them from the stored arrays):
  * no pre-ReLU value is within 1e-5 of zero in fp64 -- offending elements of ``x`` are redrawn -- so a 1-ulp difference cannot flip a branch;
  * the zero pattern of ``dx32`` equals that of ``dx64``;
  * between 30 % and 70 % of the pre-ReLU values are positive;
  * nothing is NaN."""
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
import gn_stage_checker as GN            # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20
MARGIN = 1e-5
FEATURE_CH = (64, 128, 256, 256, 512, 1024)
GRADS = ("dx", "dgw", "dgb", "dW", "db")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.abs(a).max())


def pre_relu(p):
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    return GN.pre_relu(t(p["x"]), t(p["gn_weight"]), t(p["gn_bias"]), p["G"])[0].numpy()


def draw(rng, B, C, G, H, W):
    """x = N(0,1); GroupNorm scales N(0,1) with negative ones and one exact zero, biases 0.3 N(0,1); convolution weights N(0, 1/(9 C)); x redrawn
    where the ReLU's argument is within 10 MARGIN of zero"""
    p = dict(x=rng.standard_normal((B, C, H, W)).astype(np.float32), G=G)
    p["gn_weight"] = rng.standard_normal(C).astype(np.float32)
    p["gn_weight"][C // 3] = 0.0
    assert (p["gn_weight"] < 0).sum() >= 4
    p["gn_bias"] = (0.3 * rng.standard_normal(C)).astype(np.float32)
    p["gn_bias"][np.abs(p["gn_bias"]) < 1e-3] = 0.05
    p["Wt"] = (rng.standard_normal((3, C, 3, 3)) / np.sqrt(9.0 * C)).astype(np.float32)
    p["bias"] = (0.1 * rng.standard_normal(3)).astype(np.float32)
    p["ct"] = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    for _ in range(200):
        bad = np.abs(pre_relu(p)) < 10 * MARGIN
        if not bad.any():
            return p
        p["x"] = np.where(bad, rng.standard_normal(p["x"].shape).astype(np.float32), p["x"])
    raise AssertionError("redrawing did not converge")


def decoder(M, p, dtype):
    torch.manual_seed(2000)
    dec = M.decoder0(mode=0).to(dtype)
    assert isinstance(dec.dpadFinal, torch.nn.ReplicationPad2d) and tuple(dec.dconvFinal.weight.shape) == tuple(p["Wt"].shape)
    with torch.no_grad():
        dec.dconvFinal.weight.copy_(torch.from_numpy(p["Wt"]).to(dtype))
        dec.dconvFinal.bias.copy_(torch.from_numpy(p["bias"]).to(dtype))
    return dec


def run_fused(M, p, dtype):
    """the unmodified decoder0 with ``x`` returned from dconv6 -> (x_orig, gradients at x, dgn6.*, dconvFinal.*)"""
    dec = decoder(M, p, dtype)
    gn = dec.dgn6
    with torch.no_grad():
        gn.weight.copy_(torch.from_numpy(p["gn_weight"]).to(dtype))
        gn.bias.copy_(torch.from_numpy(p["gn_bias"]).to(dtype))
    assert gn.num_groups == p["G"] and gn.num_channels == p["x"].shape[1] and gn.eps == 1e-5
    leaf = torch.from_numpy(p["x"]).to(dtype).requires_grad_(True)
    B, _, H, W = leaf.shape
    got = []
    h1 = dec.dconv6.register_forward_hook(lambda m, i, o: leaf)
    h2 = dec.dconvFinal.register_forward_hook(lambda m, i, o: got.append(o))
    dec(torch.zeros(B, 3, H, W, dtype=dtype), *[torch.zeros(B, c, 1, 1, dtype=dtype) for c in FEATURE_CH])
    h1.remove()
    h2.remove()
    out, = got
    assert out.dtype == dtype and tuple(out.shape) == (B, 3, H, W), out.shape
    g = torch.autograd.grad(out, [leaf, gn.weight, gn.bias, dec.dconvFinal.weight, dec.dconvFinal.bias], grad_outputs=torch.from_numpy(p["ct"]).to(dtype))
    return out.detach().numpy(), [t.numpy() for t in g]


def run_plain(M, p, dtype):
    """the module's own dconvFinal(dpadFinal(y)) -> (x_orig, gradients at y, dconvFinal.*)"""
    dec = decoder(M, p, dtype)
    leaf = torch.from_numpy(p["y"]).to(dtype).requires_grad_(True)
    out = dec.dconvFinal(dec.dpadFinal(leaf))
    g = torch.autograd.grad(out, [leaf, dec.dconvFinal.weight, dec.dconvFinal.bias], grad_outputs=torch.from_numpy(p["ct"]).to(dtype))
    return out.detach().numpy(), [t.numpy() for t in g]


def save(name, p, o32, g32, o64, g64, keys):
    for a in [o32, o64] + g32 + g64:
        assert np.isfinite(a).all(), name
    blob = {k: (np.int64(v) if k == "G" else v) for k, v in p.items()}
    blob["out32"], blob["out64"], blob["e_ref_out"] = o32, o64, np.float64(rel(o32, o64))
    for k, a, b in zip(keys, g32, g64):
        blob[f"{k}32"], blob[f"{k}64"], blob[f"e_ref_{k}"] = a, b, np.float64(rel(a, b))
    path = os.path.join(OUT, f"g20_finalconv_{name}.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name:5s} {size / 1024:6.1f} KiB  e_ref " + " ".join(f"{k} {float(blob[f'e_ref_{k}']):.1e}" for k in ("out",) + tuple(keys)))


def fused_case(M, name, B, C, G, H, W, seed):
    p = draw(np.random.default_rng(seed), B, C, G, H, W)
    o64, g64 = run_fused(M, p, torch.float64)
    o32, g32 = run_fused(M, p, torch.float32)
    pre = pre_relu(p)
    share = float((pre > 0).mean())
    assert np.abs(pre).min() >= MARGIN and 0.30 <= share <= 0.70, (name, np.abs(pre).min(), share)
    assert np.array_equal(g32[0] == 0, g64[0] == 0), (name, "zero pattern of dx")
    save(name, p, o32, g32, o64, g64, GRADS)


def plain_case(M, name, B, C, H, W, seed):
    rng = np.random.default_rng(seed)
    p = dict(y=rng.standard_normal((B, C, H, W)).astype(np.float32), Wt=(rng.standard_normal((3, C, 3, 3)) / np.sqrt(9.0 * C)).astype(np.float32),
             bias=(0.1 * rng.standard_normal(3)).astype(np.float32), ct=rng.standard_normal((B, 3, H, W)).astype(np.float32))
    assert (p["y"] < 0).mean() > 0.3      # signed: not a ReLU's output
    o64, g64 = run_plain(M, p, torch.float64)
    o32, g32 = run_plain(M, p, torch.float32)
    save(name, p, o32, g32, o64, g64, ("dy", "dW", "db"))


def main():
    if not RI.available():
        raise SystemExit("reference not mounted")
    M = RI.models()
    fused_case(M, "vec", 2, 64, 4, 6, 10, 2001)
    fused_case(M, "odd", 3, 64, 4, 5, 7, 2002)      # nothing on a 16-byte boundary
    fused_case(M, "one", 1, 64, 4, 1, 1, 2003)      # all nine taps are the same pixel
    fused_case(M, "row", 2, 64, 4, 1, 9, 2004)
    fused_case(M, "col", 1, 64, 4, 7, 1, 2005)
    fused_case(M, "two", 1, 64, 4, 2, 2, 2006)      # every pixel on two borders
    plain_case(M, "plain", 2, 64, 4, 6, 2007)


if __name__ == "__main__":
    main()
