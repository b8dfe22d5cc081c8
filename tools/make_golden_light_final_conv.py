"""Golden vectors for the light decoders' final pad + 3x3 convolution, produced by the UNMODIFIED reference (models.decoderLight).  TEST
INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout, oracle/ref_import.py); never runs on the GPU machine:

    python tools/make_golden_light_final_conv.py   # writes tests/golden/g21_lightconv_{ax,lam,one,row,col,two,k1m0,k1m1,k5,plain}.npz

The decoder runs as it is, with the hook trick of tools/make_golden_gn_stage.py: a forward hook on ``dgn6`` RETURNS a copy of a chosen,
strictly positive leaf ``y`` (fp32 values cast to the run's dtype), so that ``dx6 = relu(y) = y`` exactly in both precisions (models.py:330);
``env`` has the leaf's size (so the reference's final resize, models.py:332-333, does not fire); ``dconvFinal.*`` are set to stored values
and a forward hook on ``dconvFinal`` captures ``x_orig = dconvFinal(dpadFinal(dx6))`` (models.py:334; the hook fires again for the second,
identical call of models.py:336 and only the first capture is differentiated).  Gradients are taken at the leaf and at
``dconvFinal.weight`` / ``bias`` for a stored cotangent.  ``plain`` is the pair ``dconvFinal(dpadFinal(y))`` of the same module on a signed
``y``.  Every run is repeated in fp64.  The input channels are 128 everywhere: the reference fixes them.

A file holds ``y, Wt, bias, ct``, the output ``out32`` / ``out64``, the gradients ``dy, dW, db`` as ``32`` and ``64`` and
``e_ref_{out,dy,dW,db}`` = the rel-L2 distance between the reference's two runs.  ``ax`` also holds the decoder's own return value
(``ret32`` / ``ret64`` / ``e_ref_ret``: the normalised axes ``[B,12,3,H,W]``).  ``k1`` of the plan (SGNum = 1 in modes 0 and 1: 3 and 1
outputs) is the two files ``k1m0`` and ``k1m1``.

Conditions asserted here (tests/test_light_final_conv.py re-asserts them from the stored arrays): the hooked leaf is strictly positive,
nothing is NaN, every file is under the 1 MiB cap."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_import as RI      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20
C_IN = 128
FEATURE_CH = (128, 256, 256, 512, 512, 1024)
GRADS = ("dy", "dW", "db")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.abs(a).max())


def draw(rng, B, O, H, W, positive=True):
    y = rng.standard_normal((B, C_IN, H, W)).astype(np.float32)
    if positive:
        y = (np.abs(y) + np.float32(0.05)).astype(np.float32)
    return dict(y=y, Wt=(rng.standard_normal((O, C_IN, 3, 3)) / np.sqrt(9.0 * C_IN)).astype(np.float32),
                bias=(0.1 * rng.standard_normal(O)).astype(np.float32), ct=rng.standard_normal((B, O, H, W)).astype(np.float32))


def decoder(M, p, SGNum, mode, dtype):
    torch.manual_seed(2100)
    dec = M.decoderLight(SGNum=SGNum, mode=mode).to(dtype)
    assert isinstance(dec.dpadFinal, torch.nn.ReplicationPad2d) and tuple(dec.dconvFinal.weight.shape) == tuple(p["Wt"].shape)
    with torch.no_grad():
        dec.dconvFinal.weight.copy_(torch.from_numpy(p["Wt"]).to(dtype))
        dec.dconvFinal.bias.copy_(torch.from_numpy(p["bias"]).to(dtype))
    return dec


def run_decoder(M, p, SGNum, mode, dtype):
    """the unmodified decoderLight with a copy of ``y`` returned from dgn6 -> (x_orig, the decoder's return, gradients at y, dconvFinal.*)"""
    dec = decoder(M, p, SGNum, mode, dtype)
    leaf = torch.from_numpy(p["y"]).to(dtype).requires_grad_(True)
    assert float(leaf.detach().min()) > 0
    B, _, H, W = leaf.shape
    got = []
    h1 = dec.dgn6.register_forward_hook(lambda m, i, o: leaf.clone())      # a copy: the reference's ReLU works in place
    h2 = dec.dconvFinal.register_forward_hook(lambda m, i, o: got.append((i[0], o)))
    ret = dec(*[torch.zeros(B, c, 1, 1, dtype=dtype) for c in FEATURE_CH], env=torch.zeros(B, 1, H, W, dtype=dtype))
    h1.remove()
    h2.remove()
    assert len(got) == 2 and torch.equal(got[0][1], got[1][1])      # models.py:334 and :336
    padded, out = got[0]
    assert torch.equal(padded[:, :, 1:-1, 1:-1], leaf)              # dx6 = relu(y) = y exactly
    assert out.dtype == dtype and tuple(out.shape) == (B, p["Wt"].shape[0], H, W), out.shape
    g = torch.autograd.grad(out, [leaf, dec.dconvFinal.weight, dec.dconvFinal.bias], grad_outputs=torch.from_numpy(p["ct"]).to(dtype))
    return out.detach().numpy(), ret.detach().numpy(), [t.numpy() for t in g]


def run_plain(M, p, dtype):
    """the module's own dconvFinal(dpadFinal(y)) -> (x_orig, gradients at y, dconvFinal.*)"""
    dec = decoder(M, p, 12, 0, dtype)
    leaf = torch.from_numpy(p["y"]).to(dtype).requires_grad_(True)
    out = dec.dconvFinal(dec.dpadFinal(leaf))
    g = torch.autograd.grad(out, [leaf, dec.dconvFinal.weight, dec.dconvFinal.bias], grad_outputs=torch.from_numpy(p["ct"]).to(dtype))
    return out.detach().numpy(), [t.numpy() for t in g]


def save(name, p, o32, g32, o64, g64, extra=None):
    for a in [o32, o64] + g32 + g64:
        assert np.isfinite(a).all(), name
    blob = dict(p)
    blob["out32"], blob["out64"], blob["e_ref_out"] = o32, o64, np.float64(rel(o32, o64))
    for k, a, b in zip(GRADS, g32, g64):
        blob[f"{k}32"], blob[f"{k}64"], blob[f"e_ref_{k}"] = a, b, np.float64(rel(a, b))
    blob.update(extra or {})
    path = os.path.join(OUT, f"g21_lightconv_{name}.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name:5s} {size / 1024:6.1f} KiB  e_ref " + " ".join(f"{k} {float(blob[f'e_ref_{k}']):.1e}" for k in ("out",) + GRADS))


def decoder_case(M, name, SGNum, mode, B, H, W, seed, keep_return=False):
    O = SGNum if mode == 1 else 3 * SGNum
    p = draw(np.random.default_rng(seed), B, O, H, W)
    o64, r64, g64 = run_decoder(M, p, SGNum, mode, torch.float64)
    o32, r32, g32 = run_decoder(M, p, SGNum, mode, torch.float32)
    p["SGNum"], p["mode"] = np.int64(SGNum), np.int64(mode)
    extra = dict(ret32=r32, ret64=r64, e_ref_ret=np.float64(rel(r32, r64))) if keep_return else None
    save(name, p, o32, g32, o64, g64, extra)


def plain_case(M, name, B, H, W, seed):
    p = draw(np.random.default_rng(seed), B, 36, H, W, positive=False)
    assert (p["y"] < 0).mean() > 0.3      # signed: not a ReLU's output
    o64, g64 = run_plain(M, p, torch.float64)
    o32, g32 = run_plain(M, p, torch.float32)
    save(name, p, o32, g32, o64, g64)


def main():
    if not RI.available():
        raise SystemExit("reference not mounted")
    M = RI.models()
    decoder_case(M, "ax", 12, 0, 2, 5, 7, 2101, keep_return=True)      # nothing on a 16-byte boundary
    decoder_case(M, "lam", 12, 1, 2, 6, 10, 2102)
    decoder_case(M, "one", 12, 2, 1, 1, 1, 2103)                        # every tap clamped
    decoder_case(M, "row", 12, 1, 1, 1, 9, 2104)
    decoder_case(M, "col", 12, 1, 1, 7, 1, 2105)
    decoder_case(M, "two", 12, 1, 1, 2, 2, 2106)
    decoder_case(M, "k1m0", 1, 0, 3, 4, 6, 2107)                        # 3 outputs
    decoder_case(M, "k1m1", 1, 1, 3, 4, 6, 2108)                        # a single live column of an N tile
    decoder_case(M, "k5", 5, 0, 1, 4, 6, 2109)                          # 15 outputs: a tile one short of full
    plain_case(M, "plain", 1, 4, 6, 2110)


if __name__ == "__main__":
    main()
