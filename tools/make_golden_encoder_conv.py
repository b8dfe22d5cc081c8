"""Golden vectors for the encoders' pad + 4x4 stride-2 convolution, produced by the UNMODIFIED reference (models.encoder0 /
models.encoderLight).  TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout, oracle/ref_import.py); never runs on the
GPU machine:

    python tools/make_golden_encoder_conv.py   # writes tests/golden/g22_encconv_{rgb,c17,pre,two,three,row,col,zero,zero3}.npz

The encoder runs as it is: a forward pre-hook on the layer's pad module substitutes a chosen leaf ``x`` for whatever reaches the pad, the
convolution's parameters are set to stored values, and a forward hook on the convolution captures its input and output and then ends the
forward with an exception of this tool's (the tiny maps of the fixtures are too small for the layers below).  Gradients at the leaf and at
the convolution's ``weight`` / ``bias`` come from ``torch.autograd.grad`` with a stored cotangent.  Every run is repeated in fp64 with the
same weights.

A file holds ``x, Wt, bias, ct``, ``pad_mode`` (0 replicate, 1 zeros), the output ``out32`` / ``out64``, the gradients ``dx, dW, db`` as
``32`` and ``64`` and ``e_ref_{out,dx,dW,db}`` = the rel-L2 distance between the reference's two runs.  Conditions asserted here
(tests/test_encoder_conv.py re-asserts them from the stored arrays): the pad module is of the expected class, the convolution saw the
padded leaf, nothing is NaN, every file is under the 1 MiB cap."""
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
GRADS = ("dx", "dW", "db")


class Captured(Exception):
    pass


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.abs(a).max())


def draw(rng, B, C, O, H, W):
    return dict(x=rng.standard_normal((B, C, H, W)).astype(np.float32), Wt=(rng.standard_normal((O, C, 4, 4)) / np.sqrt(16.0 * C)).astype(np.float32),
                bias=(0.1 * rng.standard_normal(O)).astype(np.float32), ct=rng.standard_normal((B, O, H // 2, W // 2)).astype(np.float32))


# layer -> (the model, its pad module, its convolution, the model's dummy arguments for a leaf [B,C,H,W])
def encoder0_conv1(M, level):
    def make(B, C, H, W, dtype):
        enc = M.encoder0(cascadeLevel=level).to(dtype)
        return enc, enc.pad1, enc.conv1, (torch.zeros(B, C, H, W, dtype=dtype),)
    return make, torch.nn.ReplicationPad2d


def light_pre(M, first):
    def make(B, C, H, W, dtype):
        enc = M.encoderLight(SGNum=12, cascadeLevel=0).to(dtype)
        s = 1 if first == 0 else 2      # preProcess[4] sees the map at half the input's size
        return enc, enc.preProcess[first], enc.preProcess[first + 1], (torch.zeros(B, 11, s * H, s * W, dtype=dtype),)
    return make, (torch.nn.ReplicationPad2d if first == 0 else torch.nn.ZeroPad2d)


def run(layer, p, dtype):
    make, pad_cls = layer
    leaf = torch.from_numpy(p["x"]).to(dtype).requires_grad_(True)
    torch.manual_seed(2200)
    enc, pad, conv, args = make(*leaf.shape, dtype)
    assert isinstance(pad, pad_cls) and tuple(pad.padding) == (1, 1, 1, 1), pad
    assert tuple(conv.weight.shape) == tuple(p["Wt"].shape) and conv.stride == (2, 2) and conv.padding == (0, 0), conv
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(p["Wt"]).to(dtype))
        conv.bias.copy_(torch.from_numpy(p["bias"]).to(dtype))
    got = []

    def capture(m, i, o):
        got.append((i[0], o))
        raise Captured
    h1 = pad.register_forward_pre_hook(lambda m, i: (leaf,))
    h2 = conv.register_forward_hook(capture)
    try:
        enc(*args)
        raise AssertionError("the convolution did not run")
    except Captured:
        pass
    finally:
        h1.remove()
        h2.remove()
    padded, out = got[0]
    assert torch.equal(padded[:, :, 1:-1, 1:-1], leaf) and out.dtype == dtype
    assert tuple(out.shape) == tuple(p["ct"].shape), out.shape
    g = torch.autograd.grad(out, [leaf, conv.weight, conv.bias], grad_outputs=torch.from_numpy(p["ct"]).to(dtype))
    return out.detach().numpy(), [t.numpy() for t in g]


def case(name, layer, B, C, O, H, W, seed):
    p = draw(np.random.default_rng(seed), B, C, O, H, W)
    o64, g64 = run(layer, p, torch.float64)
    o32, g32 = run(layer, p, torch.float32)
    for a in [o32, o64] + g32 + g64:
        assert np.isfinite(a).all(), name
    blob = dict(p)
    blob["pad_mode"] = np.int64(0 if layer[1] is torch.nn.ReplicationPad2d else 1)
    blob["out32"], blob["out64"], blob["e_ref_out"] = o32, o64, np.float64(rel(o32, o64))
    for k, a, b in zip(GRADS, g32, g64):
        blob[f"{k}32"], blob[f"{k}64"], blob[f"e_ref_{k}"] = a, b, np.float64(rel(a, b))
    path = os.path.join(OUT, f"g22_encconv_{name}.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name:6s} {size / 1024:6.1f} KiB  e_ref " + " ".join(f"{k} {float(blob[f'e_ref_{k}']):.1e}" for k in ("out",) + GRADS))


def main():
    if not RI.available():
        raise SystemExit("reference not mounted")
    M = RI.models()
    case("rgb", encoder0_conv1(M, 0), 2, 3, 64, 6, 10, 2201)
    case("c17", encoder0_conv1(M, 1), 3, 17, 64, 5, 7, 2202)        # odd sizes, nothing on a 16-byte boundary
    case("pre", light_pre(M, 0), 2, 11, 32, 9, 13, 2203)
    case("two", light_pre(M, 0), 1, 11, 32, 2, 2, 2204)             # one output, every tap of the pad live
    case("three", light_pre(M, 0), 1, 11, 32, 3, 3, 2205)           # one output, the last row and column read by tap 3 alone
    case("row", encoder0_conv1(M, 0), 1, 3, 64, 2, 9, 2206)
    case("col", encoder0_conv1(M, 0), 1, 3, 64, 7, 2, 2207)
    case("zero", light_pre(M, 4), 2, 32, 64, 5, 8, 2208)            # the largest file
    case("zero3", light_pre(M, 4), 1, 32, 64, 3, 3, 2209)


if __name__ == "__main__":
    main()
