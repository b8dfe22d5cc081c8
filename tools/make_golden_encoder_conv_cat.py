"""The golden vector for the encoders' convolution over several sources (sgr.encoder_conv_cat), produced by the UNMODIFIED reference:
``models.encoderLight(SGNum=1, cascadeLevel=1)``, whose ``conv1`` reads ``torch.cat([input1, input2], dim=1)`` (models.py:254-262) -- 64
``preProcess`` channels and 7 channels of ``envs``.  TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout,
oracle/ref_import.py); never runs on the GPU machine:

    python tools/make_golden_encoder_conv_cat.py   # writes tests/golden/g24_enccat_light.npz

The encoder runs as it is, ``B = 2``: a forward hook on ``preProcess`` returns a chosen ``[2,64,5,7]`` leaf in place of its output, ``envs``
is a ``[2,7,5,7]`` leaf, ``conv1``'s parameters are set to stored values, and a forward hook on ``conv1`` captures its output and ends the
forward with an exception of this tool's (a 2 x 3 map is too small for the layers below).  The gradients at the two leaves and at
``conv1.weight`` / ``conv1.bias`` come from ``torch.autograd.grad`` with a stored cotangent: the reference's own ``torch.cat`` backward
splits ``dx`` between the sources.  The run is repeated in fp64 with the same numbers.

The file holds ``x1, x2, Wt, bias, ct``, the output ``out32`` / ``out64``, the source gradients ``dx1, dx2`` and ``db`` whole as ``32`` and
``64``, ``dW`` for every eighth output channel only (``dW_rows`` lists them), and ``e_ref_{out,dx1,dx2,dW,db}`` = the rel-L2 distance between
the reference's two runs (``dW``'s over the stored rows).  To stay under the 1 MiB cap BOTH allowed savings are used: the ``dW`` rows, and
weights drawn from a short dyadic grid (multiples of 1/64 in [-1/4, 1/4]) so that they compress."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_import as RI      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g24_enccat_light.npz")
MAX_BYTES = 1 << 20
B, C1, C2, O, H, W = 2, 64, 7, 128, 5, 7
ROWS = np.arange(0, O, 8)


class Captured(Exception):
    pass


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.abs(a).max())


def draw(rng):
    return dict(x1=rng.standard_normal((B, C1, H, W)).astype(np.float32), x2=rng.standard_normal((B, C2, H, W)).astype(np.float32),
                Wt=(rng.integers(-16, 17, (O, C1 + C2, 4, 4)) / 64.0).astype(np.float32), bias=(rng.integers(-8, 9, O) / 64.0).astype(np.float32),
                ct=rng.standard_normal((B, O, H // 2, W // 2)).astype(np.float32))


def run(M, p, dtype):
    x1 = torch.from_numpy(p["x1"]).to(dtype).requires_grad_(True)
    x2 = torch.from_numpy(p["x2"]).to(dtype).requires_grad_(True)
    torch.manual_seed(2400)
    enc = M.encoderLight(SGNum=1, cascadeLevel=1).to(dtype)
    conv = enc.conv1
    assert isinstance(enc.pad1, torch.nn.ReplicationPad2d) and tuple(enc.pad1.padding) == (1, 1, 1, 1)
    assert tuple(conv.weight.shape) == (O, C1 + C2, 4, 4) and conv.stride == (2, 2) and conv.padding == (0, 0), conv
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(p["Wt"]).to(dtype))
        conv.bias.copy_(torch.from_numpy(p["bias"]).to(dtype))
    got = []

    def capture(m, i, o):
        got.append((i[0], o))
        raise Captured
    h1 = enc.preProcess.register_forward_hook(lambda m, i, o: x1)
    h2 = conv.register_forward_hook(capture)
    try:
        enc(torch.zeros(B, 11, 4 * H, 4 * W, dtype=dtype), x2)
        raise AssertionError("conv1 did not run")
    except Captured:
        pass
    finally:
        h1.remove()
        h2.remove()
    padded, out = got[0]
    assert torch.equal(padded[:, :C1, 1:-1, 1:-1], x1) and torch.equal(padded[:, C1:, 1:-1, 1:-1], x2) and out.dtype == dtype
    assert tuple(out.shape) == tuple(p["ct"].shape), out.shape
    g = torch.autograd.grad(out, [x1, x2, conv.weight, conv.bias], grad_outputs=torch.from_numpy(p["ct"]).to(dtype))
    return out.detach().numpy(), [t.numpy() for t in g]


def main():
    if not RI.available():
        raise SystemExit("reference not mounted")
    M = RI.models()
    p = draw(np.random.default_rng(2401))
    o64, g64 = run(M, p, torch.float64)
    o32, g32 = run(M, p, torch.float32)
    for a in [o32, o64] + g32 + g64:
        assert np.isfinite(a).all()
    blob = dict(p)
    blob["pad_mode"] = np.int64(0)
    blob["dW_rows"] = ROWS.astype(np.int64)
    blob["out32"], blob["out64"], blob["e_ref_out"] = o32, o64, np.float64(rel(o32, o64))
    for k, a, b in zip(("dx1", "dx2", "dW", "db"), g32, g64):
        if k == "dW":
            a, b = a[ROWS], b[ROWS]
        blob[f"{k}32"], blob[f"{k}64"], blob[f"e_ref_{k}"] = a, b, np.float64(rel(a, b))
    np.savez_compressed(OUT, **blob)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, size
    print(f"light {size / 1024:6.1f} KiB  e_ref " + " ".join(f"{k} {float(blob[f'e_ref_{k}']):.1e}" for k in ("out", "dx1", "dx2", "dW", "db")))


if __name__ == "__main__":
    main()
