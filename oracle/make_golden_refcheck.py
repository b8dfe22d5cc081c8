"""Golden vectors for tests/test_oracle_vs_reference.py produced by the UNMODIFIED reference.
TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout, oracle/ref_import.py):

    python -m oracle.make_golden_refcheck        # writes tests/golden/g11_refcheck.npz and g11_refcheck_views.npz

Stored: the small forward case of the test (its inputs and the reference's output2env + forwardEnv images, LSregressDiffSpec and
LSregress on them) in float64 and float32, the view vectors renderingLayer builds for three (R, C, fov) with and without a moved
camera (in a file of their own: each file stays under 1 MiB), and the direction / quadrature tables of output2env and renderingLayer
for three env grids.  The test holds the oracle to these whether or not the reference is mounted."""
from __future__ import annotations

import os

import numpy as np
import torch

from oracle import ref_import as RI
from oracle import sg_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

FWD_CASE = dict(bn=1, imH=12, imW=16, R=6, C=8, K=12, seed=99)
VIEW_CASES = [(120, 160, 57.0), (6, 8, 42.75), (90, 160, 57.0)]
CAM = [0.1, -0.05, 0.2]
ENV_GRIDS = [(8, 16), (16, 32), (4, 8)]


def main():
    if not RI.available():
        raise SystemExit("reference not mounted")
    M = RI.models()
    c = FWD_CASE
    out, views = {}, {}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        inp = O.synthetic_inputs(c["bn"], c["imH"], c["imW"], c["R"], c["C"], c["K"], seed=c["seed"], dtype=dtype)
        o2e, rl = RI.make_layers(c["K"], c["R"], c["C"], dtype=dtype)
        env_r, _, _, _ = o2e.output2env(inp["axis"], inp["lamb"], inp["weight"])
        d_r, s_r = rl.forwardEnv(inp["albedo"], inp["normal"], inp["rough"], env_r)
        im_s = torch.nn.functional.adaptive_avg_pool2d(inp["im"], (c["R"], c["C"]))
        a, b = M.LSregressDiffSpec(d_r, s_r, im_s, d_r, s_r)
        lsr = M.LSregress(env_r, inp["env_gt"], env_r)
        for k in ("albedo", "normal", "rough", "axis", "lamb", "weight", "im", "env_gt"):
            out[f"{tag}_in_{k}"] = inp[k].numpy()
        for k, v in (("env", env_r), ("diffuse", d_r), ("spec", s_r), ("im_s", im_s), ("ls_a", a), ("ls_b", b), ("lsregress", lsr)):
            out[f"{tag}_ref_{k}"] = v.detach().numpy()
    for i, (R, C, fov) in enumerate(VIEW_CASES):
        _, rl = RI.make_layers(12, R, C, fov=fov)
        views[f"view{i}"] = rl.v[0].numpy()
        _, rl = RI.make_layers(12, R, C, fov=fov, cameraPos=CAM)
        views[f"view{i}_cam"] = rl.v[0].numpy()
    for i, (eh, ew) in enumerate(ENV_GRIDS):
        _, rl = RI.make_layers(12, 6, 8, eh, ew)
        out[f"ls{i}"] = rl.ls.numpy()
        out[f"env_weight{i}"] = rl.envWeight.reshape(-1).numpy()
    for name, arrays in (("g11_refcheck.npz", out), ("g11_refcheck_views.npz", views)):
        path = os.path.join(GOLDEN, name)
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
