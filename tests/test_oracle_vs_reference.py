"""CPU: oracle against the unmodified reference -- its outputs recorded in tests/golden/g11_refcheck*.npz
(oracle/make_golden_refcheck.py), and, where the reference checkout is mounted (oracle/ref_import.py), the live reference too."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, rel_l2
from oracle import make_golden_refcheck as G
from oracle import ref_import as RI
from oracle import sg_oracle as O


def _golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 5e-6)])
def test_forward_matches_live_reference(dtype, tol):
    c = G.FWD_CASE
    bn, imH, imW, R, C, K = c["bn"], c["imH"], c["imW"], c["R"], c["C"], c["K"]
    z, tag = _golden("g11_refcheck"), ("f64" if dtype == torch.float64 else "f32")
    inp = {k: torch.from_numpy(z[f"{tag}_in_{k}"]) for k in ("albedo", "normal", "rough", "axis", "lamb", "weight", "im", "env_gt")}
    for k, v in inp.items():
        assert v.dtype == dtype and v.shape[0] == bn, k
    ref = {k: torch.from_numpy(z[f"{tag}_ref_{k}"]) for k in ("env", "diffuse", "spec", "im_s", "ls_a", "ls_b", "lsregress")}
    refs = [ref]
    if RI.available():      # the live reference on the stored inputs as well
        M = RI.models()
        o2e, rl = RI.make_layers(K, R, C, dtype=dtype)
        env_r, _, _, _ = o2e.output2env(inp["axis"], inp["lamb"], inp["weight"])
        d_r, s_r = rl.forwardEnv(inp["albedo"], inp["normal"], inp["rough"], env_r)
        im_s = torch.nn.functional.adaptive_avg_pool2d(inp["im"], (R, C))
        a, b = M.LSregressDiffSpec(d_r, s_r, im_s, d_r, s_r)
        refs.append(dict(env=env_r, diffuse=d_r, spec=s_r, im_s=im_s, ls_a=a, ls_b=b, lsregress=M.LSregress(env_r, inp["env_gt"], env_r)))
    env_o, d_o, s_o = O.render_from_sg(inp["albedo"], inp["normal"], inp["rough"], inp["axis"], inp["lamb"], inp["weight"])
    assert env_o.shape == (bn, 3, R, C, 8, 16) and inp["albedo"].shape == (bn, 3, imH, imW)
    for r in refs:
        assert rel_l2(env_o, r["env"]) < tol and rel_l2(d_o, r["diffuse"]) < tol and rel_l2(s_o, r["spec"]) < tol
        a2, b2 = O.lsregress_diffspec(r["diffuse"], r["spec"], r["im_s"], r["diffuse"], r["spec"])
        assert rel_l2(a2, r["ls_a"]) < tol and rel_l2(b2, r["ls_b"]) < tol
        c2 = O.lsregress(r["env"], inp["env_gt"], r["env"])
        assert rel_l2(c2, r["lsregress"]) < tol


def test_view_vectors_and_tables_bit_equal():
    z, zv = _golden("g11_refcheck"), _golden("g11_refcheck_views")
    for i, (R, C, fov) in enumerate(G.VIEW_CASES):
        v = O.view_vectors(C, R, fov)
        assert v.dtype == zv[f"view{i}"].dtype and np.array_equal(v, zv[f"view{i}"])
        assert np.array_equal(O.view_vectors(C, R, fov, G.CAM), zv[f"view{i}_cam"])
        if RI.available():
            _, rl = RI.make_layers(12, R, C, fov=fov)
            assert np.array_equal(v, rl.v[0].numpy())
            _, rl = RI.make_layers(12, R, C, fov=fov, cameraPos=G.CAM)
            assert np.array_equal(O.view_vectors(C, R, fov, G.CAM), rl.v[0].numpy())
    for i, (eh, ew) in enumerate(G.ENV_GRIDS):
        ls, om = O.direction_table(eh, ew)
        assert ls.dtype == z[f"ls{i}"].dtype and np.array_equal(ls, z[f"ls{i}"])
        assert om.dtype == z[f"env_weight{i}"].dtype and np.array_equal(om, z[f"env_weight{i}"])
        if RI.available():
            o2e, rl = RI.make_layers(12, 6, 8, eh, ew)
            assert np.array_equal(ls, rl.ls.numpy())
            assert np.array_equal(om, rl.envWeight.reshape(-1).numpy())
