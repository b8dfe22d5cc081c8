"""CPU: the bilateral solver layer without a GPU.

* tests/bilateral_checker.py (numpy fp64 restatement of DESIGN.md section 8) against every fixture the UNMODIFIED reference produced
  (tools/make_golden_bilateral.py -> tests/golden/g13_bilateral_*.npz): pixel->vertex map and nvertices exactly, every float array
  <= 1e-7 rel-L2.  This pins the checker to the reference, so the GPU tests may also use it on inputs made on the spot.
* the sgr_bs_* entry points' argument validation, the operators' schemas / Meta shapes / refusal of CPU tensors;
* sgr.BilateralLayer: state_dict keys and shapes equal the reference module's, its weights load, ``.confidence()`` reproduces the
  confidence the reference's CNN produced (<= 1e-6 max-abs: the same torch ops on the same CPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bilateral_checker as BC
from conftest import GOLDEN_DIR

import inverserenderingofindoorscene_amd as sgr
from inverserenderingofindoorscene_amd import _lib

SOLVER_CASES = ["m0c3", "m0c1", "m2c3", "m2c1", "m4c3", "m4c1", "m1wide", "batch3", "constch", "zeroconf", "120x160"]


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g13_bilateral_{name}.npz"))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.abs(a).max())


@pytest.mark.parametrize("name", SOLVER_CASES)
def test_checker_reproduces_the_reference(name):
    z = load(name)
    params = tuple(z["params"])
    assert params == BC.MODES[int(z["mode"])]
    B = z["image"].shape[0]
    m, n, yhat = [], [], []
    for b in range(B):
        r = BC.run_case(z["image"][b], z["pred"][b], z["conf"][b], z["grad"][b], params)
        assert r["nvertices"] == int(z["nvertices"][b])
        assert np.array_equal(r["idx"], z["idx"][b])
        for k in ("out", "grad_pred", "grad_conf"):
            e = rel(r[k], z[k][b])
            print(f"{name}[{b}] checker vs reference {k}: {e:.2e}")
            assert e <= 1e-7, (k, e)
        m.append(r["m"]); n.append(r["n"]); yhat.append(r["yhat"].ravel())
    for k, v in (("m", m), ("n", n), ("yhat", yhat)):
        assert rel(np.concatenate(v), z[k]) <= 1e-7, k
    assert float(np.min(z["margin"])) >= 1e-9
    if name != "m1wide":
        assert np.all(z["nvertices"] < 0.9 * z["idx"].shape[1] * z["idx"].shape[2])


def test_fixture_special_cases_are_what_they_claim():
    z = load("constch")
    assert np.all(z["pred"][..., 1] == z["pred"][0, 0, 0, 1]) and np.isfinite(z["out"]).all()
    assert np.abs(z["out"][..., 1] - z["pred"][0, 0, 0, 1]).max() < 1e-12        # the PCG stops at iteration 0 on that channel
    z = load("zeroconf")
    assert not z["conf"].any() and not z["out"].any() and not z["grad_pred"].any() and np.isfinite(z["grad_conf"]).all() and z["grad_conf"].any()
    z = load("m1wide")
    assert z["image"].shape[2] > 128 and np.array_equal(z["out"], z["pred"].astype(np.float64))      # every pixel its own vertex


def test_c_abi_argument_validation_without_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    D = ctypes.c_double
    assert lib.sgr_bs_workspace_bytes(2, 120, 160, 3) > 2 * 120 * 160 * 3 * 8 * 6
    assert lib.sgr_bs_workspace_bytes(1, 120, 160, 4) == -1 and b"C in 1..3" in lib.sgr_last_error()
    assert lib.sgr_bs_workspace_bytes(0, 120, 160, 1) == -1
    assert lib.sgr_bs_grid_keys(None, fake, 1, 4, 4, D(8), D(2), D(7), None) == -1 and b"NULL" in lib.sgr_last_error()
    assert lib.sgr_bs_grid_keys(fake, fake, 1, 4, 4, D(8), D(0), D(7), None) == -1 and b"positive" in lib.sgr_last_error()
    assert lib.sgr_bs_grid_keys(fake, fake, 1, 4, 4, D(0.1), D(2), D(7), None) == -2 and b"0.25" in lib.sgr_last_error()
    assert lib.sgr_bs_grid_build(fake, fake, fake, fake, fake, fake, fake, fake, fake, None, 1, 4, 4, None) == -1
    assert lib.sgr_bs_grid_build(*([fake] * 10), 1, 0, 4, None) == -1 and b"shape" in lib.sgr_last_error()
    # (valid arguments would launch: every call below fails a check before any launch)
    assert lib.sgr_bs_solve_fwd(*([fake] * 11), None, 1, 3, 4, 4, D(200), D(1e-5), D(1e-5), 12, None) == -1 and b"NULL" in lib.sgr_last_error()
    assert lib.sgr_bs_solve_fwd(*([fake] * 12), 1, 4, 4, 4, D(200), D(1e-5), D(1e-5), 12, None) == -2 and b"channels" in lib.sgr_last_error()
    assert lib.sgr_bs_solve_fwd(*([fake] * 12), 1, 3, 4, 4, D(200), D(1e-5), D(1e-5), 65, None) == -2 and b"cg_maxiter" in lib.sgr_last_error()
    assert lib.sgr_bs_solve_fwd(*([fake] * 12), 1, 3, 4, 4, D(200), D(0), D(1e-5), 12, None) == -1 and b"parameter" in lib.sgr_last_error()
    assert lib.sgr_bs_solve_bwd(*([fake] * 13), None, 1, 3, 4, 4, D(200), D(1e-5), D(1e-5), 12, None) == -1
    assert lib.sgr_bs_solve_bwd(*([fake] * 14), 1, 0, 4, 4, D(200), D(1e-5), D(1e-5), 12, None) == -2
    assert lib.sgr_abi_version() == 6


def m(*s, dtype=torch.float32, grad=False):
    return torch.empty(*s, device="meta", dtype=dtype, requires_grad=grad)


def test_operator_schemas_and_meta_shapes():
    ops = torch.ops.sgrender
    for name in ("bilateral_grid", "bilateral_solve_fwd", "bilateral_solve_bwd", "bilateral_solve"):
        assert str(getattr(ops, name).default._schema).startswith(f"sgrender::{name}("), name
        for key in ("Meta", "CUDA", "CPU"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sgrender::{name}", key), (name, key)
    assert "int cg_maxiter" in str(ops.bilateral_solve.default._schema)
    B, C, H, W = 2, 3, 12, 20
    g = ops.bilateral_grid(m(B, 3, H, W), 8.0, 2.0, 7.0)
    assert [tuple(t.shape) for t in g] == [(B, H * W)] * 3 + [(B, H * W, 10), (B,), (B, H * W), (B, H * W)]
    assert [t.dtype for t in g] == [torch.int32] * 5 + [torch.float64] * 2
    out, yhat = ops.bilateral_solve_fwd(*g, m(B, C, H, W), m(B, 1, H, W), 200.0, 1e-5, 1e-5, 12)
    assert tuple(out.shape) == (B, C, H, W) and tuple(yhat.shape) == (B, H * W, C) and yhat.dtype == torch.float64
    gp, gc = ops.bilateral_solve_bwd(*g, m(B, C, H, W), m(B, C, H, W), m(B, 1, H, W), yhat, 200.0, 1e-5, 1e-5, 12)
    assert tuple(gp.shape) == (B, C, H, W) and tuple(gc.shape) == (B, 1, H, W)
    # through autograd: gradients for the target and the confidence, none for the guide
    image, pred, conf = m(B, 3, H, W, grad=True), m(B, 1, H, W, grad=True), m(B, 1, H, W, grad=True)
    out = sgr.bilateral_solve(image, pred, conf, 8, 2, 8, 300, cg_maxiter=10)
    assert tuple(out.shape) == (B, 1, H, W) and out.requires_grad
    g_pred, g_conf, g_img = torch.autograd.grad(out.sum(), [pred, conf, image], allow_unused=True)
    assert g_pred.shape == pred.shape and g_conf.shape == conf.shape and g_img is None
    with pytest.raises(RuntimeError, match="C in 1..3"):
        ops.bilateral_solve(m(B, 3, H, W), m(B, 4, H, W), m(B, 1, H, W), 8.0, 2.0, 7.0, 200.0, 1e-5, 1e-5, 12)
    with pytest.raises(RuntimeError, match=r"\[B,3,H,W\]"):
        ops.bilateral_grid(m(B, 1, H, W), 8.0, 2.0, 7.0)


def test_cpu_tensors_are_rejected():
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU path"):
        sgr.bilateral_solve(z(1, 3, 4, 4), z(1, 3, 4, 4), z(1, 1, 4, 4), 8, 2, 7, 200)
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.sgrender.bilateral_grid(z(1, 3, 4, 4), 8.0, 2.0, 7.0)
    layer = sgr.BilateralLayer(mode=2, isCuda=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        layer(z(1, 3, 8, 8) + 0.5, z(1, 3, 8, 8) + 0.5, z(1, 1, 8, 8))


def test_a_stale_library_is_named_by_its_missing_symbol(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.SIGNATURES, "sgr_bs_not_there", ([], ctypes.c_int))
    with pytest.raises(sgr.SgrenderUnavailable, match="sgr_bs_not_there"):
        _lib.load()


def test_layer_mirrors_the_reference_module():
    z = load("layer")
    layer = sgr.BilateralLayer(mode=int(z["mode"]), isCuda=False)
    sd = layer.state_dict()
    assert list(sd.keys()) == [str(k) for k in z["state_keys"]]
    assert all(tuple(sd[k].shape) == z["w_" + k].shape for k in sd)
    layer.load_state_dict({k: torch.from_numpy(z["w_" + k]) for k in sd}, strict=True)
    with torch.no_grad():
        conf = layer.confidence(torch.from_numpy(z["image"]), torch.from_numpy(z["feature"]), torch.from_numpy(z["pred"]))
        _, guide = layer._scaled(torch.from_numpy(z["image"]), torch.from_numpy(z["feature"]))
    assert float((conf - torch.from_numpy(z["conf"])).abs().max()) <= 1e-6
    assert torch.equal(guide, torch.from_numpy(z["guide"]))
    for mode, cin in ((0, 6), (1, 6), (2, 4), (4, 4)):
        L = sgr.BilateralLayer(mode=mode, isCuda=False)
        assert L.conv1.in_channels == cin
        sl, sc, ss, lam, amin, tol, mi = BC.MODES[mode]
        assert L.grid_params == dict(sigma_luma=sl, sigma_chroma=sc, sigma_spatial=ss) and L.bs_params == dict(lam=lam, A_diag_min=amin, cg_tol=tol, cg_maxiter=mi)
    with pytest.raises(ValueError):
        sgr.BilateralLayer(mode=3)
