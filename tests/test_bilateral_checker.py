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


_RECORDED = {}


def recorded(name):
    """every image of a fixture through the checker with the PCG record, once"""
    if name not in _RECORDED:
        z = load(name)
        _RECORDED[name] = [BC.run_case(z["image"][b], z["pred"][b], z["conf"][b], z["grad"][b], tuple(z["params"])) for b in range(z["image"].shape[0])]
    return _RECORDED[name]


@pytest.mark.parametrize("name", SOLVER_CASES)
def test_recording_the_pcg_changes_no_bit(name):
    z = load(name)
    for b, rec in enumerate(recorded(name)):
        plain = BC.run_case(z["image"][b], z["pred"][b], z["conf"][b], z["grad"][b], tuple(z["params"]), record=False)
        assert not {"stops_fwd", "stops_bwd", "margin"} & set(plain) and set(plain) | {"stops_fwd", "stops_bwd", "margin"} == set(rec)
        for k, v in plain.items():
            assert np.array_equal(v, rec[k]), (b, k)


@pytest.mark.parametrize("name", SOLVER_CASES)
def test_no_fixture_system_stops_in_mid_run(name):
    """A recorded fact about the fixtures: with cg_tol = 1e-5 and 10 or 12 iterations every PCG either stops at iteration 0 (a constant
    channel, or a start vector that already solves the system), has |b| = 0, or runs all its iterations -- the stop tests in between
    never fire, by a margin of ln 2 at the least.  The one exception is m1wide, whose grid has no neighbour at all: its systems are
    diagonal, the first step of a diagonally preconditioned CG solves them exactly, and its backward solves stop at iteration 1, all
    channels together.  No fixture has channels of one image stopping at different iterations, or any stop after iteration 1.
    tests/test_gpu_bilateral_edges.py makes the inputs that do."""
    maxiter = int(load(name)["params"][6])
    for b, rec in enumerate(recorded(name)):
        stops = np.concatenate([rec["stops_fwd"], rec["stops_bwd"]])
        print(f"{name}[{b}]: stops {stops.tolist()}  margin {rec['margin']:.3g}")
        diagonal = bool(np.all(rec["nbr"] < 0))
        assert diagonal == (name == "m1wide")
        if diagonal:
            assert np.all(rec["stops_fwd"] == 0) and np.all(rec["stops_bwd"] == 1), stops
        else:
            assert np.all((stops == 0) | (stops == BC.B_ZERO) | (stops == maxiter)), stops
        assert rec["margin"] >= np.log(2.0)


def test_pcg_record():
    rng = np.random.default_rng(0)
    q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
    A = q @ np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]) @ q.T
    b, x0, minv = rng.standard_normal(6), np.zeros(6), np.ones(6)
    rec = {}
    x = BC.pcg(lambda v: A @ v, b, x0, minv, 1e-8, 20, rec)
    assert np.array_equal(x, BC.pcg(lambda v: A @ v, b, x0, minv, 1e-8, 20))
    assert 1 <= rec["stop"] <= 7 and len(rec["ratios"]) == rec["stop"] + 1          # six distinct eigenvalues: done after six steps
    assert all(r >= 1 for r in rec["ratios"][:-1]) and rec["ratios"][-1] < 1
    assert np.linalg.norm(A @ x - b) < 1e-8 * np.linalg.norm(b) * 1.0001
    assert BC.stop_margin([rec]) == min(abs(np.log(r)) for r in rec["ratios"])
    BC.pcg(lambda v: A @ v, b, x0, minv, 1e-8, 3, rec)
    assert rec["stop"] == 3 and len(rec["ratios"]) == 3                              # never stopped: maxiter
    assert not BC.pcg(lambda v: A @ v, np.zeros(6), b, minv, 1e-8, 3, rec).any() and rec["stop"] == BC.B_ZERO and rec["ratios"] == []
    assert BC.stop_margin([rec]) == float("inf")


def test_cg_maxiter_0_returns_the_start_vector():
    z = load("m0c3")
    params = tuple(z["params"][:6]) + (0,)
    image, pred, conf, grad = z["image"][0], z["pred"][0], z["conf"][0], z["grad"][0]
    r = BC.run_case(image, pred, conf, grad, params)
    g = BC.Grid(image, *params[:3])
    w = conf.astype(np.float64).reshape(-1)
    t = pred.astype(np.float64).reshape(g.npixels, -1)
    y0 = g.splat(t * w[:, None]) / np.maximum(g.splat(w), 1e-10)[:, None]
    assert np.array_equal(r["yhat"], y0) and np.array_equal(r["out"].reshape(g.npixels, -1), y0[g.idx])
    yb0 = g.splat(grad.astype(np.float64).reshape(g.npixels, -1)) / g.splat(np.ones(g.npixels))[:, None]
    assert np.array_equal(r["grad_pred"].reshape(g.npixels, -1), yb0[g.idx] * w[:, None])
    assert np.all(r["stops_fwd"] == 0) and np.all(r["stops_bwd"] == 0) and r["margin"] == float("inf")


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
