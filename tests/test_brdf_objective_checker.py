"""CPU: tests/brdf_objective_checker.py (the contract of sgr.brdf_objective / sgr.batch_ranking_loss in fp64, own code) against the
fixtures the UNMODIFIED reference produced (tests/golden/g14_brdfobj_*.npz, tools/make_golden_brdf_objective.py).

Values and gradients agree with the reference's fp64 run to 1e-12 relative -- the level at which bilateral_checker is pinned (1e-13
there; 1e-12 leaves room for the summation order of a second fp64 implementation).  The checker departs from the reference in two
stated places only: an empty mask / an image without judgements gives 0 where the reference gives NaN, and a judgement outside the
image counts as weight 0 where the reference raises."""
import os

import numpy as np
import pytest
import torch

import brdf_objective_checker as C
from conftest import GOLDEN_DIR

SYN = ["syn_small", "syn_clip", "syn_softmask", "syn_coefclamp", "syn_odd"]
VALUES = ("total", "albedoErr", "normalErr", "roughErr", "depthErr")
GRADS = ("g_albedo", "g_normal", "g_rough", "g_depth")


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g14_brdfobj_{name}.npz"))


def t64(z, k):
    return torch.from_numpy(z[k]).double() if k in z.files else None


def objective_args(z):
    """(positional arguments of the checker / of sgr.brdf_objective, keyword arguments) as fp64 tensors; absent terms are None"""
    args = [t64(z, k) for k in ("albedoPred", "normalPred", "roughPred", "depthPred", "albedo", "normal", "rough", "depth", "segBRDF", "segAll")]
    for i in range(4):
        if args[i] is None:
            args[i + 4] = None
    return args, dict(weights=tuple(z["weights"]), depth_offset=float(z["depth_offset"]), segDepth=t64(z, "segDepth"))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.abs(a).max())


@pytest.mark.parametrize("name", SYN + ["nyu_small"])
def test_checker_matches_the_reference_fp64(name):
    z = load(name)
    args, kw = objective_args(z)
    out = C.brdf_objective(*args, **kw)
    for k in VALUES + ("angleMean",):
        if "ref64_" + k in z.files:
            ref = float(z["ref64_" + k])
            assert abs(float(out[k]) - ref) <= 1e-12 * abs(ref), (name, k, float(out[k]), ref)
    for k in GRADS:
        if "ref64_" + k in z.files:
            assert rel(out[k].numpy(), z["ref64_" + k]) <= 1e-12, (name, k)
        else:
            assert out[k] is None
    if name == "nyu_small":
        assert float(out["albedoErr"]) == 0.0 and float(out["roughErr"]) == 0.0


def test_fixture_conditions():
    """what the issue asks of the cases, re-derived from the stored inputs with the checker"""
    z = load("syn_clip")
    args, kw = objective_args(z)
    out = C.brdf_objective(*args, **kw)
    prod = (args[0] * out["coef"][:, 0].reshape(-1, 1, 1, 1))[(args[8] > 0).expand_as(args[0])]
    share = float((prod > 1).double().mean())
    assert 0.05 <= share <= 0.5 and float(torch.minimum(prod.abs(), (prod - 1).abs()).min()) > 1e-6
    z = load("syn_coefclamp")
    args, kw = objective_args(z)
    coef = C.brdf_objective(*args, **kw)["coef"][:, 0]
    assert float(coef[0]) == 1e3 and float(coef[1]) == 1e-3 and float(args[8][1].sum()) == 0.0 and float(args[8].sum()) > 0
    z = load("syn_softmask")
    frac = z["segBRDF"][(z["segBRDF"] > 0) & (z["segBRDF"] < 1)]
    assert frac.size > 0.9 * z["segBRDF"].size and float(z["segAll"].max()) <= 1.0 and float((z["segAll"] - z["segBRDF"]).min()) >= 0
    assert tuple(load("syn_odd")["albedoPred"].shape) == (3, 3, 30, 41)
    z = load("nyu_small")
    assert not np.array_equal(z["segAll"], z["segDepth"]) and float(z["depth_offset"]) == 0.1
    for name in SYN + ["nyu_small", "rank_small"]:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, f"g14_brdfobj_{name}.npz")) <= 1 << 20


def test_gradient_routing_of_the_five_scalars_matches_autograd():
    """the checker's hand-written gradients against torch.autograd on the checker's own values, for each scalar alone and a mix"""
    z = load("syn_clip")
    args, kw = objective_args(z)
    for up in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (0.7, -1.3, 2.0, 0.25, 3.0)):
        live = [a.clone().requires_grad_(True) for a in args[:4]]
        val = C.brdf_objective(*live, *args[4:], **kw)
        obj = sum(u * val[k] for u, k in zip(up, VALUES))
        want = torch.autograd.grad(obj, live, allow_unused=True)
        got = C.brdf_objective(*args, upstream=up, **kw)
        for k, w in zip(GRADS, want):
            w = torch.zeros_like(got[k]) if w is None else w
            assert float((got[k] - w).abs().max()) <= 1e-13 * max(float(w.abs().max()), 1e-30), (up, k)


def test_empty_mask_gives_zero_where_the_reference_gives_nan():
    z = load("syn_small")
    args, kw = objective_args(z)
    args[8] = torch.zeros_like(args[8])
    args[9] = torch.zeros_like(args[9])
    out = C.brdf_objective(*args, **kw)
    for k in VALUES + ("angleMean",):
        assert float(out[k]) == 0.0
    for k in GRADS:
        assert float(out[k].abs().max()) == 0.0
    assert torch.all(out["coef"] == 1e-3)


def rank_args(z, dtype=torch.float64):
    return [torch.from_numpy(z["albedoPred"]).to(dtype)] + [torch.from_numpy(z[k]) for k in ("eqPoint", "eqWeight", "eqNum", "darkerPoint", "darkerWeight", "darkerNum")]


def test_ranking_checker_matches_the_reference_fp64():
    z = load("rank_small")
    args = rank_args(z)
    for up, key in (((1.0, 0.0), "g_eq"), ((0.0, 1.0), "g_darker")):
        out = C.batch_ranking_loss(*args, tau=float(z["tau"]), upstream=up)
        for k in ("eqLoss", "darkerLoss"):
            ref = float(z["ref64_" + k])
            assert abs(float(out[k]) - ref) <= 1e-12 * abs(ref), (k, float(out[k]), ref)
        assert rel(out["g_albedo"].numpy(), z["ref64_" + key]) <= 1e-12, key
    # the fixture has what the issue asks for: different counts, garbage in the padding, repeated pixels
    assert len(set(z["eqNum"].tolist())) == 3 and int(np.abs(z["eqPoint"][0, z["eqNum"][0]:]).max()) > 10 ** 4 and float(z["eqWeight"][0, -1]) > 1e29
    px = z["eqPoint"][0, :z["eqNum"][0], 0] * 32 + z["eqPoint"][0, :z["eqNum"][0], 1]
    assert len(set(px.tolist())) < len(px)


def test_ranking_deviations():
    z = load("rank_small")
    args = rank_args(z)
    base = C.batch_ranking_loss(*args)
    # an image without judgements contributes 0 (the reference: NaN) -- and only that image's share goes
    a2 = [t.clone() for t in args]
    a2[3][1] = 0
    a2[6][1] = 0
    out = C.batch_ranking_loss(*a2)
    assert torch.isfinite(out["eqLoss"]) and torch.isfinite(out["g_albedo"]).all() and float(out["g_albedo"][1].abs().max()) == 0.0
    assert torch.equal(out["g_albedo"][0], base["g_albedo"][0])
    # a judgement outside the image = the same judgement with weight 0
    a3, a4 = [t.clone() for t in args], [t.clone() for t in args]
    a3[1][0, 3] = torch.tensor([0, 0, 24, 5])      # row == H
    a3[4][2, 0] = torch.tensor([-1, 3, 2, 2])
    a4[2][0, 3] = 0.0
    a4[5][2, 0] = 0.0
    o3, o4 = C.batch_ranking_loss(*a3), C.batch_ranking_loss(*a4)
    for k in ("eqLoss", "darkerLoss", "g_albedo"):
        assert torch.equal(o3[k], o4[k]), k
