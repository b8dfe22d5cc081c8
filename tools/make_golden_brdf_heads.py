"""Golden vectors for the BRDF decoder output heads, produced by the UNMODIFIED reference (models.decoder0, models.py:132-203).
TEST INFRASTRUCTURE ONLY -- authoring container (needs the reference checkout, oracle/ref_import.py); never runs on the GPU machine:

    python tools/make_golden_brdf_heads.py        # writes tests/golden/g16_brdfheads_{vec,odd,sat,nyu}.npz

``models.decoder0(mode)`` runs as it is, for modes 0 / 1 / 2 / 4, with its random initial weights on small random feature maps.  A
forward hook on its ``dconvFinal`` RETURNS a chosen pre-activation leaf (fp32 values cast to the run's dtype), so the reference's fp32 and
fp64 runs see the same bits and everything after ``dconvFinal`` -- the lines this project restates -- is the reference's own code.  Per
decoder the file holds ``x``, the outputs ``y32`` / ``y64``, a cotangent ``ct`` and the gradients ``gx32`` / ``gx64`` at ``x``, and
``e_ref_*`` = the rel-L2 distance between the two runs.  These are the decoder's own outputs (``unit=False``); the wrappers'
``0.5 * (y + 1)`` is exact arithmetic on top (``0.5 * gx`` for the gradient).

Conditions asserted here (tests/test_brdf_heads.py re-asserts them from the stored arrays):
  * every ``|1.01 tanh(x)|`` (mode 4: of the channel mean) is at least 1e-5 away from 1 in fp64 -- offending draws are resampled -- so a
    1-ulp tanh cannot flip a clamp branch;
  * the zero pattern of ``gx32`` equals that of ``gx64``: both runs took the same branches;
  * every normal norm is >= 1e-3 and nothing is NaN;
  * in ``vec`` and ``odd`` at least 10 % of each term's elements are saturated and at least 50 % are not.  Pre-activations are
    ``2 N(0,1)``; the depth decoder's are ``2 sqrt(3) N(0,1)``, because mode 4 activates the channel MEAN, which has a third of the variance.

``sat`` is placed by hand (1 x 4 x 8): the ladder +-{0.5, 2.0, 2.6, 2.7, 4, 9, 30} around the kink at atanh(1 / 1.01) = 2.6517, exact zeros
in the albedo, roughness and depth terms, never a zero triplet in the normal term, and the triplets that tell mode 2 (activation, then
mean) from mode 4 (mean, then activation): roughness triplets whose channels saturate while their mean would not, and depth triplets
whose mean lies on the other side of the kink from some of their channels -- saturated mean with unsaturated channels, and unsaturated
mean with saturated channels.  (A mean cannot be saturated while NO channel is: it is a convex combination of them.)"""
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
import brdf_heads_checker as C           # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20
KINK_MARGIN = 1e-5
LADDER = (0.5, 2.0, 2.6, 2.7, 4.0, 9.0, 30.0)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.abs(a).max())


def features(B, H, W, dtype, seed):
    """(im, x1 .. x6) of the sizes models.encoder0 would hand over, tiny: the decoder resizes its last feature map to the image anyway"""
    g = torch.Generator().manual_seed(seed)
    r = lambda c, s: torch.randn(B, c, s, s, generator=g).to(dtype)
    return torch.zeros(B, 3, H, W, dtype=dtype), r(64, 16), r(128, 8), r(256, 4), r(256, 2), r(512, 1), r(1024, 1)


def run_decoder(M, mode, x32, ct32, dtype):
    """the unmodified decoder0(mode) with ``x32`` returned from dconvFinal -> (output, gradient at the pre-activation) as numpy"""
    torch.manual_seed(1600 + mode)
    dec = M.decoder0(mode=mode).to(dtype)
    leaf = torch.from_numpy(x32).to(dtype).requires_grad_(True)
    B, _, H, W = x32.shape
    seen = []

    def hook(module, inp, out):
        assert tuple(out.shape) == tuple(leaf.shape) and out.dtype == dtype, (out.shape, out.dtype)
        seen.append(1)
        return leaf
    handle = dec.dconvFinal.register_forward_hook(hook)
    y = dec(*features(B, H, W, dtype, 1650 + mode))
    handle.remove()
    assert seen == [1] and y.dtype == dtype
    gx, = torch.autograd.grad(y, [leaf], grad_outputs=torch.from_numpy(ct32).to(dtype))
    return y.detach().numpy(), gx.numpy()


def resample(rng, x, term, scale):
    """redraw the triplets that come within KINK_MARGIN of the clamp's kink in fp64"""
    for _ in range(100):
        t = torch.from_numpy(x).double()
        if term == "depth":
            t = ((t[:, 0:1] + t[:, 1:2]) + t[:, 2:3]) / 3
        bad = (((1.01 * torch.tanh(t)).abs() - 1).abs() < KINK_MARGIN).any(1, keepdim=True).expand(x.shape).numpy()
        if not bad.any():
            return x
        x = np.where(bad, (scale * rng.standard_normal(x.shape)).astype(np.float32), x)
    raise AssertionError("resampling did not converge")


def random_inputs(rng, B, H, W, terms):
    out = {}
    for term in terms:
        scale = 2.0 * np.sqrt(3.0) if term == "depth" else 2.0
        out[term] = resample(rng, (scale * rng.standard_normal((B, 3, H, W))).astype(np.float32), term, scale)
    return out


def sat_inputs():
    """1 x 4 x 8, by hand: 32 triplets per term, channel-major lists below"""
    L = [s * v for v in LADDER for s in (1.0, -1.0)]                     # 14 values
    pad = lambda v: np.array((list(v) * 3)[:32], np.float32)
    # albedo: the ladder against itself in three rotations, with exact zeros
    a = np.stack([pad(L + [0.0, 0.0]), pad(L[3:] + [0.0] + L[:3]), pad(L[7:] + L[:7] + [0.0, 1.0])])
    # normal: ladder values, every triplet with a non-zero channel (a zero may appear in one channel, never in all three)
    n = np.stack([pad(L + [0.0, 1.5]), pad(L[5:] + L[:5] + [2.0, 0.0]), pad(L[9:] + L[:9] + [0.25, 0.25])])
    # roughness: channels saturate, the mean of x does not (first rows), then ladder and exact zeros
    r_special = [(4.0, -4.0, 0.5), (9.0, -30.0, 2.0), (30.0, -9.0, -2.6), (2.7, -2.7, 0.0), (4.0, 2.7, -9.0), (-30.0, 9.0, 4.0), (0.0, 0.0, 0.0), (2.7, 0.0, 0.0)]
    r = np.array(r_special + [(L[i % 14], L[(i + 4) % 14], L[(i + 8) % 14]) for i in range(24)], np.float32).T.copy()
    # depth: the mean on the other side of the kink from some channels (both directions), an exact-zero triplet, then the ladder
    d_special = [(9.0, 2.6, 0.5), (30.0, -2.0, 0.5), (-9.0, -2.6, -0.5), (4.0, 2.6, 2.0),            # mean saturated, some channels not
                 (4.0, -2.7, 0.5), (9.0, -4.0, 2.0), (-30.0, 30.0, 2.6), (2.7, 2.6, 2.0),            # mean unsaturated, some channels saturated
                 (0.0, 0.0, 0.0), (2.6, 2.6, 2.6), (2.7, 2.7, 2.7), (-2.7, -2.7, -2.7)]
    d = np.array(d_special + [(L[i % 14], L[(i + 2) % 14], L[(i + 5) % 14]) for i in range(20)], np.float32).T.copy()
    shape = lambda p: np.ascontiguousarray(p.reshape(1, 3, 4, 8))
    return dict(albedo=shape(a), normal=shape(n), rough=shape(r), depth=shape(d))


def check_conditions(name, term, x, y32, y64, gx32, gx64):
    xt = torch.from_numpy(x)
    kink = C.kink_distance(xt, term)
    assert kink >= KINK_MARGIN, (name, term, kink)
    assert np.array_equal(gx32 == 0, gx64 == 0), (name, term, "zero pattern")
    for a in (y32, y64, gx32, gx64):
        assert np.isfinite(a).all(), (name, term)
    share = float(C.saturated(xt, term).double().mean())
    if name in ("vec", "odd", "nyu"):
        assert 0.10 <= share <= 0.50, (name, term, share)
    if term == "normal":
        t = (1.01 * torch.tanh(xt.double())).clamp(-1, 1)
        nmin = float(t.norm(dim=1).min())
        assert nmin >= 1e-3, (name, nmin)
    return kink, share


def case(M, name, x_by_term, seed):
    rng = np.random.default_rng(seed)
    blob = {}
    for term, x in x_by_term.items():
        mode = C.MODES[term]
        B, _, H, W = x.shape
        ct = rng.standard_normal((B, 3 if mode < 2 else 1, H, W)).astype(np.float32)
        y64, gx64 = run_decoder(M, mode, x, ct, torch.float64)
        y32, gx32 = run_decoder(M, mode, x, ct, torch.float32)
        kink, share = check_conditions(name, term, x, y32, y64, gx32, gx64)
        blob.update({f"x_{term}": x, f"ct_{term}": ct, f"y32_{term}": y32, f"y64_{term}": y64, f"gx32_{term}": gx32, f"gx64_{term}": gx64,
                     f"e_ref_y_{term}": np.float64(rel(y32, y64)), f"e_ref_gx_{term}": np.float64(rel(gx32, gx64))})
        print(f"  {name:4s} {term:7s} e_ref values {rel(y32, y64):.1e} gradients {rel(gx32, gx64):.1e}  saturated {share:.3f}  distance to the kink {kink:.1e}")
    path = os.path.join(OUT, f"g16_brdfheads_{name}.npz")
    np.savez_compressed(path, **blob)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size / 1024:.1f} KiB")


def main():
    if not RI.available():
        raise SystemExit("reference not mounted")
    M = RI.models()
    case(M, "vec", random_inputs(np.random.default_rng(1601), 2, 6, 10, C.TERMS), 1611)
    case(M, "odd", random_inputs(np.random.default_rng(1602), 3, 5, 7, C.TERMS), 1612)
    sat = sat_inputs()
    mean_sat, ch_sat = C.saturated(torch.from_numpy(sat["depth"]), "depth")[:, 0], C.saturated(torch.from_numpy(sat["depth"]), "albedo")
    assert int((mean_sat & ~ch_sat.all(1)).sum()) >= 3 and int((~mean_sat & ch_sat.any(1)).sum()) >= 3
    r_mean, r_ch = C.saturated(torch.from_numpy(sat["rough"]), "depth")[:, 0], C.saturated(torch.from_numpy(sat["rough"]), "rough")
    assert int((~r_mean & r_ch.any(1)).sum()) >= 4
    assert not (sat["normal"] == 0).all(1).any() and all((sat[k] == 0).any() for k in ("albedo", "rough", "depth"))
    case(M, "sat", sat, 1613)
    case(M, "nyu", random_inputs(np.random.default_rng(1604), 2, 6, 10, ("normal", "depth")), 1614)


if __name__ == "__main__":
    main()
