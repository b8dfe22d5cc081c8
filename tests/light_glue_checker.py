"""Checker for the light-side glue operators: ``sgr.predToShading``, ``sgr.light_albedo_scale``, ``sgr.light_encoder_input`` and the two
regression-coefficient operators ``torch.ops.sgrender.lsregress_coef`` / ``lsregress_diffspec_coef``.
TEST INFRASTRUCTURE ONLY; own code, written from the reference's lines (utils.py:156-195, testReal.py:421-432,
wrapperBRDFLight.py:138-156, models.py:7-21 and 23-84), not from the kernels.  Every function takes a ``dtype``: fp64 is the arbiter,
the same code in fp32 is the yardstick ``e_ref`` (as ``conftest.oracle_with_noise`` does for the render path).
tests/test_light_glue_checker.py pins it at 1e-12 to the fixtures the unmodified reference produced (tests/golden/g18_lightglue_*.npz,
oracle/make_golden_light_glue.py)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

GROUPS = dict(im=(0, 3), albedo=(3, 6), normal=(6, 9), rough=(9, 10), depth=(10, 11))      # wrapperBRDFLight.py:155-156

# thresholds a result is discontinuous in: (name of the branch quantity, threshold)
DET_FLOOR, SUM_FLOOR, SPEC_FLOOR = 1e-2, 1e-5, 1e-3


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).detach().cpu().to(dtype)


# ---- utils.py:156-195, batched ------------------------------------------------------------------------------------------------------
def shading(pred, eh, ew, K, premap=1, dtype=torch.float64):
    """``[bn,7K,R,C]`` packed light prediction -> ``[bn,3,R,C]``: the SG mixture summed over the ``eh x ew`` upper-hemisphere grid with the
    weight cos(El) sin(El), floored at zero.  ``premap=1``: lamb / weight arrive in (0,1) and go through ``tan(pi/2 * 0.999 x)`` (:177-178,
    :184-185); ``premap=0``: they arrive already mapped."""
    p = _t(pred, dtype)
    bn, ch, R, C = p.shape
    assert ch == 7 * K
    az = ((torch.arange(ew, dtype=dtype) + 0.5) / ew - 0.5) * 2 * math.pi
    el = ((torch.arange(eh, dtype=dtype) + 0.5) / eh) * math.pi / 2.0
    el, az = torch.meshgrid(el, az, indexing="ij")                                   # [eh,ew]
    ls = torch.stack([torch.sin(el) * torch.cos(az), torch.sin(el) * torch.sin(az), torch.cos(el)], 0)      # [3,eh,ew]
    env_w = torch.cos(el) * torch.sin(el)
    axis = p[:, :3 * K].reshape(bn, K, 3, R, C)
    lamb = p[:, 3 * K:4 * K].reshape(bn, K, 1, R, C)
    weight = p[:, 4 * K:].reshape(bn, K, 3, R, C)
    if premap:
        lamb = torch.tan(math.pi / 2.0 * (lamb * 0.999))
        weight = torch.tan(math.pi / 2.0 * (weight * 0.999))
    cos = torch.einsum("bkdrc,dhw->bkrchw", axis, ls).unsqueeze(2)                   # [bn,K,1,R,C,eh,ew]
    mi = lamb[..., None, None] * (cos - 1)
    env = (weight[..., None, None] * torch.exp(mi)).sum(1)                           # [bn,3,R,C,eh,ew]
    return torch.clamp((env * env_w).reshape(bn, 3, R, C, -1).sum(-1), min=0.0)


# ---- testReal.py:421-432 --------------------------------------------------------------------------------------------------------------
def albedo_scale(dNew, d, sNew, s, albedo, dtype=torch.float64):
    """-> ``(cLight, cAlbedo, cDiff, cSpec), branch``: the sums and the maximum in ``dtype``, the branch and the clip in Python floats, as
    there.  ``branch`` is one of ``"nospec"``, ``"clip_lo"``, ``"clip_hi"``, ``"noclip"``."""
    dNew, d, sNew, s, albedo = [_t(x, dtype) for x in (dNew, d, sNew, s, albedo)]
    cDiff, cSpec = (dNew.sum() / d.sum()).item(), (sNew.sum() / s.sum()).item()
    inv_max = 1 / albedo.max().item()
    if cSpec < SPEC_FLOOR:
        cAlbedo, branch = inv_max, "nospec"
        cLight = cDiff / cAlbedo
    else:
        raw = cDiff / cSpec
        cAlbedo = min(max(raw, 1e-3), inv_max)
        branch = "clip_lo" if raw < 1e-3 else ("clip_hi" if raw > inv_max else "noclip")
        cLight = cDiff / cAlbedo
    return (cLight, cAlbedo, cDiff, cSpec), branch


# ---- wrapperBRDFLight.py:138-156 ------------------------------------------------------------------------------------------------------
def encoder_input(im, albedo, normal, rough, depth, size=(480, 640), dtype=torch.float64):
    """-> ``(input [bn,11,H,W], albedo_n, depth_n)``: mean-normalise albedo and depth per image (mean floored at 1e-10, then / 3),
    ``F.interpolate(.., mode="bilinear")`` of the five maps to ``size``, ``0.5 (x + 1)`` on normal and rough AFTER the resize."""
    im, albedo, normal, rough, depth = [_t(x, dtype) for x in (im, albedo, normal, rough, depth)]
    bn = im.shape[0]

    def norm(t):
        flat = t.reshape(bn, -1)
        return (flat / torch.clamp(flat.mean(dim=1), min=1e-10).unsqueeze(1) / 3.0).reshape(t.shape)
    albedo_n, depth_n = norm(albedo), norm(depth)
    up = lambda t: F.interpolate(t, [int(size[0]), int(size[1])], mode="bilinear")
    out = torch.cat([up(im), up(albedo_n), 0.5 * (up(normal) + 1), 0.5 * (up(rough) + 1), up(depth_n)], dim=1)
    return out, albedo_n, depth_n


# ---- models.py:7-21 -------------------------------------------------------------------------------------------------------------------
def lsregress_coef(pred, gt, dtype=torch.float64):
    """-> ``coef [bn]``, ``info``: ``clamp(<pred,gt> / max(<pred,pred>, 1e-5), 1e-3, 1e3)`` per image.  ``info``: ``den`` = <pred,pred>
    (against the 1e-5 floor) and ``raw`` = the quotient before the clamp."""
    pred, gt = _t(pred, dtype), _t(gt, dtype)
    nb = pred.shape[0]
    p, g = pred.reshape(nb, -1), gt.reshape(nb, -1)
    den = (p * p).sum(1)
    raw = (p * g).sum(1) / torch.clamp(den, min=SUM_FLOOR)
    return torch.clamp(raw, 1e-3, 1e3), dict(den=den, raw=raw)


# ---- models.py:23-84 ------------------------------------------------------------------------------------------------------------------
def diffspec_coef(diff, spec, im, dtype=torch.float64):
    """-> ``coef [bn,2]`` = ``coefIm * (coefDiffuse, coefSpecular)``, ``info``.  ``info``: the branch quantities ``det_over_n`` = frac / n
    (against 1e-2), ``a11`` and ``den2`` = the second regression's <rendered,rendered> (against 1e-5); and the factors ``cd``, ``cs``,
    ``cim`` with their values before the last clamp (``cd_raw``, ``cs_raw``, ``cim_raw``; ``c3_raw`` = the one-column quotient before its own)."""
    diff, spec, im = _t(diff, dtype), _t(spec, dtype), _t(im, dtype)
    nb = diff.shape[0]
    n = diff[0].numel()
    mask = (im < 0.9).to(dtype)
    d, s, i = (diff * mask).reshape(nb, -1), (spec * mask).reshape(nb, -1), (im * mask).reshape(nb, -1)
    a11, a22, a12 = (d * d).sum(1), (s * s).sum(1), (d * s).sum(1)
    b1, b2 = (d * i).sum(1), (s * i).sum(1)
    frac = a11 * a22 - a12 * a12
    c1 = (b1 * a22 - b2 * a12) / torch.clamp(frac, min=DET_FLOOR)
    c2 = (-b1 * a12 + a11 * b2) / torch.clamp(frac, min=DET_FLOOR)
    c3_raw = b1 / torch.clamp(a11, min=SUM_FLOOR)
    c3 = torch.clamp(c3_raw, 0.001, 1000)
    det_over_n = frac / n
    two = det_over_n > DET_FLOOR
    cd_raw, cs_raw = torch.where(two, c1, c3), torch.where(two, c2, torch.zeros_like(c2))
    cd, cs = torch.clamp(cd_raw, 0, 1000), torch.clamp(cs_raw, 0, 1000)
    v = lambda c: c.reshape(nb, 1, 1, 1)
    rendered = torch.clamp(v(cd) * diff + v(cs) * spec, 0, 1).reshape(nb, -1)
    den2 = (rendered * rendered).sum(1)
    cim_raw = (rendered * im.reshape(nb, -1)).sum(1) / torch.clamp(den2, min=SUM_FLOOR)
    cim = torch.clamp(cim_raw, 0.001, 1000)
    info = dict(det_over_n=det_over_n, a11=a11, den2=den2, two=two, cd=cd, cs=cs, cim=cim, cd_raw=cd_raw, cs_raw=cs_raw, c3_raw=c3_raw,
                cim_raw=cim_raw)
    return torch.stack([cim * cd, cim * cs], 1), info


# ---- the margin condition ---------------------------------------------------------------------------------------------------------------
def clear_of(q, threshold):
    """a branch quantity is at least a factor 2 from its threshold: at or above twice it, or at or below half of it (a quantity built to sit
    on a floor is a factor 2 inside it)"""
    q = float(q)
    return q >= 2.0 * threshold or q <= 0.5 * threshold


def diffspec_margins_ok(diff, spec, im):
    """every branch quantity of every image a factor 2 from its threshold in BOTH the fp32 and the fp64 evaluation, and both take the same
    branch.  -> (ok, report)"""
    ok, rep = True, []
    infos = [diffspec_coef(diff, spec, im, dt)[1] for dt in (torch.float32, torch.float64)]
    for b in range(infos[0]["a11"].numel()):
        for key, thr in (("det_over_n", DET_FLOOR), ("a11", SUM_FLOOR), ("den2", SUM_FLOOR)):
            q = [float(i[key][b]) for i in infos]
            good = all(clear_of(x, thr) for x in q) and (q[0] > thr) == (q[1] > thr)
            rep.append((b, key, q, good))
            ok = ok and good
    return ok, rep


def lsregress_margins_ok(pred, gt):
    q = [lsregress_coef(pred, gt, dt)[1]["den"] for dt in (torch.float32, torch.float64)]
    ok = all(clear_of(x, SUM_FLOOR) for t in q for x in t) and bool(((q[0] > SUM_FLOOR) == (q[1] > SUM_FLOOR)).all())
    return ok, [t.tolist() for t in q]


def albedo_scale_margins_ok(dNew, d, sNew, s, albedo):
    r = [albedo_scale(dNew, d, sNew, s, albedo, dt) for dt in (torch.float32, torch.float64)]
    ok = all(clear_of(x[0][3], SPEC_FLOOR) for x in r) and r[0][1] == r[1][1]
    return ok, [(x[0][3], x[1]) for x in r]


# ---- shared inputs of the CPU and the GPU tests (seeded; chosen so that the margin condition holds) ---------------------------------------
DIFFSPEC_BRANCH_CASES = ("regular", "spec_small", "spec_parallel", "cs_zero", "cd_1000", "all_masked")


def diffspec_case(kind, R, C, seed):
    """one image ``(diff, spec, im)`` [3,R,C] fp32 of the named branch case"""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(3, R, C, generator=g)
    diff, spec, im = r(), r(), 0.85 * r()
    if kind == "regular":
        pass
    elif kind == "spec_small":            # det / n far below 1e-2: the one-column fallback
        spec = 1e-3 * spec
    elif kind == "spec_parallel":         # det = 0 up to rounding
        spec = 0.5 * diff
    elif kind == "cs_zero":               # the specular coefficient comes out negative: clamped to 0
        im = torch.clamp(1.2 * diff - 0.5 * spec, 0, 1)
    elif kind in ("cd_1000", "a11_floor"):      # fallback with b1 / a11 above 1000; on a 1x1 image a11 is below its 1e-5 floor instead
        diff = 5e-4 * diff
    elif kind == "cd_0001":               # fallback with b1 / a11 below 0.001
        diff = 4000.0 * (diff + 1.0)
        spec = 1e-6 * spec
        im = 0.5 * r() + 0.2
    elif kind == "all_masked":            # every pixel at or above 0.9: all five sums are zero
        im = 0.9 + 0.1 * r()
    else:
        raise KeyError(kind)
    return diff.contiguous(), spec.contiguous(), im.contiguous()


def diffspec_raw_clear(info):
    """no factor sits within 10 % of a clamp it is not on (0 for cd / cs in the two-column branch, 0.001 and 1000 for c3 and c_im): a clamp
    the fp64 evaluation applies is then applied by any fp32 evaluation too"""
    ok = True
    for b in range(info["a11"].numel()):
        two = bool(info["two"][b])
        if two:
            ok = ok and abs(float(info["cd_raw"][b])) > 1e-3 and abs(float(info["cs_raw"][b])) > 1e-3
        for key in (("cd_raw", "cs_raw") if two else ("c3_raw",)) + ("cim_raw",):
            x = float(info[key][b])
            ok = ok and not (0.9e-3 < x < 1.1e-3) and not (900.0 < x < 1100.0)
    return ok


def diffspec_case_is(kind, info, b=0):
    """image ``b`` takes the path its case is named for"""
    two, cs, cd = bool(info["two"][b]), float(info["cs"][b]), float(info["cd"][b])
    lo = abs(cd - 0.001) < 1e-9                          # 0.001 as fp32 or as fp64
    return (two == (kind in ("regular", "cs_zero")) and (cs == 0.0) == (kind != "regular") and (cd == 1000.0) == (kind == "cd_1000")
            and lo == (kind in ("cd_0001", "all_masked")) and (float(info["a11"][b]) < SUM_FLOOR) == (kind in ("a11_floor", "all_masked")))


def diffspec_batch(kinds, R, C, seed):
    """``(diff, spec, im)`` [len(kinds),3,R,C]: a different case per image.  Each image's seed is the first of ``seed, seed + 1, ...`` at
    which the margin condition holds and the image takes the path it is named for, in fp32 and in fp64 -- chosen by this checker alone, never by the code under test."""
    parts = []
    for j, k in enumerate(kinds):
        for s in range(seed + 100 * j, seed + 100 * j + 100):
            one = [t.unsqueeze(0) for t in diffspec_case(k, R, C, s)]
            infos = [diffspec_coef(*one, dtype=dt)[1] for dt in (torch.float32, torch.float64)]
            if diffspec_margins_ok(*one)[0] and all(diffspec_raw_clear(i) and diffspec_case_is(k, i) for i in infos):
                break
        else:
            raise AssertionError(f"no seed in [{seed + 100 * j}, +100) gives {k} at {R}x{C} a factor 2 of margin")
        parts.append(diffspec_case(k, R, C, s))
    return tuple(torch.stack([p[i] for p in parts]) for i in range(3))


def lsregress_case(kind, n, seed):
    """one flat image ``(pred, gt)`` [n] fp32"""
    g = torch.Generator().manual_seed(seed)
    pred, gt = torch.rand(n, generator=g) + 0.1, torch.rand(n, generator=g) + 0.1
    if kind == "regular":
        pass
    elif kind == "clamp_lo":              # quotient below 0.001
        gt = 2e-5 * gt
    elif kind == "clamp_hi":              # quotient above 1000
        gt = 1e5 * gt
    elif kind == "floor":                 # <pred,pred> below 1e-5
        pred = pred * (1e-3 / math.sqrt(n))
        gt = gt * (1e-3 / math.sqrt(n))
    else:
        raise KeyError(kind)
    return pred, gt


# ---- the checker-driven cases of tests/test_gpu_light_glue.py; tests/test_light_glue_checker.py asserts the margin condition on each ----
# (kinds of the three images, R, C, base seed): a different case per image, so that a per-image fold reading a neighbour's partials shows
DIFFSPEC_BATCHES = [
    (("regular", "spec_small", "spec_parallel"), 12, 16, 1000), (("cs_zero", "cd_1000", "all_masked"), 12, 16, 1300),
    (("cd_0001", "regular", "cs_zero"), 12, 16, 1600),
    (("regular", "spec_small", "spec_parallel"), 1, 1, 2000), (("cs_zero", "a11_floor", "all_masked"), 1, 1, 2300),
    # tails either side of one round of the first pass (64 x 256 = 16 384 elements) and of the second (16 x 256 x 16 = 65 536)
    (("regular", "cs_zero", "spec_small"), 5, 7, 3000), (("cs_zero", "all_masked", "regular"), 73, 75, 3300),
    (("regular", "spec_parallel", "cs_zero"), 74, 74, 3600), (("cd_1000", "regular", "cs_zero"), 120, 160, 3900),
    (("regular", "cs_zero", "all_masked"), 148, 148, 4200),
]
LSREGRESS_SIZES = (1, 255, 256, 4096, 4097, 8193)
LSREGRESS_BATCHES = [(("regular", "clamp_lo", "clamp_hi"), n, 5000 + n) for n in LSREGRESS_SIZES] + [(("floor", "regular", "floor"), 576, 5900)]


def lsregress_batch(kinds, n, seed):
    parts = [lsregress_case(k, n, seed + 31 * j) for j, k in enumerate(kinds)]
    return torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])


SCALE_BRANCHES = dict(nospec=(0.75, 2.5e-4), clip_lo=(1e-3, 4.0), clip_hi=(2.0, 0.5), noclip=(0.3, 1.5))      # (cDiff, cSpec) aimed at
# (n, where the albedo maximum sits, branch); n_albedo = 4 n.  "second": an index only the second step of the grid-stride loop reaches
SCALE_CASES = [(16384, "first", "noclip"), (16385, "last", "clip_hi"), (16428, "second", "clip_hi"), (57600, "second", "nospec"),
               (57600, "last", "clip_lo"), (16385, "first", "nospec"), (576, "negative", "noclip"), (576, "negative", "nospec")]


def scale_case(n, where, branch, seed):
    """``(dNew, d, sNew, s, albedo)`` flat fp32.  The scaled images are NOT multiples of the unscaled ones: a ratio of two sums over the
    same wrong index set would otherwise come out right."""
    g = torch.Generator().manual_seed(seed)
    r = lambda m: torch.rand(m, generator=g) + 0.25
    cd, cs = SCALE_BRANCHES[branch]
    d, s, dNew, sNew = r(n), r(n), cd * r(n), cs * r(n)
    albedo = 0.5 * torch.rand(4 * n, generator=g)
    if where == "negative":
        albedo = -(albedo + 0.5)
    else:
        albedo[dict(first=0, last=4 * n - 1, second=64 * 256 + 4 * n // 2)[where]] = 0.8125
    return dNew, d, sNew, s, albedo
