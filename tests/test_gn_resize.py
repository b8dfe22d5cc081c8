"""CPU: the decoders' resize-to-skip stage (GroupNorm + ReLU + bilinear resize + skip concat + 2x upsample; the final stage's resize)
without a GPU.

  * tests/gn_resize_checker.py (the contract of DESIGN.md section 8e in torch, own code) is pinned at 1e-12, in fp64, to the fixtures the
    UNMODIFIED reference produced (tests/golden/g19_gnresize_*.npz, tools/make_golden_gn_resize.py) and to ``F.interpolate`` composed as the
    reference composes it; run in fp32 it forms ``scale`` in fp32 and lands where torch's fp32 run lands;
  * the fixtures hold what they were made for (the conditions of g17, re-asserted from the stored arrays, and the size cap);
  * ``torch.ops.sgrender.gn_resize`` / ``gn_resize_bwd`` are registered by the C++ extension with Meta kernels of the documented shapes, and
    the autograd graph gives a gradient exactly where one is required, for both forms and every subset of ``requires_grad``;
  * the wrapper, the module and the C ABI refuse what the contract refuses, before anything is dereferenced;
  * the kernels' per-element arithmetic (csrc/sgr_gn_stage.h compiled for the host, tests/host_emul/gn_resize_emul.cpp) stays within the
    GPU tests' bounds on every fixture, and the adjoint's window holds every resized index that names a source index, on axes 1 .. 12 at
    every target size of the domain and at the sizes of the GPU tests."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import gn_resize_checker as R
import gn_stage_checker as C
from conftest import GOLDEN_DIR, ROOT

import inverserenderingofindoorscene_amd as sgr
from inverserenderingofindoorscene_amd import _lib

# name -> parts: (part, B, C, G, H, W, Hs, Ws, Cs)
CASES = {
    "h1": [("s", 2, 64, 4, 5, 8, 6, 8, 64)],
    "hw": [("s", 3, 64, 4, 3, 5, 4, 6, 64)],
    "dbl": [("s", 1, 64, 4, 2, 3, 4, 6, 64)],
    "one": [("w", 2, 128, 8, 1, 1, 1, 2, 128), ("hw", 2, 128, 8, 1, 1, 2, 2, 128)],
    "fin": [("d0", 2, 64, 4, 6, 9, 7, 10, 0), ("dl", 2, 128, 8, 2, 4, 3, 4, 0)],
}
PARTS = [(name, spec) for name, specs in CASES.items() for spec in specs]
IDS = [f"{name}-{spec[0]}" for name, spec in PARTS]
GRADS = ("dx", "dw", "db", "ds")
PIN = 1e-12
FP = ctypes.POINTER(ctypes.c_float)


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g19_gnresize_{name}.npz"))


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


def value_bound(e_ref):
    return max(2.0 * float(e_ref), 1e-6)


def grad_bound(e_ref):
    return max(4.0 * float(e_ref), 1e-6)


def part_arrays(z, part):
    get = lambda k: z[f"{part}_{k}"] if f"{part}_{k}" in z.files else None
    return get("x"), get("weight"), get("bias"), int(z[f"{part}_G"]), tuple(int(v) for v in z[f"{part}_size"]), get("skip"), get("ct")


@pytest.mark.parametrize("name,spec", PARTS, ids=IDS)
def test_checker_is_pinned_to_the_reference_fixture(name, spec):
    z = load(name)
    part = spec[0]
    x, w, b, G, size, skip, ct = part_arrays(z, part)
    t64 = lambda a: None if a is None else torch.from_numpy(a).double()
    y, grads = R.gn_resize(t64(x), t64(w), t64(b), G, size, t64(skip), cotangent=t64(ct))
    assert err(y, z[f"{part}_y64"]) <= PIN, (name, part, err(y, z[f"{part}_y64"]))
    for k, g in zip(GRADS, grads):
        if g is None:
            assert k == "ds" and skip is None and f"{part}_ds64" not in z.files
            continue
        assert err(g, z[f"{part}_{k}64"]) <= PIN, (name, part, k, err(g, z[f"{part}_{k}64"]))
    assert np.array_equal(grads[0].numpy() == 0, z[f"{part}_dx64"] == 0)
    assert err(R.reference_lines(t64(x), t64(w), t64(b), G, size, t64(skip)), z[f"{part}_y64"]) <= PIN


# (B, C, G, H, W, Hs, Ws, Cs): the training sizes, the corners of the domain, one axis equal, a testReal-like size (at 1x1 sixteen channels
# per group: with two elements in a group dx is zero in exact arithmetic and a relative error means nothing)
SHAPES = [(1, 8, 2, 14, 20, 15, 20, 3), (1, 8, 2, 6, 10, 7, 10, 3), (2, 32, 2, 1, 1, 1, 2, 2), (1, 32, 2, 1, 1, 2, 2, 0), (1, 4, 1, 33, 41, 66, 82, 1),
          (1, 2, 1, 106, 160, 107, 160, 0), (1, 4, 2, 7, 10, 7, 11, 2), (1, 4, 2, 5, 9, 9, 17, 0), (1, 4, 2, 3, 5, 4, 6, 3), (1, 2, 1, 30, 41, 31, 41, 2),
          (1, 2, 1, 12, 7, 13, 14, 0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_checker_is_torchs_own_composition_with_its_gradients(shape):
    """values and all four gradients against autograd through F.interpolate composed as the reference composes it: 1e-12 in fp64; in fp32,
    where the checker forms `scale` in fp32 as torch does, within a few fp32 roundings (1e-6) of torch's fp32 run"""
    B, Cc, G, H, W, Hs, Ws, Cs = shape
    g = torch.Generator().manual_seed(1900 + H * W)
    x = torch.randn(B, Cc, H, W, generator=g, dtype=torch.float64)
    w, b = torch.randn(Cc, generator=g, dtype=torch.float64), torch.randn(Cc, generator=g, dtype=torch.float64)
    skip = torch.randn(B, Cs, Hs, Ws, generator=g, dtype=torch.float64) if Cs else None
    ct = torch.randn(B, Cc + Cs, 2 * Hs, 2 * Ws, generator=g, dtype=torch.float64) if Cs else torch.randn(B, Cc, Hs, Ws, generator=g, dtype=torch.float64)
    for dtype, tol in ((torch.float64, PIN), (torch.float32, 1e-6)):
        cast = lambda t: None if t is None else t.to(dtype)
        leaves = [cast(t).clone().requires_grad_(True) if t is not None else None for t in (x, w, b, skip)]
        y = R.reference_lines(leaves[0], leaves[1], leaves[2], G, (Hs, Ws), leaves[3])
        want = torch.autograd.grad(y, [t for t in leaves if t is not None], grad_outputs=cast(ct))
        got_y, got = R.gn_resize(cast(x), cast(w), cast(b), G, (Hs, Ws), cast(skip), cotangent=cast(ct))
        y = y.detach()
        assert err(got_y, y) <= tol, (dtype, err(got_y, y))
        for k, a, c in zip(GRADS, got, want):
            assert err(a, c) <= tol, (dtype, k, err(a, c))


def test_inside_the_domain_a_source_index_is_referenced_by_at_most_four():
    """what keeps the adjoint a bounded gather (the dense restatement of the issue)"""
    for n in list(range(1, 41)) + [106, 160, 212, 320]:
        for ns in range(n, 2 * n + 1):
            assert R.max_fan_in(n, ns) <= 4, (n, ns)
    assert R.max_fan_in(4, 13) > 4      # and outside it is not


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_conditions(name):
    z = load(name)
    assert os.path.getsize(os.path.join(GOLDEN_DIR, f"g19_gnresize_{name}.npz")) <= 1 << 20
    assert list(z["parts"]) == [s[0] for s in CASES[name]]
    for part, B, Cc, G, H, W, Hs, Ws, Cs in CASES[name]:
        x, w, b, g, size, skip, ct = part_arrays(z, part)
        assert tuple(x.shape) == (B, Cc, H, W) and x.dtype == np.float32 and g == G and w.shape == (Cc,) and b.shape == (Cc,) and size == (Hs, Ws)
        assert (Hs, Ws) != (H, W) and H <= Hs <= 2 * H and W <= Ws <= 2 * W      # the reference's `if` fired, inside the domain
        out_shape = (B, Cc + Cs, 2 * Hs, 2 * Ws) if Cs else (B, Cc, Hs, Ws)
        assert (skip is None) == (Cs == 0) and (skip is None or tuple(skip.shape) == (B, Cs, Hs, Ws))
        assert tuple(ct.shape) == out_shape and z[f"{part}_y64"].shape == out_shape and z[f"{part}_y32"].shape == out_shape
        assert z[f"{part}_y64"].dtype == np.float64 and z[f"{part}_y32"].dtype == np.float32
        assert z[f"{part}_dx64"].shape == x.shape and z[f"{part}_dw64"].shape == (Cc,) and z[f"{part}_db64"].shape == (Cc,)
        assert (f"{part}_ds64" in z.files) == (Cs > 0)
        pre, _, _ = C.pre_relu(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), G)
        assert float(pre.abs().min()) >= 1e-5, (name, part)                                   # a 1-ulp difference cannot flip a branch
        assert 0.30 <= float((pre > 0).double().mean()) <= 0.70, (name, part)
        assert np.array_equal(z[f"{part}_dx32"] == 0, z[f"{part}_dx64"] == 0), (name, part)    # both runs took the same branches
        assert int((w < 0).sum()) >= 4 and int((w == 0).sum()) == 1                           # negative scales, one exact zero
        for k in z.files:
            if k.startswith(part + "_") and z[k].dtype.kind == "f":
                assert np.isfinite(z[k]).all(), (name, k)
        # skip and cotangent come from dyadic grids (the files compress; dskip is exact in both precisions)
        assert np.array_equal(ct * 4, np.round(ct * 4)) and (skip is None or np.array_equal(skip * 16, np.round(skip * 16)))
        e = err(z[f"{part}_y32"], z[f"{part}_y64"])
        assert abs(float(z[f"{part}_e_ref_y"]) - e) <= 1e-12 + 1e-9 * e
        assert 0 < float(z[f"{part}_e_ref_y"]) < 1e-6 and 0 < float(z[f"{part}_e_ref_dx"]) < 2e-6


def m(*shape, grad=False):
    return torch.empty(*shape, device="meta", requires_grad=grad)


def test_operators_are_registered_with_meta_shapes_and_the_autograd_graph():
    ops = torch.ops.sgrender
    assert str(ops.gn_resize.default._schema).startswith(
        "sgrender::gn_resize(Tensor x, Tensor weight, Tensor bias, Tensor? skip, int num_groups, int out_h, int out_w, float eps=")
    assert str(ops.gn_resize_bwd.default._schema).startswith(
        "sgrender::gn_resize_bwd(Tensor g, Tensor? x, Tensor? weight, Tensor? bias, Tensor? stats, int channels, int skip_channels, int num_groups, int height, int width")
    for name in ("gn_resize", "gn_resize_bwd"):
        for key in ("Meta", "CUDA"):      # registered from C++ (TORCH_LIBRARY), not by a Python torch.library.custom_op
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sgrender::{name}", key), (name, key)
    B, Cc, G, H, W, Hs, Ws, Cs = 3, 12, 4, 5, 7, 6, 7, 5
    for with_skip in (False, True):
        for need in itertools.product((False, True), repeat=4 if with_skip else 3):
            x, w, b = m(B, Cc, H, W, grad=need[0]), m(Cc, grad=need[1]), m(Cc, grad=need[2])
            skip = m(B, Cs, Hs, Ws, grad=need[3]) if with_skip else None
            y = sgr.group_norm_relu_resize_upcat(x, w, b, G, skip) if with_skip else sgr.group_norm_relu_resize(x, w, b, G, (Hs, Ws))
            assert tuple(y.shape) == ((B, Cc + Cs, 2 * Hs, 2 * Ws) if with_skip else (B, Cc, Hs, Ws)) and y.dtype == torch.float32 and y.is_contiguous()
            assert y.requires_grad == any(need), (with_skip, need)
            leaves = [t for t, n in zip((x, w, b, skip), need) if n]
            if leaves:
                gs = torch.autograd.grad(y.sum(), leaves)
                assert [tuple(g.shape) for g in gs] == [tuple(t.shape) for t in leaves]
            # the backward operator itself: a gradient only where wanted, a [0] tensor elsewhere
            if any(need):
                full = need if with_skip else need + (False,)
                side = any(full[:3])
                gx = ops.gn_resize_bwd(m(*y.shape), x.detach() if side else None, w.detach() if side else None, b.detach() if side else None,
                                       m(B, G, 4) if side else None, Cc, Cs if with_skip else 0, G, H, W, *full)
                want = [(B, Cc, H, W), (Cc,), (Cc,), (B, Cs, Hs, Ws)]
                assert [tuple(g.shape) for g in gx] == [s if n else (0,) for s, n in zip(want, full)]
    # channels-last inputs give contiguous outputs; the statistics are [B,G,4]
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    y, stats = ops.gn_resize(cl(m(B, Cc, H, W)), m(Cc), m(Cc), cl(m(B, Cs, Hs, Ws)), G, Hs, Ws, 1e-5)
    assert y.is_contiguous() and tuple(stats.shape) == (B, G, 4)
    with torch.no_grad():
        assert not sgr.group_norm_relu_resize(m(B, Cc, H, W, grad=True), m(Cc), m(Cc), G, (Hs, Ws)).requires_grad
    # equal sizes are the existing operator's shapes
    assert tuple(sgr.group_norm_relu_resize_upcat(m(B, Cc, H, W), m(Cc), m(Cc), G, m(B, Cs, H, W)).shape) == (B, Cc + Cs, 2 * H, 2 * W)
    assert tuple(sgr.group_norm_relu_resize(m(B, Cc, H, W), m(Cc), m(Cc), G, (H, W)).shape) == (B, Cc, H, W)


def test_the_modules_resize_flag_both_ways():
    assert {"group_norm_relu_resize", "group_norm_relu_resize_upcat"} <= set(sgr.__all__)
    plain, flagged = sgr.GroupNormReLU(4, 12).to("meta"), sgr.GroupNormReLU(4, 12, resize=True).to("meta")
    assert not plain.resize and flagged.resize and "resize=True" in repr(flagged) and "resize" not in repr(plain)
    assert [k for k, _ in flagged.named_parameters()] == ["weight", "bias"]
    # the default still refuses a skip of another size, with the message tests/test_gn_stage.py pins
    with pytest.raises(RuntimeError, match=r"skip is 4x5 but x is 3x5.*models\.py:165-166"):
        plain(m(2, 12, 3, 5), m(2, 7, 4, 5))
    with pytest.raises(RuntimeError, match="size= is the final-stage form of resize=True"):
        plain(m(2, 12, 3, 5), size=(4, 5))
    with pytest.raises(RuntimeError, match="takes no skip"):
        flagged(m(2, 12, 3, 5), m(2, 7, 4, 5), size=(4, 5))
    assert tuple(flagged(m(2, 12, 3, 5), m(2, 7, 4, 5)).shape) == (2, 19, 8, 10)
    assert tuple(flagged(m(2, 12, 3, 5), m(2, 7, 3, 5)).shape) == (2, 19, 6, 10)
    assert tuple(flagged(m(2, 12, 3, 5), size=(4, 6)).shape) == (2, 12, 4, 6)
    assert tuple(flagged(m(2, 12, 3, 5)).shape) == (2, 12, 3, 5) and tuple(plain(m(2, 12, 3, 5), m(2, 7, 3, 5)).shape) == (2, 19, 6, 10)


def test_refusals():
    z = torch.zeros
    up, rs = sgr.group_norm_relu_resize_upcat, sgr.group_norm_relu_resize
    with pytest.raises(RuntimeError, match="no CPU path"):
        rs(z(2, 8, 3, 5), z(8), z(8), 2, (4, 5))
    with pytest.raises(RuntimeError, match="no CPU path"):
        up(z(2, 8, 3, 5, requires_grad=True), z(8), z(8), 2, z(2, 4, 4, 5))
    with pytest.raises(RuntimeError, match="no CPU path"):      # equal sizes: the existing operator's refusal
        up(z(2, 8, 3, 5), z(8), z(8), 2, z(2, 4, 3, 5))
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.sgrender.gn_resize_bwd(z(2, 8, 4, 5), z(2, 8, 3, 5), z(8), z(8), z(2, 2, 4), 8, 0, 2, 3, 5, True, False, False, False)
    # the domain, below and above on each axis; the message names the torch composition
    for hs, ws in ((2, 5), (7, 5), (3, 4), (3, 11), (7, 11), (2, 4)):
        with pytest.raises(RuntimeError, match=rf"the target {hs}x{ws} is outside the resize domain of x 3x5.*F\.interpolate\(\., \[h, w\], mode='bilinear'\), torch\.cat"):
            up(m(2, 8, 3, 5), m(8), m(8), 2, m(2, 4, hs, ws))
        with pytest.raises(RuntimeError, match=rf"the target {hs}x{ws} is outside the resize domain"):
            rs(m(2, 8, 3, 5), m(8), m(8), 2, (hs, ws))
    for hs, ws in ((6, 10), (3, 10), (6, 5), (4, 5), (3, 6)):      # the corners and the edges of the domain are inside
        assert tuple(rs(m(2, 8, 3, 5), m(8), m(8), 2, (hs, ws)).shape) == (2, 8, hs, ws)
    with pytest.raises(RuntimeError, match="target size must be positive"):
        rs(m(2, 8, 3, 5), m(8), m(8), 2, (0, 5))
    with pytest.raises(RuntimeError, match="fp32 tensors required"):
        rs(m(2, 8, 3, 5).half(), m(8).half(), m(8).half(), 2, (4, 5))
    with pytest.raises(RuntimeError, match="fp32 tensors required"):
        up(m(2, 8, 3, 5), m(8), m(8), 2, m(2, 4, 4, 5).half())
    with pytest.raises(RuntimeError, match="skip is None"):
        up(m(2, 8, 3, 5), m(8), m(8), 2, None)
    with pytest.raises(RuntimeError, match=r"skip must be \[2,Cs,4,5\]"):      # a batch mismatch
        up(m(2, 8, 3, 5), m(8), m(8), 2, m(3, 4, 4, 5))
    with pytest.raises(RuntimeError, match="not a multiple of num_groups 3"):
        rs(m(2, 8, 3, 5), m(8), m(8), 3, (4, 5))
    with pytest.raises(RuntimeError, match=r"weight and bias must be \[8\]"):
        rs(m(2, 8, 3, 5), m(4), m(8), 2, (4, 5))
    with pytest.raises(RuntimeError, match="zero-sized"):
        rs(m(0, 8, 3, 5), m(8), m(8), 2, (4, 5))
    bwd = torch.ops.sgrender.gn_resize_bwd
    with pytest.raises(RuntimeError, match="no gradient requested"):
        bwd(m(2, 8, 4, 5), None, None, None, None, 8, 0, 2, 3, 5, False, False, False, False)
    with pytest.raises(RuntimeError, match="without skip channels"):
        bwd(m(2, 8, 4, 5), None, None, None, None, 8, 0, 2, 3, 5, False, False, False, True)
    with pytest.raises(RuntimeError, match="cotangent must be fp32"):
        bwd(m(2, 9, 8, 10), None, None, None, None, 8, 4, 2, 3, 5, False, False, False, True)
    with pytest.raises(RuntimeError, match="outside the resize domain"):
        bwd(m(2, 12, 14, 10), None, None, None, None, 8, 4, 2, 3, 5, False, False, False, True)


def test_c_abi_refusals_without_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused before a launch
    strides = (ctypes.c_longlong * 4)(120, 15, 5, 1)
    eps = ctypes.c_float(1e-5)
    sizes = dict(B=2, C=8, G=2, Cs=4, H=3, W=5, Hs=4, Ws=5)

    def fwd(x=fake, w=fake, b=fake, skip=fake, out=fake, stats=fake, ws=fake, xs=strides, ss=strides, **kw):
        s = {**sizes, **kw}
        return lib.sgr_gn_resize_fwd(x, w, b, skip, out, stats, ws, s["B"], s["C"], s["G"], s["Cs"], s["H"], s["W"], s["Hs"], s["Ws"], xs, ss, eps, None)

    def bwd(g=fake, x=fake, w=fake, b=fake, stats=fake, dx=fake, dw=fake, db=fake, ds=fake, ws=fake, xs=strides, **kw):
        s = {**sizes, **kw}
        return lib.sgr_gn_resize_bwd(g, x, w, b, stats, dx, dw, db, ds, ws, s["B"], s["C"], s["G"], s["Cs"], s["H"], s["W"], s["Hs"], s["Ws"], xs, None)
    q = lib.sgr_gn_resize_workspace_floats
    for k in ("x", "w", "b", "out", "stats", "ws", "xs"):
        assert fwd(**{k: None}) == -1 and b"NULL tensor" in lib.sgr_last_error(), k
    assert fwd(skip=None) == -1 and b"do not agree" in lib.sgr_last_error()
    assert fwd(Cs=0) == -1 and b"do not agree" in lib.sgr_last_error()
    assert fwd(ss=None) == -1 and b"do not agree" in lib.sgr_last_error()
    assert bwd(g=None) == -1 and b"NULL cotangent" in lib.sgr_last_error()
    assert bwd(dx=None, dw=None, db=None, ds=None) == -1 and b"no gradient requested" in lib.sgr_last_error()
    for k in ("x", "w", "b", "stats", "ws", "xs"):
        assert bwd(**{k: None}) == -1 and b"NULL tensor" in lib.sgr_last_error(), k
    assert bwd(Cs=0) == -1 and b"dskip requested without skip channels" in lib.sgr_last_error()
    for k in ("B", "C", "G", "H", "W", "Hs", "Ws"):      # each size in turn, zero and negative
        for bad in (0, -3):
            assert fwd(**{k: bad}) == -1 and b"non-positive" in lib.sgr_last_error(), (k, bad)
            assert bwd(**{k: bad}) == -1 and b"non-positive" in lib.sgr_last_error(), (k, bad)
            args = dict(B=2, C=8, G=2, H=3, W=5, Hs=4, Ws=5, upcat=1, backward=1)
            args[k] = bad
            assert q(*args.values()) == 0
    assert fwd(G=3) == -1 and b"not a multiple of num_groups" in lib.sgr_last_error()
    assert bwd(G=3) == -1 and b"not a multiple of num_groups" in lib.sgr_last_error()
    for hs, ws in ((2, 5), (7, 5), (4, 4), (4, 11)):      # below and above the domain on each axis
        assert fwd(Hs=hs, Ws=ws) == -2 and b"outside the resize domain" in lib.sgr_last_error(), (hs, ws)
        assert bwd(Hs=hs, Ws=ws) == -2 and b"outside the resize domain" in lib.sgr_last_error(), (hs, ws)
        assert q(2, 8, 2, 3, 5, hs, ws, 1, 1) == 0
    assert fwd(B=65536) == -2 and b"65535" in lib.sgr_last_error()
    assert bwd(C=65535, G=1) == -2 and b"65535" in lib.sgr_last_error()
    neg = (ctypes.c_longlong * 4)(120, 15, -5, 1)      # a plane is indexed with 32-bit offsets: no negative strides
    assert fwd(xs=neg) == -2 and b"plane strides" in lib.sgr_last_error()
    assert fwd(ss=neg) == -2 and b"plane strides" in lib.sgr_last_error()
    assert bwd(xs=neg) == -2 and b"plane strides" in lib.sgr_last_error()
    # the workspace query: the forward's partials; the backward's partials, coefficients, the masked adjoint at the source resolution and,
    # with a skip, the upsample's adjoint at the skip's
    assert q(2, 8, 2, 3, 5, 4, 5, 1, 0) == 4 * 2 * 2 and q(2, 8, 2, 3, 5, 4, 5, 0, 0) == 4 * 2 * 2
    assert q(2, 8, 2, 3, 5, 4, 5, 0, 1) == 4 * 2 * 8 + 8 + 2 * 8 * 15 and q(2, 8, 2, 3, 5, 4, 5, 1, 1) == 4 * 2 * 8 + 8 + 2 * 8 * 15 + 2 * 8 * 20
    assert q(2, 8, 2, 3, 5, 3, 5, 1, 1) > 0 and q(2, 8, 2, 3, 5, 6, 10, 1, 1) > 0      # equal sizes and the top corner are inside
    assert _lib.ABI_VERSION == 6 and lib.sgr_abi_version() == 6      # additive: the version did not move


@pytest.fixture(scope="module")
def emul():
    d = os.path.join(ROOT, "tests", "host_emul")
    so, src = os.path.join(d, "libgn_resize_emul.so"), os.path.join(d, "gn_resize_emul.cpp")
    hdrs = [os.path.join(ROOT, "inverserenderingofindoorscene_amd", "csrc", h) for h in ("sgr_gn_stage.h", "sgr_regress.h", "sgr_math.h")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", so])
    return ctypes.CDLL(so)


def _p(a):
    return None if a is None else a.ctypes.data_as(FP)


def test_the_adjoints_window_holds_every_index_that_names_a_source(emul):
    """the backward gathers over six consecutive resized indices starting at a rounded bound (csrc/sgr_gn_stage.h: rs_adj_first,
    rs_adj_weights): no tap of the rule falls outside its source's window, the window's weights add up to the rule's column sum and at most
    four are non-zero -- on axes 1 .. 12 and at the GPU tests' sizes, for every target size of the domain"""
    for n in list(range(1, 13)) + [14, 20, 33, 41, 106, 160, 212, 320]:
        for ns in range(n, 2 * n + 1):
            assert emul.emul_rs_window_mismatch(n, ns) == 0, (n, ns)


@pytest.mark.parametrize("name,spec", PARTS, ids=IDS)
def test_the_kernels_arithmetic_on_the_host_stays_within_the_gpu_bounds(emul, name, spec):
    z = load(name)
    part, B, Cc, G, H, W, Hs, Ws, Cs = spec
    x, w, b, _, _, skip, ct = part_arrays(z, part)
    out = np.full_like(z[f"{part}_y32"], np.nan)
    stats = np.empty((B, G, 4), np.float32)
    emul.emul_gn_resize_fwd(_p(x), _p(w), _p(b), _p(skip), _p(out), _p(stats), B, Cc, G, Cs, H, W, Hs, Ws, ctypes.c_float(1e-5))
    dx, dw, db = np.full_like(x, np.nan), np.full_like(w, np.nan), np.full_like(b, np.nan)
    ds = np.full_like(skip, np.nan) if Cs else None
    emul.emul_gn_resize_bwd(_p(ct), _p(x), _p(w), _p(b), _p(stats), _p(dx), _p(dw), _p(db), _p(ds), B, Cc, G, Cs, H, W, Hs, Ws)
    e, lim = err(out, z[f"{part}_y64"]), value_bound(z[f"{part}_e_ref_y"])
    print(f"{name} {part}: values {e:.2e} (bound {lim:.1e})")
    assert np.isfinite(out).all() and e <= lim, (name, part, e, lim)
    for k, g in zip(GRADS, (dx, dw, db, ds)):
        if g is None:
            continue
        e, lim = err(g, z[f"{part}_{k}64"]), grad_bound(z[f"{part}_e_ref_{k}"])
        print(f"{name} {part}: {k} {e:.2e} (bound {lim:.1e})")
        assert np.isfinite(g).all() and e <= lim, (name, part, k, e, lim)
    assert np.array_equal(dx == 0, z[f"{part}_dx64"] == 0)
