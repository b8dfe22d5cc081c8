"""CPU: the BRDF decoders' final pad + 3x3 convolution (sgr.final_conv / sgr.group_norm_relu_final_conv / sgr.FinalConv) without a GPU.

  * tests/final_conv_checker.py (the contract of DESIGN.md section 8g in torch, explicit index arithmetic) is pinned at 1e-12, in fp64, to the
    fixtures the UNMODIFIED reference produced (tests/golden/g20_finalconv_*.npz, tools/make_golden_final_conv.py) and to torch's own
    ``F.pad`` + ``F.conv2d`` + ``F.group_norm`` under autograd at a dozen shapes with ``H`` or ``W`` in {1, 2, 3};
  * ``R_n(h)`` has exactly three pairs and is the exact preimage of ``h``, exhaustively for ``n = 1..6`` -- the checker's and the kernels';
  * the fixtures hold what they were made for;
  * ``torch.ops.sgrender.final_conv`` / ``final_conv_bwd`` are registered by the C++ extension with Meta kernels of the documented shapes, and
    the autograd graph gives a gradient exactly where one is required, for both forms and every subset of ``requires_grad``;
  * the fused node keeps ``x``, the parameters and the statistics: no second tensor of ``y``'s shape;
  * the wrapper, the operators and the C ABI refuse what the contract refuses, before anything is dereferenced;
  * the kernels' arithmetic (csrc/sgr_final_conv.h compiled for the host, tests/host_emul/final_conv_emul.cpp) stays within HALF of every
    bound of tests/test_gpu_final_conv.py on every fixture."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import final_conv_checker as C
from conftest import GOLDEN_DIR, ROOT

import inverserenderingofindoorscene_amd as sgr
from inverserenderingofindoorscene_amd import _lib

# name -> (B, C, G, H, W); G = 0: the plain form
CASES = {"vec": (2, 64, 4, 6, 10), "odd": (3, 64, 4, 5, 7), "one": (1, 64, 4, 1, 1), "row": (2, 64, 4, 1, 9), "col": (1, 64, 4, 7, 1),
         "two": (1, 64, 4, 2, 2), "plain": (2, 64, 0, 4, 6)}
FUSED_GRADS = ("dx", "dgw", "dgb", "dW", "db")
PLAIN_GRADS = ("dy", None, None, "dW", "db")
PIN = 1e-12
FP = ctypes.POINTER(ctypes.c_float)


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g20_finalconv_{name}.npz"))


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


def value_bound(e_ref):
    return max(2.0 * float(e_ref), 1e-6)


def grad_bound(e_ref):
    return max(4.0 * float(e_ref), 1e-6)


def t64(a):
    return torch.from_numpy(np.asarray(a)).double()


def fixture_args(z, dtype=torch.float64):
    """-> (x, Wt, bias, gn or None, ct, grad names)"""
    t = lambda k: torch.from_numpy(z[k]).to(dtype)
    if "x" in z.files:
        return t("x"), t("Wt"), t("bias"), (t("gn_weight"), t("gn_bias"), int(z["G"]), 1e-5), t("ct"), FUSED_GRADS
    return t("y"), t("Wt"), t("bias"), None, t("ct"), PLAIN_GRADS


@pytest.mark.parametrize("name", list(CASES))
def test_checker_is_pinned_to_the_reference_fixture(name):
    z = load(name)
    x, Wt, bias, gn, ct, names = fixture_args(z)
    for fn in (C.final_conv, C.composition):
        out, grads = fn(x, Wt, bias, gn, cotangent=ct)
        assert err(out, z["out64"]) <= PIN, (name, fn.__name__, err(out, z["out64"]))
        for k, g in zip(names, grads):
            assert (k is None) == (g is None)
            if k is not None:
                assert err(g, z[f"{k}64"]) <= PIN, (name, fn.__name__, k, err(g, z[f"{k}64"]))
    if gn is not None:
        assert np.array_equal(C.final_conv(x, Wt, bias, gn, cotangent=ct)[1][0].numpy() == 0, z["dx64"] == 0)


SHAPES = [(2, 5, 1, 1, 1), (2, 6, 2, 1, 2), (1, 4, 2, 2, 1), (2, 6, 3, 2, 2), (1, 8, 2, 3, 3), (2, 4, 1, 1, 7), (2, 4, 4, 6, 1), (1, 6, 2, 2, 5), (1, 6, 3, 5, 2),
          (2, 3, 1, 3, 8), (1, 9, 3, 4, 3), (2, 7, 7, 6, 9)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_checker_equals_torchs_own_composition_under_autograd(shape):
    B, Cc, G, H, W = shape
    g = torch.Generator().manual_seed(2100 + 10 * H + W)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, Wt, bias, ct = r(B, Cc, H, W), r(3, Cc, 3, 3), r(3), r(B, 3, H, W)
    for gn in (None, (r(Cc), r(Cc), G, 1e-5)):
        a, ga = C.final_conv(x, Wt, bias, gn, cotangent=ct)
        b, gb = C.composition(x, Wt, bias, gn, cotangent=ct)
        assert err(a, b) <= PIN
        for p, q in zip(ga, gb):
            assert (p is None and q is None) or err(p, q) <= PIN, (shape, gn is None, err(p, q))


@pytest.fixture(scope="module")
def emul():
    d = os.path.join(ROOT, "tests", "host_emul")
    so, src = os.path.join(d, "libfinal_conv_emul.so"), os.path.join(d, "final_conv_emul.cpp")
    hdrs = [os.path.join(ROOT, "inverserenderingofindoorscene_amd", "csrc", h) for h in ("sgr_final_conv.h", "sgr_gn_stage.h", "sgr_regress.h", "sgr_math.h")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", so])
    return ctypes.CDLL(so)


def test_the_pairs_are_exactly_three_and_the_exact_preimage(emul):
    for n in range(1, 7):
        seen = set()
        for h in range(n):
            ps = C.pairs(h, n)
            assert len(ps) == 3 == len(set(ps)), (n, h, ps)
            assert all(0 <= i < n and k in (0, 1, 2) and C.cl(i + k - 1, n) == h for i, k in ps)
            seen.update((i, k) for i, k in ps)
        assert seen == {(i, k) for i in range(n) for k in range(3)}      # every (output, tap) reads exactly one input: a partition
        assert C.pairs(0, n) == ([(0, 0), (0, 1), (0, 2)] if n == 1 else [(0, 0), (1, 0), (0, 1)])
        if n >= 3:
            assert C.pairs(1, n) == [(2, 0), (1, 1), (0, 2)]
    # the kernels' own table (csrc/sgr_final_conv.h: fc_pairs) against the definition, a long axis included
    for n in list(range(1, 13)) + [320]:
        assert emul.emul_fc_pairs_mismatch(n) == 0, n


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_conditions(name):
    z = load(name)
    B, Cc, G, H, W = CASES[name]
    assert os.path.getsize(os.path.join(GOLDEN_DIR, f"g20_finalconv_{name}.npz")) <= 1 << 20
    x = z["x"] if G else z["y"]
    names = [k for k in (FUSED_GRADS if G else PLAIN_GRADS) if k]
    assert tuple(x.shape) == (B, Cc, H, W) and x.dtype == np.float32 and z["Wt"].shape == (3, Cc, 3, 3) and z["bias"].shape == (3,)
    assert z["ct"].shape == (B, 3, H, W) and z["out64"].shape == (B, 3, H, W) and z["out64"].dtype == np.float64 and z["out32"].dtype == np.float32
    shapes = dict(dx=x.shape, dy=x.shape, dgw=(Cc,), dgb=(Cc,), dW=(3, Cc, 3, 3), db=(3,))
    for k in names:
        assert z[f"{k}64"].shape == shapes[k] and z[f"{k}64"].dtype == np.float64 and z[f"{k}32"].dtype == np.float32
        assert abs(float(z[f"e_ref_{k}"]) - err(z[f"{k}32"], z[f"{k}64"])) <= 1e-12 and 0 <= float(z[f"e_ref_{k}"]) < 2e-6
    assert abs(float(z["e_ref_out"]) - err(z["out32"], z["out64"])) <= 1e-12 and 0 < float(z["e_ref_out"]) < 2e-6
    for k in z.files:
        if z[k].dtype.kind == "f":
            assert np.isfinite(z[k]).all(), (name, k)
    if G:
        assert int(z["G"]) == G
        pre, _, _ = C.GN.pre_relu(t64(x), t64(z["gn_weight"]), t64(z["gn_bias"]), G)
        assert float(pre.abs().min()) >= 1e-5                                   # a 1-ulp difference cannot flip a branch
        assert 0.30 <= float((pre > 0).double().mean()) <= 0.70
        assert np.array_equal(z["dx32"] == 0, z["dx64"] == 0)                    # both runs took the same branches
        assert int((z["gn_weight"] < 0).sum()) >= 4 and int((z["gn_weight"] == 0).sum()) == 1
    else:
        assert float((x < 0).mean()) > 0.3                                       # signed: not a ReLU's output


def m(*shape, grad=False):
    return torch.empty(*shape, device="meta", requires_grad=grad)


def test_operators_are_registered_with_meta_shapes_and_the_autograd_graph():
    ops = torch.ops.sgrender
    assert str(ops.final_conv.default._schema).startswith("sgrender::final_conv(Tensor x, Tensor weight, Tensor bias, Tensor? gn_weight, Tensor? gn_bias, int num_groups")
    assert str(ops.final_conv_bwd.default._schema).startswith("sgrender::final_conv_bwd(Tensor g, Tensor? x, Tensor? weight, Tensor? gn_weight, Tensor? gn_bias, Tensor? stats")
    for name in ("final_conv", "final_conv_bwd"):
        for key in ("Meta", "CUDA"):      # registered from C++ (TORCH_LIBRARY), not by a Python torch.library.custom_op
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sgrender::{name}", key), (name, key)
    B, Cc, G, H, W = 3, 12, 4, 5, 7
    for fused in (False, True):
        for need in itertools.product((False, True), repeat=5 if fused else 3):
            if fused:
                x, gw, gb, w, b = m(B, Cc, H, W, grad=need[0]), m(Cc, grad=need[1]), m(Cc, grad=need[2]), m(3, Cc, 3, 3, grad=need[3]), m(3, grad=need[4])
                y = sgr.group_norm_relu_final_conv(x, gw, gb, G, w, b)
                leaves = [t for t, n in zip((x, gw, gb, w, b), need) if n]
            else:
                x, w, b = m(B, Cc, H, W, grad=need[0]), m(3, Cc, 3, 3, grad=need[1]), m(3, grad=need[2])
                y = sgr.final_conv(x, w, b)
                leaves = [t for t, n in zip((x, w, b), need) if n]
            assert tuple(y.shape) == (B, 3, H, W) and y.dtype == torch.float32 and y.is_contiguous()
            assert y.requires_grad == any(need), (fused, need)
            if leaves:
                gs = torch.autograd.grad(y.sum(), leaves)
                assert [tuple(g.shape) for g in gs] == [tuple(t.shape) for t in leaves]
    # the backward operator itself: a gradient only where wanted, a [0] tensor elsewhere
    for nY, nW, nB in itertools.product((False, True), repeat=3):
        if not (nY or nW or nB):
            continue
        for fused in (False, True):
            gn = (m(Cc), m(Cc), m(B, G, 4)) if fused else (None, None, None)
            got = ops.final_conv_bwd(m(B, 3, H, W), m(B, Cc, H, W) if nW else None, m(3, Cc, 3, 3) if nY else None, *gn, Cc, G, nY, nW, nB)
            want = [(B, Cc, H, W), (3, Cc, 3, 3), (3,)]
            assert [tuple(g.shape) for g in got] == [s if n else (0,) for s, n in zip(want, (nY, nW, nB))]
    # channels-last inputs give contiguous outputs; the statistics are [B,G,4] with a GroupNorm and [0] without
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    y, stats = ops.final_conv(cl(m(B, Cc, H, W)), m(3, Cc, 3, 3), m(3), m(Cc), m(Cc), G, 1e-5)
    assert y.is_contiguous() and tuple(stats.shape) == (B, G, 4)
    assert tuple(ops.final_conv(m(B, Cc, H, W), m(3, Cc, 3, 3), m(3), None, None, 1, 1e-5)[1].shape) == (0,)
    with torch.no_grad():
        assert not sgr.final_conv(m(B, Cc, H, W, grad=True), m(3, Cc, 3, 3), m(3)).requires_grad
    for Cc in (1, 64, 128, 256):      # the channel cap: 64 and 128 inside
        assert tuple(sgr.final_conv(m(1, Cc, 1, 1), m(3, Cc, 3, 3), m(3)).shape) == (1, 3, 1, 1)


def test_the_fused_node_saves_no_map_beyond_x():
    """what the node keeps, seen through the saved-tensor hooks: x, the GroupNorm parameters, the statistics and the convolution's weight"""
    B, Cc, G, H, W = 2, 8, 2, 5, 7
    x, gw, gb, w, b = m(B, Cc, H, W, grad=True), m(Cc, grad=True), m(Cc, grad=True), m(3, Cc, 3, 3, grad=True), m(3, grad=True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t):
        sgr.group_norm_relu_final_conv(x, gw, gb, G, w, b)
    assert sorted(saved) == sorted([(B, Cc, H, W), (Cc,), (Cc,), (B, G, 4), (3, Cc, 3, 3)]), saved
    # the composition keeps the normalised map besides x
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t):
        sgr.final_conv(sgr.group_norm_relu(x, gw, gb, G), w, b)
    assert saved.count((B, Cc, H, W)) == 2
    # the plain form: y for dweight, the weight for dy, nothing without a need
    saved.clear()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t):
        sgr.final_conv(x.detach(), w, b.detach())
        sgr.final_conv(x, w.detach(), b)
    assert saved == [(B, Cc, H, W), (3, Cc, 3, 3)]


def test_the_module_takes_a_conv2d_state_dict():
    assert {"final_conv", "group_norm_relu_final_conv", "FinalConv"} <= set(sgr.__all__)
    ref = torch.nn.Conv2d(64, 3, 3)
    mod = sgr.FinalConv(in_channels=64)
    assert [k for k, _ in mod.named_parameters()] == ["weight", "bias"]
    mod.load_state_dict(ref.state_dict())
    assert torch.equal(mod.weight, ref.weight) and torch.equal(mod.bias, ref.bias)
    mod = mod.to("meta")
    stage = sgr.GroupNormReLU(4, 64).to("meta")
    assert tuple(mod(m(2, 64, 3, 5)).shape) == (2, 3, 3, 5) and tuple(mod(m(2, 64, 3, 5), gn=stage).shape) == (2, 3, 3, 5)
    with pytest.raises(ValueError, match="outside 1..256"):
        sgr.FinalConv(in_channels=512)
    with pytest.raises(RuntimeError, match="GroupNormReLU"):
        mod(m(2, 64, 3, 5), gn=torch.nn.GroupNorm(4, 64))


def test_refusals():
    z = torch.zeros
    compose = r"compose F\.pad\(\., \(1, 1, 1, 1\), mode='replicate'\) and F\.conv2d"
    with pytest.raises(RuntimeError, match="no CPU path"):
        sgr.final_conv(z(2, 8, 3, 5), z(3, 8, 3, 3), z(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        sgr.group_norm_relu_final_conv(z(2, 8, 3, 5, requires_grad=True), z(8), z(8), 2, z(3, 8, 3, 3), z(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.sgrender.final_conv_bwd(z(2, 3, 3, 5), z(2, 8, 3, 5), z(3, 8, 3, 3), None, None, None, 8, 1, True, True, True)
    with pytest.raises(RuntimeError, match="exactly 3 output channels.*got 12.*" + compose):      # decoderLight's 128 -> 12
        sgr.final_conv(m(2, 128, 3, 5), m(12, 128, 3, 3), m(12))
    with pytest.raises(RuntimeError, match="exactly 3 output channels.*got 1"):
        sgr.final_conv(m(2, 8, 3, 5), m(1, 8, 3, 3), m(1))
    with pytest.raises(RuntimeError, match="257 input channels, at most 256.*" + compose):
        sgr.final_conv(m(2, 257, 3, 5), m(3, 257, 3, 3), m(3))
    with pytest.raises(RuntimeError, match=r"weight must be \[3,8,3,3\].*" + compose):
        sgr.final_conv(m(2, 8, 3, 5), m(3, 8, 5, 5), m(3))
    with pytest.raises(RuntimeError, match=r"weight must be \[3,8,3,3\]"):
        sgr.final_conv(m(2, 8, 3, 5), m(3, 4, 3, 3), m(3))
    with pytest.raises(RuntimeError, match=r"weight must be \[3,8,3,3\]"):
        sgr.final_conv(m(2, 8, 3, 5), m(3, 8, 3), m(3))
    with pytest.raises(RuntimeError, match=r"bias must be \[3\]"):
        sgr.final_conv(m(2, 8, 3, 5), m(3, 8, 3, 3), m(4))
    with pytest.raises(RuntimeError, match="not a multiple of num_groups 3"):
        sgr.group_norm_relu_final_conv(m(2, 8, 3, 5), m(8), m(8), 3, m(3, 8, 3, 3), m(3))
    with pytest.raises(RuntimeError, match=r"GroupNorm weight and bias must be \[8\]"):
        sgr.group_norm_relu_final_conv(m(2, 8, 3, 5), m(4), m(8), 2, m(3, 8, 3, 3), m(3))
    with pytest.raises(RuntimeError, match="fp32 tensors required"):
        sgr.final_conv(m(2, 8, 3, 5).half(), m(3, 8, 3, 3).half(), m(3).half())
    with pytest.raises(RuntimeError, match="zero-sized"):
        sgr.final_conv(m(2, 8, 0, 5), m(3, 8, 3, 3), m(3))
    with pytest.raises(RuntimeError, match=r"x must be \[B,C,H,W\]"):
        sgr.final_conv(m(8, 3, 5), m(3, 8, 3, 3), m(3))
    with pytest.raises(RuntimeError, match="come together"):
        torch.ops.sgrender.final_conv(m(2, 8, 3, 5), m(3, 8, 3, 3), m(3), m(8), None, 2, 1e-5)
    with pytest.raises(RuntimeError, match="no gradient requested"):
        torch.ops.sgrender.final_conv_bwd(m(2, 3, 3, 5), None, None, None, None, None, 8, 1, False, False, False)
    with pytest.raises(RuntimeError, match=r"cotangent must be fp32 \[B,3,H,W\]"):
        torch.ops.sgrender.final_conv_bwd(m(2, 4, 3, 5), None, m(3, 8, 3, 3), None, None, None, 8, 1, True, False, False)
    with pytest.raises(RuntimeError, match="x is needed for dweight"):
        torch.ops.sgrender.final_conv_bwd(m(2, 3, 3, 5), None, None, None, None, None, 8, 1, False, True, False)


def test_c_abi_refusals_without_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused before a launch
    strides = (ctypes.c_longlong * 4)(120, 15, 5, 1)
    sizes = dict(B=2, C=8, O=3, G=2, H=3, W=5)

    def fwd(x=fake, w=fake, b=fake, gw=fake, gb=fake, stats=fake, out=fake, xs=strides, **kw):
        s = {**sizes, **kw}
        return lib.sgr_final_conv_fwd(x, w, b, gw, gb, stats, out, s["B"], s["C"], s["O"], s["G"], s["H"], s["W"], xs, None)

    def bwd(g=fake, x=fake, w=fake, gw=fake, gb=fake, stats=fake, dy=fake, dw=fake, db=fake, ws=fake, xs=strides, **kw):
        s = {**sizes, **kw}
        return lib.sgr_final_conv_bwd(g, x, w, gw, gb, stats, dy, dw, db, ws, s["B"], s["C"], s["O"], s["G"], s["H"], s["W"], xs, None)

    def mom(x=fake, stats=fake, ws=fake, xs=strides, eps=1e-5, **kw):
        s = {**sizes, **kw}
        return lib.sgr_gn_moments(x, stats, ws, s["B"], s["C"], s["G"], s["H"], s["W"], xs, ctypes.c_float(eps), None)
    for k in ("x", "w", "b", "out", "xs"):
        assert fwd(**{k: None}) == -1 and b"NULL tensor" in lib.sgr_last_error(), k
    assert fwd(gw=None) == -1 and b"prologue needs" in lib.sgr_last_error()
    assert bwd(g=None) == -1 and b"NULL cotangent" in lib.sgr_last_error()
    assert bwd(dy=None, dw=None, db=None) == -1 and b"no gradient requested" in lib.sgr_last_error()
    for k in ("x", "w", "ws", "xs"):
        assert bwd(**{k: None}) == -1 and b"NULL tensor" in lib.sgr_last_error(), k
    assert bwd(gb=None) == -1 and b"prologue needs" in lib.sgr_last_error()
    for k in ("x", "stats", "ws", "xs"):
        assert mom(**{k: None}) == -1 and b"NULL tensor" in lib.sgr_last_error(), k
    for k in ("B", "C", "H", "W"):      # each size in turn, zero and negative
        for bad in (0, -3):
            assert fwd(**{k: bad}) == -1 and b"non-positive" in lib.sgr_last_error(), (k, bad)
            assert bwd(**{k: bad}) == -1 and b"non-positive" in lib.sgr_last_error(), (k, bad)
            assert mom(**{k: bad}) == -1 and b"non-positive" in lib.sgr_last_error(), (k, bad)
            args = dict(B=2, C=8, O=3, H=3, W=5)
            args[k] = bad
            assert lib.sgr_final_conv_workspace_floats(*args.values()) == 0
    for call in (fwd, bwd):
        assert call(O=12) == -2 and b"exactly 3" in lib.sgr_last_error() and b"F.conv2d" in lib.sgr_last_error()
        assert call(C=257, G=1) == -2 and b"256 input channels" in lib.sgr_last_error() and b"F.pad" in lib.sgr_last_error()
        assert call(G=3) == -1 and b"not a multiple of num_groups" in lib.sgr_last_error()
        assert call(B=65536) == -2 and b"65535" in lib.sgr_last_error()
    assert mom(G=3) == -1 and b"not a multiple of num_groups" in lib.sgr_last_error()
    assert mom(eps=0.0) == -1 and b"eps" in lib.sgr_last_error()
    neg = (ctypes.c_longlong * 4)(120, 15, -5, 1)      # a plane is indexed with 32-bit offsets: no negative strides
    assert fwd(xs=neg) == -2 and b"plane strides" in lib.sgr_last_error()
    assert bwd(xs=neg) == -2 and b"plane strides" in lib.sgr_last_error()
    assert mom(xs=neg) == -2 and b"plane strides" in lib.sgr_last_error()
    # the workspace query: 28 floats per (image, channel, strip) and 4 per (image, strip); a strip is 8192 pixels of whole runs of four
    q = lib.sgr_final_conv_workspace_floats
    assert q(2, 8, 3, 3, 5) == 2 * 8 * 28 + 2 * 4 and q(16, 64, 3, 240, 320) == 16 * 64 * 10 * 28 + 16 * 10 * 4
    assert q(2, 8, 12, 3, 5) == 0 and q(2, 257, 3, 3, 5) == 0 and q(1, 128, 3, 1, 1) == 128 * 28 + 4
    assert _lib.ABI_VERSION == 6 and lib.sgr_abi_version() == 6      # additive: the version did not move


def _p(a):
    return None if a is None else a.ctypes.data_as(FP)


@pytest.mark.parametrize("name", list(CASES))
def test_the_kernels_arithmetic_on_the_host_stays_within_half_the_gpu_bounds(emul, name):
    z = load(name)
    B, Cc, G, H, W = CASES[name]
    x = np.ascontiguousarray(z["x"] if G else z["y"])
    Wt, bias, ct = (np.ascontiguousarray(z[k]) for k in ("Wt", "bias", "ct"))
    gw, gb, stats = (np.ascontiguousarray(z["gn_weight"]), np.ascontiguousarray(z["gn_bias"]), np.empty((B, G, 4), np.float32)) if G else (None, None, None)
    if G:
        emul.emul_gn_moments(_p(x), _p(stats), B, Cc, G, H, W, ctypes.c_float(1e-5))
    out = np.full((B, 3, H, W), np.nan, np.float32)
    emul.emul_final_conv_fwd(_p(x), _p(Wt), _p(bias), _p(gw), _p(gb), _p(stats), _p(out), B, Cc, max(G, 1), H, W)
    dy, dW, db = np.full_like(x, np.nan), np.full_like(Wt, np.nan), np.full_like(bias, np.nan)
    emul.emul_final_conv_bwd(_p(ct), _p(x), _p(Wt), _p(gw), _p(gb), _p(stats), _p(dy), _p(dW), _p(db), B, Cc, max(G, 1), H, W)
    e, lim = err(out, z["out64"]), 0.5 * value_bound(z["e_ref_out"])
    print(f"{name}: values {e:.2e} (half bound {lim:.1e})")
    assert np.isfinite(out).all() and e <= lim, (name, e, lim)
    got = dict(dW=dW, db=db)
    if G:      # dy is the gradient at the ReLU's output: the stage's own backward (the checker's restatement of it, in fp64) carries it on to x
        _, (dx, dgw, dgb, _) = C.GN.gn_stage(t64(x), t64(gw), t64(gb), G, None, cotangent=t64(dy))
        got.update(dx=dx, dgw=dgw, dgb=dgb)
    else:
        got["dy"] = dy
    for k, g in got.items():
        e, lim = err(g, z[f"{k}64"]), 0.5 * grad_bound(z[f"e_ref_{k}"])
        print(f"{name}: {k} {e:.2e} (half bound {lim:.1e})")
        assert bool(torch.isfinite(torch.as_tensor(g)).all()) and e <= lim, (name, k, e, lim)
