"""CPU: the encoders' pad + 4x4 stride-2 convolution (sgr.encoder_conv / sgr.EncoderConv) without a GPU.

  * tests/encoder_conv_checker.py (the contract of DESIGN.md section 8i in torch, explicit index arithmetic) is pinned at 1e-12, in fp64, to
    the fixtures the UNMODIFIED reference produced (tests/golden/g22_encconv_*.npz, tools/make_golden_encoder_conv.py) and to torch's own
    ``F.pad`` + ``F.conv2d(stride=2)`` under autograd at twelve shapes with ``H, W`` in {2, 3, 4, 5}, ``C`` in {1, 3, 148, 160} and ``O`` in
    {16, 128} among them, in both modes;
  * ``R_n(h)`` -- the checker's enumeration and the kernels' ``ec_pairs`` (through the host emulation's library) -- for ``n = 2..12``;
  * the fixtures hold what they were made for;
  * ``torch.ops.sgrender.encoder_conv`` / ``encoder_conv_bwd`` are registered by the C++ extension with Meta kernels of the documented shapes,
    the autograd graph gives a gradient exactly where one is required, and the node keeps ``x`` only for ``dWt`` and ``Wt`` only for ``dx``;
  * the wrapper, the operators and the C ABI refuse what the contract refuses, before anything is dereferenced, naming the composition;
  * the kernels' tile loops on the host (csrc/sgr_encoder_conv.h behind a software MFMA, tests/host_emul/encoder_conv_emul.cpp) stay within
    HALF of every bound of tests/test_gpu_encoder_conv.py on every fixture, and equal the checker exactly on small-integer data."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import encoder_conv_checker as C
from conftest import GOLDEN_DIR, ROOT

import inverserenderingofindoorscene_amd as sgr
from inverserenderingofindoorscene_amd import _lib

# name -> (pad, B, C, O, H, W)
CASES = {"rgb": ("replicate", 2, 3, 64, 6, 10), "c17": ("replicate", 3, 17, 64, 5, 7), "pre": ("replicate", 2, 11, 32, 9, 13),
         "two": ("replicate", 1, 11, 32, 2, 2), "three": ("replicate", 1, 11, 32, 3, 3), "row": ("replicate", 1, 3, 64, 2, 9),
         "col": ("replicate", 1, 3, 64, 7, 2), "zero": ("zeros", 2, 32, 64, 5, 8), "zero3": ("zeros", 1, 32, 64, 3, 3)}
GRADS = ("dx", "dW", "db")
PIN = 1e-12
FP = ctypes.POINTER(ctypes.c_float)
COMPOSE = r"compose F\.pad\(x, \(1, 1, 1, 1\), mode=\.\.\.\) and F\.conv2d\(\., stride=2\)"


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, f"g22_encconv_{name}.npz"))


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


def value_bound(e_ref):
    return max(2.0 * float(e_ref), 1e-6)


def grad_bound(e_ref):
    return max(4.0 * float(e_ref), 1e-6)


@pytest.mark.parametrize("name", list(CASES))
def test_checker_is_pinned_to_the_reference_fixture(name):
    z = load(name)
    x, Wt, bias, ct = (torch.from_numpy(z[k]).double() for k in ("x", "Wt", "bias", "ct"))
    for fn in (C.encoder_conv, C.composition):
        out, grads = fn(x, Wt, bias, CASES[name][0], cotangent=ct)
        assert err(out, z["out64"]) <= PIN, (name, fn.__name__, err(out, z["out64"]))
        for k, g in zip(GRADS, grads):
            assert err(g, z[f"{k}64"]) <= PIN, (name, fn.__name__, k, err(g, z[f"{k}64"]))


# (mode, B, C, O, H, W)
SHAPES = [("replicate", 2, 1, 16, 2, 2), ("zeros", 1, 3, 16, 2, 3), ("replicate", 1, 3, 128, 3, 2), ("zeros", 2, 1, 16, 3, 3), ("replicate", 1, 148, 128, 4, 4),
          ("zeros", 1, 160, 16, 4, 5), ("replicate", 1, 160, 16, 5, 4), ("zeros", 1, 148, 16, 5, 5), ("replicate", 2, 3, 16, 5, 3), ("zeros", 1, 17, 32, 2, 5),
          ("replicate", 1, 11, 32, 7, 12), ("zeros", 2, 5, 48, 8, 9)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_checker_equals_torchs_own_composition_under_autograd(shape):
    mode, B, Cc, O, H, W = shape
    g = torch.Generator().manual_seed(2250 + 10 * H + W + O)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, Wt, bias, ct = r(B, Cc, H, W), r(O, Cc, 4, 4), r(O), r(B, O, H // 2, W // 2)
    a, ga = C.encoder_conv(x, Wt, bias, mode, cotangent=ct)
    b, gb = C.composition(x, Wt, bias, mode, cotangent=ct)
    assert err(a, b) <= PIN
    for p, q in zip(ga, gb):
        assert err(p, q) <= PIN, (shape, err(p, q))


@pytest.fixture(scope="module")
def emul():
    d = os.path.join(ROOT, "tests", "host_emul")
    so, src = os.path.join(d, "libencoder_conv_emul.so"), os.path.join(d, "encoder_conv_emul.cpp")
    hdrs = [os.path.join(ROOT, "inverserenderingofindoorscene_amd", "csrc", h) for h in ("sgr_encoder_conv.h", "sgr_light_final_conv.h", "sgr_final_conv.h", "sgr_math.h")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", so])
    return ctypes.CDLL(so)


@pytest.mark.parametrize("mode", C.MODES)
def test_the_index_rule_exhaustively(emul, mode):
    """R_n(h) for n = 2..12: at most two members; every (i, kh) is claimed by exactly one h (replicate) or at most one (zeros); the header's
    ec_pairs, which the kernels and the emulation call, lists the same sets"""
    ip = ctypes.c_int * 4
    for n in range(2, 13):
        claimed = {}
        for h in range(n):
            R = C.pairs(h, n, mode)
            assert len(R) <= 2, (n, h, R)
            for m in R:
                assert m not in claimed, (n, h, m)
                claimed[m] = h
            buf = ip()
            emul.emul_encoder_conv_pairs(h, n, C.MODES.index(mode), buf)
            assert sorted(R) == sorted((buf[2 * s], buf[2 * s + 1]) for s in range(2) if buf[2 * s] >= 0), (n, h, R, list(buf))
        every = {(i, k) for i in range(n // 2) for k in range(4)}
        if mode == "replicate":
            assert set(claimed) == every, n
        else:
            assert set(claimed) <= every and every - set(claimed) == {m for m in every if not 0 <= 2 * m[0] + m[1] - 1 < n}, n
        if mode == "replicate":      # the cases DESIGN.md section 8i names
            assert sorted(C.pairs(0, n, mode)) == [(0, 0), (0, 1)]
            if n % 2 == 0:
                assert sorted(C.pairs(n - 1, n, mode)) == [(n // 2 - 1, 2), (n // 2 - 1, 3)]
            else:
                assert C.pairs(n - 1, n, mode) == [(n // 2 - 1, 3)] and C.pairs(n - 2, n, mode)[-1] == (n // 2 - 1, 2)
        for h in range(1, n - 1):      # interior rows: the taps of the row's own parity class
            assert all(k % 2 == (h + 1) % 2 for _, k in C.pairs(h, n, mode)), (n, h)


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_conditions(name):
    z = load(name)
    mode, B, Cc, O, H, W = CASES[name]
    assert os.path.getsize(os.path.join(GOLDEN_DIR, f"g22_encconv_{name}.npz")) <= 1 << 20
    x = z["x"]
    assert int(z["pad_mode"]) == C.MODES.index(mode)
    assert tuple(x.shape) == (B, Cc, H, W) and x.dtype == np.float32 and z["Wt"].shape == (O, Cc, 4, 4) and z["bias"].shape == (O,)
    so = (B, O, H // 2, W // 2)
    assert z["ct"].shape == so and z["out64"].shape == so and z["out64"].dtype == np.float64 and z["out32"].dtype == np.float32
    shapes = dict(dx=x.shape, dW=(O, Cc, 4, 4), db=(O,))
    for k in GRADS:
        assert z[f"{k}64"].shape == shapes[k] and z[f"{k}64"].dtype == np.float64 and z[f"{k}32"].dtype == np.float32
        assert f"e_ref_{k}" in z.files and abs(float(z[f"e_ref_{k}"]) - err(z[f"{k}32"], z[f"{k}64"])) <= 1e-12 and 0 <= float(z[f"e_ref_{k}"]) < 2e-6
    assert "e_ref_out" in z.files and abs(float(z["e_ref_out"]) - err(z["out32"], z["out64"])) <= 1e-12 and 0 < float(z["e_ref_out"]) < 2e-6
    for k in z.files:
        if z[k].dtype.kind == "f":
            assert np.isfinite(z[k]).all(), (name, k)
    assert float((x < 0).mean()) > 0.3      # signed maps
    if name in ("two", "three", "zero3"):
        assert so == (1, O, 1, 1)
    if name == "three":                      # the last row and column are read by tap 3 alone; the bottom pad of an odd map by nobody
        assert C.pairs(2, 3, "replicate") == [(0, 3)] and C.pairs(1, 3, "replicate") == [(0, 2)]
    if mode == "zeros" and H % 2 == 1:       # the last row of an odd zero-padded map: one tap, no member from the pad
        assert C.pairs(H - 1, H, "zeros") == [(H // 2 - 1, 3)]


def m(*shape, grad=False):
    return torch.empty(*shape, device="meta", requires_grad=grad)


def test_operators_are_registered_with_meta_shapes_and_the_autograd_graph():
    ops = torch.ops.sgrender
    assert str(ops.encoder_conv.default._schema) == "sgrender::encoder_conv(Tensor x, Tensor weight, Tensor bias, int pad_mode) -> Tensor"
    assert str(ops.encoder_conv_bwd.default._schema) == ("sgrender::encoder_conv_bwd(Tensor g, Tensor? x, Tensor? weight, int H, int W, int pad_mode, bool need_x, "
                                                         "bool need_w, bool need_b) -> (Tensor, Tensor, Tensor)")
    for name in ("encoder_conv", "encoder_conv_bwd"):
        for key in ("Meta", "CUDA"):      # registered from C++ (TORCH_LIBRARY), not by a Python torch.library.custom_op
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sgrender::{name}", key), (name, key)
    B, Cc, O, H, W = 3, 17, 32, 5, 7
    for padding in C.MODES:
        for need in itertools.product((False, True), repeat=3):
            x, w, b = m(B, Cc, H, W, grad=need[0]), m(O, Cc, 4, 4, grad=need[1]), m(O, grad=need[2])
            out = sgr.encoder_conv(x, w, b, padding)
            leaves = [t for t, n in zip((x, w, b), need) if n]
            assert tuple(out.shape) == (B, O, 2, 3) and out.dtype == torch.float32 and out.is_contiguous()
            assert out.requires_grad == any(need), need
            if leaves:
                gs = torch.autograd.grad(out.sum(), leaves)
                assert [tuple(g.shape) for g in gs] == [tuple(t.shape) for t in leaves]
    # the backward operator itself: a gradient only where wanted, a [0] tensor elsewhere
    for nX, nW, nB in itertools.product((False, True), repeat=3):
        if not (nX or nW or nB):
            continue
        got = ops.encoder_conv_bwd(m(B, O, 2, 3), m(B, Cc, H, W) if nW else None, m(O, Cc, 4, 4) if nX else None, H, W, 0, nX, nW, nB)
        want = [(B, Cc, H, W), (O, Cc, 4, 4), (O,)]
        assert [tuple(g.shape) for g in got] == [s if n else (0,) for s, n in zip(want, (nX, nW, nB))]
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    assert ops.encoder_conv(cl(m(B, Cc, H, W)), m(O, Cc, 4, 4), m(O), 1).is_contiguous()
    with torch.no_grad():
        assert not sgr.encoder_conv(m(B, Cc, H, W, grad=True), m(O, Cc, 4, 4), m(O)).requires_grad
    for Cc, O in ((1, 16), (3, 64), (148, 128), (160, 128)):      # the corners of the domain
        assert tuple(sgr.encoder_conv(m(1, Cc, 2, 2), m(O, Cc, 4, 4), m(O)).shape) == (1, O, 1, 1)
    assert tuple(sgr.encoder_conv(m(16, 11, 480, 640), m(32, 11, 4, 4), m(32)).shape) == (16, 32, 240, 320)


def test_the_node_keeps_x_only_for_dweight_and_the_weight_only_for_dx():
    """what the node keeps, seen through the saved-tensor hooks"""
    B, Cc, O, H, W = 2, 11, 32, 5, 7
    x, w, b = m(B, Cc, H, W, grad=True), m(O, Cc, 4, 4, grad=True), m(O, grad=True)
    saved = []

    def kept(*args):
        saved.clear()
        with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t):
            sgr.encoder_conv(*args)
        return list(saved)
    assert sorted(kept(x, w, b)) == sorted([(B, Cc, H, W), (O, Cc, 4, 4)])
    assert kept(x.detach(), w, b.detach()) == [(B, Cc, H, W)]
    assert kept(x, w.detach(), b) == [(O, Cc, 4, 4)]
    assert kept(x.detach(), w.detach(), b) == []
    assert kept(x.detach(), w.detach(), b.detach()) == []


def test_the_module_takes_a_conv2d_state_dict():
    assert {"encoder_conv", "EncoderConv"} <= set(sgr.__all__)
    for Cc, O, padding in ((3, 64, "replicate"), (17, 64, "replicate"), (64, 128, "zeros"), (11, 32, "replicate"), (148, 128, "replicate")):
        ref = torch.nn.Conv2d(Cc, O, 4, stride=2)
        mod = sgr.EncoderConv(Cc, O, padding)
        assert [k for k, _ in mod.named_parameters()] == ["weight", "bias"] and list(mod.state_dict()) == list(ref.state_dict())
        mod.load_state_dict(ref.state_dict())
        assert torch.equal(mod.weight, ref.weight) and torch.equal(mod.bias, ref.bias)
        assert tuple(mod.to("meta")(m(2, Cc, 6, 10)).shape) == (2, O, 3, 5)

    class Pre(torch.nn.Module):      # a reference checkpoint's keys under the encoder's own prefixes; the pad modules become nn.Identity
        def __init__(self):
            super().__init__()
            self.preProcess = torch.nn.Sequential(torch.nn.Identity(), sgr.EncoderConv(11, 32), torch.nn.GroupNorm(2, 32), torch.nn.ReLU(),
                                                  torch.nn.Identity(), sgr.EncoderConv(32, 64, padding="zeros"), torch.nn.GroupNorm(4, 64), torch.nn.ReLU())
            self.conv1 = sgr.EncoderConv(64, 128)
    ref = torch.nn.ModuleDict(dict(preProcess=torch.nn.Sequential(torch.nn.ReplicationPad2d(1), torch.nn.Conv2d(11, 32, 4, stride=2), torch.nn.GroupNorm(2, 32),
                                                                  torch.nn.ReLU(), torch.nn.ZeroPad2d(1), torch.nn.Conv2d(32, 64, 4, stride=2),
                                                                  torch.nn.GroupNorm(4, 64), torch.nn.ReLU()), conv1=torch.nn.Conv2d(64, 128, 4, stride=2)))
    pre = Pre()
    assert sorted(pre.state_dict()) == sorted(ref.state_dict())
    pre.load_state_dict(ref.state_dict())
    assert torch.equal(pre.preProcess[1].weight, ref["preProcess"][1].weight) and torch.equal(pre.preProcess[5].bias, ref["preProcess"][5].bias)
    assert torch.equal(pre.conv1.weight, ref["conv1"].weight) and pre.preProcess[5].padding == "zeros"
    torch.manual_seed(7)
    a = sgr.EncoderConv(17, 64)
    torch.manual_seed(7)
    b = torch.nn.Conv2d(17, 64, 4, stride=2)
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)      # initialised as nn.Conv2d
    for bad in (dict(in_channels=0, out_channels=64), dict(in_channels=161, out_channels=64), dict(in_channels=3, out_channels=8),
                dict(in_channels=3, out_channels=24), dict(in_channels=3, out_channels=144), dict(in_channels=3, out_channels=64, padding="reflect")):
        with pytest.raises(ValueError, match="F.pad"):
            sgr.EncoderConv(**bad)


def test_refusals():
    z = torch.zeros
    ops = torch.ops.sgrender
    with pytest.raises(RuntimeError, match="no CPU path"):
        sgr.encoder_conv(z(2, 3, 4, 6), z(16, 3, 4, 4), z(16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        sgr.encoder_conv(z(2, 3, 4, 6, requires_grad=True), z(16, 3, 4, 4), z(16), "zeros")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.encoder_conv_bwd(z(2, 16, 2, 3), z(2, 3, 4, 6), z(16, 3, 4, 4), 4, 6, 0, True, True, True)
    with pytest.raises(ValueError, match="padding 'reflect'.*" + COMPOSE):
        sgr.encoder_conv(m(2, 3, 4, 6), m(16, 3, 4, 4), m(16), "reflect")
    with pytest.raises(RuntimeError, match="pad_mode 2, 0 .replicate. or 1 .zeros.*" + COMPOSE):
        ops.encoder_conv(m(2, 3, 4, 6), m(16, 3, 4, 4), m(16), 2)
    with pytest.raises(RuntimeError, match="pad_mode -1.*" + COMPOSE):
        ops.encoder_conv_bwd(m(2, 16, 2, 3), None, m(16, 3, 4, 4), 4, 6, -1, True, False, False)
    for Cc in (0, 161):
        with pytest.raises(RuntimeError, match=f"{Cc} input channels, 1..160 are supported .the deeper encoder layers.*" + COMPOSE):
            sgr.encoder_conv(m(2, Cc, 4, 6), m(16, Cc, 4, 4), m(16))
    with pytest.raises(RuntimeError, match="161 input channels.*" + COMPOSE):
        ops.encoder_conv_bwd(m(2, 16, 2, 3), None, m(16, 161, 4, 4), 4, 6, 0, True, False, False)
    for O in (8, 24, 144, 0):
        with pytest.raises(RuntimeError, match=f"{O} output channels, a multiple of 16 in 16..128.*" + COMPOSE):
            sgr.encoder_conv(m(2, 3, 4, 6), m(O, 3, 4, 4), m(O), "zeros")
        with pytest.raises(RuntimeError, match=f"{O} output channels.*" + COMPOSE):
            ops.encoder_conv_bwd(m(2, O, 2, 3), None, None, 4, 6, 0, False, False, True)
    for H, W in ((1, 6), (4, 1)):
        with pytest.raises(RuntimeError, match=f"a {H} x {W} map, H and W must be at least 2.*" + COMPOSE):
            sgr.encoder_conv(m(2, 3, H, W), m(16, 3, 4, 4), m(16))
    with pytest.raises(RuntimeError, match=r"weight must be \[O,3,4,4\].*" + COMPOSE):      # a 3x3 kernel
        sgr.encoder_conv(m(2, 3, 4, 6), m(16, 3, 3, 3), m(16))
    with pytest.raises(RuntimeError, match=r"weight must be \[O,3,4,4\].*" + COMPOSE):
        sgr.encoder_conv(m(2, 3, 4, 6), m(16, 4, 4, 4), m(16))
    with pytest.raises(RuntimeError, match=r"bias must be \[16\].*" + COMPOSE):
        sgr.encoder_conv(m(2, 3, 4, 6), m(16, 3, 4, 4), m(17))
    with pytest.raises(RuntimeError, match="fp32 tensors required.*" + COMPOSE):
        sgr.encoder_conv(m(2, 3, 4, 6).half(), m(16, 3, 4, 4).half(), m(16).half())
    with pytest.raises(RuntimeError, match="fp32 tensors required.*" + COMPOSE):
        sgr.encoder_conv(m(2, 3, 4, 6).double(), m(16, 3, 4, 4).double(), m(16).double())
    with pytest.raises(RuntimeError, match="zero-sized"):
        sgr.encoder_conv(m(0, 3, 4, 6), m(16, 3, 4, 4), m(16))
    with pytest.raises(RuntimeError, match=r"x must be \[B,C,H,W\].*" + COMPOSE):
        sgr.encoder_conv(m(3, 4, 6), m(16, 3, 4, 4), m(16))
    with pytest.raises(RuntimeError, match="no gradient requested"):
        ops.encoder_conv_bwd(m(2, 16, 2, 3), None, None, 4, 6, 0, False, False, False)
    with pytest.raises(RuntimeError, match=r"cotangent must be fp32 \[B,O,H/2,W/2\]"):
        ops.encoder_conv_bwd(m(2, 16, 2), None, m(16, 3, 4, 4), 4, 6, 0, True, False, False)
    with pytest.raises(RuntimeError, match=r"cotangent must be fp32 \[B,O,H/2,W/2\] for H = 4, W = 8"):
        ops.encoder_conv_bwd(m(2, 16, 2, 3), None, m(16, 3, 4, 4), 4, 8, 0, True, False, False)
    with pytest.raises(RuntimeError, match=r"weight must be fp32 \[16,C,4,4\]"):
        ops.encoder_conv_bwd(m(2, 16, 2, 3), None, m(32, 3, 4, 4), 4, 6, 0, True, False, False)
    with pytest.raises(RuntimeError, match="x is needed for dweight"):
        ops.encoder_conv_bwd(m(2, 16, 2, 3), None, None, 4, 6, 0, False, True, False)
    with pytest.raises(RuntimeError, match="weight is needed for dx"):
        ops.encoder_conv_bwd(m(2, 16, 2, 3), None, None, 4, 6, 0, True, False, False)


def test_c_abi_refusals_without_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused before a launch
    strides = (ctypes.c_longlong * 4)(72, 24, 6, 1)
    sizes = dict(B=2, C=3, O=16, H=4, W=6)

    def fwd(x=fake, w=fake, b=fake, out=fake, xs=strides, mode=0, **kw):
        s = {**sizes, **kw}
        return lib.sgr_encoder_conv_fwd(x, w, b, out, s["B"], s["C"], s["O"], s["H"], s["W"], xs, mode, None)

    def bwd(g=fake, x=fake, w=fake, dx=fake, dw=fake, db=fake, ws=fake, xs=strides, mode=0, **kw):
        s = {**sizes, **kw}
        return lib.sgr_encoder_conv_bwd(g, x, w, dx, dw, db, ws, s["B"], s["C"], s["O"], s["H"], s["W"], xs, mode, None)
    q = lib.sgr_encoder_conv_workspace_floats
    for k in ("x", "w", "b", "out", "xs"):
        assert fwd(**{k: None}) == -1 and b"NULL tensor" in lib.sgr_last_error(), k
    assert bwd(g=None) == -1 and b"NULL cotangent" in lib.sgr_last_error()
    assert bwd(dx=None, dw=None, db=None) == -1 and b"no gradient requested" in lib.sgr_last_error()
    for k in ("x", "w", "ws", "xs"):
        assert bwd(**{k: None}) == -1 and b"NULL tensor" in lib.sgr_last_error(), k
    for k in ("B", "C", "O", "H", "W"):      # each size in turn, zero and negative
        for bad in (0, -3):
            assert fwd(**{k: bad}) == -1 and b"non-positive" in lib.sgr_last_error(), (k, bad)
            assert bwd(**{k: bad}) == -1 and b"non-positive" in lib.sgr_last_error(), (k, bad)
            assert q(*{**sizes, k: bad}.values()) == 0
    compose = b"F.pad(x, (1, 1, 1, 1), mode=...) and F.conv2d(., stride=2)"
    for call in (fwd, bwd):
        assert call(C=161) == -2 and b"160 input channels" in lib.sgr_last_error() and b"deeper encoder layers" in lib.sgr_last_error() and compose in lib.sgr_last_error()
        for O in (8, 24, 144):
            assert call(O=O) == -2 and b"multiple of 16 in 16..128" in lib.sgr_last_error() and compose in lib.sgr_last_error(), O
        assert call(H=1) == -2 and b"at least 2" in lib.sgr_last_error() and compose in lib.sgr_last_error()
        assert call(W=1) == -2 and b"at least 2" in lib.sgr_last_error()
        for mode in (2, -1):
            assert call(mode=mode) == -2 and b"pad_mode" in lib.sgr_last_error() and compose in lib.sgr_last_error()
        assert call(B=65536) == -2 and b"65535" in lib.sgr_last_error()
        assert call(H=1 << 14, W=1 << 14) == -2 and b"Ho * Wo" in lib.sgr_last_error()
    neg = (ctypes.c_longlong * 4)(72, 24, -6, 1)      # a plane is indexed with 32-bit offsets: no negative strides
    assert fwd(xs=neg) == -2 and b"plane strides" in lib.sgr_last_error()
    assert bwd(xs=neg) == -2 and b"plane strides" in lib.sgr_last_error()
    # the workspace query: 16 C O floats per (image, strip of 25 16 x 4 pixel tiles) and one per (image, output, slice of 8192 pixels)
    assert q(2, 3, 16, 4, 6) == 2 * 16 * 3 * 16 + 2 * 16 and q(16, 148, 128, 120, 160) == 16 * 3 * 16 * 148 * 128 + 16 * 128
    assert q(16, 11, 32, 480, 640) == 16 * 48 * 16 * 11 * 32 + 16 * 32 * 10
    assert q(2, 161, 16, 4, 6) == 0 and q(2, 3, 24, 4, 6) == 0 and q(2, 3, 16, 1, 6) == 0
    assert _lib.ABI_VERSION == 6 and lib.sgr_abi_version() == 6      # additive: the version did not move


def _p(a):
    return a.ctypes.data_as(FP)


def run_emul(emul, x, Wt, bias, ct, mode):
    B, Cc, H, W = x.shape
    O = Wt.shape[0]
    x, Wt, bias, ct = (np.ascontiguousarray(a, np.float32) for a in (x, Wt, bias, ct))
    out = np.full((B, O, H // 2, W // 2), np.nan, np.float32)
    emul.emul_encoder_conv_fwd(_p(x), _p(Wt), _p(bias), _p(out), B, Cc, O, H, W, C.MODES.index(mode))
    dx, dW, db = np.full_like(x, np.nan), np.full_like(Wt, np.nan), np.full_like(bias, np.nan)
    emul.emul_encoder_conv_bwd(_p(ct), _p(x), _p(Wt), _p(dx), _p(dW), _p(db), B, Cc, O, H, W, C.MODES.index(mode))
    return out, dict(dx=dx, dW=dW, db=db)


@pytest.mark.parametrize("name", list(CASES))
def test_the_kernels_tile_loops_on_the_host_stay_within_half_the_gpu_bounds(emul, name):
    z = load(name)
    out, got = run_emul(emul, z["x"], z["Wt"], z["bias"], z["ct"], CASES[name][0])
    e, lim = err(out, z["out64"]), 0.5 * value_bound(z["e_ref_out"])
    print(f"{name}: values {e:.2e} (half bound {lim:.1e})")
    assert np.isfinite(out).all() and e <= lim, (name, e, lim)
    for k, g in got.items():
        e, lim = err(g, z[f"{k}64"]), 0.5 * grad_bound(z[f"e_ref_{k}"])
        print(f"{name}: {k} {e:.2e} (half bound {lim:.1e})")
        assert np.isfinite(g).all() and e <= lim, (name, k, e, lim)


# two forward tiles per axis (32 x 8 outputs) with ragged edges; two output passes and a last N tile short of a pass (O = 80); three channel
# passes of the data gradient (C = 148) and a ragged last chunk (C = 5, 17); two strips of the weight gradient (26 pixel tiles); odd and
# even maps in both modes; the smallest maps
EXACT = [("replicate", 1, 5, 80, 19, 70), ("zeros", 1, 17, 16, 18, 67), ("replicate", 1, 148, 128, 5, 6), ("zeros", 1, 3, 32, 9, 420), ("replicate", 2, 1, 16, 2, 2),
         ("zeros", 1, 2, 16, 3, 3), ("replicate", 1, 66, 48, 11, 9)]


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "x".join(map(str, s)))
def test_the_software_mfma_places_every_element_exactly(emul, shape):
    """integer data, every fp32 sum exact: the tile loops equal the fp64 checker bit for bit"""
    mode, B, Cc, O, H, W = shape
    g = torch.Generator().manual_seed(2290 + O + H)
    ri = lambda *s: torch.randint(-3, 4, s, generator=g).double()
    x, Wt, bias, ct = ri(B, Cc, H, W), ri(O, Cc, 4, 4), ri(O), ri(B, O, H // 2, W // 2)
    out, got = run_emul(emul, x.numpy(), Wt.numpy(), bias.numpy(), ct.numpy(), mode)
    o64, (dx, dW, db) = C.encoder_conv(x, Wt, bias, mode, cotangent=ct)
    assert np.array_equal(out, o64.numpy()) and np.array_equal(got["dx"], dx.numpy()) and np.array_equal(got["dW"], dW.numpy()) and np.array_equal(got["db"], db.numpy())
