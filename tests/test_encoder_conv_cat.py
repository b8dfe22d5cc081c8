"""CPU: the encoders' convolution over several sources (sgr.encoder_conv_cat / sgr.EncoderConv((C_1, C_2, ..), O)) without a GPU.

  * ``torch.ops.sgrender.encoder_conv_cat`` / ``encoder_conv_cat_bwd`` are registered by the C++ extension with Meta kernels of the documented
    shapes and dtypes; the autograd graph gives a gradient exactly where one is required, for every subset of ``requires_grad`` over two
    sources, weight and bias, and the node keeps the sources only for ``dWt`` and ``Wt`` only for some ``dx``;
  * the wrapper, the module, the operators and the C ABI refuse what the contract refuses, in the words of ``encoder_conv``'s refusals, naming
    ``torch.cat(xs, 1)`` + ``F.pad`` + ``F.conv2d``; the ABI version did not move;
  * the autocast rule on fake device tensors: bf16 sources give an fp32 result, and bf16 is refused with autocast off;
  * the module's state-dict keys are ``nn.Conv2d(71, 128, 4, stride=2)``'s;
  * the kernels' tile loops on the host with a source table (tests/host_emul/encoder_conv_cat_emul.cpp) equal the single-source emulation on
    the concatenated data bit for bit -- value, ``dW``, ``db`` and each ``dx`` -- over the splits and planes of
    tests/test_gpu_encoder_conv_cat.py (every split on two planes), also as a stand-alone program built with ``-fsanitize=address,undefined``;
  * the fixture the UNMODIFIED reference produced (tests/golden/g24_enccat_light.npz, tools/make_golden_encoder_conv_cat.py) is held against
    tests/encoder_conv_checker.py applied to the concatenation, at 1e-12."""
import contextlib
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

PIN = 1e-12
COMPOSE = r"compose torch\.cat\(xs, 1\), F\.pad\(x, \(1, 1, 1, 1\), mode=\.\.\.\) and F\.conv2d\(\., stride=2\)"
ops = torch.ops.sgrender


def m(*shape, grad=False, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype, requires_grad=grad)


def err(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


def test_operators_are_registered_with_meta_shapes_and_dtypes():
    assert str(ops.encoder_conv_cat.default._schema) == "sgrender::encoder_conv_cat(Tensor[] xs, Tensor weight, Tensor bias, int pad_mode) -> Tensor"
    assert str(ops.encoder_conv_cat_bwd.default._schema) == ("sgrender::encoder_conv_cat_bwd(Tensor g, Tensor[] xs, Tensor? weight, int[] channels, int H, int W, int pad_mode, "
                                                             "int need_x, bool need_w, bool need_b) -> (Tensor[], Tensor, Tensor)")
    for name in ("encoder_conv_cat", "encoder_conv_cat_bwd"):
        for key in ("Meta", "CUDA", "CPU", "AutocastCUDA"):      # registered from C++ (TORCH_LIBRARY), not by a Python torch.library.custom_op
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sgrender::{name}", key), (name, key)
    assert torch._C._dispatch_has_kernel_for_dispatch_key("sgrender::encoder_conv_cat", "Autograd")
    B, O, H, W = 3, 48, 5, 7
    for split in ((1, 1), (3, 5, 1), (64, 84), (1, 1, 1, 1), (40, 40, 40, 40), (17,)):
        Ct = sum(split)
        for padding in C.MODES:
            out = sgr.encoder_conv_cat([m(B, c, H, W) for c in split], m(O, Ct, 4, 4), m(O), padding)
            assert tuple(out.shape) == (B, O, 2, 3) and out.dtype == torch.float32 and out.is_contiguous() and not out.requires_grad
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    assert ops.encoder_conv_cat([cl(m(B, 5, H, W)), m(B, 9, H, W)[:, 2:6]], m(O, 9, 4, 4), m(O), 1).is_contiguous()
    assert tuple(sgr.encoder_conv_cat((m(16, 64, 120, 160), m(16, 84, 120, 160)), m(128, 148, 4, 4), m(128)).shape) == (16, 128, 60, 80)
    # the backward operator itself: a gradient only where wanted, a [0] tensor elsewhere
    split, Ct = (3, 5, 1), 9
    for nX in range(8):
        for nW, nB in itertools.product((False, True), repeat=2):
            if not (nX or nW or nB):
                continue
            xs = [m(B, c, H, W) if nW else m(0) for c in split]
            dxs, dw, db = ops.encoder_conv_cat_bwd(m(B, O, 2, 3), xs, m(O, Ct, 4, 4) if nX else None, list(split), H, W, 0, nX, nW, nB)
            assert [tuple(d.shape) for d in dxs] == [(B, c, H, W) if (nX >> i) & 1 else (0,) for i, c in enumerate(split)]
            assert tuple(dw.shape) == ((O, Ct, 4, 4) if nW else (0,)) and tuple(db.shape) == ((O,) if nB else (0,))
            assert all(d.dtype == torch.float32 and d.is_contiguous() for d in list(dxs) + [dw, db])


@pytest.mark.parametrize("need", list(itertools.product((False, True), repeat=4)), ids=lambda n: "".join("xywb"[i] if f else "-" for i, f in enumerate(n)))
def test_the_autograd_graph_and_what_the_node_keeps(need):
    """every subset of requires_grad over two sources, weight and bias: a gradient exactly where one is required; through the saved-tensor
    hooks, the node keeps the sources only if dweight is wanted and the weight only if some dx is"""
    B, c1, c2, O, H, W = 2, 64, 7, 32, 5, 7
    x1, x2, w, b = m(B, c1, H, W, grad=need[0]), m(B, c2, H, W, grad=need[1]), m(O, c1 + c2, 4, 4, grad=need[2]), m(O, grad=need[3])
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t):
        out = sgr.encoder_conv_cat([x1, x2], w, b)
    assert out.requires_grad == any(need)
    want = ([(B, c1, H, W), (B, c2, H, W)] if need[2] else []) + ([(O, c1 + c2, 4, 4)] if need[0] or need[1] else [])
    assert sorted(saved) == sorted(want), (need, saved)
    leaves = [t for t, n in zip((x1, x2, w, b), need) if n]
    if leaves:
        gs = torch.autograd.grad(out.sum(), leaves, allow_unused=False)
        assert [tuple(g.shape) for g in gs] == [tuple(t.shape) for t in leaves] and all(g.is_contiguous() for g in gs)
        x1.grad = x2.grad = None
        sgr.encoder_conv_cat([x1, x2], w, b, "zeros").sum().backward()
        assert (x1.grad is not None) == need[0] and (x2.grad is not None) == need[1]      # a source without grad gets None
    with torch.no_grad():
        assert not sgr.encoder_conv_cat([x1, x2], w, b).requires_grad


def test_the_module_takes_a_conv2d_state_dict():
    assert {"encoder_conv_cat", "EncoderConv"} <= set(sgr.__all__)
    ref = torch.nn.Conv2d(71, 128, 4, stride=2)
    mod = sgr.EncoderConv(in_channels=(64, 7), out_channels=128)
    assert [k for k, _ in mod.named_parameters()] == ["weight", "bias"] and list(mod.state_dict()) == list(ref.state_dict())
    mod.load_state_dict(ref.state_dict())
    assert torch.equal(mod.weight, ref.weight) and torch.equal(mod.bias, ref.bias) and mod.in_channels == 71 and mod.sources == (64, 7)
    assert "64+7, 128" in repr(mod)
    mm = mod.to("meta")
    assert tuple(mm(m(2, 64, 6, 10), m(2, 7, 6, 10)).shape) == (2, 128, 3, 5)
    torch.manual_seed(7)
    a = sgr.EncoderConv((64, 84), 128)
    torch.manual_seed(7)
    b = torch.nn.Conv2d(148, 128, 4, stride=2)
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)      # initialised as nn.Conv2d(148, 128)

    class Light(torch.nn.Module):      # a reference checkpoint's conv1.* under the encoder's own prefix
        def __init__(self):
            super().__init__()
            self.conv1 = sgr.EncoderConv((64, 7), 128)
    ckpt = torch.nn.ModuleDict(dict(conv1=ref)).state_dict()
    light = Light()
    assert sorted(light.state_dict()) == sorted(ckpt)
    light.load_state_dict(ckpt)
    assert torch.equal(light.conv1.weight, ref.weight)
    # an integer in_channels with one argument is the module as it was
    one = sgr.EncoderConv(17, 64)
    assert one.sources is None and tuple(one.to("meta")(m(2, 17, 6, 10)).shape) == (2, 64, 3, 5) and "17, 64" in repr(one)
    single = sgr.EncoderConv((17,), 64)
    assert tuple(single.to("meta")(m(2, 17, 6, 10)).shape) == (2, 64, 3, 5)
    for bad in ((), (1, 2, 3, 4, 5), (64, 0), (3, -1)):
        with pytest.raises(ValueError, match="positive channel counts.*" + COMPOSE):
            sgr.EncoderConv(bad, 64)
    with pytest.raises(ValueError, match="in_channels 161 is outside 1..160"):
        sgr.EncoderConv((80, 81), 64)
    with pytest.raises(ValueError, match="multiple of 16"):
        sgr.EncoderConv((3, 4), 24)
    with pytest.raises(ValueError, match="2 sources given to a module built with an integer in_channels.*" + COMPOSE):
        one.to("meta")(m(2, 10, 6, 10), m(2, 7, 6, 10))
    for args in ((m(2, 64, 6, 10),), (m(2, 7, 6, 10), m(2, 64, 6, 10)), (m(2, 64, 6, 10), m(2, 7, 6, 10), m(2, 1, 6, 10)), (m(2, 64, 6, 10), m(7, 6, 10))):
        with pytest.raises(ValueError, match=r"the sources must be \[B,C_i,H,W\] with C_i = \(64, 7\).*" + COMPOSE):
            mm(*args)


def test_refusals():
    z = torch.zeros
    two = lambda B=2, H=4, W=6: [m(B, 3, H, W), m(B, 5, H, W)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        sgr.encoder_conv_cat([z(2, 3, 4, 6), z(2, 5, 4, 6)], z(16, 8, 4, 4), z(16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        sgr.encoder_conv_cat([z(2, 3, 4, 6, requires_grad=True), z(2, 5, 4, 6)], z(16, 8, 4, 4), z(16), "zeros")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.encoder_conv_cat_bwd(z(2, 16, 2, 3), [z(2, 3, 4, 6), z(2, 5, 4, 6)], z(16, 8, 4, 4), [3, 5], 4, 6, 0, 3, True, True)
    with pytest.raises(ValueError, match="padding 'reflect'.*" + COMPOSE):
        sgr.encoder_conv_cat(two(), m(16, 8, 4, 4), m(16), "reflect")
    with pytest.raises(TypeError, match="xs must be a list of tensors.*" + COMPOSE):
        sgr.encoder_conv_cat(m(2, 8, 4, 6), m(16, 8, 4, 4), m(16))
    with pytest.raises(RuntimeError, match="pad_mode 2, 0 .replicate. or 1 .zeros.*" + COMPOSE):
        ops.encoder_conv_cat(two(), m(16, 8, 4, 4), m(16), 2)
    # an empty list, five sources
    with pytest.raises(RuntimeError, match="the number of sources must be 1 .. 4, got 0.*" + COMPOSE):
        sgr.encoder_conv_cat([], m(16, 8, 4, 4), m(16))
    with pytest.raises(RuntimeError, match="the number of sources must be 1 .. 4, got 5.*" + COMPOSE):
        sgr.encoder_conv_cat([m(2, 1, 4, 6)] * 5, m(16, 5, 4, 4), m(16))
    with pytest.raises(RuntimeError, match="the number of sources must be 1 .. 4, got 5.*" + COMPOSE):
        sgr.encoder_conv_cat([m(2, 1, 4, 6, grad=True)] * 5, m(16, 5, 4, 4), m(16))
    with pytest.raises(RuntimeError, match="the number of sources must be 1 .. 4, got 5"):
        ops.encoder_conv_cat_bwd(m(2, 16, 2, 3), [m(0)] * 5, m(16, 5, 4, 4), [1] * 5, 4, 6, 0, 1, False, False)
    # differing planes or batches, dims, dtypes
    for bad in (m(2, 5, 4, 8), m(2, 5, 6, 6), m(3, 5, 4, 6)):
        with pytest.raises(RuntimeError, match="the sources must have one batch and one plane.*" + COMPOSE):
            sgr.encoder_conv_cat([m(2, 3, 4, 6), bad], m(16, 8, 4, 4), m(16))
    with pytest.raises(RuntimeError, match=r"xs\[1\] must be \[B,C,H,W\].*" + COMPOSE):
        sgr.encoder_conv_cat([m(2, 3, 4, 6), m(5, 4, 6)], m(16, 8, 4, 4), m(16))
    with pytest.raises(RuntimeError, match="fp32 tensors required.*" + COMPOSE):
        sgr.encoder_conv_cat([m(2, 3, 4, 6), m(2, 5, 4, 6).half()], m(16, 8, 4, 4), m(16))
    with pytest.raises(RuntimeError, match="fp32 tensors required.*" + COMPOSE):
        sgr.encoder_conv_cat([t.double() for t in two()], m(16, 8, 4, 4).double(), m(16).double())
    # a weight whose channel count is not the sum; a 3x3 kernel
    for w in (m(16, 3, 4, 4), m(16, 9, 4, 4), m(16, 8, 3, 3)):
        with pytest.raises(RuntimeError, match=r"weight must be \[O,8,4,4\].*" + COMPOSE):
            sgr.encoder_conv_cat(two(), w, m(16))
    with pytest.raises(RuntimeError, match=r"bias must be \[16\].*" + COMPOSE):
        sgr.encoder_conv_cat(two(), m(16, 8, 4, 4), m(17))
    # the sizes, in encoder_conv's words
    with pytest.raises(RuntimeError, match="161 input channels, 1..160 are supported .the deeper encoder layers.*" + COMPOSE):
        sgr.encoder_conv_cat([m(2, 80, 4, 6), m(2, 81, 4, 6)], m(16, 161, 4, 4), m(16))
    with pytest.raises(RuntimeError, match="a source with 0 channels.*" + COMPOSE):
        sgr.encoder_conv_cat([m(2, 3, 4, 6), m(2, 0, 4, 6)], m(16, 3, 4, 4), m(16))
    for O in (8, 24, 144, 0):
        with pytest.raises(RuntimeError, match=f"{O} output channels, a multiple of 16 in 16..128"):
            sgr.encoder_conv_cat(two(), m(O, 8, 4, 4), m(O), "zeros")
        with pytest.raises(RuntimeError, match=f"{O} output channels"):
            ops.encoder_conv_cat_bwd(m(2, O, 2, 3), [m(0), m(0)], None, [3, 5], 4, 6, 0, 0, False, True)
    for H, W in ((1, 6), (4, 1)):
        with pytest.raises(RuntimeError, match=f"a {H} x {W} map, H and W must be at least 2"):
            sgr.encoder_conv_cat(two(H=H, W=W), m(16, 8, 4, 4), m(16))
    with pytest.raises(RuntimeError, match="zero-sized"):
        sgr.encoder_conv_cat(two(B=0), m(16, 8, 4, 4), m(16))
    # the backward operator
    g = m(2, 16, 2, 3)
    with pytest.raises(RuntimeError, match="no gradient requested"):
        ops.encoder_conv_cat_bwd(g, [m(0), m(0)], None, [3, 5], 4, 6, 0, 0, False, False)
    with pytest.raises(RuntimeError, match="a gradient requested for a source that does not exist"):
        ops.encoder_conv_cat_bwd(g, [m(0), m(0)], m(16, 8, 4, 4), [3, 5], 4, 6, 0, 4, False, False)
    with pytest.raises(RuntimeError, match="2 channel counts but 1 xs"):
        ops.encoder_conv_cat_bwd(g, [m(0)], m(16, 8, 4, 4), [3, 5], 4, 6, 0, 1, False, False)
    with pytest.raises(RuntimeError, match=r"cotangent must be fp32 \[B,O,H/2,W/2\] for H = 4, W = 8"):
        ops.encoder_conv_cat_bwd(g, [m(0), m(0)], m(16, 8, 4, 4), [3, 5], 4, 8, 0, 1, False, False)
    with pytest.raises(RuntimeError, match=r"weight must be fp32 \[16,8,4,4\]"):
        ops.encoder_conv_cat_bwd(g, [m(0), m(0)], m(16, 9, 4, 4), [3, 5], 4, 6, 0, 1, False, False)
    with pytest.raises(RuntimeError, match="weight is needed for dx"):
        ops.encoder_conv_cat_bwd(g, [m(0), m(0)], None, [3, 5], 4, 6, 0, 2, False, False)
    with pytest.raises(RuntimeError, match="xs are needed for dweight"):
        ops.encoder_conv_cat_bwd(g, [m(2, 3, 4, 6), m(0)], None, [3, 5], 4, 6, 0, 0, True, False)
    with pytest.raises(RuntimeError, match=r"xs\[1\] must be fp32 \[2,5,4,6\]"):
        ops.encoder_conv_cat_bwd(g, [m(2, 3, 4, 6), m(2, 4, 4, 6)], None, [3, 5], 4, 6, 0, 0, True, False)
    with pytest.raises(RuntimeError, match="pad_mode -1.*" + COMPOSE):
        ops.encoder_conv_cat_bwd(g, [m(0), m(0)], m(16, 8, 4, 4), [3, 5], 4, 6, -1, 1, False, False)


def test_c_abi_refusals_without_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused before a launch
    ptrs = (ctypes.c_void_p * 4)(4096, 8192, 12288, 16384)
    chan = (ctypes.c_int * 4)(3, 5, 1, 1)
    strides = (ctypes.c_longlong * 16)(72, 24, 6, 1, 120, 24, 6, 1, 24, 24, 6, 1, 24, 24, 6, 1)
    sizes = dict(B=2, O=16, H=4, W=6)

    def fwd(S=2, xs=ptrs, ch=chan, st=strides, w=fake, b=fake, out=fake, mode=0, **kw):
        s = {**sizes, **kw}
        return lib.sgr_encoder_conv_cat_fwd(S, xs, ch, st, w, b, out, s["B"], s["O"], s["H"], s["W"], mode, None)

    def bwd(S=2, g=fake, xs=ptrs, ch=chan, st=strides, w=fake, dxs=ptrs, dw=fake, db=fake, ws=fake, mode=0, **kw):
        s = {**sizes, **kw}
        return lib.sgr_encoder_conv_cat_bwd(S, g, xs, ch, st, w, dxs, dw, db, ws, s["B"], s["O"], s["H"], s["W"], mode, None)
    compose = b"torch.cat(xs, 1), F.pad(x, (1, 1, 1, 1), mode=...) and F.conv2d(., stride=2)"
    for call in (fwd, bwd):
        for S in (0, 5, -1):
            assert call(S=S) == -2 and b"the number of sources must be 1 .. 4" in lib.sgr_last_error() and compose in lib.sgr_last_error(), S
        assert call(ch=None) == -1 and b"NULL tensor" in lib.sgr_last_error()
        assert call(ch=(ctypes.c_int * 4)(3, 0, 1, 1)) == -1 and b"non-positive" in lib.sgr_last_error()
        assert call(ch=(ctypes.c_int * 4)(80, 81, 1, 1)) == -2 and b"160 input channels" in lib.sgr_last_error() and b"deeper encoder layers" in lib.sgr_last_error() \
            and compose in lib.sgr_last_error()
        assert call(ch=(ctypes.c_int * 4)(161, 1, 1, 1)) == -2 and b"160 input channels" in lib.sgr_last_error()
        for k in ("B", "O", "H", "W"):
            for bad in (0, -3):
                assert call(**{k: bad}) == -1 and b"non-positive" in lib.sgr_last_error(), (k, bad)
        for O in (8, 24, 144):
            assert call(O=O) == -2 and b"multiple of 16 in 16..128" in lib.sgr_last_error() and compose in lib.sgr_last_error(), O
        assert call(H=1) == -2 and b"at least 2" in lib.sgr_last_error() and compose in lib.sgr_last_error()
        assert call(W=1) == -2 and b"at least 2" in lib.sgr_last_error()
        for mode in (2, -1):
            assert call(mode=mode) == -2 and b"pad_mode" in lib.sgr_last_error() and compose in lib.sgr_last_error()
        assert call(B=65536) == -2 and b"65535" in lib.sgr_last_error()
        assert call(H=1 << 14, W=1 << 14) == -2 and b"Ho * Wo" in lib.sgr_last_error()
        neg = (ctypes.c_longlong * 16)(72, 24, 6, 1, 120, 24, -6, 1)      # the second source's plane: no negative strides
        assert call(st=neg) == -2 and b"plane strides" in lib.sgr_last_error()
        one_null = (ctypes.c_void_p * 4)(4096, None, 12288, 16384)
        assert call(xs=one_null) == -1 and b"NULL tensor" in lib.sgr_last_error()
    for k in ("xs", "st", "w", "b", "out"):
        assert fwd(**{k: None}) == -1 and b"NULL tensor" in lib.sgr_last_error(), k
    assert bwd(g=None) == -1 and b"NULL cotangent" in lib.sgr_last_error()
    assert bwd(dxs=None, dw=None, db=None) == -1 and b"no gradient requested" in lib.sgr_last_error()
    assert bwd(dxs=(ctypes.c_void_p * 4)(), dw=None, db=None) == -1 and b"no gradient requested" in lib.sgr_last_error()
    for k in ("xs", "st", "w", "ws"):
        assert bwd(**{k: None}) == -1 and b"NULL tensor" in lib.sgr_last_error(), k
    # one source: encoder_conv's own entry points, and their words
    assert fwd(S=1, H=1) == -2 and b"sgr_encoder_conv_fwd" in lib.sgr_last_error()
    assert bwd(S=1, O=24) == -2 and b"sgr_encoder_conv_bwd" in lib.sgr_last_error()
    assert _lib.ABI_VERSION == 6 and lib.sgr_abi_version() == 6      # additive: the version did not move


@contextlib.contextmanager
def autocast_cuda(dtype):
    """what ``torch.autocast('cuda', dtype=dtype)`` switches on, set through the functions it calls: the context manager itself turns into a
    warning where no GPU is present (tests/test_gn_stage_bf16.py); ``torch.autocast`` proper runs in tests/test_gpu_encoder_conv_cat.py"""
    was, was_dtype = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    torch.set_autocast_enabled("cuda", True)
    torch.set_autocast_dtype("cuda", dtype)
    torch.autocast_increment_nesting()
    try:
        yield
    finally:
        if torch.autocast_decrement_nesting() == 0:
            torch.clear_autocast_cache()
        torch.set_autocast_enabled("cuda", was)
        torch.set_autocast_dtype("cuda", was_dtype)


def test_the_autocast_rule_on_fake_device_tensors():
    """bf16 sources give an fp32 result inside an autocast region; with autocast off bf16 is refused"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        mk = lambda *s, dtype=torch.float32, grad=False: torch.empty(*s, device="cuda", dtype=dtype, requires_grad=grad)
        xs = [mk(2, 64, 6, 10, dtype=torch.bfloat16, grad=True), mk(2, 7, 6, 10, dtype=torch.bfloat16)]
        w, b = mk(32, 71, 4, 4, grad=True), mk(32)
        with autocast_cuda(torch.bfloat16):
            out = sgr.encoder_conv_cat(xs, w, b)
            assert out.dtype == torch.float32 and tuple(out.shape) == (2, 32, 3, 5) and out.requires_grad
        with autocast_cuda(torch.bfloat16):      # the backward operator, called directly
            dxs, dw, db = ops.encoder_conv_cat_bwd(mk(2, 32, 3, 5, dtype=torch.bfloat16), [t.detach() for t in xs], w.detach().bfloat16(), [64, 7], 6, 10, 0, 3, True, True)
        assert [d.dtype for d in dxs] == [torch.float32] * 2 and dw.dtype == torch.float32
        with pytest.raises(RuntimeError, match="fp32 tensors required.*" + COMPOSE):
            sgr.encoder_conv_cat(xs, w, b)


@pytest.fixture(scope="module")
def emul():
    d = os.path.join(ROOT, "tests", "host_emul")
    so, srcs = os.path.join(d, "libencoder_conv_cat_emul.so"), [os.path.join(d, "encoder_conv_cat_emul.cpp"), os.path.join(d, "encoder_conv_emul.cpp")]
    hdrs = [os.path.join(ROOT, "inverserenderingofindoorscene_amd", "csrc", h) for h in ("sgr_encoder_conv.h", "sgr_light_final_conv.h", "sgr_final_conv.h", "sgr_math.h")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", srcs[0], "-o", so])
    return ctypes.CDLL(so)


def test_the_tile_loops_with_a_source_table_equal_the_concatenation_bit_for_bit(emul):
    """value, dW, db and each dx against the single-source emulation on the concatenated data, over the GPU test's splits and planes, every
    source in a layout of its own, some sources without a gradient"""
    cases = ctypes.c_int(0)
    assert emul.emul_encoder_conv_cat_selfcheck(ctypes.byref(cases)) == 0 and cases.value == 18


def test_the_host_emulation_runs_clean_under_the_sanitizers(tmp_path):
    """the same self-check as a stand-alone program built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "encoder_conv_cat_emul")
    src = os.path.join(ROOT, "tests", "host_emul", "encoder_conv_cat_emul.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEC_CAT_EMUL_MAIN", src,
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "18 cases, 0 arrays differ" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-2000:])


def load_fixture():
    return np.load(os.path.join(GOLDEN_DIR, "g24_enccat_light.npz"))


def test_the_fixture_is_the_checker_on_the_concatenation():
    z = load_fixture()
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "g24_enccat_light.npz")) <= 1 << 20
    x1, x2, Wt, bias, ct = (torch.from_numpy(z[k]).double() for k in ("x1", "x2", "Wt", "bias", "ct"))
    assert tuple(x1.shape) == (2, 64, 5, 7) and tuple(x2.shape) == (2, 7, 5, 7) and tuple(Wt.shape) == (128, 71, 4, 4) and int(z["pad_mode"]) == 0
    rows = z["dW_rows"]
    assert list(rows) == list(range(0, 128, 8))
    for fn in (C.encoder_conv, C.composition):
        out, (dx, dW, db) = fn(torch.cat([x1, x2], 1), Wt, bias, "replicate", cotangent=ct)
        got = dict(out=out, dx1=dx[:, :64], dx2=dx[:, 64:], dW=dW[rows], db=db)
        for k, v in got.items():
            assert tuple(v.shape) == z[f"{k}64"].shape and err(v, z[f"{k}64"]) <= PIN, (fn.__name__, k, err(v, z[f"{k}64"]))
    for k in ("out", "dx1", "dx2", "dW", "db"):
        assert z[f"{k}64"].dtype == np.float64 and z[f"{k}32"].dtype == np.float32 and np.isfinite(z[f"{k}64"]).all() and np.isfinite(z[f"{k}32"]).all()
        assert abs(float(z[f"e_ref_{k}"]) - err(z[f"{k}32"], z[f"{k}64"])) <= 1e-12 and 0 < float(z[f"e_ref_{k}"]) < 2e-6, k
    assert float((z["x1"] < 0).mean()) > 0.3 and float((z["x2"] < 0).mean()) > 0.3      # signed maps
    assert np.array_equal(z["Wt"] * 64, np.round(z["Wt"] * 64)) and np.abs(z["Wt"]).max() <= 0.25      # the dyadic grid that lets the weights compress
