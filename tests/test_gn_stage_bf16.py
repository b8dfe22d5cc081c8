"""CPU: the same-size GroupNorm stage in bf16 and the autocast rules, without a GPU.

  * ``torch.ops.sgrender.gn_stage`` / ``gn_stage_bwd`` take a bf16 ``x`` (with a bf16 ``skip`` and cotangent): Meta kernels give bf16 results,
    fp32 statistics, bf16 ``dx`` / ``dskip`` and fp32 ``dweight`` / ``dbias`` for every subset of the four flags;
  * mixed ``x`` / ``skip`` dtypes, bf16 parameters and fp16 are refused by the wrapper and the operator (fp16 with today's words), and the
    new C-ABI entries refuse what ``sgr_gn_stage_fwd`` / ``_bwd`` refuse;
  * every functional operator has a kernel for the ``AutocastCUDA`` key, and on fake device tensors under a bf16 autocast ``gn_stage`` keeps
    a bf16 ``x`` while the fp32-policy operators return fp32;
  * the conversions of csrc/sgr_gn_stage.h, compiled for the host (tests/host_emul/gn_stage_bf16_emul.cpp), agree with torch's CPU casts on
    every pattern asked for;
  * the kernels' per-element arithmetic on the host in bf16 equals the existing fp32 emulation's result on the upcast input, rounded once,
    and that fp32 result stays within the GPU tests' bounds of the fp64 checker;
  * the same arithmetic as a stand-alone program runs clean under ``-fsanitize=address,undefined``."""
import contextlib
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import gn_stage_checker as C
from conftest import GOLDEN_DIR, ROOT

import inverserenderingofindoorscene_amd as sgr
from inverserenderingofindoorscene_amd import _lib

BF = torch.bfloat16
FP = ctypes.POINTER(ctypes.c_float)
HP = ctypes.POINTER(ctypes.c_ushort)
EMUL_DIR = os.path.join(ROOT, "tests", "host_emul")
HDRS = [os.path.join(ROOT, "inverserenderingofindoorscene_amd", "csrc", h) for h in ("sgr_gn_stage.h", "sgr_regress.h", "sgr_math.h")]

# the g17 fixtures: (name, part, B, C, G, H, W, Cs)
PARTS = [("dec", "s", 2, 64, 4, 6, 10, 64), ("odd", "s", 3, 256, 16, 3, 5, 256), ("one", "s", 1, 512, 32, 1, 1, 512), ("row", "s", 2, 128, 8, 1, 7, 128),
         ("enc", "gn1", 2, 64, 4, 5, 7, 0), ("enc", "gn6", 2, 1024, 64, 1, 2, 0), ("big", "gn1", 1, 64, 4, 16, 23, 0)]
IDS = [f"{p[0]}-{p[1]}" for p in PARTS]


def m(*shape, dtype=torch.float32, grad=False):
    return torch.empty(*shape, device="meta", dtype=dtype, requires_grad=grad)


def test_meta_kernels_give_bf16_results_and_fp32_statistics_and_parameter_gradients():
    ops = torch.ops.sgrender
    B, Cc, G, H, W, Cs = 3, 12, 4, 5, 7, 5
    for with_skip in (False, True):
        out_shape = (B, Cc + Cs, 2 * H, 2 * W) if with_skip else (B, Cc, H, W)
        skip = m(B, Cs, H, W, dtype=BF) if with_skip else None
        y, stats = ops.gn_stage(m(B, Cc, H, W, dtype=BF), m(Cc), m(Cc), skip, G, 1e-5)
        assert y.dtype == BF and tuple(y.shape) == out_shape and y.is_contiguous()
        assert stats.dtype == torch.float32 and tuple(stats.shape) == (B, G, 4)
        # channels-last bf16 in, contiguous bf16 out
        cl = lambda t: None if t is None else t.contiguous(memory_format=torch.channels_last)
        assert ops.gn_stage(cl(m(B, Cc, H, W, dtype=BF)), m(Cc), m(Cc), cl(skip), G, 1e-5)[0].is_contiguous()
        for need in itertools.product((False, True), repeat=4):
            if not any(need) or (need[3] and not with_skip):
                continue
            side = any(need[:3])
            gx = ops.gn_stage_bwd(m(*out_shape, dtype=BF), m(B, Cc, H, W, dtype=BF) if side else None, m(Cc) if side else None, m(Cc) if side else None,
                                  m(B, G, 4) if side else None, Cc, Cs if with_skip else 0, G, *need)
            want = [((B, Cc, H, W), BF), ((Cc,), torch.float32), ((Cc,), torch.float32), ((B, Cs, H, W), BF)]
            assert [(tuple(t.shape), t.dtype) for t in gx] == [(s if n else (0,), d) for (s, d), n in zip(want, need)], (with_skip, need)
        # through autograd: gradients in the dtype of the tensor they belong to
        x, w, b = m(B, Cc, H, W, dtype=BF, grad=True), m(Cc, grad=True), m(Cc, grad=True)
        s = m(B, Cs, H, W, dtype=BF, grad=True) if with_skip else None
        y = sgr.group_norm_relu_upcat(x, w, b, G, s) if with_skip else sgr.group_norm_relu(x, w, b, G)
        leaves = [x, w, b] + ([s] if with_skip else [])
        gs = torch.autograd.grad(y.sum(), leaves)
        assert [(g.dtype, tuple(g.shape)) for g in gs] == [(t.dtype, tuple(t.shape)) for t in leaves]
    # the module and the equal-size branch of the resize wrappers
    mod = sgr.GroupNormReLU(4, 12, resize=True).to("meta")
    assert mod(m(2, 12, 3, 5, dtype=BF)).dtype == BF and mod(m(2, 12, 3, 5, dtype=BF), m(2, 7, 3, 5, dtype=BF)).dtype == BF
    assert mod(m(2, 12, 3, 5, dtype=BF), size=(3, 5)).dtype == BF
    assert sgr.group_norm_relu_resize_upcat(m(2, 12, 3, 5, dtype=BF), m(12), m(12), 4, m(2, 7, 3, 5, dtype=BF)).dtype == BF
    # fp32 stays fp32
    assert ops.gn_stage(m(B, Cc, H, W), m(Cc), m(Cc), None, G, 1e-5)[0].dtype == torch.float32


def test_refusals_of_the_wrapper_and_the_operator():
    x, w, b, s = m(2, 8, 3, 5, dtype=BF), m(8), m(8), m(2, 4, 3, 5, dtype=BF)
    for call in (lambda *a: sgr.group_norm_relu_upcat(a[0], a[1], a[2], 2, a[3]), lambda *a: torch.ops.sgrender.gn_stage(a[0], a[1], a[2], a[3], 2, 1e-5)):
        with pytest.raises(RuntimeError, match="x BFloat16 and skip Float"):      # both dtypes named
            call(x, w, b, s.float())
        with pytest.raises(RuntimeError, match="x Float and skip BFloat16"):
            call(x.float(), w, b, s)
        with pytest.raises(RuntimeError, match="fp32 weight and bias.*weight BFloat16 and bias Float"):
            call(x, w.to(BF), b, s)
        with pytest.raises(RuntimeError, match="fp32 weight and bias.*weight Float and bias BFloat16"):
            call(x, w, b.to(BF), s)
        with pytest.raises(RuntimeError, match=r"fp32 tensors required \(x Half, weight Float, bias Float, skip Half\)"):      # today's words
            call(x.half(), w, b, s.half())
        with pytest.raises(RuntimeError, match=r"fp32 tensors required \(x BFloat16, weight Float, bias Float, skip Half\)"):
            call(x, w, b, s.half())
        with pytest.raises(RuntimeError, match="fp32 tensors required"):
            call(x.float(), w.to(BF), b, s.float())      # bf16 parameters beside an fp32 x
    with pytest.raises(RuntimeError, match=r"fp32 tensors required \(x Half, weight Half, bias Half\)"):
        sgr.group_norm_relu(x.half(), w.half(), b.half(), 2)
    bwd = torch.ops.sgrender.gn_stage_bwd
    with pytest.raises(RuntimeError, match="x and the cotangent must have one dtype, got x BFloat16 and the cotangent Float"):
        bwd(m(2, 8, 3, 5), x, w, b, m(2, 2, 4), 8, 0, 2, True, False, False, False)
    with pytest.raises(RuntimeError, match="x and the cotangent must have one dtype, got x Float and the cotangent BFloat16"):
        bwd(m(2, 8, 3, 5, dtype=BF), x.float(), w, b, m(2, 2, 4), 8, 0, 2, True, False, False, False)
    with pytest.raises(RuntimeError, match="cotangent must be fp32 or bf16"):
        bwd(m(2, 8, 3, 5).half(), None, None, None, None, 4, 4, 2, False, False, False, True)
    with pytest.raises(RuntimeError, match="weight and bias must be fp32"):
        bwd(m(2, 8, 3, 5, dtype=BF), x, w.to(BF), b, m(2, 2, 4), 8, 0, 2, True, False, False, False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sgr.group_norm_relu(torch.zeros(2, 8, 3, 5, dtype=BF), torch.zeros(8), torch.zeros(8), 2)


def test_the_bf16_c_abi_entries_refuse_what_the_fp32_ones_refuse():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused before a launch
    strides = (ctypes.c_longlong * 4)(120, 15, 5, 1)
    eps = ctypes.c_float(1e-5)
    sizes = dict(B=2, C=8, G=2, Cs=4, H=3, W=5)

    def fwd(x=fake, w=fake, b=fake, skip=fake, out=fake, stats=fake, ws=fake, xs=strides, ss=strides, **kw):
        s = {**sizes, **kw}
        return lib.sgr_gn_stage_fwd_bf16(x, w, b, skip, out, stats, ws, s["B"], s["C"], s["G"], s["Cs"], s["H"], s["W"], xs, ss, eps, None)

    def bwd(g=fake, x=fake, w=fake, b=fake, stats=fake, dx=fake, dw=fake, db=fake, ds=fake, ws=fake, xs=strides, **kw):
        s = {**sizes, **kw}
        return lib.sgr_gn_stage_bwd_bf16(g, x, w, b, stats, dx, dw, db, ds, ws, s["B"], s["C"], s["G"], s["Cs"], s["H"], s["W"], xs, None)
    for k in ("x", "w", "b", "out", "stats", "ws", "xs"):
        assert fwd(**{k: None}) == -1 and b"NULL tensor" in lib.sgr_last_error(), k
    assert fwd(skip=None) == -1 and b"do not agree" in lib.sgr_last_error()
    assert fwd(Cs=0) == -1 and b"do not agree" in lib.sgr_last_error()
    assert bwd(g=None) == -1 and b"NULL cotangent" in lib.sgr_last_error()
    assert bwd(dx=None, dw=None, db=None, ds=None) == -1 and b"no gradient requested" in lib.sgr_last_error()
    for k in ("x", "w", "b", "stats", "ws", "xs"):
        assert bwd(**{k: None}) == -1 and b"NULL tensor" in lib.sgr_last_error(), k
    assert bwd(Cs=0) == -1 and b"dskip requested without skip channels" in lib.sgr_last_error()
    for k in ("B", "C", "G", "H", "W"):
        for bad in (0, -3):
            assert fwd(**{k: bad}) == -1 and b"non-positive" in lib.sgr_last_error(), (k, bad)
            assert bwd(**{k: bad}) == -1 and b"non-positive" in lib.sgr_last_error(), (k, bad)
    assert fwd(G=3) == -1 and bwd(G=3) == -1 and b"not a multiple of num_groups" in lib.sgr_last_error()
    assert fwd(B=65536) == -2 and b"65535" in lib.sgr_last_error()
    neg = (ctypes.c_longlong * 4)(120, 15, -5, 1)
    assert fwd(xs=neg) == -2 and bwd(xs=neg) == -2 and b"plane strides" in lib.sgr_last_error()
    assert fwd(ws=ctypes.c_void_p(4100)) == -1 and b"8-byte aligned" in lib.sgr_last_error()
    assert _lib.ABI_VERSION == 6 and lib.sgr_abi_version() == 6      # additive: the version did not move


# ---- autocast ---------------------------------------------------------------------------------------------------------------------------------

def functional_operators():
    """every sgrender operator that takes a tensor and writes into no argument"""
    names = []
    for s in torch._C._jit_get_all_schemas():
        if s.name.startswith("sgrender::") and not s.is_mutable and any("Tensor" in str(a.type) for a in s.arguments):
            names.append(s.name.split("::")[1])
    return sorted(set(names))


def test_every_functional_operator_has_an_autocast_kernel():
    from test_ops_registration import ALL_OPS
    names = functional_operators()
    writers = {"rescale_grads_", "rescale_grads6_", "allreduce_sum_", "light_objective_stage2", "light_objective_stage2_brdf"}      # `Tensor(a!)` arguments
    listed = set(ALL_OPS) - writers
    since = {"brdf_objective", "brdf_objective_fwd", "brdf_objective_bwd", "batch_ranking_loss", "brdf_encoder_input", "brdf_heads", "brdf_heads_bwd", "bilateral_grid",
             "bilateral_solve", "bilateral_solve_fwd", "bilateral_solve_bwd", "gn_stage", "gn_stage_bwd", "gn_resize", "gn_resize_bwd", "final_conv", "final_conv_bwd",
             "light_final_conv", "light_final_conv_bwd", "encoder_conv", "encoder_conv_bwd", "light_objective_brdf", "attach_grads6"}
    assert listed | since <= set(names), sorted((listed | since) - set(names))
    for name in names:
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sgrender::{name}", "AutocastCUDA"), name
    # operators that write into an argument fall through untouched
    for name in sorted(writers):
        assert getattr(torch.ops.sgrender, name).default._schema.is_mutable, name
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"sgrender::{name}", "AutocastCUDA"), name


@contextlib.contextmanager
def autocast_cuda(dtype):
    """what ``torch.autocast('cuda', dtype=dtype)`` switches on.  The context manager itself turns into a warning where no GPU is
    present, so the state is set through the functions it calls; ``torch.autocast`` proper runs in tests/test_gpu_gn_stage_bf16.py."""
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


def test_autocast_on_fake_device_tensors():
    """Meta kernels behind the Autocast kernels: fake tensors that report a cuda device carry the AutocastCUDA key as real ones do (a plain
    meta tensor does not, and would never reach an autocast rule)"""
    ops = torch.ops.sgrender
    with FakeTensorMode():
        d = lambda *s, dtype=torch.float32, grad=False: torch.empty(*s, device="cuda", dtype=dtype, requires_grad=grad)
        x, w, b = d(2, 8, 3, 5, dtype=BF), d(8, grad=True), d(8, grad=True)
        fc_w, fc_b = d(3, 8, 3, 3), d(3)
        planes = [d(2, c, 3, 5, dtype=BF) for c in (3, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1)]      # (prediction, target) of albedo .. depth, then the three masks
        with autocast_cuda(BF):
            y, stats = ops.gn_stage(x, w, b, None, 2, 1e-5)
            assert y.dtype == BF and stats.dtype == torch.float32 and y.requires_grad
            y, _ = ops.gn_stage(x, w, b, d(2, 4, 3, 5), 2, 1e-5)                         # an fp32 skip is cast to x's dtype
            assert y.dtype == BF and tuple(y.shape) == (2, 12, 6, 10)
            y, _ = ops.gn_stage(x, w.detach().to(BF), b.detach().to(BF), None, 2, 1e-5)  # parameters are cast to fp32
            assert y.dtype == BF
            y, _ = ops.gn_stage(x.float(), w, b, d(2, 4, 3, 5, dtype=BF), 2, 1e-5)       # an fp32 x stays fp32, with its skip
            assert y.dtype == torch.float32
            with torch.device("cuda"):
                mod = sgr.GroupNormReLU(2, 8)
            assert sgr.group_norm_relu(x, w, b, 2).dtype == BF and mod(x).dtype == BF and mod(x, d(2, 4, 3, 5)).dtype == BF
            assert ops.gn_resize(x, w, b, None, 2, 4, 6, 1e-5)[0].dtype == torch.float32
            assert ops.final_conv(x, fc_w, fc_b, None, None, 1, 1e-5)[0].dtype == torch.float32
            assert all(t.dtype == torch.float32 for t in ops.brdf_heads(planes[0], planes[2], None, None, True))
            assert ops.brdf_objective(*planes, None, None, [1.5, 1.0, 0.5, 0.5], 1.0)[0].dtype == torch.float32
            g = ops.gn_stage_bwd(d(2, 8, 3, 5, dtype=BF), x, w.detach(), b.detach(), d(2, 2, 4), 8, 0, 2, True, True, False, False)
            assert g[0].dtype == BF and g[1].dtype == torch.float32
        with autocast_cuda(torch.float16):      # an fp16 autocast: fp16 in, fp32 through the stage
            y, _ = ops.gn_stage(x.half(), w, b, d(2, 4, 3, 5, dtype=torch.float16), 2, 1e-5)
            assert y.dtype == torch.float32
        # autocast off: nothing changes for any input
        assert not torch.is_autocast_enabled("cuda")
        for call in (lambda: ops.gn_resize(x, w, b, None, 2, 4, 6, 1e-5), lambda: ops.final_conv(x, fc_w, fc_b, None, None, 1, 1e-5),
                     lambda: ops.brdf_heads(planes[0], planes[2], None, None, True), lambda: ops.brdf_objective(*planes, None, None, [1.5, 1.0, 0.5, 0.5], 1.0)):
            with pytest.raises(RuntimeError, match="fp32|float32|Float"):
                call()
        assert ops.gn_stage(x, w, b, None, 2, 1e-5)[0].dtype == BF
        with pytest.raises(RuntimeError, match="x BFloat16 and skip Float"):
            ops.gn_stage(x, w, b, d(2, 4, 3, 5), 2, 1e-5)


# ---- the header's conversions and the kernels' arithmetic on the host ---------------------------------------------------------------------

def build(out, flags):
    src = os.path.join(EMUL_DIR, "gn_stage_bf16_emul.cpp")
    if (not os.path.exists(out)) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [src] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + flags + [src, "-o", out])
    return out


@pytest.fixture(scope="module")
def emul():
    return ctypes.CDLL(build(os.path.join(EMUL_DIR, "libgn_stage_bf16_emul.so"), ["-fPIC", "-shared"]))


@pytest.fixture(scope="module")
def emul32():
    """the existing fp32 emulation, built as tests/test_gn_stage.py builds it"""
    so, src = os.path.join(EMUL_DIR, "libgn_stage_emul.so"), os.path.join(EMUL_DIR, "gn_stage_emul.cpp")
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", so])
    return ctypes.CDLL(so)


def test_upcast_of_every_bf16_pattern_is_torchs(emul):
    out = np.empty(65536, np.float32)
    emul.emul_bf16_up_all(out.ctypes.data_as(FP))
    want = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF).float().numpy()      # int32 -> int16 wraps: pattern h
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))                            # bit for bit, NaN payloads included


def test_rounding_is_torchs_round_to_nearest_even(emul):
    lows = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], np.uint32)
    bits = ((np.arange(65536, dtype=np.uint32)[:, None] << 16) | lows[None, :]).reshape(-1)
    f = bits.view(np.float32)
    got = np.empty(f.size, np.uint16)
    emul.emul_bf16_round(f.ctypes.data_as(FP), got.ctypes.data_as(HP), ctypes.c_longlong(f.size))
    want = torch.from_numpy(f.copy()).to(BF).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(f)
    assert nan.sum() == 6 * 2 * 127 + 5 * 2      # every NaN pattern of the probe: exponent all ones, a non-zero mantissa
    assert np.array_equal(got[~nan], want[~nan])
    is_nan16 = lambda h: ((h & 0x7F80) == 0x7F80) & ((h & 0x007F) != 0)
    assert is_nan16(got[nan]).all() and is_nan16(want[nan]).all()                     # NaN stays NaN
    inf = np.isinf(f)
    assert inf.sum() == 2 and np.array_equal(got[inf], (bits[inf] >> 16).astype(np.uint16))      # infinities pass through
    # ties go to even, the largest finite values round up to infinity
    assert got[(bits == 0x3F808000)][0] == 0x3F80 and got[(bits == 0x3F818000)][0] == 0x3F82 and got[(bits == 0x7F7F8000)][0] == 0x7F80


def bf16_bits(a):
    """fp32 array -> (its bf16 rounding as uint16 patterns, the upcast of those as fp32), by torch's CPU cast"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(BF)
    return t.view(torch.int16).numpy().view(np.uint16).copy(), t.float().numpy().copy()


def err(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


@pytest.mark.parametrize("name,part,B,Cc,G,H,W,Cs", PARTS, ids=IDS)
def test_the_bf16_arithmetic_on_the_host_is_the_fp32_emulation_rounded_once(emul, emul32, name, part, B, Cc, G, H, W, Cs):
    z = np.load(os.path.join(GOLDEN_DIR, f"g17_gnstage_{name}.npz"))
    get = lambda k: z[f"{part}_{k}"] if f"{part}_{k}" in z.files else None
    w, b = get("weight"), get("bias")
    xh, x = bf16_bits(get("x"))
    sh, skip = bf16_bits(get("skip")) if Cs else (None, None)
    ch, ct = bf16_bits(get("ct"))
    fp = lambda a: None if a is None else a.ctypes.data_as(FP)
    hp = lambda a: None if a is None else a.ctypes.data_as(HP)
    eps = ctypes.c_float(1e-5)
    out_shape = (B, Cc + Cs, 2 * H, 2 * W) if Cs else (B, Cc, H, W)
    # the existing fp32 emulation on the upcast input
    y32, st32 = np.full(out_shape, np.nan, np.float32), np.empty((B, G, 4), np.float32)
    emul32.emul_gn_stage_fwd(fp(x), fp(w), fp(b), fp(skip), fp(y32), fp(st32), B, Cc, G, Cs, H, W, eps)
    dx32, dw32, db32 = np.full_like(x, np.nan), np.full_like(w, np.nan), np.full_like(b, np.nan)
    ds32 = np.full_like(skip, np.nan) if Cs else None
    emul32.emul_gn_stage_bwd(fp(ct), fp(x), fp(w), fp(b), fp(st32), fp(dx32), fp(dw32), fp(db32), fp(ds32), B, Cc, G, Cs, H, W)
    # the bf16 arithmetic
    y16, st16 = np.zeros(out_shape, np.uint16), np.empty((B, G, 4), np.float32)
    emul.emul_gn_stage_fwd_bf16(hp(xh), fp(w), fp(b), hp(sh), hp(y16), fp(st16), B, Cc, G, Cs, H, W, eps)
    dx16, dw16, db16 = np.zeros(x.shape, np.uint16), np.full_like(w, np.nan), np.full_like(b, np.nan)
    ds16 = np.zeros(skip.shape, np.uint16) if Cs else None
    emul.emul_gn_stage_bwd_bf16(hp(ch), hp(xh), fp(w), fp(b), fp(st16), hp(dx16), fp(dw16), fp(db16), hp(ds16), B, Cc, G, Cs, H, W)
    same = lambda a, c: np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint16), c.view(np.uint32 if c.dtype == np.float32 else np.uint16))
    assert same(st16, st32) and same(dw16, dw32) and same(db16, db32)      # fp32 results: the fp32 emulation's bits
    assert same(y16, bf16_bits(y32)[0]) and same(dx16, bf16_bits(dx32)[0]) and (not Cs or same(ds16, bf16_bits(ds32)[0]))
    assert np.array_equal(dx16 == 0, dx32 == 0)
    # the template on fp32 is the existing emulation, bit for bit: the loops of the two files are the same loops
    y_t, st_t = np.full(out_shape, np.nan, np.float32), np.empty((B, G, 4), np.float32)
    emul.emul_gn_stage_fwd_f32(fp(x), fp(w), fp(b), fp(skip), fp(y_t), fp(st_t), B, Cc, G, Cs, H, W, eps)
    dx_t, dw_t, db_t = np.full_like(x, np.nan), np.full_like(w, np.nan), np.full_like(b, np.nan)
    ds_t = np.full_like(skip, np.nan) if Cs else None
    emul.emul_gn_stage_bwd_f32(fp(ct), fp(x), fp(w), fp(b), fp(st_t), fp(dx_t), fp(dw_t), fp(db_t), fp(ds_t), B, Cc, G, Cs, H, W)
    assert same(y_t, y32) and same(st_t, st32) and same(dx_t, dx32) and same(dw_t, dw32) and same(db_t, db32) and (not Cs or same(ds_t, ds32))
    # that fp32 result against the fp64 checker on the same (bf16-valued) input; e_ref: torch's eager fp32 composition against the checker
    t64 = lambda a: None if a is None else torch.from_numpy(a).double()
    y64, g64 = C.gn_stage(t64(x), t64(w), t64(b), G, t64(skip), cotangent=t64(ct))
    leaves = [torch.from_numpy(a).requires_grad_(True) for a in (x, w, b) + ((skip,) if Cs else ())]
    ye = C.reference_lines(leaves[0], leaves[1], leaves[2], G, leaves[3] if Cs else None)
    ge = torch.autograd.grad(ye, leaves, grad_outputs=torch.from_numpy(ct))
    e, e_ref = err(y32, y64), err(ye.detach(), y64)
    print(f"{name} {part}: values {e:.2e} (bound {max(2 * e_ref, 1e-6):.1e}, e_ref {e_ref:.1e})")
    assert np.isfinite(y32).all() and e <= max(2.0 * e_ref, 1e-6), (name, part, e, e_ref)
    for k, got, eager, ref in zip(("dx", "dw", "db", "ds"), (dx32, dw32, db32, ds32), ge, g64):
        e, e_ref = err(got, ref), err(eager, ref)
        print(f"{name} {part}: {k} {e:.2e} (bound {max(4 * e_ref, 1e-6):.1e}, e_ref {e_ref:.1e})")
        assert np.isfinite(got).all() and e <= max(4.0 * e_ref, 1e-6), (name, part, k, e, e_ref)


def test_the_arithmetic_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """a stand-alone program (its own main, nothing preloaded): the conversions over every pattern and both forms forward and backward"""
    exe = str(tmp_path / "gn_stage_bf16_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-DGN_BF16_EMUL_MAIN", os.path.join(EMUL_DIR, "gn_stage_bf16_emul.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "checksum" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
