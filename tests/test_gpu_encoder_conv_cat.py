"""GPU: sgr.encoder_conv_cat / sgr.EncoderConv((C_1, C_2, ..), O) -- the encoders' convolution over several sources.

The contract is bit equality with ``sgr.encoder_conv(torch.cat(xs, 1), ...)``: the value, ``dweight``, ``dbias`` and every ``dxs[i]`` against
its channel slice, for splits that straddle a forward chunk (4 channels), a weight-gradient block (16) and a data-gradient pass (64), in both
pad modes; then the invariances (which sources require grad, their layouts, the batch, the route into the kernels), one exact case against
torch's fp64 convolution, and parity with the fixture the UNMODIFIED reference produced (tests/golden/g24_enccat_light.npz) under the
project's rule: values against fp64 in rel-L2 ``max(2 e_ref, 1e-6)``, gradients ``max(4 e_ref, 1e-6)``."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

F = torch.nn.functional
MODES = ("replicate", "zeros")
SPLITS = [(1, 1), (3, 5, 1), (15, 2), (63, 2), (17, 47, 3), (64, 7), (64, 84), (1, 1, 1, 1), (40, 40, 40, 40)]
PLANES = [(2, 2), (3, 3), (5, 7), (6, 10), (17, 4), (18, 70)]
OUTS = (16, 48, 128)
# the sparse cover: split si meets plane pi where (si + pi) % 3 != 2 -- 36 cases; every split sees four planes, both modes, B = 2 and 3
COVER = [(SPLITS[si], PLANES[pi], OUTS[(si + pi) % 3], 2 + (si + pi) % 2, MODES[(si + pi // 2) % 2]) for si in range(len(SPLITS)) for pi in range(len(PLANES))
         if (si + pi) % 3 != 2]


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


def value_bound(e_ref):
    return max(2.0 * float(e_ref), 1e-6)


def grad_bound(e_ref):
    return max(4.0 * float(e_ref), 1e-6)


def err(got, ref):
    """rel-L2, or max-abs where the reference is zero"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    d = float(ref.norm())
    return float((got - ref).norm()) / d if d > 0 else float(got.abs().max())


def draw(split, O, B, H, W, seed):
    """signed N(0,1) sources, weights N(0, 1/(16 C)), an N(0,1) cotangent"""
    g = torch.Generator().manual_seed(seed)
    Ct = sum(split)
    xs = [torch.randn(B, c, H, W, generator=g).cuda() for c in split]
    Wt = (torch.randn(O, Ct, 4, 4, generator=g) / (16.0 * Ct) ** 0.5).cuda()
    return xs, Wt, (0.1 * torch.randn(O, generator=g)).cuda(), torch.randn(B, O, H // 2, W // 2, generator=g).cuda()


def run_cat(sgr, xs, Wt, bias, ct, mode, need_x=None, need_w=True, need_b=True):
    """-> (out, dxs (None where not required), dW, db)"""
    need_x = [True] * len(xs) if need_x is None else need_x
    lx = [t.detach().requires_grad_(n) for t, n in zip(xs, need_x)]
    lw, lb = Wt.detach().requires_grad_(need_w), bias.detach().requires_grad_(need_b)
    out = sgr.encoder_conv_cat(lx, lw, lb, mode)
    live = [t for t in lx + [lw, lb] if t.requires_grad]
    gs = list(torch.autograd.grad(out, live, grad_outputs=ct, allow_unused=False)) if live else []
    got = [gs.pop(0) if t.requires_grad else None for t in lx + [lw, lb]]
    return out.detach(), got[:len(xs)], got[-2], got[-1]


def run_one(sgr, x, Wt, bias, ct, mode):
    """sgr.encoder_conv on one tensor -> (out, dx, dW, db)"""
    leaves = [t.detach().requires_grad_(True) for t in (x, Wt, bias)]
    out = sgr.encoder_conv(*leaves, padding=mode)
    return (out.detach(), *torch.autograd.grad(out, leaves, grad_outputs=ct))


def slices(dx, split):
    return list(torch.split(dx, list(split), dim=1))


def assert_bits(tag, got, want):
    out, dxs, dW, db = got
    o1, dx1, dW1, db1 = want
    assert torch.equal(out, o1), (tag, "value")
    assert torch.equal(dW, dW1), (tag, "dweight")
    assert torch.equal(db, db1), (tag, "dbias")
    for i, (a, b) in enumerate(zip(dxs, slices(dx1, [t.shape[1] for t in dxs]))):
        assert a.is_contiguous() and torch.equal(a, b), (tag, "dx", i)


@pytest.mark.parametrize("case", COVER, ids=lambda c: "-".join(map(str, c[0])) + f"_{c[1][0]}x{c[1][1]}_O{c[2]}_B{c[3]}_{c[4]}")
def test_bit_equality_with_the_operator_on_the_concatenation(sgr, case):
    split, (H, W), O, B, mode = case
    xs, Wt, bias, ct = draw(split, O, B, H, W, 2400 + 7 * H + W + O + sum(split))
    assert_bits(case, run_cat(sgr, xs, Wt, bias, ct, mode), run_one(sgr, torch.cat(xs, 1), Wt, bias, ct, mode))


@pytest.fixture(scope="module")
def three(sgr):
    """one case for the invariances: (3, 5, 1) on 6 x 10, O = 48, B = 3, both modes -> the bits of the operator on the concatenation"""
    xs, Wt, bias, ct = draw((3, 5, 1), 48, 3, 6, 10, 2450)
    return (xs, Wt, bias, ct), {mode: run_one(sgr, torch.cat(xs, 1), Wt, bias, ct, mode) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_every_subset_of_requires_grad(sgr, three, mode):
    """a source without grad returns None, and the bits of everything else do not change"""
    (xs, Wt, bias, ct), want = three
    o1, dx1, dW1, db1 = want[mode]
    for need in itertools.product((False, True), repeat=5):
        if not any(need):
            continue
        out, dxs, dW, db = run_cat(sgr, xs, Wt, bias, ct, mode, need_x=list(need[:3]), need_w=need[3], need_b=need[4])
        assert torch.equal(out, o1)
        for n, a, b in zip(need[:3], dxs, slices(dx1, (3, 5, 1))):
            assert (a is None) == (not n) and (a is None or torch.equal(a, b)), need
        assert (dW is None) == (not need[3]) and (dW is None or torch.equal(dW, dW1)), need
        assert (db is None) == (not need[4]) and (db is None or torch.equal(db, db1)), need
    x0 = xs[0].detach().requires_grad_(True)      # through .backward(): .grad stays None on a source that does not require it
    sgr.encoder_conv_cat([x0, xs[1], xs[2]], Wt, bias, mode).backward(ct)
    assert torch.equal(x0.grad, slices(dx1, (3, 5, 1))[0]) and xs[1].grad is None


@pytest.mark.parametrize("mode", MODES)
def test_layouts_two_runs_and_an_image_against_its_batch(sgr, three, mode):
    (xs, Wt, bias, ct), want = three
    B, H, W = 3, 6, 10
    cl = xs[0].contiguous(memory_format=torch.channels_last)      # one source channels-last
    big = torch.randn(B, 9, H, W, device="cuda")
    big[:, 2:7] = xs[1]
    part = big[:, 2:7]                                            # another a channel slice of a larger tensor
    wide = torch.zeros(B, 1, H, W + 3, device="cuda")
    wide[..., :W] = xs[2]
    assert not cl.is_contiguous() and not part.is_contiguous() and not wide[..., :W].is_contiguous()
    views = [cl, part, wide[..., :W]]
    assert_bits("layouts", run_cat(sgr, views, Wt, bias, ct, mode), want[mode])
    assert_bits("two runs", run_cat(sgr, views, Wt, bias, ct, mode), want[mode])
    out, dx1 = want[mode][0], want[mode][1]
    for b in range(B):      # an image does not depend on its batch: the value and its dx (dweight and dbias sum over the batch)
        o, dxs, _, _ = run_cat(sgr, [t[b:b + 1] for t in xs], Wt, bias, ct[b:b + 1], mode)
        assert torch.equal(o, out[b:b + 1]) and all(torch.equal(a, s[b:b + 1]) for a, s in zip(dxs, slices(dx1, (3, 5, 1))))


@pytest.mark.parametrize("mode", MODES)
def test_one_source_the_module_and_the_raw_c_entries(sgr, three, mode):
    (xs, Wt, bias, ct), want = three
    cat = torch.cat(xs, 1)
    o, dxs, dW, db = run_cat(sgr, [cat], Wt, bias, ct, mode)      # S == 1 is sgr.encoder_conv
    assert_bits("S == 1", (o, dxs, dW, db), want[mode])
    mod = sgr.EncoderConv((3, 5, 1), 48, padding=mode).cuda()
    with torch.no_grad():
        mod.weight.copy_(Wt)
        mod.bias.copy_(bias)
    lx = [t.detach().requires_grad_(True) for t in xs]
    out = mod(*lx)
    gs = torch.autograd.grad(out, lx + [mod.weight, mod.bias], grad_outputs=ct)
    assert_bits("module", (out.detach(), list(gs[:3]), gs[3], gs[4]), want[mode])
    # the raw C entries: outputs pre-filled with NaN; the second source wants no gradient and its buffer is not passed
    from inverserenderingofindoorscene_amd import _lib
    lib = _lib.load()
    B, H, W, O, pm = 3, 6, 10, 48, MODES.index(mode)
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in xs])
    chan = (ctypes.c_int * 4)(3, 5, 1)
    strides = (ctypes.c_longlong * 16)(*[s for t in xs for s in t.stride()])
    out_r, ws = f(B, O, H // 2, W // 2), f(lib.sgr_encoder_conv_workspace_floats(B, 9, O, H, W))
    _lib.call("sgr_encoder_conv_cat_fwd", 3, ptrs, chan, strides, ctypes.c_void_p(Wt.data_ptr()), ctypes.c_void_p(bias.data_ptr()), ctypes.c_void_p(out_r.data_ptr()), B, O,
              H, W, pm, stream)
    d0, d2, dW_r, db_r = f(B, 3, H, W), f(B, 1, H, W), f(O, 9, 4, 4), f(O)
    dptr = (ctypes.c_void_p * 4)(d0.data_ptr(), None, d2.data_ptr())
    _lib.call("sgr_encoder_conv_cat_bwd", 3, ctypes.c_void_p(ct.data_ptr()), ptrs, chan, strides, ctypes.c_void_p(Wt.data_ptr()), dptr, ctypes.c_void_p(dW_r.data_ptr()),
              ctypes.c_void_p(db_r.data_ptr()), ctypes.c_void_p(ws.data_ptr()), B, O, H, W, pm, stream)
    torch.cuda.synchronize()
    s = slices(want[mode][1], (3, 5, 1))
    assert torch.equal(out_r, want[mode][0]) and torch.equal(d0, s[0]) and torch.equal(d2, s[2]) and torch.equal(dW_r, want[mode][2]) and torch.equal(db_r, want[mode][3])


def test_a_replayed_hip_graph_opcheck_and_deterministic_mode(sgr, three):
    (xs, Wt, bias, ct), want = three
    ops = torch.ops.sgrender
    # a captured graph: the table travels in the kernel arguments, so the replay reads the sources where they are
    sx = [t.clone() for t in xs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up outside the capture (the recipe of tests/test_gpu_graph.py)
        for _ in range(3):
            ops.encoder_conv_cat(sx, Wt, bias, 0)
            ops.encoder_conv_cat_bwd(ct, sx, Wt, [3, 5, 1], 6, 10, 0, 5, True, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.encoder_conv_cat(sx, Wt, bias, 0)
        dxs, dW, db = ops.encoder_conv_cat_bwd(ct, sx, Wt, [3, 5, 1], 6, 10, 0, 5, True, True)
    for t in sx:
        t.zero_()
    for t, src in zip(sx, xs):
        t.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    s = slices(want["replicate"][1], (3, 5, 1))
    assert torch.equal(out, want["replicate"][0]) and torch.equal(dxs[0], s[0]) and dxs[1].numel() == 0 and torch.equal(dxs[2], s[2])
    assert torch.equal(dW, want["replicate"][2]) and torch.equal(db, want["replicate"][3])
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")      # aot_dispatch compares gradients through a second path
    live = [t.detach().requires_grad_(True) for t in xs]
    torch.library.opcheck(ops.encoder_conv_cat, (live, Wt.detach().requires_grad_(True), bias.detach().requires_grad_(True), 0), test_utils=tests)
    torch.library.opcheck(ops.encoder_conv_cat, ([live[0], xs[1], xs[2]], Wt, bias, 1), test_utils=tests)
    torch.library.opcheck(ops.encoder_conv_cat_bwd, (ct, xs, Wt, [3, 5, 1], 6, 10, 0, 7, True, True), test_utils=tests)
    empty = torch.empty(0, device="cuda")
    torch.library.opcheck(ops.encoder_conv_cat_bwd, (ct, [empty] * 3, Wt, [3, 5, 1], 6, 10, 1, 2, False, True), test_utils=tests)
    torch.use_deterministic_algorithms(True)
    try:
        assert_bits("deterministic", run_cat(sgr, xs, Wt, bias, ct, "replicate"), want["replicate"])
    finally:
        torch.use_deterministic_algorithms(False)


@pytest.mark.parametrize("mode", MODES)
def test_exact_case_over_every_boundary_at_once(sgr, mode):
    """one-hot and small-integer weights and sources, every fp32 sum exact, over a split that straddles a forward chunk (3 | 4), a
    weight-gradient block (.. 15 | 16 ..) and a data-gradient pass (.. 63 | 64 ..): equal to torch's fp64 convolution of the concatenation"""
    split, O, B, H, W = (3, 12, 48, 3), 32, 2, 7, 10
    assert sum(split[:1]) == 3 and sum(split[:2]) == 15 and sum(split[:3]) == 63
    g = torch.Generator().manual_seed(2460)
    xs = [torch.randint(-3, 4, (B, c, H, W), generator=g).float().cuda() for c in split]
    Ct = sum(split)
    Wt = torch.randint(-2, 3, (O, Ct, 4, 4), generator=g).float()
    for o in range(0, O, 2):      # every other output is a one-hot tap of one channel
        Wt[o] = 0
        Wt[o, (5 * o) % Ct, o % 4, (o // 4) % 4] = 1
    Wt, bias = Wt.cuda(), torch.randint(-3, 4, (O,), generator=g).float().cuda()
    ct = torch.randint(-2, 3, (B, O, H // 2, W // 2), generator=g).float().cuda()
    out, dxs, dW, db = run_cat(sgr, xs, Wt, bias, ct, mode)
    x64 = torch.cat(xs, 1).double().requires_grad_(True)
    w64, b64 = Wt.double().requires_grad_(True), bias.double().requires_grad_(True)
    o64 = F.conv2d(F.pad(x64, (1, 1, 1, 1), mode="replicate" if mode == "replicate" else "constant"), w64, b64, stride=2)
    gx, gw, gb = torch.autograd.grad(o64, [x64, w64, b64], grad_outputs=ct.double())
    assert torch.equal(out.double(), o64.detach()) and torch.equal(dW.double(), gw) and torch.equal(db.double(), gb)
    assert all(torch.equal(a.double(), s) for a, s in zip(dxs, slices(gx, split)))


def test_parity_with_the_reference_fixture(sgr):
    """models.encoderLight(SGNum=1, cascadeLevel=1).conv1 on (preProcess's 64 channels, envs' 7): values max(2 e_ref, 1e-6), gradients
    max(4 e_ref, 1e-6) rel-L2 of the reference's fp64 arrays; dweight on the stored rows"""
    z = np.load(os.path.join(GOLDEN_DIR, "g24_enccat_light.npz"))
    x1, x2, Wt, bias, ct = (torch.from_numpy(z[k]).cuda() for k in ("x1", "x2", "Wt", "bias", "ct"))
    out, (dx1, dx2), dW, db = run_cat(sgr, [x1, x2], Wt, bias, ct, "replicate")
    got = dict(out=out, dx1=dx1, dx2=dx2, dW=dW[torch.from_numpy(z["dW_rows"]).cuda()], db=db)
    for k, v in got.items():
        e, e_ref = err(v, z[f"{k}64"]), float(z[f"e_ref_{k}"])
        lim = value_bound(e_ref) if k == "out" else grad_bound(e_ref)
        print(f"g24_enccat_light: {k} {e:.2e} (bound {lim:.1e}, e_ref {e_ref:.1e})")
        assert torch.isfinite(v).all() and e <= lim, (k, e, lim)


def test_the_chain_of_a_cascade_1_light_encoder(sgr):
    """sgr.light_encoder_input -> EncoderConv(11, 32) -> GroupNormReLU -> EncoderConv(32, 64, 'zeros') -> GroupNormReLU ->
    EncoderConv((64, 7), 128)(input1, envs) on a 2 x 24 x 32 image, against the fp64 torch composition on the same input batch"""
    g = torch.Generator().manual_seed(2470)
    r = lambda *s: torch.rand(*s, generator=g).cuda()
    B, h, w = 2, 12, 16
    batch = sgr.light_encoder_input(r(B, 3, h, w), r(B, 3, h, w), r(B, 3, h, w) - 0.5, r(B, 1, h, w), r(B, 1, h, w) + 0.1, size=(24, 32))[0]
    envs = (r(B, 7, 6, 8) - 0.5).requires_grad_(True)
    torch.manual_seed(2471)
    mods = [sgr.EncoderConv(11, 32), sgr.GroupNormReLU(2, 32), sgr.EncoderConv(32, 64, "zeros"), sgr.GroupNormReLU(4, 64), sgr.EncoderConv((64, 7), 128)]
    c0, g0, c1, g1, c2 = [mod.cuda() for mod in mods]
    with torch.no_grad():
        for gn in (g0, g1):
            gn.weight.uniform_(0.5, 1.5)
            gn.bias.uniform_(-0.2, 0.2)
    ct = torch.randn(B, 128, 3, 4, generator=g).cuda()
    out = c2(g1(c1(g0(c0(batch)))), envs)
    params = [c0.weight, c1.weight, c2.weight, c2.bias]
    grads = torch.autograd.grad(out, [envs] + params, grad_outputs=ct)

    def eager(dt):
        p = lambda t: t.detach().to(dt).requires_grad_(True)
        e, w0, w1, w2, b2 = p(envs), p(c0.weight), p(c1.weight), p(c2.weight), p(c2.bias)
        y = F.conv2d(F.pad(batch.to(dt), (1, 1, 1, 1), mode="replicate"), w0, c0.bias.detach().to(dt), stride=2)
        y = F.relu(F.group_norm(y, 2, g0.weight.detach().to(dt), g0.bias.detach().to(dt)))
        y = F.conv2d(F.pad(y, (1, 1, 1, 1)), w1, c1.bias.detach().to(dt), stride=2)
        y = F.relu(F.group_norm(y, 4, g1.weight.detach().to(dt), g1.bias.detach().to(dt)))
        o = F.conv2d(F.pad(torch.cat([y, e], 1), (1, 1, 1, 1), mode="replicate"), w2, b2, stride=2)
        return o.detach(), torch.autograd.grad(o, [e, w0, w1, w2, b2], grad_outputs=ct.to(dt))
    o64, g64 = eager(torch.float64)
    o32, g32 = eager(torch.float32)
    out = out.detach()
    e, lim = err(out, o64), value_bound(err(o32, o64))
    print(f"chain: values {e:.2e} (bound {lim:.1e}, e_ref {err(o32, o64):.1e})")
    assert tuple(out.shape) == (B, 128, 3, 4) and e <= lim, (e, lim)
    for name, a, b64, b32 in zip(("denvs", "dW preProcess.1", "dW preProcess.5", "dW conv1", "db conv1"), grads, g64, g32):
        e, lim = err(a, b64), grad_bound(err(b32, b64))
        print(f"chain: {name} {e:.2e} (bound {lim:.1e}, e_ref {err(b32, b64):.1e})")
        assert e <= lim, (name, e, lim)


def test_autocast(sgr):
    """inside a bf16 region on bf16 sources the call gives the bits of the call with autocast off on the upcast sources, and a bf16 leaf gets
    that gradient rounded once"""
    xs, Wt, bias, ct = draw((64, 7), 32, 2, 6, 10, 2480)
    hs = [t.bfloat16() for t in xs]
    want = run_cat(sgr, [t.float() for t in hs], Wt, bias, ct, "replicate")
    leaf = hs[0].detach().requires_grad_(True)
    w = Wt.detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = sgr.encoder_conv_cat([leaf, hs[1]], w, bias)
    assert out.dtype == torch.float32 and torch.equal(out.detach(), want[0])
    gx, gw = torch.autograd.grad(out, [leaf, w], grad_outputs=ct)
    assert gx.dtype == torch.bfloat16 and torch.equal(gx, want[1][0].bfloat16()) and gw.dtype == torch.float32 and torch.equal(gw, want[2])
    with pytest.raises(RuntimeError, match="fp32 tensors required"):
        sgr.encoder_conv_cat(hs, Wt, bias)
