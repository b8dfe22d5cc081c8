"""GPU: the same-size GroupNorm stage in bf16 (csrc/sgr_gn_stage.hip instantiated on the I/O type) and the autocast
rules of torch.ops.sgrender.* (csrc/sgr_torch_autocast.cpp).

The yardstick is the fp32 operator already in the tree, which tests/test_gpu_gn_stage.py pins to the reference's fixtures: every bf16
result must be the fp32 operator's result on the upcast input, rounded once to bf16 (torch's ``.to(torch.bfloat16)``, round to nearest
even), bit for bit -- the value and dx / dskip; dweight and dbias must be the fp32 operator's bits.  At the two 30-row shapes, which no
fixture covers, the fp32 operator on the bf16-valued input is itself held to the fp64 checker (tests/gn_stage_checker.py) with the
project's bounds, ``max(2 e_ref, 1e-6)`` for values and ``max(4 e_ref, 1e-6)`` for gradients, ``e_ref`` being the distance of torch's
eager fp32 composition from the checker on the same input: with the equality, every bf16 element is within half a bf16 unit of a pinned
value.

The autocast case compares a small module written here (package operators) with the same module built from torch's own operators, both
under ``torch.autocast('cuda', dtype=torch.bfloat16)``, against the fp64 run: ours may be at most twice as far as torch's (``e_amp``).
Measured on an MI355X (printed by the test): see README.md, "Mixed precision"."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

import gn_stage_checker as C

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# id -> (B, C, G, H, W, Cs for the upcat form, forms, offset, sliced)
SHAPES = {
    "2x64x4x8-vector": (2, 64, 4, 4, 8, 64, ("upcat",), 0.0, False),
    "2x64x6x10": (2, 64, 4, 6, 10, 64, ("upcat", "plain"), 0.0, False),
    "3x256x3x5-unaligned": (3, 256, 16, 3, 5, 256, ("upcat", "plain"), 0.0, False),
    "1x512x1x1-clamped": (1, 512, 32, 1, 1, 512, ("upcat", "plain"), 0.0, False),
    "2x128x1x7-row": (2, 128, 8, 1, 7, 128, ("upcat", "plain"), 0.0, False),
    "2x64x5x8-sliced": (2, 64, 4, 5, 8, 64, ("upcat", "plain"), 0.0, True),
    "1x64x30x40-slices": (1, 64, 2, 30, 40, 64, ("upcat", "plain"), 0.0, False),      # 32 x 1200 elements per group: two moments slices
    "1x64x30x41-slices": (1, 64, 2, 30, 41, 64, ("upcat", "plain"), 0.0, False),
    "1x64x16x24-mean100": (1, 64, 4, 16, 24, 0, ("plain",), 100.0, False),
    "2x1024x1x2": (2, 1024, 64, 1, 2, 0, ("plain",), 0.0, False),
}
CASES = [(sid, form) for sid, s in SHAPES.items() for form in s[6]]
IDS = [f"{sid}-{form}" for sid, form in CASES]
FP64_CASES = [(sid, form) for sid, form in CASES if sid.startswith("1x64x30x4")]


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


def draw(sid, form):
    """bf16-valued x = offset + N(0,1), skip and cotangent; fp32 scales with negative ones and one exact zero.  Every ReLU argument of the
    bf16-valued x is at least 1e-5 from zero in fp64 (elements nearer than 1e-4 are moved by a few bf16 steps; asserted), so that the fp64
    check cannot hinge on a branch.  x of a `sliced` shape is a view x[..., 1:W+1] of a tensor two columns wider: rows of an aligned
    width on a base that is 2 bytes off every boundary."""
    B, Cc, G, H, W, Cs, _, offset, sliced = SHAPES[sid]
    Cs = Cs if form == "upcat" else 0
    g = torch.Generator().manual_seed(1900 + sum(map(ord, sid)))
    x = (offset + torch.randn(B, Cc, H, W, generator=g)).to(BF)
    w = torch.randn(Cc, generator=g)
    w[Cc // 3] = 0.0
    assert int((w < 0).sum()) >= 4
    b = 0.3 * torch.randn(Cc, generator=g)
    b[b.abs() < 1e-3] = 0.05
    skip = torch.randn(B, Cs, H, W, generator=g).to(BF) if Cs else None
    ct = (torch.randn(B, Cc + Cs, 2 * H, 2 * W, generator=g) if Cs else torch.randn(B, Cc, H, W, generator=g)).to(BF)
    for _ in range(12):
        pre, _, _ = C.pre_relu(x.double(), w.double(), b.double(), G)
        bad = pre.abs() < 1e-4
        if not bool(bad.any()):
            break
        x = torch.where(bad, (x.float() * 1.03125 + 0.0625).to(BF), x)
    pre, _, _ = C.pre_relu(x.double(), w.double(), b.double(), G)
    assert float(pre.abs().min()) >= 1e-5, sid
    cu = lambda t: None if t is None else t.cuda()
    x, w, b, skip, ct = cu(x), cu(w), cu(b), cu(skip), cu(ct)
    if sliced:
        def view(t):
            if t is None:
                return None
            wide = torch.zeros(t.shape[0], t.shape[1], t.shape[2], t.shape[3] + 2, device="cuda", dtype=t.dtype)
            v = wide[..., 1:t.shape[3] + 1]
            v.copy_(t)
            assert not v.is_contiguous() and v.data_ptr() % 8 != 0
            return v
        x, skip = view(x), view(skip)
    return x, w, b, G, skip, ct


def run(sgr, x, w, b, G, skip, ct, need=(True, True, True, True)):
    """-> (out, [dx, dw, db, ds]) with None where not required or absent; any dtype"""
    leaves = [t.detach().requires_grad_(n) if t is not None else None for t, n in zip((x, w, b, skip), need)]
    xl, wl, bl, sl = leaves
    y = sgr.group_norm_relu(xl, wl, bl, G) if skip is None else sgr.group_norm_relu_upcat(xl, wl, bl, G, sl)
    live = [t for t in leaves if t is not None and t.requires_grad]
    gs = list(torch.autograd.grad(y, live, grad_outputs=ct)) if live else []
    return y.detach(), [gs.pop(0) if t is not None and t.requires_grad else None for t in leaves]


_CACHE = {}


def case(sgr, sid, form):
    """inputs, the bf16 operator's results and the yardstick (the fp32 operator on the upcast inputs), computed once per case"""
    key = (sid, form)
    if key not in _CACHE:
        args = draw(sid, form)
        x, w, b, G, skip, ct = args
        f = lambda t: None if t is None else t.float()
        _CACHE[key] = (args, run(sgr, *args), run(sgr, f(x), w, b, G, f(skip), f(ct)))
    return _CACHE[key]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.dtype == BF else a, b.view(torch.int16) if b.dtype == BF else b)


@pytest.mark.parametrize("sid,form", CASES, ids=IDS)
def test_bf16_equals_the_fp32_operator_rounded_once(sgr, sid, form):
    (x, w, b, G, skip, ct), (y, gs), (y32, g32) = case(sgr, sid, form)
    assert y.dtype == BF and y.is_contiguous() and y32.dtype == torch.float32 and torch.isfinite(y32).all()
    assert same_bits(y, y32.to(BF)), (sid, form, "value")
    dx, dw, db, ds = gs
    assert dx.dtype == BF and same_bits(dx, g32[0].to(BF)), (sid, form, "dx")
    assert torch.equal(dx == 0, g32[0] == 0), (sid, form, "zero pattern")
    assert dw.dtype == torch.float32 and same_bits(dw, g32[1]) and db.dtype == torch.float32 and same_bits(db, g32[2]), (sid, form, "dweight / dbias")
    if skip is not None:
        assert ds.dtype == BF and same_bits(ds, g32[3].to(BF)), (sid, form, "dskip")
    # every subset of requires_grad: the same bits, a gradient exactly where one is required
    n = 4 if skip is not None else 3
    for need in itertools.product((False, True), repeat=n):
        if not any(need) or all(need):
            continue
        yk, gk = run(sgr, x, w, b, G, skip, ct, need=need + (False,) * (4 - n))
        assert same_bits(yk, y), (sid, form, need)
        for j in range(n):
            assert (gk[j] is None) if not need[j] else same_bits(gk[j], gs[j]), (sid, form, need, j)


@pytest.mark.parametrize("sid,form", CASES, ids=IDS)
def test_two_runs_layouts_the_module_and_the_raw_c_abi_give_the_same_bits(sgr, sid, form):
    (x, w, b, G, skip, ct), (y, gs), _ = case(sgr, sid, form)
    y2, g2 = run(sgr, x, w, b, G, skip, ct)
    assert same_bits(y, y2) and all((a is None and c is None) or same_bits(a, c) for a, c in zip(gs, g2))
    # channels-last and contiguous inputs (and, for the sliced shape, the view): one result
    for f in (lambda t: None if t is None else t.contiguous(), lambda t: None if t is None else t.contiguous(memory_format=torch.channels_last)):
        yl, gl = run(sgr, f(x), w, b, G, f(skip), f(ct))
        assert yl.is_contiguous() and same_bits(y, yl)
        assert all((a is None and c is None) or same_bits(a, c) for a, c in zip(gs, gl))
    # an image does not depend on its batch
    for i in range(x.shape[0] if x.shape[0] > 1 else 0):
        yb, gb = run(sgr, x[i:i + 1], w, b, G, None if skip is None else skip[i:i + 1], ct[i:i + 1])
        assert same_bits(yb, y[i:i + 1]) and same_bits(gb[0], gs[0][i:i + 1]) and (skip is None or same_bits(gb[3], gs[3][i:i + 1])), (sid, form, i)
    # the module in either form
    mod = sgr.GroupNormReLU(G, x.shape[1]).cuda()
    mod.load_state_dict({"weight": w, "bias": b})
    with torch.no_grad():
        assert same_bits(mod(x, skip), y)
    # the raw C-ABI entries
    from inverserenderingofindoorscene_amd import _lib
    lib = _lib.load()
    B, Cc, H, W = x.shape
    Cs = 0 if skip is None else skip.shape[1]
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = lambda t: (ctypes.c_longlong * 4)(*t.stride()) if t is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.full_like(y, float("nan"))
    stats = torch.full((B, G, 4), float("nan"), device="cuda")
    ws = torch.empty(max(lib.sgr_gn_stage_workspace_floats(B, Cc, G, H, W, int(Cs > 0), k) for k in (0, 1)), device="cuda")
    _lib.call("sgr_gn_stage_fwd_bf16", p(x), p(w), p(b), p(skip), p(out), p(stats), p(ws), B, Cc, G, Cs, H, W, st(x), st(skip), ctypes.c_float(1e-5), stream)
    raw = [torch.full_like(g, float("nan")) if g is not None else None for g in gs]
    _lib.call("sgr_gn_stage_bwd_bf16", p(ct), p(x), p(w), p(b), p(stats), *[p(g) for g in raw], p(ws), B, Cc, G, Cs, H, W, st(x), stream)
    torch.cuda.synchronize()
    assert same_bits(out, y) and all((a is None and c is None) or same_bits(a, c) for a, c in zip(raw, gs))
    assert torch.equal(stats, torch.ops.sgrender.gn_stage(x.float(), w, b, None if skip is None else skip.float(), G, 1e-5)[1])      # the fp32 operator's statistics


@pytest.mark.parametrize("sid,form", FP64_CASES, ids=[f"{s}-{f}" for s, f in FP64_CASES])
def test_the_fp32_yardstick_against_the_fp64_checker_at_the_30_row_shapes(sgr, sid, form):
    (x, w, b, G, skip, ct), _, (y32, g32) = case(sgr, sid, form)
    d = lambda t: None if t is None else t.double()
    y64, g64 = C.gn_stage(d(x), d(w), d(b), G, d(skip), cotangent=d(ct))
    # e_ref: torch's eager fp32 composition on the same (bf16-valued) input against the checker
    f = lambda t: None if t is None else t.float().detach().requires_grad_(True)
    leaves = [f(x), f(w), f(b), f(skip)]
    ye = C.reference_lines(leaves[0], leaves[1], leaves[2], G, leaves[3])
    ge = torch.autograd.grad(ye, [t for t in leaves if t is not None], grad_outputs=ct.float())
    e_y, e, lim = err(ye.detach(), y64), err(y32, y64), value_bound(err(ye.detach(), y64))
    print(f"{sid} {form}: values {e:.2e} (bound {lim:.1e}, e_ref {e_y:.1e})")
    assert e <= lim, (sid, form, "values", e, lim)
    for k, got, eager, ref in zip(("dx", "dw", "db", "ds"), g32, list(ge) + [None], g64):
        if ref is None:
            continue
        e_ref = err(eager, ref)
        e, lim = err(got, ref), grad_bound(e_ref)
        print(f"{sid} {form}: {k} {e:.2e} (bound {lim:.1e}, e_ref {e_ref:.1e})")
        assert e <= lim, (sid, form, k, e, lim)
    assert torch.equal(g32[0] == 0, g64[0] == 0)


def test_direct_calls_refuse_what_the_contract_refuses(sgr):
    x, w, b, G, skip, ct = draw("2x64x6x10", "upcat")
    with pytest.raises(RuntimeError, match="x BFloat16 and skip Float"):
        sgr.group_norm_relu_upcat(x, w, b, G, skip.float())
    with pytest.raises(RuntimeError, match="x Float and skip BFloat16"):
        sgr.group_norm_relu_upcat(x.float(), w, b, G, skip)
    with pytest.raises(RuntimeError, match="fp32 weight and bias"):
        sgr.group_norm_relu(x, w.to(BF), b.to(BF), G)
    with pytest.raises(RuntimeError, match="fp32 tensors required"):
        sgr.group_norm_relu(x.half(), w, b, G)
    with pytest.raises(RuntimeError, match="x and the cotangent must have one dtype"):
        torch.ops.sgrender.gn_stage_bwd(ct.float(), x, w, b, torch.zeros(2, G, 4, device="cuda"), 64, 64, G, True, False, False, False)


# ---- autocast, end to end -----------------------------------------------------------------------------------------------------------------

class Net(torch.nn.Module):
    """conv -> stage with an 8-channel skip (upcat) -> conv -> plain stage -> final 3x3 convolution -> albedo head -> masked squared error;
    `ours`: the package's operators, otherwise torch's own for the same function.  The parameter names are the same in both."""

    def __init__(self, sgr, ours):
        super().__init__()
        self.ours, self.sgr = ours, sgr
        self.conv1 = torch.nn.Conv2d(8, 16, 3, padding=1)
        self.conv2 = torch.nn.Conv2d(24, 64, 3, padding=1)
        if ours:
            self.gn1, self.gn2, self.final = sgr.GroupNormReLU(4, 16), sgr.GroupNormReLU(4, 64), sgr.FinalConv(64)
        else:
            self.gn1, self.gn2, self.final = torch.nn.GroupNorm(4, 16), torch.nn.GroupNorm(4, 64), torch.nn.Conv2d(64, 3, 3)

    def forward(self, x, skip, target, mask):
        h1 = self.conv1(x)
        if self.ours:
            s1 = self.gn1(h1, skip)
            s2 = self.gn2(self.conv2(s1))
            a = self.sgr.brdf_head(self.final(s2), 0)
        else:
            s1 = F.interpolate(torch.cat([F.relu(self.gn1(h1)), skip], 1), scale_factor=2, mode="bilinear")
            s2 = F.relu(self.gn2(self.conv2(s1)))
            a = torch.clamp(1.01 * torch.tanh(self.final(F.pad(s2, (1, 1, 1, 1), mode="replicate"))), -1, 1)
        loss = (mask * (a - target) ** 2).sum() / mask.sum() / 3.0
        return loss, s1, s2, a, h1


def test_autocast_end_to_end(sgr):
    torch.manual_seed(1950)
    ours, theirs = Net(sgr, True).cuda(), Net(sgr, False).cuda()
    with torch.no_grad():
        for m in (ours.gn1, ours.gn2):
            m.weight.normal_()
            m.bias.normal_(std=0.3)
    theirs.load_state_dict(ours.state_dict())
    g = torch.Generator().manual_seed(1951)
    x, skip = torch.randn(2, 8, 6, 8, generator=g).cuda(), torch.randn(2, 8, 6, 8, generator=g).cuda()
    target = torch.rand(2, 3, 12, 16, generator=g).cuda() * 2 - 1
    mask = (torch.rand(2, 1, 12, 16, generator=g) > 0.3).float().cuda()
    names = [n for n, _ in ours.named_parameters()]
    assert names == [n for n, _ in theirs.named_parameters()]

    def step(net, amp, dtype=torch.float32):
        net.zero_grad(set_to_none=True)
        c = lambda t: t.to(dtype)
        with torch.autocast("cuda", dtype=BF, enabled=amp):
            loss, s1, s2, a, h1 = net(c(x), c(skip), c(target), c(mask))
        loss.backward()
        return loss.detach(), [p.grad.detach().clone() for p in net.parameters()], (s1, s2, a, h1.detach())

    loss, grads, (s1, s2, a, _) = step(ours, True)
    assert s1.dtype == BF and s2.dtype == BF and a.dtype == torch.float32 and loss.dtype == torch.float32
    assert tuple(s1.shape) == (2, 24, 12, 16) and tuple(s2.shape) == (2, 64, 12, 16)
    for n, p, gr in zip(names, ours.parameters(), grads):
        assert gr.dtype == torch.float32 and p.dtype == torch.float32 and torch.isfinite(gr).all(), n
    loss_t, grads_t, _ = step(theirs, True)
    ref = Net(sgr, False).cuda().double()
    ref.load_state_dict({k: v.double() for k, v in ours.state_dict().items()})
    loss64, grads64, _ = step(ref, False, torch.float64)
    rel = lambda got, want: abs(float(got) - float(want)) / abs(float(want))
    e_amp, e_ours = {"loss": rel(loss_t, loss64)}, {"loss": rel(loss, loss64)}
    for n, go, gt, gr in zip(names, grads, grads_t, grads64):
        e_amp[n], e_ours[n] = err(gt, gr), err(go, gr)
    for k in e_amp:
        print(f"autocast {k}: ours {e_ours[k]:.3e}, torch's own operators under the same autocast (e_amp) {e_amp[k]:.3e}")
    for k in e_amp:
        assert e_ours[k] <= 2.0 * e_amp[k], (k, e_ours[k], e_amp[k])

    # autocast off, fp32 inputs: the fp32 operators as they were -- fp32 throughout, two runs the same bits, and the first stage's bits are
    # those of the fp32 C-ABI entry point (unchanged by this feature) called directly on the same convolution output
    loss0, grads0, (p1, p2, a0, h1) = step(ours, False)
    assert p1.dtype == p2.dtype == a0.dtype == torch.float32
    net_loss, net_grads, (q1, _, _, _) = step(ours, False)
    assert torch.equal(loss0, net_loss) and all(torch.equal(a_, b_) for a_, b_ in zip(grads0, net_grads)) and torch.equal(p1, q1)
    from inverserenderingofindoorscene_amd import _lib
    lib = _lib.load()
    raw = torch.empty(2, 24, 12, 16, device="cuda")
    stats = torch.empty(2, 4, 4, device="cuda")
    ws = torch.empty(lib.sgr_gn_stage_workspace_floats(2, 16, 4, 6, 8, 1, 0), device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda t: (ctypes.c_longlong * 4)(*t.stride())
    _lib.call("sgr_gn_stage_fwd", p(h1), p(ours.gn1.weight), p(ours.gn1.bias), p(skip), p(raw), p(stats), p(ws), 2, 16, 4, 8, 6, 8, st(h1), st(skip),
              ctypes.c_float(ours.gn1.eps), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(raw, p1.detach())
