"""GPU: every fp32-policy operator of torch.ops.sgrender.* through its autocast rule (csrc/sgr_torch_autocast.cpp), by
way of the public wrappers, values and gradients.

The contract is "cast, then the fp32 operator", so the yardstick is exact: the inputs are drawn in fp32 and rounded to the low-precision
type, and a call inside ``torch.autocast('cuda', dtype=...)`` on the low-precision tensors must give the BITS of the same call with autocast
off on the upcast tensors (which the operators' own test files pin against fp64) -- fp32 outputs ``torch.equal``, integer and bool outputs
equal, the gradient of a low-precision leaf that gradient's fp32 value rounded once (``g32.to(dtype)``), the gradient of an fp32 parameter
fp32 with equal bits.  Two autocast-off runs are compared first (every operator here is bit-reproducible).  Per wrapper, ``VARIANTS``:

  low        every floating input bf16 (parameters stay fp32, as under a real autocast), ``backward`` outside the region
  fp32       fp32 inputs inside the region: the rule is a no-op
  first      only the first floating input bf16          rest      all but the first bf16 (siblings: one fp32 sibling beside bf16 ones)
  inside     ``torch.autograd.grad`` within the ``with``: the ``*_bwd`` operators go through their own rule
  fp16       fp16 inputs under an fp16 autocast
  cl         bf16 inputs, the 4-D ones channels-last (what ``nn.Conv2d`` hands over under autocast)

Each low-precision leaf enters one argument only (a leaf used twice would accumulate twice in bf16).  Then: autocast off refuses bf16
(one operator per family), a step captured in a HIP graph inside the region, the sharded route (world of one, in a subprocess) and one
light step end to end against fp64 beside torch's own operators under the same autocast (``e_ours <= 2 e_amp``, both printed)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from autocast_cases import CASE_IDS, Case, flatten, get_case, is_float, rnd, sg_inputs, uni
from conftest import ROOT
from oracle import sg_oracle as O

pytestmark = pytest.mark.gpu

BF, HF, FP = torch.bfloat16, torch.float16, torch.float32
VARIANTS = ("low", "fp32", "first", "rest", "inside", "fp16", "cl")


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


def run(case, low, lows, amp, inside=False, channels_last=False):
    """One call of the case: the floating arguments hold values representable in ``low`` (rounded here), those named in ``lows`` in that
    dtype and the others upcast to fp32; under ``torch.autocast('cuda', dtype=low)`` when ``amp``.  -> (outputs, gradients by leaf name)"""
    leaves, kw = {}, {}
    case.bind(lambda make: make().cuda())
    for name, t in case.args.items():
        if not isinstance(t, torch.Tensor):
            kw[name] = t
            continue
        x = t.cuda()
        if is_float(x):
            x = x.to(low) if name not in case.params else x
            x = x if name in lows else x.float()
            if channels_last and x.dim() == 4 and name in lows:
                x = x.contiguous(memory_format=torch.channels_last)
            x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(name in case.grads)
            if x.requires_grad:
                leaves[name] = x
        kw[name] = x
    if case.module is not None:
        case.module.zero_grad(set_to_none=True)
        leaves.update({"module." + n: p for n, p in case.module.named_parameters()})

    def backward(outs):
        live = [o for o in outs if o is not None and is_float(o) and o.requires_grad]
        g = torch.Generator().manual_seed(77)
        cts = [torch.randn(o.shape, generator=g).to(o.dtype).cuda() for o in live]
        if not live or not leaves:
            return {}
        gs = torch.autograd.grad(live, list(leaves.values()), grad_outputs=cts, allow_unused=True)
        return {n: v for n, v in zip(leaves, gs) if v is not None}

    with torch.autocast("cuda", dtype=low, enabled=amp):
        outs = flatten(case.fn(**kw))
        grads = backward(outs) if inside else None
    if grads is None:
        grads = backward(outs)
    torch.cuda.synchronize()
    return [None if o is None else o.detach() for o in outs], grads, {n: v.dtype for n, v in leaves.items()}


def bits(t):
    return t.view(torch.int16) if t.dtype in (BF, HF) else t


def check_contract(case, variants=VARIANTS):
    names = [n for n, t in case.args.items() if is_float(t) and n not in case.params]
    ref = {}
    for low in (BF, HF):
        if low is HF and "fp16" not in variants:
            continue
        outs, grads, _ = run(case, low, (), False)
        outs2, grads2, _ = run(case, low, (), False)
        assert len(outs) == len(outs2) and grads.keys() == grads2.keys()
        for a, c in zip(outs, outs2):      # two autocast-off runs: the same bits
            assert (a is None and c is None) or torch.equal(a, c), "the operator is not bit-reproducible"
        assert all(torch.equal(grads[k], grads2[k]) for k in grads), "the gradients are not bit-reproducible"
        assert any(o is not None for o in outs) and all(o is None or not is_float(o) or (o.dtype == FP and bool(torch.isfinite(o).all())) for o in outs)
        assert set(grads) >= set(case.grads), (sorted(grads), case.grads)      # every leaf that asks for a gradient gets one
        ref[low] = (outs, grads)
    for v in variants:
        low = HF if v == "fp16" else BF
        lows = {"low": names, "fp32": [], "first": names[:1], "rest": names[1:], "inside": names, "fp16": names, "cl": names}[v]
        outs, grads, dtypes = run(case, low, lows, True, inside=(v == "inside"), channels_last=(v == "cl"))
        want, want_g = ref[low]
        assert len(outs) == len(want), v
        for i, (a, c) in enumerate(zip(outs, want)):
            assert (a is None) == (c is None), (v, i)
            if a is not None:
                assert a.dtype == c.dtype and a.shape == c.shape and torch.equal(a, c), (v, "output", i, a.dtype)
        assert grads.keys() == want_g.keys(), (v, sorted(grads), sorted(want_g))
        for n, g in grads.items():
            dt = dtypes[n]
            assert dt == (low if n in lows else FP), (v, n, dt)
            assert g.dtype == dt and torch.equal(bits(g), bits(want_g[n].to(dt))), (v, "gradient", n)


@pytest.mark.parametrize("family,name", [(f, n) for f, ns in CASE_IDS.items() for n in ns], ids=[n for ns in CASE_IDS.values() for n in ns])
def test_autocast_is_the_fp32_operator_on_the_upcast_input(sgr, family, name):
    case = get_case(sgr, family, name)
    if name.endswith("-fp16"):      # the same-size stage keeps bf16: its fp32 rule is the fp16 one
        check_contract(case, variants=("fp16",))
    else:
        check_contract(case)


def test_the_live_regression_runs_in_fp32_inside_the_region(sgr):
    """LSregressDiffSpec with grad-carrying ``diff`` / ``spec`` differentiates through the coefficients with torch's own matrix products,
    which autocast would run in bf16: the wrapper keeps them out of it"""
    R, C = 5, 7
    ds = dict(diff=uni(2, 3, R, C, seed=99), spec=uni(2, 3, R, C, seed=100), imOrig=uni(2, 3, R, C, seed=101), diffOrig=uni(2, 3, R, C, seed=102), specOrig=uni(2, 3, R, C, seed=103))
    check_contract(Case(sgr.LSregressDiffSpec, ds, grads=("diff", "spec", "diffOrig", "specOrig")), variants=("low", "fp32", "first", "inside"))


def test_backward_operators_called_directly_inside_the_region(sgr):
    """An autograd node keeps the tensors its forward saw AFTER the cast, so through ``backward`` a ``*_bwd`` operator's rule only ever
    sees fp32.  Called directly with bf16 tensors (a caller of ``torch.ops`` composing its own backward) the rule itself has to cast."""
    ops = torch.ops.sgrender
    K, R, C = 12, 5, 7
    calls = {
        "encoder_conv_bwd": lambda c: ops.encoder_conv_bwd(c(rnd(2, 16, 3, 4, seed=150)), c(rnd(2, 5, 7, 9, seed=1)), rnd(16, 5, 4, 4, seed=2, scale=0.2).cuda(), 7, 9, 0, True, True, True),
        "light_final_conv_bwd": lambda c: ops.light_final_conv_bwd(c(rnd(2, 17, 5, 7, seed=151)), c(rnd(2, 16, 5, 7, seed=4)), rnd(17, 16, 3, 3, seed=5, scale=0.2).cuda(), True, True, True),
        "light_heads_bwd": lambda c: ops.light_heads_bwd(c(rnd(2, 3 * K, R, C, seed=80)), c(rnd(2, K, R, C, seed=81)), c(rnd(2, 3 * K, R, C, seed=82)), c(rnd(2, K, 3, R, C, seed=152)),
                                                          c(rnd(2, K, R, C, seed=153)), c(rnd(2, 3 * K, R, C, seed=154)), None),
        "brdf_heads_bwd": lambda c: ops.brdf_heads_bwd(*[c(rnd(2, 3, 5, 7, seed=40 + i)) for i in range(4)], c(rnd(2, 3, 5, 7, seed=155)), c(rnd(2, 3, 5, 7, seed=156)), c(rnd(2, 1, 5, 7, seed=157)),
                                                        c(rnd(2, 1, 5, 7, seed=158)), True, True, True, True, True),
    }
    x = sg_inputs(K, 8, 16, 1)
    calls["sg_to_env_bwd"] = lambda c: ops.sg_to_env_bwd(c(rnd(2, 3, R, C, 8, 16, seed=159)), c(x["axis"]), c(x["lamb"]), c(x["weight"]), 8, 16, 1)
    for name, call in calls.items():
        want = call(lambda t: t.to(BF).float().cuda())
        with torch.autocast("cuda", dtype=BF):
            got = call(lambda t: t.to(BF).cuda())
            same = call(lambda t: t.to(BF).float().cuda())
        with pytest.raises(RuntimeError, match="fp32"):      # autocast off: refused, in each operator's own words
            call(lambda t: t.to(BF).cuda())
        for a, b, c in zip(got, same, want):
            assert a.dtype == FP and torch.isfinite(c).all() and torch.equal(a, c) and torch.equal(b, c), name


def test_autocast_off_refuses_bf16(sgr):
    """one operator per family, with that operator's message; the operators allocate their results after the check, and the same call in
    fp32 gives its usual bits afterwards"""
    calls = {}
    for family, name, arg in (("conv", "encoder_conv-replicate", "x"), ("conv", "light_final_conv", "y"), ("conv", "final_conv", "y"), ("gn", "group_norm_relu_resize", "x"),
                              ("gn", "group_norm_relu_resize_upcat_siblings", "x1"), ("brdf", "brdf_heads-unit1", "xN"), ("brdf", "brdf_encoder_input", "albedoPre"),
                              ("brdf", "brdf_objective", "normalPred"), ("brdf", "batch_ranking_loss", "albedoPred"), ("bilateral", "bilateral_solve-mode0", "pred"),
                              ("glue", "light_heads", "xLamb"), ("glue", "LSregress", "pred"), ("render", "forwardSG-k12_8x16-1x", "axis"),
                              ("render", "render_loss-k12_8x16-1x", "im"), ("render", "recon_loss-k12_8x16-1x", "env"), ("objective", "light_objective-2x", "lamb"),
                              ("objective", "light_objective-brdf_grads-2x", "rough")):
        calls[name] = (get_case(sgr, family, name), arg)
    words = {"encoder_conv-replicate": "encoder_conv: fp32 tensors required", "light_final_conv": "light_final_conv: fp32 tensors required", "final_conv": "final_conv: fp32 tensors required",
             "group_norm_relu_resize": "gn_resize: fp32 tensors required", "brdf_heads-unit1": "brdf_heads: fp32 tensors required, .* is BFloat16",
             "brdf_encoder_input": "brdf_encoder_input: fp32 tensors required", "brdf_objective": "brdf_objective: fp32 tensors required",
             "group_norm_relu_resize_upcat_siblings": "one dtype", "batch_ranking_loss": "batch_ranking_loss: fp32 albedoPred required, got BFloat16"}
    for name, (case, arg) in calls.items():
        before, _, _ = run(case, BF, (), False)
        with pytest.raises(RuntimeError, match=words.get(name, "fp32 tensors required")):
            run(case, BF, (arg,), False)
        after, _, _ = run(case, BF, (), False)
        assert all((a is None and c is None) or torch.equal(a, c) for a, c in zip(before, after)), name


# ---- a captured step ------------------------------------------------------------------------------------------------------------------------
def test_a_step_captured_inside_the_region_replays_the_eager_autocast_bits(sgr):
    """encoder_conv -> group_norm_relu -> light_final_conv x 3 -> light_objective(decoder_outputs=True), forward and backward, on bf16 inputs"""
    K, R, C = 12, 6, 8
    layer = sgr.renderingLayer(imWidth=C, imHeight=R)
    torch.manual_seed(140)
    enc, gn = sgr.EncoderConv(11, 32).cuda(), sgr.GroupNormReLU(4, 32).cuda()
    fins = [sgr.LightFinalConv(32, o).cuda() for o in (3 * K, K, 3 * K)]
    params = [p for m in [enc, gn] + fins for p in m.parameters()]

    def draw(seed):
        inp = O.synthetic_inputs(2, 2 * R, 2 * C, R, C, K, seed=seed)
        ind = torch.ones(2, 1, 1, 1)
        t = [rnd(2, 11, 2 * R, 2 * C, seed=seed + 1)] + [inp[k] for k in ("albedo", "normal", "rough", "im", "seg", "env_gt")] + [ind]
        return [v.to(BF).cuda() for v in t]

    def step(x, albedo, normal, rough, im, seg, env_gt, ind):
        h = gn(enc(x))
        obj = sgr.light_objective(layer, albedo, normal, rough, fins[0](h), fins[1](h), fins[2](h), im, seg, env_gt, ind, 1.0, 10.0, decoder_outputs=True)
        return tuple(obj) + tuple(torch.autograd.grad(obj[0], params))
    static = draw(141)
    with torch.autocast("cuda", dtype=BF):
        captured = sgr.capture_step(lambda: step(*static))
        for seed in (143, 145):
            fresh = draw(seed)
            with torch.no_grad():
                for s, f in zip(static, fresh):
                    s.copy_(f)
            got = [o.clone() for o in captured()]
            torch.cuda.synchronize()
            want = step(*fresh)
            torch.cuda.synchronize()
            assert len(got) == 5 + len(params)
            for a, c in zip(got, want):
                assert a.dtype == FP and torch.equal(a, c) and torch.isfinite(a).all()


# ---- the sharded route: a world of one over RCCL, in a subprocess ----------------------------------------------------------------------------
WORKER = r'''
import json, os, sys, torch
import torch.distributed as dist
sys.path.insert(0, os.environ["SGR_ROOT"])
import inverserenderingofindoorscene_amd as sgr
from oracle import sg_oracle as O          # checker-side input generator only
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
BF = torch.bfloat16
K, R, C = 12, 5, 7
layer = sgr.renderingLayer(imWidth=C, imHeight=R)
out = {}
names = ("albedo", "normal", "rough", "axis", "lamb", "weight", "im", "seg", "env_gt", "ind")

def inputs(ratio, heads):
    inp = O.synthetic_inputs(2, ratio * R, ratio * C, R, C, K, seed=900 + ratio)
    inp["seg"][0, :, :2] = 0.0
    inp["ind"] = torch.ones(2, 1, 1, 1); inp["ind"][-1] = 0.0
    if heads:
        g = torch.Generator().manual_seed(5)
        inp["axis"], inp["lamb"], inp["weight"] = (torch.randn(2, 3 * K, R, C, generator=g), torch.randn(2, K, R, C, generator=g), torch.randn(2, 3 * K, R, C, generator=g))
    return {k: inp[k].to(BF).to(dev) for k in names}

def objective(x, low, amp, flags, wrt):
    t = {k: (v if low else v.float()).detach().clone().requires_grad_(k in wrt) for k, v in x.items()}
    with torch.autocast("cuda", dtype=BF, enabled=amp):
        obj = sgr.light_objective(layer, *[t[k] for k in names], 1.0, 10.0, group=dist.group.WORLD, **flags)
    gs = torch.autograd.grad(obj[0], [t[k] for k in wrt])
    torch.cuda.synchronize()
    return [o.detach() for o in obj], gs

def same(got, want, low):
    (o, g), (o32, g32) = got, want
    ok = all(a.dtype == torch.float32 and torch.equal(a, c) for a, c in zip(o, o32))
    dt = BF if low else torch.float32
    return ok and all(a.dtype == dt and torch.equal(a.view(torch.int16) if low else a, c.to(dt).view(torch.int16) if low else c) for a, c in zip(g, g32))

sg, maps = ("axis", "lamb", "weight"), ("albedo", "normal", "rough")
for tag, ratio, flags, wrt in (("plain", 2, {}, sg), ("plain_3x", 3, {}, sg), ("decoder_outputs", 2, dict(decoder_outputs=True), sg), ("brdf_grads", 2, dict(brdf_grads=True), sg + maps),
                               ("brdf_grads_3x", 3, dict(brdf_grads=True), sg + maps), ("decoder_outputs_brdf_grads", 1, dict(decoder_outputs=True, brdf_grads=True), sg + maps)):
    x = inputs(ratio, bool(flags.get("decoder_outputs")))
    want = objective(x, False, False, flags, wrt)
    rec = dict(reproducible=same(objective(x, False, False, flags, wrt), want, False))
    rec["bf16_autocast"] = same(objective(x, True, True, flags, wrt), want, True)
    rec["fp32_autocast"] = same(objective(x, False, True, flags, wrt), want, False)
    unsharded = sgr.light_objective(layer, *[x[k].float() for k in names], 1.0, 10.0, **flags)
    rec["finite_nonzero"] = all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in want[1]) and bool(torch.equal(unsharded[1], want[0][1]))
    try:      # autocast off: bf16 is still refused
        objective(x, True, False, flags, wrt)
        rec["refused_without_autocast"] = "no error"
    except RuntimeError as e:
        rec["refused_without_autocast"] = "fp32 tensors required" in str(e) or str(e)
    out["light_objective/" + tag] = rec

for ratio in (1, 2, 3):
    x = inputs(ratio, False)
    g = torch.Generator().manual_seed(7)
    d, s = (torch.rand(2, 3, R, C, generator=g) * 0.8).to(BF).to(dev), (torch.rand(2, 3, R, C, generator=g) * 0.5).to(BF).to(dev)
    def loss(low, amp):
        c = lambda t: (t if low else t.float()).detach().clone()
        dd, ss = c(d).requires_grad_(True), c(s).requires_grad_(True)
        with torch.autocast("cuda", dtype=BF, enabled=amp):
            err, rendered = sgr.render_loss(dd, ss, c(x["im"]), c(x["seg"]), R, C, group=dist.group.WORLD)
        gs = torch.autograd.grad(err, [dd, ss])
        torch.cuda.synchronize()
        return [err.detach(), rendered.detach()], gs
    want = loss(False, False)
    out["render_loss/%dx" % ratio] = dict(reproducible=same(loss(False, False), want, False), bf16_autocast=same(loss(True, True), want, True), fp32_autocast=same(loss(False, True), want, False),
                                          finite_nonzero=all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in want[1]), refused_without_autocast=True)
dist.barrier()
dist.destroy_process_group()
print("RESULT " + json.dumps(out))
'''


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_the_sharded_route_under_autocast_through_rccl_world_of_one():
    """``light_objective(..., group=WORLD)`` and ``render_loss(..., group=WORLD)`` with bf16 maps and bf16 SG tensors inside the region against
    the same sharded call on the upcast inputs with autocast off; the stage-2 operators have no autocast rule (they write into ``ws``), the
    wrapper casts once for all three stages.  In a subprocess: a process group must not outlive the test; the limit is process-group start-up."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), SGR_ROOT=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-c", WORKER], env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:]
    out = json.loads(line[-1][7:])
    print(json.dumps(out))
    assert len(out) == 9
    for case, rec in out.items():
        for k in ("reproducible", "finite_nonzero", "bf16_autocast", "fp32_autocast", "refused_without_autocast"):
            assert rec[k] is True, (case, k, rec)


# ---- one light step end to end against fp64 ---------------------------------------------------------------------------------------------------
class LightNet(torch.nn.Module):
    """EncoderConv(11, 32) -> GroupNormReLU -> nn.Conv2d -> the upcat stage with a 16-channel skip -> three LightFinalConv -> the light
    objective from the decoders' outputs.  ``ours``: the package's operators; otherwise torch's own and oracle.sg_oracle for the same function.
    The parameter names are the same in both."""
    K, R, C = 12, 6, 8

    def __init__(self, sgr, ours):
        super().__init__()
        self.ours, self.sgr, K = ours, sgr, self.K
        self.conv2 = torch.nn.Conv2d(32, 48, 3, padding=1)
        if ours:
            self.enc, self.gn1, self.gn2 = sgr.EncoderConv(11, 32), sgr.GroupNormReLU(4, 32), sgr.GroupNormReLU(4, 48)
            self.fa, self.fl, self.fw = sgr.LightFinalConv(64, 3 * K), sgr.LightFinalConv(64, K), sgr.LightFinalConv(64, 3 * K)
            self.layer = sgr.renderingLayer(imWidth=self.C, imHeight=self.R)
        else:
            self.enc, self.gn1, self.gn2 = torch.nn.Conv2d(11, 32, 4, stride=2), torch.nn.GroupNorm(4, 32), torch.nn.GroupNorm(4, 48)
            self.fa, self.fl, self.fw = torch.nn.Conv2d(64, 3 * K, 3), torch.nn.Conv2d(64, K, 3), torch.nn.Conv2d(64, 3 * K, 3)

    def forward(self, x, skip, albedo, normal, rough, im, seg, env_gt, ind):
        R, C = self.R, self.C
        if self.ours:
            h = self.gn2(self.conv2(self.gn1(self.enc(x))), skip)
            return self.sgr.light_objective(self.layer, albedo, normal, rough, self.fa(h), self.fl(h), self.fw(h), im, seg, env_gt, ind, 1.0, 10.0, decoder_outputs=True)[0]
        pad = lambda t: F.pad(t, (1, 1, 1, 1), mode="replicate")
        h = F.relu(self.gn2(self.conv2(F.relu(self.gn1(self.enc(pad(x)))))))
        h = pad(F.interpolate(torch.cat([h, skip], 1), scale_factor=2, mode="bilinear"))
        axis, lamb, weight, _ = O.light_heads(self.fa(h), self.fl(h), self.fw(h))
        env, d, s = O.render_from_sg(albedo, normal, rough, axis, lamb, weight)
        return O.render_loss(d, s, im, seg, R, C)[0] + 10.0 * O.recon_loss(env, env_gt, seg, ind, R, C)[0]


def test_a_light_step_under_autocast_against_fp64(sgr):
    """the rule of test_gpu_gn_stage_bf16.py::test_autocast_end_to_end: loss and every parameter gradient at most twice as far from the fp64
    run as the same network from torch's own operators under the same autocast (``e_amp``, measured here from that network)"""
    torch.manual_seed(1960)
    ours, theirs = LightNet(sgr, True).cuda(), LightNet(sgr, False).cuda()
    with torch.no_grad():
        for m in (ours.gn1, ours.gn2):
            m.weight.normal_()
            m.bias.normal_(std=0.3)
    theirs.load_state_dict(ours.state_dict())
    names = [n for n, _ in ours.named_parameters()]
    assert names == [n for n, _ in theirs.named_parameters()]
    K, R, C = LightNet.K, LightNet.R, LightNet.C
    inp = O.synthetic_inputs(2, 2 * R, 2 * C, R, C, K, seed=1961)
    data = [rnd(2, 11, R, C, seed=1962), rnd(2, 16, R // 2, C // 2, seed=1963)] + [inp[k] for k in ("albedo", "normal", "rough", "im", "seg", "env_gt")] + [torch.ones(2, 1, 1, 1)]
    data = [t.cuda() for t in data]

    def step(net, amp, dtype=FP):
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF, enabled=amp):
            loss = net(*[t.to(dtype) for t in data])
        loss.backward()
        return loss.detach(), [p.grad.detach().clone() for p in net.parameters()]

    loss, grads = step(ours, True)
    assert loss.dtype == FP and all(g.dtype == FP and torch.isfinite(g).all() for g in grads)
    loss_t, grads_t = step(theirs, True)
    ref = LightNet(sgr, False).cuda().double()
    ref.load_state_dict({k: v.double() for k, v in ours.state_dict().items()})
    loss64, grads64 = step(ref, False, torch.float64)
    rel = lambda got, want: abs(float(got) - float(want)) / abs(float(want))
    err = lambda got, want: float((got.double() - want).norm() / want.norm())
    e_amp, e_ours = {"loss": rel(loss_t, loss64)}, {"loss": rel(loss, loss64)}
    for n, go, gt, gr in zip(names, grads, grads_t, grads64):
        e_amp[n], e_ours[n] = err(gt, gr), err(go, gr)
    for k in e_amp:
        print(f"light step under autocast, {k}: ours {e_ours[k]:.3e}, torch's own operators under the same autocast (e_amp) {e_amp[k]:.3e}")
    for k in e_amp:
        assert e_ours[k] <= 2.0 * e_amp[k], (k, e_ours[k], e_amp[k])
