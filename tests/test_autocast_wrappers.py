"""CPU: the public wrappers under a bf16 autocast on fake device tensors (the recipe of
tests/test_gn_stage_bf16.py::test_autocast_on_fake_device_tensors: FakeTensorMode, fake tensors that report a cuda device and so carry the
AutocastCUDA key), the cases of tests/autocast_cases.py -- the ones tests/test_gpu_autocast_ops.py runs for values on a GPU.

  * inside the region every wrapper takes bf16 inputs and returns fp32 (integer outputs aside); a bf16 leaf gets a bf16 gradient, an fp32
    parameter an fp32 one;
  * with autocast off the same bf16 call is refused by the Meta kernels as the device kernels refuse it: a fake-tensor run must not pass
    where the device raises;
  * the sharded light objective (``losses._allreduce_sum_`` replaced by a no-op) hands its stage operators, ``attach_grads`` and
    ``attach_grads6`` fp32 tensors only -- the stage-2 operators write into ``ws`` and have no autocast rule."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from autocast_cases import CASE_IDS, OBJ_ARGS, flatten, get_case, is_float, objective_case
from test_gn_stage_bf16 import autocast_cuda

import inverserenderingofindoorscene_amd as sgr
from inverserenderingofindoorscene_amd import losses

BF, HF, FP = torch.bfloat16, torch.float16, torch.float32


def fake_run(case, low, amp):
    """the case on fake cuda tensors, floating arguments in ``low`` (parameters fp32); call inside FakeTensorMode.
    -> the outputs (no backward: the autograd engine needs the device itself; tests/test_gpu_autocast_ops.py has the gradients)"""
    def place(make):
        with torch.device("cuda"):
            return make()
    case.bind(place)
    kw = {}
    for name, t in case.args.items():
        if isinstance(t, torch.Tensor):
            dtype = (low if name not in case.params else FP) if is_float(t) else t.dtype
            t = torch.empty(t.shape, device="cuda", dtype=dtype, requires_grad=name in case.grads)
        kw[name] = t
    with autocast_cuda(low) if amp else torch.enable_grad():
        return flatten(case.fn(**kw))


@pytest.mark.parametrize("family,name", [(f, n) for f, ns in CASE_IDS.items() for n in ns], ids=[n for ns in CASE_IDS.values() for n in ns])
def test_wrapper_dtypes_under_autocast_and_the_refusal_without_it(family, name):
    case = get_case(sgr, family, name)
    low = HF if name.endswith("-fp16") else BF      # the same-size GroupNorm stage keeps bf16; fp16 takes its fp32 rule
    with FakeTensorMode():
        outs = fake_run(case, low, True)
        assert any(o is not None for o in outs)
        for i, o in enumerate(outs):
            assert o is None or o.device.type == "cuda", (name, i)
            assert o is None or not is_float(o) or o.dtype == FP, (name, i, o.dtype)
        assert not case.grads or any(o is not None and o.requires_grad for o in outs), name      # the casts are differentiable
        assert not torch.is_autocast_enabled("cuda")
        with pytest.raises(RuntimeError, match="fp32|Float|one dtype|same dtype|should be the same"):
            fake_run(case, low, False)


class Recorder:
    """torch.ops.sgrender with the floating dtypes that reach chosen operators written down"""

    def __init__(self, watch):
        self.watch, self.seen = watch, {}

    def __getattr__(self, name):
        op = getattr(torch.ops.sgrender, name)
        if name not in self.watch:
            return op

        def call(*args):
            self.seen.setdefault(name, []).append([a.dtype for a in args if is_float(a)])
            return op(*args)
        return call


STAGES = ("light_objective_stage1", "light_objective_stage2", "light_objective_stage2_brdf", "light_objective_stage3", "attach_grads", "attach_grads6")


@pytest.mark.parametrize("ratio", [1, 2, 3])
@pytest.mark.parametrize("flags", [{}, dict(decoder_outputs=True), dict(brdf_grads=True), dict(decoder_outputs=True, brdf_grads=True)], ids=lambda f: "+".join(f) or "plain")
def test_the_sharded_objective_hands_its_stage_operators_fp32_only(monkeypatch, flags, ratio):
    case = objective_case(sgr, 12, 8, 16, ratio, **flags)
    layer = sgr.renderingLayer(imWidth=7, imHeight=5)
    group = object()      # any explicit group takes the sharded route; the collective is replaced
    reduced = []
    monkeypatch.setattr(losses, "_allreduce_sum_", lambda t, g: reduced.append((t.dtype, g is group)))
    rec = Recorder(STAGES)
    monkeypatch.setattr(losses, "_sg", rec)
    case.fn = lambda **kw: sgr.light_objective(layer, *[kw[k] for k in OBJ_ARGS], 1.0, 10.0, group=group, **flags)
    with FakeTensorMode():
        outs = fake_run(case, BF, True)
        assert all(o.dtype == FP for o in outs) and outs[0].requires_grad
        stage2 = "light_objective_stage2_brdf" if flags.get("brdf_grads") else "light_objective_stage2"
        attach = "attach_grads6" if flags.get("brdf_grads") else "attach_grads"
        assert set(rec.seen) == {"light_objective_stage1", stage2, "light_objective_stage3", attach}, sorted(rec.seen)
        for name, calls in rec.seen.items():
            assert len(calls) == 1 and calls[0] and all(d == FP for d in calls[0]), (name, calls)
        assert reduced == [(FP, True), (FP, True)]
        # fp32 inputs inside the region, and autocast off: as before
        rec.seen.clear()
        assert all(o.dtype == FP for o in fake_run(case, FP, True)) and all(o.dtype == FP for o in fake_run(case, FP, False))
        with pytest.raises(RuntimeError, match="fp32 tensors required, got BFloat16"):      # autocast off: bf16 is still refused, on fake tensors too
            fake_run(case, BF, False)


def test_the_stage2_meta_kernels_refuse_what_the_device_kernels_refuse():
    """a bf16 tensor straight into ``light_objective_stage2`` / ``_brdf`` (no autocast rule: they write into ``ws``), inside the region or not"""
    ops = torch.ops.sgrender
    bn, K, R, C, eh, ew = 2, 12, 5, 7, 8, 16
    with FakeTensorMode():
        d = lambda *s, dtype=FP: torch.empty(*s, device="cuda", dtype=dtype)
        maps = [d(bn, 3, R, C), d(bn, 3, R, C), d(bn, 1, R, C)]
        sg = [d(bn, K, 3, R, C), d(bn, K, R, C), d(bn, 3 * K, R, C)]
        im, seg, env_gt, ind = d(bn, 3, R, C), d(bn, 1, R, C), d(bn, 3, R, C, eh, ew), d(bn, 1, 1, 1)
        s1 = ops.light_objective_stage1(*maps, *sg, im, seg, env_gt, ind, eh, ew, 57.0, 0.05, [0.0, 0.0, 0.0], False, False)
        diffuse, spec, mask, coef, im_s, seg_s, rendered, coef_ds, sums, ws, lam_t, w_t = s1
        tail = (eh, ew, 57.0, 0.05, [0.0, 0.0, 0.0], 1.0, 10.0, 1.0, False)

        def stage2(maps, sg, brdf):
            args = (*maps, *sg, env_gt, mask, coef, diffuse, spec, im_s, seg_s, coef_ds, sums, ws, lam_t, w_t, *tail)
            return ops.light_objective_stage2_brdf(*args, True, True, True) if brdf else ops.light_objective_stage2(*args, True)
        assert all(t.dtype == FP for t in stage2(maps, sg, False)) and all(t.dtype == FP for t in stage2(maps, sg, True))
        low = lambda ts, i: [t.to(BF) if j == i else t for j, t in enumerate(ts)]
        for brdf in (False, True):
            for i in range(3):
                for amp in (False, True):
                    with autocast_cuda(BF) if amp else torch.no_grad():
                        with pytest.raises(RuntimeError, match="fp32 tensors required, got BFloat16"):
                            stage2(low(maps, i), sg, brdf)
                        with pytest.raises(RuntimeError, match="fp32 tensors required, got BFloat16"):
                            stage2(maps, low(sg, i), brdf)
