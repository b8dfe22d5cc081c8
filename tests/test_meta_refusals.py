"""CPU: the Meta kernels of the render-path operators and of the bilateral solve operators make every refusal their device kernels make
(one check function per operator serves both: a traced graph cannot pass tracing and then fail on the device), and a valid call
returns the documented shapes and dtypes.  The cases are the table of tests/refusal_cases.py; tests/test_gpu_refusals.py holds the
device kernels to the same messages."""
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import inverserenderingofindoorscene_amd as sgr  # noqa: F401  (registers the operators)
import refusal_cases as RC


@pytest.mark.parametrize("name", [op.name for op in RC.OPS])
def test_operator_is_registered_by_the_cpp_extension(name):
    op = getattr(torch.ops.sgrender, name).default
    assert str(op._schema).startswith(f"sgrender::{name}("), name
    assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sgrender::{name}", "Meta"), name
    assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sgrender::{name}", "CUDA"), name


@pytest.mark.parametrize("name", [op.name for op in RC.OPS])
def test_valid_call_returns_the_documented_shapes(name):
    op = RC.BY_NAME[name]
    out = op.call(op.build("meta"))
    assert [(tuple(t.shape), t.dtype) for t in out] == op.outputs
    assert all(t.device.type == "meta" and t.is_contiguous() for t in out)


@pytest.mark.parametrize("name,label", RC.MUTATIONS, ids=[f"{n}-{l}" for n, l in RC.MUTATIONS])
def test_meta_kernel_refuses_what_the_device_kernel_refuses(name, label):
    op = RC.BY_NAME[name]
    args, message = RC.mutated(op, label, "meta")
    with pytest.raises(RuntimeError, match=re.escape(message)):
        op.call(args)


FAKE = [("sg_to_env_bwd", "cotangent-grid"), ("render_bwd_brdf", "no-light"), ("fused_render", "premap-2"), ("fused_render", "maps-batch"), ("render_loss", "seg-size"),
        ("light_heads_bwd", "cotangent-bf16"), ("bilateral_solve_bwd", "perm-length")]


@pytest.mark.parametrize("name,label", FAKE, ids=[f"{n}-{l}" for n, l in FAKE])
def test_fake_device_tensors_are_refused_alike(name, label):
    """what torch.compile traces with: fake tensors that report a cuda device and reach the Meta kernels"""
    op = RC.BY_NAME[name]
    valid, (args, message) = op.build("meta"), RC.mutated(op, label, "meta")
    with FakeTensorMode():
        fake = lambda a: [torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device="cuda") if isinstance(t, torch.Tensor) else t for t in a]
        out = op.call(fake(valid))
        assert [(tuple(t.shape), t.dtype) for t in out] == op.outputs and all(t.device.type == "cuda" for t in out)
        with pytest.raises(RuntimeError, match=re.escape(message)):
            op.call(fake(args))
