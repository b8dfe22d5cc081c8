"""GPU: the device kernels of the render-path operators and of the bilateral solve operators refuse what their Meta kernels refuse, with
the same message, before anything is copied or allocated; a valid call returns what the Meta kernel announces.  The cases are the table
of tests/refusal_cases.py (tests/test_meta_refusals.py holds the Meta kernels to it without a GPU).  A refusal is raised on the host, before
any launch: no kernel runs in a refused case."""
import pytest
import torch

import inverserenderingofindoorscene_amd as sgr  # noqa: F401  (registers the operators)
import refusal_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [f"{n}-{l}" for n, l in RC.MUTATIONS]


def refusal(op, args):
    with pytest.raises(RuntimeError) as e:
        op.call(args)
    return RC.message_of(e.value)


@pytest.mark.parametrize("name,label", RC.MUTATIONS, ids=IDS)
def test_device_kernel_refuses_with_the_meta_kernels_message(name, label):
    op = RC.BY_NAME[name]
    (on_meta, message), (on_device, _) = RC.mutated(op, label, "meta"), RC.mutated(op, label, DEV)
    expected = refusal(op, on_meta)
    assert message in expected
    assert refusal(op, on_device) == expected


@pytest.mark.parametrize("name,label", RC.MUTATIONS, ids=IDS)
def test_nothing_is_allocated_before_the_refusal(name, label):
    """non-contiguous inputs (channels-last maps, strided views): a kernel that made them contiguous before it checked would allocate"""
    op = RC.BY_NAME[name]
    args, message = RC.mutated(op, label, DEV, strided=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    assert message in refusal(op, args)
    assert torch.cuda.max_memory_allocated() == before


@pytest.mark.parametrize("name", [op.name for op in RC.OPS])
def test_valid_call_returns_what_the_meta_kernel_announces(name):
    op = RC.BY_NAME[name]
    announced, out = op.call(op.build("meta")), op.call(op.build(DEV))
    torch.cuda.synchronize()
    assert len(out) == len(announced) == len(op.outputs)
    for got, want, (shape, dtype) in zip(out, announced, op.outputs):
        assert (tuple(got.shape), got.stride(), got.dtype) == (tuple(want.shape), want.stride(), want.dtype) and (tuple(got.shape), got.dtype) == (shape, dtype)
        assert got.device == torch.device(DEV)
