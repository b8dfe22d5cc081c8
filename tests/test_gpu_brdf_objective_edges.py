"""GPU: sgr.brdf_objective (csrc/sgr_brdf_loss.hip) where tests/test_gpu_brdf_objective.py never goes: the element-wise (V = 1) loops of
brdf_pass_a, brdf_pass_b and brdf_bwd taking a second and a third round, the alignment half of ``brdf_vec4``, and reads at the edges of
the planes.

Inputs and bounds are those of ``test_full_size_against_the_checker`` there, imported: ``full_size_inputs`` at smaller sizes, the six
values by ``conftest.scalar_close(got, ref64, e_ref)``, the gradients in rel-L2 by ``grad_bound(e_ref)``, ``e_ref`` the checker in fp32 on
the same inputs."""
import pytest
import torch

from conftest import scalar_close
from test_gpu_brdf_objective import GRADS, VALUES, checker, err, full_size_inputs, grad_bound

pytestmark = pytest.mark.gpu

SPLIT_THREADS = 64 * 256      # kBSplit * kBThreads: pixels per round of the element-wise loops


@pytest.fixture(scope="module")
def sgr():
    import inverserenderingofindoorscene_amd as pkg
    from inverserenderingofindoorscene_amd import _lib
    _lib.load()
    return pkg


def inputs(B, H, W, seed, nyu):
    args, seg_depth = full_size_inputs(B=B, H=H, W=W, seed=seed, nyu=nyu)
    args = [a.cuda() if a is not None else None for a in args]
    kw = dict(weights=(6.0, 1.0, 0.5, 0.5), depth_offset=0.1 if nyu else 1.0)
    return args, (seg_depth.cuda() if seg_depth is not None else None), kw


def run_in_place(sgr, args, kw, seg_depth):
    """as test_gpu_brdf_objective.run, but on the tensors where they lie (no clone: a clone would come back from the allocator aligned)"""
    live = [a.detach().requires_grad_(True) if a is not None else None for a in args[:4]]
    for a, t in zip(args[:4], live):
        assert t is None or t.data_ptr() == a.data_ptr()
    out = sgr.brdf_objective(*live, *args[4:], segDepthBatch=seg_depth, **kw)
    present = [t for t in live if t is not None]
    g = list(torch.autograd.grad(out.total, present))
    return out, [g.pop(0) if t is not None else None for t in live]


def against_the_checker(tag, out, grads, args, kw, seg_depth):
    r64, r32 = checker(args, kw, seg_depth, torch.float64), checker(args, kw, seg_depth, torch.float32)
    if args[0] is not None:      # the condition on the inputs of the full-size test: the clamp is live and nothing sits on its kink
        prod = (args[0].double() * r64["coef"][:, 0].reshape(-1, 1, 1, 1))[(args[8] > 0).expand_as(args[0])]
        share, kink = float((prod > 1).double().mean()), float(torch.minimum(prod.abs(), (prod - 1).abs()).min())
        print(f"{tag}: clipped share {share:.3f}, distance to the kink {kink:.2e}")
        assert 0.05 <= share <= 0.5 and kink > 1e-4
    missed = []      # every figure is printed before the first assertion, so that a failure names all the values that missed
    for k in VALUES + ("angleMean",):
        got, ref, e = float(getattr(out, k).detach()), float(r64[k]), abs(float(r32[k]) - float(r64[k]))
        print(f"{tag} {k}: got {got:.9g} ref {ref:.9g} |diff| {abs(got - ref):.2e} (e_ref {e:.1e})")
        if not scalar_close(got, ref, e):
            missed.append((k, got, ref, e))
    for k, g in zip(GRADS, grads):
        if g is None:
            assert r64[k] is None
            continue
        e_ref = err(r32[k], r64[k])
        e, lim = err(g, r64[k]), grad_bound(e_ref)
        print(f"{tag} {k}: {e:.2e} (bound {lim:.1e}, e_ref {e_ref:.2e})")
        if not (bool(torch.isfinite(g).all()) and e <= lim):
            missed.append((k, e, lim))
    assert not missed, (tag, missed)


def shifted(t):
    buf = torch.empty(t.numel() + 1, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# brdf_vec4 asks for H W % 4 == 0 (not W % 4 == 0): 200 x 201 = 40200 pixels would go in 128-bit vectors, in ONE round (10050 vectors), so
# that shape reaches the element-wise kernels through the other half of the rule, with every tensor one float off its boundary;
# 201 x 201 reaches them by its size
@pytest.mark.parametrize("nyu", [False, True], ids=["synthetic_offset_1", "nyu_offset_0.1"])
@pytest.mark.parametrize("shape,rounds,shift", [((2, 129, 131), 2, False), ((1, 200, 201), 3, True), ((1, 201, 201), 3, False)],
                         ids=["2x129x131", "1x200x201_shifted", "1x201x201"])
def test_element_wise_loops_stride_against_the_checker(sgr, shape, rounds, shift, nyu):
    """all three kernels go element by element, and above 16384 pixels, so their threads take a second (third) round -- the second of
    129 x 131 with 515 pixels, the third ragged too.  The NYU mode has its own depth mask"""
    B, H, W = shape
    args, seg_depth, kw = inputs(B, H, W, 4100 + H + W, nyu)
    assert (seg_depth is not None) == nyu
    placed, placed_depth = args, seg_depth
    if shift:
        placed, placed_depth = [shifted(a) if a is not None else None for a in args], shifted(seg_depth) if nyu else None
    every = [a for a in placed + [placed_depth] if a is not None]
    assert (H * W % 4 != 0 or any(a.data_ptr() % 16 for a in every)) and shift == (H * W % 4 == 0)      # brdf_vec4 says no
    assert -(-H * W // SPLIT_THREADS) == rounds
    out, grads = run_in_place(sgr, placed, kw, placed_depth)
    against_the_checker(f"{B}x{H}x{W} {'nyu' if nyu else 'synthetic'}", out, grads, args, kw, seg_depth)


# index into the ten arguments: one prediction, one ground truth, one mask
@pytest.mark.parametrize("which", [1, 7, 8], ids=["normalPred", "depth", "segBRDF"])
def test_one_tensor_off_its_boundary_takes_the_element_wise_kernels(sgr, which):
    """2 x 24 x 32: H W % 4 == 0, so only the address of one tensor sends brdf_vec4 to the element-wise kernels, in forward and backward
    (the backward checks the input planes too; the gradients it allocates are aligned).  The element-wise path differs from the 128-bit
    one in which thread adds which pixel, so the values are held to the checker, not to the aligned run; the backward has no reduction:
    with the same coefficients and totals its two instantiations would agree, and two element-wise runs on the same values must"""
    args, _, kw = inputs(2, 24, 32, 4200, False)
    assert all(a.data_ptr() % 16 == 0 for a in args)
    one = list(args)
    one[which] = shifted(args[which])
    every = [shifted(a) for a in args]
    out1, g1 = run_in_place(sgr, one, kw, None)
    out7, g7 = run_in_place(sgr, every, kw, None)
    against_the_checker(f"2x24x32 argument {which} shifted", out1, g1, args, kw, None)
    against_the_checker("2x24x32 all shifted", out7, g7, args, kw, None)
    for k in VALUES + ("angleMean", "coef"):      # both ran brdf_pass_a<1> / brdf_pass_b<1> on the same values
        assert torch.equal(getattr(out1, k), getattr(out7, k)), k
    for k, a, b in zip(GRADS, g1, g7):            # and brdf_bwd<1>
        assert torch.equal(a, b), k


def banded(t, fill):
    """-> (buffer, the view of `t`'s shape in its middle) with one plane of `fill` on either side"""
    band, n = t.shape[2] * t.shape[3], t.numel()
    buf = torch.full((n + 2 * band,), fill, device=t.device)
    v = buf[band:band + n].view(t.shape)
    v.copy_(t)
    return buf, v


@pytest.mark.parametrize("nyu", [False, True], ids=["synthetic", "nyu"])
@pytest.mark.parametrize("shape", [(2, 30, 41), (2, 24, 32)], ids=["2x30x41", "2x24x32"])
def test_reads_stay_inside_the_planes(sgr, shape, nyu):
    """every input in the middle of a larger buffer, a plane of guard band on either side; the bands zero, then NaN, at the same addresses:
    the same bits, all finite.  30 x 41 goes element by element, 24 x 32 in 128-bit vectors (a band of 768 floats keeps the alignment)"""
    B, H, W = shape
    args, seg_depth, kw = inputs(B, H, W, 4300 + W, nyu)
    everything = args + [seg_depth]
    held = [banded(a, 0.0) if a is not None else None for a in everything]
    views = [h[1] if h is not None else None for h in held]
    if H * W % 4 == 0:
        assert all(v is None or v.data_ptr() % 16 == 0 for v in views)
    clean, gc = run_in_place(sgr, views[:10], kw, views[10])
    for h, a in zip(held, everything):
        if h is not None:
            h[0].fill_(float("nan"))
            h[1].copy_(a)
    dirty, gd = run_in_place(sgr, views[:10], kw, views[10])
    for k in VALUES + ("angleMean", "coef"):
        a, b = getattr(clean, k).detach(), getattr(dirty, k).detach()
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b), k
    for k, a, b in zip(GRADS, gc, gd):
        assert (a is None and b is None) or (bool(torch.isfinite(b).all()) and torch.equal(a, b)), k
    plain, gp = run_in_place(sgr, args, kw, seg_depth)      # and the placement changes nothing
    for k in VALUES + ("angleMean", "coef"):
        assert torch.equal(getattr(plain, k).detach(), getattr(clean, k).detach()), k
    for a, b in zip(gp, gc):
        assert (a is None and b is None) or torch.equal(a, b)
