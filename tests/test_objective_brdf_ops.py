"""CPU (no GPU needed): the operators and C entry points of ``light_objective(..., brdf_grads=True)`` -- schemas, Meta shapes through
autograd, the refusal of CPU tensors, the C ABI's argument checks, and the refusal of image gradients before any collective."""
import ctypes

import pytest
import torch

import inverserenderingofindoorscene_amd as sgr
from inverserenderingofindoorscene_amd import _lib

bn, R, C, K, eh, ew = 2, 6, 8, 12, 8, 16
NEW_OPS = ("rescale_grads6_", "attach_grads6", "light_objective_brdf_fwdbwd", "light_objective_brdf", "light_objective_stage2_brdf")
CFG = (eh, ew, 57.0, 0.05, [0.0, 0.0, 0.0], 1.0, 10.0, 1.0, False, False)


def m(*s):
    return torch.empty(*s, device="meta")


def _args(h, w, live=("albedo", "normal", "rough", "axis", "lamb", "weight")):
    t = dict(albedo=m(bn, 3, h, w), normal=m(bn, 3, h, w), rough=m(bn, 1, h, w), axis=m(bn, K, 3, R, C), lamb=m(bn, K, R, C), weight=m(bn, 3 * K, R, C))
    for k in live:
        t[k].requires_grad_(True)
    return t, (m(bn, 3, h, w), m(bn, 1, h, w), m(bn, 3, R, C, eh, ew), m(bn, 1, 1, 1))


def test_new_operators_have_schemas():
    for name in NEW_OPS:
        op = getattr(torch.ops.sgrender, name)
        assert str(op.default._schema).startswith(f"sgrender::{name}("), name
    assert "bool want_rough" in str(torch.ops.sgrender.light_objective_brdf_fwdbwd.default._schema)
    assert "Tensor(a!) ws" in str(torch.ops.sgrender.light_objective_stage2_brdf.default._schema)


@pytest.mark.parametrize("h,w", [(R, C), (2 * R, 2 * C)])
def test_meta_shapes_through_autograd(h, w):
    ops = torch.ops.sgrender
    t, (im, seg, gt, ind) = _args(h, w)
    out = ops.light_objective_brdf(t["albedo"], t["normal"], t["rough"], t["axis"], t["lamb"], t["weight"], im, seg, gt, ind, *CFG)
    assert out[0].dim() == 0 and out[0].requires_grad and tuple(out[3].shape) == (bn, 3, R, C)
    g = torch.autograd.grad(out[0], [t[k] for k in ("albedo", "normal", "rough", "axis", "lamb", "weight")])
    assert [tuple(x.shape) for x in g] == [(bn, 3, h, w), (bn, 3, h, w), (bn, 1, h, w), (bn, K, 3, R, C), (bn, K, R, C), (bn, 3 * K, R, C)]
    # a subset: only the roughness map
    t, _ = _args(h, w, live=("rough",))
    out = ops.light_objective_brdf(t["albedo"], t["normal"], t["rough"], t["axis"], t["lamb"], t["weight"], im, seg, gt, ind, *CFG)
    assert tuple(torch.autograd.grad(out[0], [t["rough"]])[0].shape) == (bn, 1, h, w)
    # no map live: the plain operator's node, SG gradients only
    t, _ = _args(h, w, live=("axis", "lamb", "weight"))
    out = ops.light_objective_brdf(t["albedo"], t["normal"], t["rough"], t["axis"], t["lamb"], t["weight"], im, seg, gt, ind, *CFG)
    assert out[0].requires_grad
    # the one-rank backend: empty outputs for maps not asked for
    full = ops.light_objective_brdf_fwdbwd(t["albedo"], t["normal"], t["rough"], t["axis"].detach(), t["lamb"].detach(), t["weight"].detach(), im, seg, gt, ind,
                                           *CFG, False, True, False)
    assert len(full) == 12 and full[8].numel() == 0 and tuple(full[9].shape) == (bn, 3, h, w) and full[10].numel() == 0 and tuple(full[11].shape) == (2,)


def test_stage2_brdf_meta_and_attach6():
    ops = torch.ops.sgrender
    t, (im, seg, gt, ind) = _args(2 * R, 2 * C)
    d = {k: v.detach() for k, v in t.items()}
    st1 = ops.light_objective_stage1(d["albedo"], d["normal"], d["rough"], d["axis"], d["lamb"], d["weight"], im, seg, gt, ind, eh, ew, 57.0, 0.05,
                                     [0.0, 0.0, 0.0], False, False)
    diffuse, spec, mask, coef, im_s, seg_s, rendered, coef_ds, sums, ws, lam_t, w_t = st1
    st2 = ops.light_objective_stage2_brdf(d["albedo"], d["normal"], d["rough"], d["axis"], d["lamb"], d["weight"], gt, mask, coef, diffuse, spec, im_s, seg_s,
                                          coef_ds, sums, ws, lam_t, w_t, eh, ew, 57.0, 0.05, [0.0, 0.0, 0.0], 1.0, 10.0, 1.0, False, True, True, False)
    assert len(st2) == 8 and tuple(st2[4].shape) == (bn, 3, 2 * R, 2 * C) and tuple(st2[5].shape) == (bn, 3, 2 * R, 2 * C) and st2[6].numel() == 0
    with pytest.raises(RuntimeError, match="light_objective_stage2"):
        ops.light_objective_stage2_brdf(d["albedo"], d["normal"], d["rough"], d["axis"], d["lamb"], d["weight"], gt, mask, coef[:1], diffuse, spec, im_s,
                                        seg_s, coef_ds, sums, ws, lam_t, w_t, eh, ew, 57.0, 0.05, [0.0, 0.0, 0.0], 1.0, 10.0, 1.0, False, True, True, True)
    obj, _ = ops.light_objective_stage3(st2[0], st2[7][0:1], sums, 1.0, 10.0, eh, ew)
    out = ops.attach_grads6(obj, t["axis"], t["lamb"], t["weight"], t["albedo"], t["normal"], t["rough"], *st2[1:7], m(2))
    g = torch.autograd.grad(out, [t["albedo"], t["normal"], t["axis"]])
    assert [tuple(x.shape) for x in g] == [(bn, 3, 2 * R, 2 * C), (bn, 3, 2 * R, 2 * C), (bn, K, 3, R, C)]


def test_new_operators_reject_cpu_tensors():
    z = torch.zeros
    ops = torch.ops.sgrender
    args = (z(1, 3, 2, 2), z(1, 3, 2, 2), z(1, 1, 2, 2), z(1, 2, 3, 2, 2), z(1, 2, 2, 2), z(1, 6, 2, 2), z(1, 3, 2, 2), z(1, 1, 2, 2), z(1, 3, 2, 2, 8, 16),
            z(1, 1, 1, 1), 8, 16, 57.0, 0.05, [0.0, 0.0, 0.0], 1.0, 10.0, 1.0, False, False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.light_objective_brdf(*args)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.light_objective_brdf_fwdbwd(*args, True, True, True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rescale_grads6_(z(4), z(4), z(4), z(4), z(4), z(4), z(1), z(2), 0)


def _call(fn, ptrs, dims, imHW=(2 * R, 2 * C), tail=()):
    return fn(*ptrs, bn, K, R, C, eh, ew, imHW[0], imHW[1], ctypes.c_float(0.05), 1, ctypes.c_float(1.0), ctypes.c_float(10.0), *tail)


def test_c_abi_argument_checks_without_a_gpu():
    L = _lib.load()
    assert L.sgr_abi_version() == _lib.ABI_VERSION == 6
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # sgr_fused_bwd_recon_brdf: 22 pointers, then sizes; NULL inputs -> SGR_ERR_BAD_ARG
    assert _call(L.sgr_fused_bwd_recon_brdf, [None] * 22, None, tail=(None,)) == -1
    # the BRDF outputs without the SG gradient trio -> SGR_ERR_BAD_ARG
    ptrs = [p] * 14 + [None, None, None] + [p, p, p] + [p, p]
    assert _call(L.sgr_fused_bwd_recon_brdf, ptrs, None, tail=(None,)) == -1
    # the three BRDF outputs come together: one of them alone -> SGR_ERR_BAD_ARG
    ptrs = [p] * 17 + [p, None, None] + [p, p]
    assert _call(L.sgr_fused_bwd_recon_brdf, ptrs, None, tail=(None,)) == -1
    # decoder outputs (premap 3) with the BRDF outputs -> SGR_ERR_UNSUPPORTED (no launch)
    assert L.sgr_fused_bwd_recon_brdf(*([p] * 22), bn, K, R, C, eh, ew, 2 * R, 2 * C, ctypes.c_float(0.05), 3, ctypes.c_float(1.0),
                                      ctypes.c_float(10.0), None) == -2
    # an unsupported configuration: BRDF maps at 3x the env grid -> SGR_ERR_UNSUPPORTED (no launch)
    ptrs = [p] * 22
    assert _call(L.sgr_fused_bwd_recon_brdf, ptrs, None, imHW=(3 * R, 3 * C), tail=(None,)) == -2
    # the one-rank entry point: NULL scalars -> SGR_ERR_BAD_ARG; unsupported grid -> SGR_ERR_UNSUPPORTED
    ptrs = [p] * 21
    total_tail = (p, ctypes.c_float(1.0), p, p, p, None)
    assert _call(L.sgr_fused_bwd_recon_total_brdf, ptrs, None, tail=(None, ctypes.c_float(1.0), None, None, None, None)) == -1
    assert _call(L.sgr_fused_bwd_recon_total_brdf, ptrs, None, imHW=(3 * R, 3 * C), tail=total_tail) == -2
    assert L.sgr_last_error() and b"sgr_fused_bwd_recon" in L.sgr_last_error()


def test_image_gradient_refusal_comes_before_any_collective():
    import torch.distributed as dist
    from inverserenderingofindoorscene_amd import losses
    t, (im, seg, gt, ind) = _args(R, C)
    layer = sgr.renderingLayer(imWidth=C, imHeight=R, isCuda=False)

    class _Group:      # any explicit group selects the sharded route (losses._sharded)
        pass
    for group in (None, _Group()):
        for k, bad in (("im", im), ("seg", seg), ("gt", gt), ("ind", ind)):
            args = dict(im=im, seg=seg, gt=gt, ind=ind)
            args[k] = bad.clone().requires_grad_(True)
            with pytest.raises(RuntimeError, match="BRDF maps only"):
                losses.light_objective(layer, t["albedo"], t["normal"], t["rough"], t["axis"], t["lamb"], t["weight"], args["im"], args["seg"], args["gt"],
                                       args["ind"], group=group, brdf_grads=True)
    # the default still refuses a grad-requiring map
    with pytest.raises(RuntimeError, match="SG parameters only"):
        losses.light_objective(layer, t["albedo"], t["normal"], t["rough"], t["axis"], t["lamb"], t["weight"], im, seg, gt, ind)
    assert not dist.is_initialized()
