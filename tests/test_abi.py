"""CPU: the C-ABI library loads and exports every symbol include/sgrender.h declares; argument
validation works without a GPU (no kernel is launched)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from inverserenderingofindoorscene_amd import _lib


def _declared():
    src = open(os.path.join(ROOT, "include", "sgrender.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sgr_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported_and_bound():
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/sgrender.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in _lib.SIGNATURES"
    assert sorted(_lib.SIGNATURES) == names
    assert lib.sgr_abi_version() == _lib.ABI_VERSION


def test_argument_validation_without_gpu():
    lib = _lib.load()
    # NULL tensors -> SGR_ERR_BAD_ARG, with a message
    rc = lib.sgr_sg_to_env_fwd(None, None, None, None, None, None, None, 1, 12, 4, 4, 8, 16, 1, None)
    assert rc == -1 and b"NULL" in lib.sgr_last_error()
    # unsupported pooling ratio / lobe count -> SGR_ERR_UNSUPPORTED (pointer values are never dereferenced)
    fake = ctypes.c_void_p(4096)
    rc = lib.sgr_fused_fwd(fake, fake, fake, fake, fake, fake, fake, fake, None, fake, fake,
                           1, 12, 4, 4, 8, 16, 12, 12, ctypes.c_float(0.05), 1, None)
    assert rc == -2 and b"ratio" in lib.sgr_last_error()
    rc = lib.sgr_fused_fwd(fake, fake, fake, fake, fake, fake, fake, fake, None, fake, fake,
                           1, 33, 4, 4, 8, 16, 4, 4, ctypes.c_float(0.05), 1, None)
    assert rc == -2
    assert lib.sgr_dirs_padded(128) == 128 and lib.sgr_dirs_padded(15) == 32


def test_cpu_tensors_are_rejected_not_emulated():
    import torch
    import inverserenderingofindoorscene_amd as pkg
    o2e = pkg.output2env(SGNum=2, envWidth=4, envHeight=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        o2e.output2env(torch.zeros(1, 2, 3, 2, 2), torch.zeros(1, 2, 2, 2), torch.zeros(1, 6, 2, 2))
    rl = pkg.renderingLayer(imWidth=2, imHeight=2, envWidth=4, envHeight=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rl.forwardEnv(torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 2, 2), torch.zeros(1, 1, 2, 2), torch.zeros(1, 3, 2, 2, 2, 4))


def test_layer_attributes_mirror_reference():
    import numpy as np
    import inverserenderingofindoorscene_amd as pkg
    rl = pkg.renderingLayer()
    assert tuple(rl.v.shape) == (1, 3, 120, 160) and tuple(rl.ls.shape) == (128, 3)
    assert tuple(rl.envWeight.shape) == (1, 128, 1, 1, 1) and abs(rl.fov - 57 / 180 * np.pi) < 1e-12
    o2e = pkg.output2env(12)
    assert tuple(o2e.ls.shape) == (1, 1, 3, 1, 1, 8, 16) and o2e.SGNum == 12


def test_premap_modes_and_configuration_queries_without_gpu():
    """premap = 3 (decoder heads as the kernels' prologue) is offered where a packed kernel implements it and refused -- before
    any launch -- elsewhere; the workspace / support queries are pure host functions."""
    lib = _lib.load()
    assert lib.sgr_heads_prologue_supported(12, 120, 160, 8, 16) == 1 and lib.sgr_heads_prologue_supported(24, 240, 320, 16, 32) == 1
    assert lib.sgr_heads_prologue_supported(6, 120, 160, 8, 16) == 0        # SGNum <= 6: no prologue (standalone heads pass)
    assert lib.sgr_heads_prologue_supported(25, 120, 160, 8, 16) == 0
    assert lib.sgr_heads_prologue_supported(12, 120, 160, 4, 8) == 0        # a direction grid without packed kernels
    assert lib.sgr_fused_recon_supported(24, 240, 320, 16, 32) == 1 and lib.sgr_fused_recon_supported(12, 120, 160, 4, 8) == 0
    assert lib.sgr_loss_workspace_floats(16) > 16 * 16 * 9 and lib.sgr_fused_recon_workspace_floats(16, 120, 160) > 0
    fake = ctypes.c_void_p(4096)
    f0 = ctypes.c_float(0.05)
    # out of range, and in range but not implemented for this shape: both rejected with a message, nothing launched
    rc = lib.sgr_fused_fwd(fake, fake, fake, fake, fake, fake, fake, fake, None, fake, fake, 1, 12, 4, 4, 8, 16, 4, 4, f0, 4, None)
    assert rc == -1 and b"premap" in lib.sgr_last_error()
    rc = lib.sgr_fused_fwd(fake, fake, fake, fake, fake, fake, fake, fake, None, fake, fake, 1, 5, 4, 4, 8, 16, 4, 4, f0, 3, None)
    assert rc == -2 and b"premap 3" in lib.sgr_last_error()
    rc = lib.sgr_fused_bwd_sg(None, fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, fake, 1, 5, 4, 4, 8, 16, 4, 4,
                              f0, 3, None)
    assert rc == -2 and b"premap 3" in lib.sgr_last_error()
    rc = lib.sgr_sg_to_env_fwd(fake, fake, fake, fake, fake, None, None, 1, 12, 4, 4, 8, 16, 3, None)
    assert rc == -1 and b"premap" in lib.sgr_last_error()


# ---- the render layer's refusals, entry point by entry point --------------------------------------------------------------------
# Every call below is refused before anything is launched (the pointers are fake).  The expected texts were recorded before the
# layer's launch code was gathered into csrc/sgr_layer_launch.h and pin, per entry point, each class of refusal and -- through
# the calls that break two rules at once -- the order of the checks: the first failing check decides code and message.
_INTS = {     # the integer arguments of each entry point, in order
    "sgr_sg_to_env_fwd": "bn K R C eh ew premap",
    "sgr_sg_shading": "bn K R C eh ew premap",
    "sgr_render_env_fwd": "bn R C eh ew imH imW",
    "sgr_fused_fwd": "bn K R C eh ew imH imW premap",
    "sgr_fused_fwd_tan": "bn K R C eh ew imH imW premap",
    "sgr_sg_to_env_bwd": "bn K R C eh ew premap",
    "sgr_fused_bwd_sg": "bn K R C eh ew imH imW premap",
    "sgr_render_env_bwd_env": "bn R C eh ew imH imW",
    "sgr_render_bwd_brdf": "bn K R C eh ew imH imW premap",
    "sgr_fused_fwd_recon": "bn K R C eh ew imH imW premap",
    "sgr_fused_fwd_recon_seg": "segH segW bn K R C eh ew imH imW premap",
    "sgr_light_objective_fwd": "bn K R C eh ew imH imW brdfH brdfW premap",
    "sgr_fused_bwd_recon": "bn K R C eh ew imH imW premap",
    "sgr_fused_bwd_recon_total_brdf": "bn K R C eh ew imH imW premap",
    "sgr_render_loss_fwd_total": "bn R C imH imW",
}
_VALID = dict(bn=2, K=12, R=4, C=6, eh=8, ew=16, imH=8, imW=12, brdfH=8, brdfW=12, segH=8, segW=12, premap=1)
_RATIO = "BRDF-map / env-grid ratio must be 1 or 2 (pool first)"
_HEADS = "premap 3 (decoder heads as a prologue) needs envWidth 16 or 32 and 6 < SGNum <= 24 (sgr_heads_prologue_supported)"
_RECON = "needs envWidth 16 or 32 and SGNum <= 24 (use the unfused calls)"
_BAD, _UNS = -1, -2

# (entry point, changed integers, indices of pointer arguments passed as NULL, return code, message)
_REFUSALS = [
    ("sgr_sg_to_env_fwd", {}, [0], _BAD, "sgr_sg_to_env_fwd: NULL tensor"),
    ("sgr_sg_to_env_fwd", dict(R=0), [], _BAD, "sgr_sg_to_env_fwd: non-positive size"),
    ("sgr_sg_to_env_fwd", dict(K=33), [], _UNS, "sgr_sg_to_env_fwd: SGNum > 32 is not supported"),
    ("sgr_sg_to_env_fwd", dict(premap=3), [], _BAD, "sgr_sg_to_env_fwd: premap must be 0, 1 or 2"),
    ("sgr_sg_to_env_fwd", dict(K=33, premap=3), [], _UNS, "sgr_sg_to_env_fwd: SGNum > 32 is not supported"),
    ("sgr_sg_shading", {}, [4], _BAD, "sgr_sg_shading: NULL tensor"),
    ("sgr_sg_shading", dict(ew=0), [], _BAD, "sgr_sg_shading: non-positive size"),
    ("sgr_sg_shading", dict(K=25), [], _UNS, "sgr_sg_shading: needs envWidth 16 or 32 and SGNum <= 24"),
    ("sgr_sg_shading", dict(eh=4, ew=8), [], _UNS, "sgr_sg_shading: needs envWidth 16 or 32 and SGNum <= 24"),
    ("sgr_sg_shading", dict(premap=-1), [], _BAD, "sgr_sg_shading: premap must be 0, 1 or 2"),
    ("sgr_render_env_fwd", {}, [3], _BAD, "sgr_render_env_fwd: NULL tensor"),
    ("sgr_render_env_fwd", dict(bn=0), [], _BAD, "sgr_render_env_fwd: non-positive size"),
    ("sgr_render_env_fwd", dict(imH=12, imW=18), [], _UNS, "sgr_render_env_fwd: " + _RATIO),
    ("sgr_render_env_fwd", dict(imH=8, imW=6), [], _UNS, "sgr_render_env_fwd: " + _RATIO),
    ("sgr_fused_fwd", {}, [9], _BAD, "sgr_fused_fwd: NULL tensor"),
    ("sgr_fused_fwd", dict(K=0), [], _BAD, "sgr_fused_fwd: non-positive size"),
    ("sgr_fused_fwd", dict(K=33), [], _UNS, "sgr_fused_fwd: SGNum > 32 is not supported"),
    ("sgr_fused_fwd", dict(imH=4, imW=12), [], _UNS, "sgr_fused_fwd: " + _RATIO),
    ("sgr_fused_fwd", dict(premap=4), [], _BAD, "sgr_fused_fwd: premap must be 0..3"),
    ("sgr_fused_fwd", dict(premap=3, K=6), [], _UNS, "sgr_fused_fwd: " + _HEADS),
    ("sgr_fused_fwd", dict(premap=3, K=25), [], _UNS, "sgr_fused_fwd: " + _HEADS),
    ("sgr_fused_fwd", dict(premap=3, eh=4, ew=8), [], _UNS, "sgr_fused_fwd: " + _HEADS),
    ("sgr_fused_fwd", dict(premap=3, R=1200, C=1200, imH=1200, imW=1200), [], _UNS, "sgr_fused_fwd: " + _HEADS),
    ("sgr_fused_fwd", dict(K=33, imH=5), [], _UNS, "sgr_fused_fwd: SGNum > 32 is not supported"),      # two at once: lobes before ratio
    ("sgr_fused_fwd", dict(premap=4, imH=5), [], _UNS, "sgr_fused_fwd: " + _RATIO),                     # ratio before premap
    ("sgr_fused_fwd_tan", {}, [0], _BAD, "sgr_fused_fwd: NULL tensor"),
    ("sgr_fused_fwd_tan", dict(C=-1), [], _BAD, "sgr_fused_fwd: non-positive size"),
    ("sgr_fused_fwd_tan", dict(K=40), [], _UNS, "sgr_fused_fwd: SGNum > 32 is not supported"),
    ("sgr_fused_fwd_tan", dict(imH=16, imW=24), [], _UNS, "sgr_fused_fwd: " + _RATIO),
    ("sgr_fused_fwd_tan", dict(premap=-1), [], _BAD, "sgr_fused_fwd: premap must be 0..3"),
    ("sgr_fused_fwd_tan", dict(premap=3, K=5), [], _UNS, "sgr_fused_fwd: " + _HEADS),
    ("sgr_sg_to_env_bwd", {}, [7], _BAD, "sgr_sg_to_env_bwd: NULL tensor"),
    ("sgr_sg_to_env_bwd", dict(eh=0), [], _BAD, "sgr_sg_to_env_bwd: non-positive size"),
    ("sgr_sg_to_env_bwd", dict(premap=3), [], _BAD, "sgr_sg_to_env_bwd: premap must be 0, 1 or 2"),
    ("sgr_fused_bwd_sg", {}, [1], _BAD, "sgr_fused_bwd_sg: NULL tensor"),
    ("sgr_fused_bwd_sg", dict(bn=-2), [], _BAD, "sgr_fused_bwd_sg: non-positive size"),
    ("sgr_fused_bwd_sg", dict(premap=4), [], _BAD, "sgr_fused_bwd_sg: premap must be 0..3"),
    ("sgr_fused_bwd_sg", dict(imH=9), [], _UNS, "sgr_fused_bwd_sg: " + _RATIO),
    ("sgr_fused_bwd_sg", dict(premap=3, K=6), [], _UNS, "sgr_fused_bwd_sg: " + _HEADS),
    ("sgr_fused_bwd_sg", dict(premap=3, eh=3, ew=6), [], _UNS, "sgr_fused_bwd_sg: " + _HEADS),
    ("sgr_fused_bwd_sg", dict(premap=4, imH=9), [], _BAD, "sgr_fused_bwd_sg: premap must be 0..3"),       # two at once: premap before ratio
    ("sgr_render_env_bwd_env", {}, [7], _BAD, "sgr_render_env_bwd_env: NULL tensor"),
    ("sgr_render_env_bwd_env", dict(C=0), [], _BAD, "sgr_render_env_bwd_env: non-positive size"),
    ("sgr_render_env_bwd_env", dict(imH=4, imW=12), [], _UNS, "sgr_render_env_bwd_env: " + _RATIO),
    ("sgr_render_bwd_brdf", {}, [13], _BAD, "sgr_render_bwd_brdf: NULL tensor"),
    ("sgr_render_bwd_brdf", {}, [5, 6], _BAD, "sgr_render_bwd_brdf: need either env or the SG parameters"),
    ("sgr_render_bwd_brdf", dict(K=0), [5], _BAD, "sgr_render_bwd_brdf: need either env or the SG parameters"),
    ("sgr_render_bwd_brdf", dict(R=0), [], _BAD, "sgr_render_bwd_brdf: non-positive size"),
    ("sgr_render_bwd_brdf", dict(K=33), [], _UNS, "sgr_render_bwd_brdf: SGNum > 32 is not supported"),
    ("sgr_render_bwd_brdf", dict(imH=12), [], _UNS, "sgr_render_bwd_brdf: " + _RATIO),
    ("sgr_render_bwd_brdf", dict(premap=3), [], _BAD, "sgr_render_bwd_brdf: premap must be 0, 1 or 2"),
    ("sgr_render_bwd_brdf", dict(premap=3, imH=12), [], _UNS, "sgr_render_bwd_brdf: " + _RATIO),         # two at once: ratio before premap
    ("sgr_fused_fwd_recon", {}, [8], _BAD, "sgr_fused_fwd_recon: NULL tensor"),
    ("sgr_fused_fwd_recon", dict(K=-1), [], _BAD, "sgr_fused_fwd_recon: non-positive size"),
    ("sgr_fused_fwd_recon", dict(K=25), [], _UNS, "sgr_fused_fwd_recon: " + _RECON),
    ("sgr_fused_fwd_recon", dict(eh=4, ew=8), [], _UNS, "sgr_fused_fwd_recon: " + _RECON),
    ("sgr_fused_fwd_recon", dict(R=1200, C=1200, imH=1200, imW=1200), [], _UNS, "sgr_fused_fwd_recon: " + _RECON),
    ("sgr_fused_fwd_recon", dict(imH=4, imW=7), [], _UNS, "sgr_fused_fwd_recon: " + _RATIO),
    ("sgr_fused_fwd_recon", dict(premap=7), [], _BAD, "sgr_fused_fwd_recon: premap must be 0..3"),
    ("sgr_fused_fwd_recon", dict(premap=3, K=6), [], _UNS, "sgr_fused_fwd_recon: premap 3 (decoder heads as a prologue) needs 6 < SGNum <= 24"),
    ("sgr_fused_fwd_recon", dict(eh=4, ew=8, imH=5), [], _UNS, "sgr_fused_fwd_recon: " + _RECON),       # two at once: grid before ratio
    ("sgr_fused_fwd_recon_seg", dict(segH=12, segW=18), [], _UNS, "sgr_fused_fwd_recon_seg: object mask / env-grid ratio must be 1 or 2 (pool first)"),
    ("sgr_fused_fwd_recon_seg", dict(segH=4, segW=12), [], _UNS, "sgr_fused_fwd_recon_seg: object mask / env-grid ratio must be 1 or 2 (pool first)"),
    ("sgr_fused_fwd_recon_seg", {}, [0], _BAD, "sgr_fused_fwd_recon: NULL tensor"),
    ("sgr_fused_fwd_recon_seg", dict(bn=0), [], _BAD, "sgr_fused_fwd_recon: non-positive size"),
    ("sgr_fused_fwd_recon_seg", dict(K=25), [], _UNS, "sgr_fused_fwd_recon: " + _RECON),
    ("sgr_fused_fwd_recon_seg", dict(imH=3), [], _UNS, "sgr_fused_fwd_recon: " + _RATIO),
    ("sgr_fused_fwd_recon_seg", dict(premap=4), [], _BAD, "sgr_fused_fwd_recon: premap must be 0..3"),
    ("sgr_fused_fwd_recon_seg", dict(premap=3, K=3), [], _UNS, "sgr_fused_fwd_recon: premap 3 (decoder heads as a prologue) needs 6 < SGNum <= 24"),
    ("sgr_light_objective_fwd", {}, [9], _BAD, "sgr_light_objective_fwd: NULL tensor"),
    ("sgr_light_objective_fwd", {}, [26], _BAD, "sgr_light_objective_fwd: g_diffuse / g_spec come together"),
    ("sgr_light_objective_fwd", dict(imH=12, imW=18), [], _UNS, "sgr_light_objective_fwd: image / env-grid ratio must be 1 or 2 (pool first)"),
    ("sgr_light_objective_fwd", dict(imH=12, imW=18), [9], _BAD, "sgr_light_objective_fwd: NULL tensor"),      # two at once: NULL before ratio
    ("sgr_light_objective_fwd", dict(imH=12, imW=18, K=0), [], _UNS, "sgr_light_objective_fwd: image / env-grid ratio must be 1 or 2 (pool first)"),
    ("sgr_light_objective_fwd", {}, [0], _BAD, "sgr_fused_fwd_recon: NULL tensor"),
    ("sgr_light_objective_fwd", dict(K=0), [], _BAD, "sgr_fused_fwd_recon: non-positive size"),
    ("sgr_light_objective_fwd", dict(eh=3, ew=6), [], _UNS, "sgr_fused_fwd_recon: " + _RECON),
    ("sgr_light_objective_fwd", dict(brdfH=12, brdfW=18), [], _UNS, "sgr_fused_fwd_recon: " + _RATIO),
    ("sgr_light_objective_fwd", dict(premap=4), [], _BAD, "sgr_fused_fwd_recon: premap must be 0..3"),
    ("sgr_light_objective_fwd", dict(premap=3, K=6), [], _UNS, "sgr_fused_fwd_recon: premap 3 (decoder heads as a prologue) needs 6 < SGNum <= 24"),
    ("sgr_fused_bwd_recon", {}, [10], _BAD, "sgr_fused_bwd_recon: NULL tensor"),
    ("sgr_fused_bwd_recon", {}, [15], _BAD, "sgr_fused_bwd_recon: the gradient outputs come all three (with g_diffuse / g_spec) or not at all"),
    ("sgr_fused_bwd_recon", dict(R=0), [], _BAD, "sgr_fused_bwd_recon: non-positive size"),
    ("sgr_fused_bwd_recon", dict(premap=4), [], _BAD, "sgr_fused_bwd_recon: premap must be 0..3"),
    ("sgr_fused_bwd_recon", dict(premap=3, K=6), [], _UNS, "sgr_fused_bwd_recon: premap 3 (decoder heads as a prologue) needs 6 < SGNum <= 24"),
    ("sgr_fused_bwd_recon", dict(K=25), [], _UNS, "sgr_fused_bwd_recon: " + _RECON),
    ("sgr_fused_bwd_recon", dict(eh=4, ew=8), [], _UNS, "sgr_fused_bwd_recon: " + _RECON),
    ("sgr_fused_bwd_recon", dict(imH=4, imW=12), [], _UNS, "sgr_fused_bwd_recon: " + _RATIO),
    ("sgr_fused_bwd_recon", dict(premap=3, K=5, eh=4, ew=8), [], _UNS,
     "sgr_fused_bwd_recon: premap 3 (decoder heads as a prologue) needs 6 < SGNum <= 24"),                  # two at once: heads before grid
    ("sgr_fused_bwd_recon_total_brdf", {}, [21], _BAD, "sgr_fused_bwd_recon_total_brdf: NULL scalar"),
    ("sgr_fused_bwd_recon_total_brdf", {}, [17], _BAD,
     "sgr_fused_bwd_recon_total_brdf: g_albedo / g_normal / g_rough come all three (with the SG gradients) or not at all"),
    ("sgr_fused_bwd_recon_total_brdf", dict(premap=3), [], _UNS,
     "sgr_fused_bwd_recon_brdf: premap 3 (decoder outputs): activate them with sgr_light_heads_fwd and pass premap 1"),
    ("sgr_fused_bwd_recon_total_brdf", {}, [0], _BAD, "sgr_fused_bwd_recon: NULL tensor"),
    ("sgr_fused_bwd_recon_total_brdf", dict(C=0), [], _BAD, "sgr_fused_bwd_recon: non-positive size"),
    ("sgr_fused_bwd_recon_total_brdf", dict(premap=-1), [], _BAD, "sgr_fused_bwd_recon: premap must be 0..3"),
    ("sgr_fused_bwd_recon_total_brdf", dict(K=25), [], _UNS, "sgr_fused_bwd_recon: " + _RECON),
    ("sgr_fused_bwd_recon_total_brdf", dict(imH=16, imW=24), [], _UNS, "sgr_fused_bwd_recon: " + _RATIO),
    ("sgr_render_loss_fwd_total", {}, [2], _BAD, "sgr_render_loss_fwd: NULL tensor"),
    ("sgr_render_loss_fwd_total", {}, [10], _BAD, "sgr_render_loss_fwd: loss / scale / divisor"),
    ("sgr_render_loss_fwd_total", dict(bn=0), [], _BAD, "sgr_render_loss_fwd: non-positive size"),
    ("sgr_render_loss_fwd_total", dict(imH=12, imW=18), [], _UNS, "sgr_render_loss_fwd: image / env-grid ratio must be 1 or 2 (pool first)"),
    ("sgr_render_loss_fwd_total", dict(imH=8, imW=6), [], _UNS, "sgr_render_loss_fwd: image / env-grid ratio must be 1 or 2 (pool first)"),
    ("sgr_render_loss_fwd_total", dict(R=-4, imH=-4), [], _BAD, "sgr_render_loss_fwd: non-positive size"),    # two at once: size before ratio
]


def _refused_call(lib, name, changed, nulls):
    """Call `name` with fake non-NULL pointers (NULL stream), the valid sizes of _VALID except `changed`, and the pointer
    arguments whose index among the pointers is in `nulls` passed as NULL."""
    argtypes = _lib.SIGNATURES[name][0]
    sizes = dict(_VALID, **changed)
    ints = [sizes[k] for k in _INTS[name].split()]
    n_ptr = sum(1 for t in argtypes if t is ctypes.c_void_p)
    args, ip, ii = [], 0, 0
    for t in argtypes:
        if t is ctypes.c_void_p:
            args.append(None if (ip in nulls or ip == n_ptr - 1) else ctypes.c_void_p(4096))     # the last pointer is the stream
            ip += 1
        elif t is ctypes.c_int:
            args.append(ints[ii])
            ii += 1
        else:
            args.append(ctypes.c_float(0.05))
    assert ii == len(ints)
    rc = getattr(lib, name)(*args)
    return rc, lib.sgr_last_error().decode().split(" [a HIP error was already pending")[0]


def test_layer_entry_points_refuse_as_before():
    lib = _lib.load()
    assert sorted(set(c[0] for c in _REFUSALS)) == sorted(_INTS)
    got = [(name, changed, nulls) + _refused_call(lib, name, changed, nulls) for name, changed, nulls, _, _ in _REFUSALS]
    assert got == [tuple(c) for c in _REFUSALS]
    # the support queries built on the same predicates, the env-bytes limit (one image's env tensor < 2^31 bytes) included
    assert lib.sgr_heads_prologue_supported(12, 1200, 1200, 8, 16) == 0 and lib.sgr_heads_prologue_supported(7, 4, 6, 16, 32) == 1
    assert lib.sgr_fused_recon_supported(12, 1200, 1200, 8, 16) == 0 and lib.sgr_fused_recon_supported(1, 4, 6, 8, 16) == 1
    assert lib.sgr_fused_recon_supported(0, 4, 6, 8, 16) == 0 and lib.sgr_fused_recon_supported(25, 4, 6, 8, 16) == 0
    # the direction table's size: 4 * padded J  +  8 * envHeight rounded up to even  +  8 * envWidth floats
    assert [lib.sgr_dirs_floats(eh, ew) for eh, ew in ((8, 16), (16, 32), (4, 8), (3, 6), (1, 2))] == [704, 2432, 224, 208, 160]
